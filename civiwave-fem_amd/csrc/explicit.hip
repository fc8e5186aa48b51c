// explicit.hip -- the explicit central-difference stepper's node pass and the power iteration's vector passes
// (abi_explicit.cpp drives them). fp64 math on f32 state, rounded exactly where the scheme of include/cwf_hip.h
// rounds; compiled with -ffp-contract=off so a host restatement of the same operations gives the same bits.
#include "cwf_internal.hpp"

namespace cwf
{
namespace
{
constexpr int kBlock = 256;

// a node's three f32: one 12-B access (4-B aligned)
struct alignas(4) F3
{
    float c[3];
};
__device__ __forceinline__ F3 load3(const float *p, uint32_t n) { return *reinterpret_cast<const F3 *>(p + 3ull * n); }
__device__ __forceinline__ void store3(float *p, uint32_t n, const F3 &v) { *reinterpret_cast<F3 *>(p + 3ull * n) = v; }

// pack.cpp:41-57 safe_cast_double_to_float, as k_scaled_load (stepper.hip)
__device__ __forceinline__ float safe_cast(double v)
{
    const double fmax = 3.4028234663852886e38;  // FLT_MAX
    if (!isfinite(v))
        return v > 0.0 ? __int_as_float(0x7f800000) : v < 0.0 ? __int_as_float((int)0xff800000u) : __int_as_float(0x7fc00000);
    if (v > fmax)
        return 3.4028234663852886e38f;
    if (v < -fmax)
        return -3.4028234663852886e38f;
    return (float)v;
}

// One step of the scheme per node. FOLD: the node's row of y = K w is folded here from the partials the FAST tile
// launch left in s.t.part, in k_keff_finalize's order and arithmetic (fast_dispatch.hip; s carries the scalars (1, 0)),
// so the bits are cwf_hip_apply_keff's and no finalize pass runs; else y holds the rows (PARITY). PATTERN: f_n from
// the f64 load pattern. DAMP: beta_R != 0, the operator's next input is its own buffer.
// Traffic per node, FOLD, no pattern, undamped: u v f read and u v written (5 x 12 B), the partial run (12 B on a
// structured block), mass and mask (8 B): 80 B; bc_value is read only by constrained nodes.
// DASH: absorbing boundaries. Every node reads its slot (+4 B: 84 B); a dashpot node then loads its P | Q record
// (18 f64, 144 B, nine 16-B loads that depend on the slot) and takes the matrix form of the scheme, the others the
// expression above. With dashpots on five faces of a 150^3-node block (3.3 % of the nodes) that is 84 + 0.033 x 144
// = 88.8 B per node. The branch diverges only in waves that touch the boundary; it is not launched without dashpots.
// MON: monitors (include/cwf_hip.h "Monitors"); which of the two is active is a launch-uniform test of a.peak and
// a.ecum. The ledger's block reduction needs every lane of the tail workgroup at the barrier, so a lane past N is
// carried through on node N - 1's loads, stores nothing and shares zeros. Peaks: three 4-B loads and up to three 4-B
// stores per node (+24 B worst case; a peak that did not rise is not stored). Ledger: a dashpot node loads its C
// (72 B); per workgroup 16 B read and written every step, 16 B more written on a sampled step.
// PLAS: plasticity (include/cwf_hip.h "Plasticity"): the node's correction force p (+12 B) enters g = ((f - y) + p) / m
// in both forms; a stepper without plasticity launches the instantiations without it, whose code is what it was.
// TIE: tied boundaries (include/cwf_hip.h "Tied boundaries"), only together with DASH: a tied node has a slot, whose
// record holds its group's P_G | Q_G, and a.dgroup names the group (+4 B, a load that depends on the slot); its g is
// the group's, three f64 from a.tg (explicit_tie_gather wrote them this step), instead of the node's own quotient. A
// slot at or past a.dash_slots carries no dashpot, so the ledger reads no C for it. Launched only while a tie set is in
// force; the instantiations without TIE are what they were.
template <bool FOLD, bool PATTERN, bool DAMP, bool DASH, bool MON, bool PLAS, bool TIE = false>
__global__ __launch_bounds__(kBlock) void k_explicit_update(DevSys s, ExplicitPass a)
{
    const uint32_t gid = blockIdx.x * kBlock + threadIdx.x;
    const bool live = gid < s.N;
    if (!MON && !live)
        return;
    const uint32_t n = MON && !live ? s.N - 1 : gid;
    const F3 u = load3(a.u, n), v = load3(a.v, n);
    const uint32_t mk = s.mask[n];
    const float mass = s.mass[n];
    uint32_t slot = kNoDashpot;
    if constexpr (DASH)
        slot = a.dslot[n];
    F3 y;
    if constexpr (FOLD)
    {
        const DevTiles &T = s.t;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (uint32_t q = T.node_part_off[n] & kPartOffBits; q < (T.node_part_off[n + 1] & kPartOffBits); ++q)
        {
            const F3 pp = load3(T.part, T.node_major ? q : T.part_slot[q]);
            a0 += pp.c[0];
            a1 += pp.c[1];
            a2 += pp.c[2];
        }
        const float m = mass * (float)s.sM;
        F3 x = u;  // the operator's input at this node, as the last pass stored it
        if constexpr (DAMP)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                x.c[k] = (float)((double)u.c[k] + a.beta * (double)v.c[k]);
        y.c[0] = fmaf(m, (mk & 1u) ? 0.f : x.c[0], a0);
        y.c[1] = fmaf(m, (mk & 2u) ? 0.f : x.c[1], a1);
        y.c[2] = fmaf(m, (mk & 4u) ? 0.f : x.c[2], a2);
    }
    else
        y = load3(a.y, n);
    F3 f;
    if constexpr (PATTERN)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            f.c[k] = safe_cast(a.lbase[3ull * n + k] + a.scale * a.lpat[3ull * n + k]);
    }
    else
        f = load3(a.f, n);
    F3 pl;
    if constexpr (PLAS)
        pl = load3(a.p, n);
    F3 un, vn, wn;
    const double m = (double)mass;
    bool bad = false;
    if (DASH && slot != kNoDashpot)
    {
        // the record is 16-B aligned (144 B records in a hipMalloc'd array)
        const double2 *rec = reinterpret_cast<const double2 *>(a.dpq + 18ull * slot);
        double pq[18];
#pragma unroll
        for (int i = 0; i < 9; ++i)
        {
            const double2 t = rec[i];
            pq[2 * i] = t.x;
            pq[2 * i + 1] = t.y;
        }
        const double *P = pq, *Q = pq + 9;
        const double v0 = (double)v.c[0], v1 = (double)v.c[1], v2 = (double)v.c[2];
        double g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            if constexpr (PLAS)
                g[k] = (((double)f.c[k] - (double)y.c[k]) + (double)pl.c[k]) / m;
            else
                g[k] = ((double)f.c[k] - (double)y.c[k]) / m;
        }
        if constexpr (TIE)
        {
            const uint32_t grp = a.dgroup[slot];
            if (grp != kNoDashpot)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    g[k] = a.tg[3ull * grp + k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            vn.c[k] = (float)(((P[3 * k] * v0 + P[3 * k + 1] * v1) + P[3 * k + 2] * v2) +
                              ((Q[3 * k] * g[0] + Q[3 * k + 1] * g[1]) + Q[3 * k + 2] * g[2]));
            un.c[k] = (float)((double)u.c[k] + a.dt * (double)vn.c[k]);
        }
    }
    else
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            if constexpr (PLAS)
                vn.c[k] = (float)(a.c1 * (double)v.c[k] +
                                  a.c2 * ((((double)f.c[k] - (double)y.c[k]) + (double)pl.c[k]) / m));
            else
                vn.c[k] = (float)(a.c1 * (double)v.c[k] + a.c2 * (((double)f.c[k] - (double)y.c[k]) / m));
            un.c[k] = (float)((double)u.c[k] + a.dt * (double)vn.c[k]);
        }
    }
    if (mk)
    {
        const F3 bc = load3(a.bcv, n);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (mk & (1u << k))
            {
                un.c[k] = bc.c[k];
                vn.c[k] = 0.f;
            }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        bad = bad || !isfinite(un.c[k]) || !isfinite(vn.c[k]);
        if constexpr (DAMP)
            wn.c[k] = (float)((double)un.c[k] + a.beta * (double)vn.c[k]);
    }
    if (live)
    {
        store3(a.u, n, un);
        store3(a.v, n, vn);
        if constexpr (DAMP)
            store3(a.w, n, wn);
        if (bad)
            atomicOr(a.non_finite, 1u);
    }
    if constexpr (MON)
    {
        if (a.peak && live)
        {
            const double a0 = ((double)vn.c[0] - (double)v.c[0]) / a.dt, a1 = ((double)vn.c[1] - (double)v.c[1]) / a.dt,
                         a2 = ((double)vn.c[2] - (double)v.c[2]) / a.dt;
            const float x[3] = {
                (float)sqrt(((double)un.c[0] * un.c[0] + (double)un.c[1] * un.c[1]) + (double)un.c[2] * un.c[2]),
                (float)sqrt(((double)vn.c[0] * vn.c[0] + (double)vn.c[1] * vn.c[1]) + (double)vn.c[2] * vn.c[2]),
                (float)sqrt((a0 * a0 + a1 * a1) + a2 * a2)};
#pragma unroll
            for (int j = 0; j < 3; ++j)
            {
                float *p = a.peak + j * a.peak_stride + n;
                if (x[j] > *p)
                    *p = x[j];
            }
        }
        if (a.ecum)
        {
            double vb[3], t[4][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                vb[k] = 0.5 * ((double)vn.c[k] + (double)v.c[k]);
            const bool dashed = DASH && slot != kNoDashpot && a.dC && (!TIE || slot < a.dash_slots);
            double Cn[9];
            if (dashed)
#pragma unroll
                for (int i = 0; i < 9; ++i)
                    Cn[i] = a.dC[9ull * slot + i];
#pragma unroll
            for (int k = 0; k < 3; ++k)
            {
                const bool free_dof = live && !(mk & (1u << k));
                double diss = a.dt * (a.alpha * (m * (vb[k] * vb[k])));
                if (dashed)
                    diss = diss + a.dt * (vb[k] * ((Cn[3 * k] * vb[0] + Cn[3 * k + 1] * vb[1]) + Cn[3 * k + 2] * vb[2]));
                t[0][k] = free_dof ? 0.5 * (m * ((double)vn.c[k] * (double)vn.c[k])) : 0.0;
                t[1][k] = free_dof ? 0.5 * ((double)un.c[k] * (double)y.c[k]) : 0.0;
                t[2][k] = free_dof ? a.dt * (vb[k] * (double)f.c[k]) : 0.0;
                t[3][k] = free_dof ? diss : 0.0;
            }
            // kinetic and potential only on a sampled step (launch-uniform)
            __shared__ double part[4][kBlock / 64];
            const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
            for (int q = 0; q < 4; ++q)
            {
                if (q < 2 && !a.esample)
                    continue;
                double x = (t[q][0] + t[q][1]) + t[q][2];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1)
                    x = x + __shfl_down(x, off, 64);
                if (lane == 0)
                    part[q][wave] = x;
            }
            __syncthreads();
            if (threadIdx.x == 0)
            {
                double sum[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q >= 2 || a.esample)
                        sum[q] = (part[q][0] + part[q][1]) + (part[q][2] + part[q][3]);
                double *cum = a.ecum + 2ull * blockIdx.x;
                cum[0] = cum[0] + sum[2];
                cum[1] = cum[1] + sum[3];
                if (a.esample)
                {
                    a.ecur[2ull * blockIdx.x] = sum[0];
                    a.ecur[2ull * blockIdx.x + 1] = sum[1];
                }
            }
        }
    }
}

// A sampled step's ledger row from the workgroups' shares, in one workgroup: thread t adds workgroups t, t + 256, ...
// in that order, then the 256 sums fold pairwise (stride 128 ... 1).
__global__ __launch_bounds__(kBlock) void k_explicit_energy_fold(uint32_t blocks, const double *__restrict__ ecum,
                                                                 const double *__restrict__ ecur,
                                                                 double *__restrict__ row)
{
    __shared__ double sh[4][kBlock];
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    // four workgroups' shares are loaded before they are added (16-B loads; both arrays are hipMalloc'd), so the
    // loop waits for memory once per four; the additions keep the order t, t + 256, ...
    const double2 *cur = reinterpret_cast<const double2 *>(ecur), *cum = reinterpret_cast<const double2 *>(ecum);
    for (uint32_t b0 = threadIdx.x; b0 < blocks; b0 += 4 * kBlock)
    {
        double2 c[4], s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            const uint32_t b = b0 + j * kBlock;
            c[j] = b < blocks ? cur[b] : make_double2(0.0, 0.0);
            s[j] = b < blocks ? cum[b] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (b0 + j * kBlock < blocks)
            {
                x[0] = x[0] + c[j].x;
                x[1] = x[1] + c[j].y;
                x[2] = x[2] + s[j].x;
                x[3] = x[3] + s[j].y;
            }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        sh[q][threadIdx.x] = x[q];
    __syncthreads();
    for (uint32_t stride = kBlock / 2; stride >= 1; stride >>= 1)
    {
        if (threadIdx.x < stride)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                sh[q][threadIdx.x] = sh[q][threadIdx.x] + sh[q][threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x < 4)
        row[threadIdx.x] = sh[threadIdx.x][0];
}

// Receivers: u and v of receiver r's node into the sample's rows, one thread per receiver (a gather proportional to
// the receivers; a per-node slot read in the update pass would cost every step 4 B per node)
__global__ __launch_bounds__(kBlock) void k_explicit_record(uint32_t count, const uint32_t *__restrict__ node,
                                                            const float *__restrict__ u, const float *__restrict__ v,
                                                            float *__restrict__ row_u, float *__restrict__ row_v)
{
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= count)
        return;
    const uint32_t n = node[r];
    store3(row_u, r, load3(u, n));
    store3(row_v, r, load3(v, n));
}

// Load sources (include/cwf_hip.h "Load sources"): std::lerp as libstdc++ has it, abi_explicit.cpp's lerp_ref
__device__ __forceinline__ double lerp_dev(double a, double b, double t)
{
    if ((a <= 0 && b >= 0) || (a >= 0 && b <= 0))
        return t * b + (1 - t) * a;
    if (t == 1)
        return b;
    const double x = a + t * (b - a);
    return ((t > 1) == (b > a)) ? (b < x ? x : b) : (b > x ? x : b);
}

// cwf_explicit_curve_value on n >= 1 points: the first knot i >= 1 with t <= times[i] by bisection (times ascend, so
// the test is monotone and the i is the linear scan's, duplicate knots included), then the same operations
__device__ __forceinline__ double curve_dev(const double *__restrict__ times, const double *__restrict__ values,
                                            uint32_t n, double t)
{
    if (t <= times[0])
        return values[0];
    uint32_t lo = 1, hi = n;
    while (lo < hi)
    {
        const uint32_t mid = (lo + hi) >> 1;
        if (t <= times[mid])
            hi = mid;
        else
            lo = mid + 1;
    }
    if (lo >= n)
        return values[n - 1];
    const double t0 = times[lo - 1], span = times[lo] - t0;
    const double w = span > 0.0 ? (t - t0) / span : 0.0;
    return lerp_dev(values[lo - 1], values[lo], w);
}

// f_n of the loaded nodes, one thread per loaded node: f_ext from the compact side array, then the node's entries in
// ascending source order, acc = acc + A c in fp64 without FMA, safe_cast, one 12-B store into the force buffer the
// update pass reads. Per entry a 32-B record (two 16-B loads), 8 B of curve directory and the bisection's knots
// (log2(points) + 3 f64 loads out of a table every thread shares: L2 hits); per node 4 + 8 B of CSR and 12 B of f_ext.
// The tables stay in global memory: a 4096-point curve is 64 KiB, all of a workgroup's LDS, of which a thread reads
// 15 values; staging it would cost each workgroup the whole table every step.
__global__ __launch_bounds__(kBlock) void k_explicit_sources(ExplicitSources a, double tnow, float *__restrict__ f)
{
    const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= a.loaded)
        return;
    const F3 fe = load3(a.fext, l);
    double acc0 = (double)fe.c[0], acc1 = (double)fe.c[1], acc2 = (double)fe.c[2];
    const uint32_t end = a.off[l + 1];
    for (uint32_t e = a.off[l]; e < end; ++e)
    {
        const double2 *rec = reinterpret_cast<const double2 *>(a.rec + 4ull * e);  // 32-B records, hipMalloc'd
        const double2 r0 = rec[0], r1 = rec[1];
        const uint2 cu = reinterpret_cast<const uint2 *>(a.cur)[e];
        const double *times = a.tab + cu.x;
        const double c = curve_dev(times, times + cu.y, cu.y, tnow - r1.y);
        acc0 = acc0 + r0.x * c;
        acc1 = acc1 + r0.y * c;
        acc2 = acc2 + r1.x * c;
    }
    F3 o;
    o.c[0] = safe_cast(acc0);
    o.c[1] = safe_cast(acc1);
    o.c[2] = safe_cast(acc2);
    store3(f, a.node[l], o);
}

// the loaded nodes' f_ext: out of the force buffer into the side array (set_sources, set_external_force), and back
// (a set replaced or removed)
template <bool GATHER>
__global__ __launch_bounds__(kBlock) void k_explicit_sources_fext(uint32_t loaded, const uint32_t *__restrict__ node,
                                                                  float *f, float *fext)
{
    const uint32_t l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= loaded)
        return;
    if (GATHER)
        store3(fext, l, load3(f, node[l]));
    else
        store3(f, node[l], load3(fext, l));
}

// w = f32(u + beta_R v): the operator's input of the first step after create or set_state (later steps' passes
// store it themselves)
__global__ __launch_bounds__(kBlock) void k_explicit_input(uint32_t N, const float *__restrict__ u,
                                                           const float *__restrict__ v, double beta,
                                                           float *__restrict__ w)
{
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N)
        return;
    const F3 uu = load3(u, n), vv = load3(v, n);
    F3 ww;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        ww.c[k] = (float)((double)uu.c[k] + beta * (double)vv.c[k]);
    store3(w, n, ww);
}

// the power iteration's start vector: a hash of the DOF's index (node and axis) in [-1, 1), 0 at constrained DOFs
__device__ __forceinline__ uint32_t mix32(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

__global__ __launch_bounds__(kBlock) void k_power_start(uint32_t N, const uint32_t *__restrict__ mask,
                                                        float *__restrict__ x)
{
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N)
        return;
    const uint32_t mk = mask[n];
    F3 o;
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        const uint32_t h = mix32(3u * n + (uint32_t)k + 0x9e3779b9u);
        o.c[k] = (mk & (1u << k)) ? 0.f : (float)(h >> 8) * (1.0f / 8388608.0f) - 1.0f;
    }
    store3(x, n, o);
}

__global__ __launch_bounds__(kBlock) void k_power_z(uint32_t N, const float *__restrict__ mass,
                                                    const uint32_t *__restrict__ mask, const float *__restrict__ y,
                                                    float *__restrict__ z)
{
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N)
        return;
    const uint32_t mk = mask[n];
    const float m = mass[n];
    const F3 yy = load3(y, n);
    F3 o;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        o.c[k] = (mk & (1u << k)) ? 0.f : yy.c[k] / m;
    store3(z, n, o);
}

// x = z / lambda with lambda = num / den of this iteration (both folded already); the quotient goes to lam[0]
__global__ __launch_bounds__(kBlock) void k_power_scale(uint32_t D, const float *__restrict__ z,
                                                        const double *__restrict__ num_den, float *__restrict__ x,
                                                        double *__restrict__ lam)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const double den = num_den[1];
    const double l = den > 0.0 ? num_den[0] / den : 0.0;
    if (i == 0)
        lam[0] = l;
    if (i >= D)
        return;
    x[i] = l > 0.0 ? (float)((double)z[i] / l) : 0.f;
}

template <bool FOLD, bool PATTERN, bool PLAS>
void launch_update(const DevSys &s, const ExplicitPass &a, hipStream_t st)
{
    // a stepper without dashpots, and one without peak maps and ledger, launches the instantiations it always did
    const uint32_t grid = explicit_update_blocks(s.N);
    if (a.tg)  // a tie set is in force: the slots cover its nodes
    {
        if (a.peak || a.ecum)
        {
            if (a.w != a.u)
                k_explicit_update<FOLD, PATTERN, true, true, true, PLAS, true><<<grid, kBlock, 0, st>>>(s, a);
            else
                k_explicit_update<FOLD, PATTERN, false, true, true, PLAS, true><<<grid, kBlock, 0, st>>>(s, a);
        }
        else if (a.w != a.u)
            k_explicit_update<FOLD, PATTERN, true, true, false, PLAS, true><<<grid, kBlock, 0, st>>>(s, a);
        else
            k_explicit_update<FOLD, PATTERN, false, true, false, PLAS, true><<<grid, kBlock, 0, st>>>(s, a);
    }
    else if (a.peak || a.ecum)
    {
        if (a.dslot)
        {
            if (a.w != a.u)
                k_explicit_update<FOLD, PATTERN, true, true, true, PLAS><<<grid, kBlock, 0, st>>>(s, a);
            else
                k_explicit_update<FOLD, PATTERN, false, true, true, PLAS><<<grid, kBlock, 0, st>>>(s, a);
        }
        else if (a.w != a.u)
            k_explicit_update<FOLD, PATTERN, true, false, true, PLAS><<<grid, kBlock, 0, st>>>(s, a);
        else
            k_explicit_update<FOLD, PATTERN, false, false, true, PLAS><<<grid, kBlock, 0, st>>>(s, a);
    }
    else if (a.dslot)
    {
        if (a.w != a.u)
            k_explicit_update<FOLD, PATTERN, true, true, false, PLAS><<<grid, kBlock, 0, st>>>(s, a);
        else
            k_explicit_update<FOLD, PATTERN, false, true, false, PLAS><<<grid, kBlock, 0, st>>>(s, a);
    }
    else if (a.w != a.u)
        k_explicit_update<FOLD, PATTERN, true, false, false, PLAS><<<grid, kBlock, 0, st>>>(s, a);
    else
        k_explicit_update<FOLD, PATTERN, false, false, false, PLAS><<<grid, kBlock, 0, st>>>(s, a);
}
}  // namespace

void explicit_update(const DevSys &s, const ExplicitPass &a, hipStream_t st)
{
    if (!s.N)
        return;
    const bool pattern = a.lbase != nullptr;
    if (a.p)
    {
        if (!a.y)
            pattern ? launch_update<true, true, true>(s, a, st) : launch_update<true, false, true>(s, a, st);
        else
            pattern ? launch_update<false, true, true>(s, a, st) : launch_update<false, false, true>(s, a, st);
    }
    else if (!a.y)
        pattern ? launch_update<true, true, false>(s, a, st) : launch_update<true, false, false>(s, a, st);
    else
        pattern ? launch_update<false, true, false>(s, a, st) : launch_update<false, false, false>(s, a, st);
}

void explicit_energy_fold(uint32_t blocks, const double *ecum, const double *ecur, double *row, hipStream_t st)
{
    k_explicit_energy_fold<<<1, kBlock, 0, st>>>(blocks, ecum, ecur, row);
}

void explicit_record(uint32_t count, const uint32_t *node, const float *u, const float *v, float *row_u, float *row_v,
                     hipStream_t st)
{
    if (count)
        k_explicit_record<<<grid_for(count, kBlock), kBlock, 0, st>>>(count, node, u, v, row_u, row_v);
}

void explicit_sources(const ExplicitSources &a, double tnow, float *f, hipStream_t st)
{
    if (a.loaded)
        k_explicit_sources<<<grid_for(a.loaded, kBlock), kBlock, 0, st>>>(a, tnow, f);
}

void explicit_sources_fext(const ExplicitSources &a, float *f, bool gather, hipStream_t st)
{
    if (!a.loaded)
        return;
    if (gather)
        k_explicit_sources_fext<true><<<grid_for(a.loaded, kBlock), kBlock, 0, st>>>(a.loaded, a.node, f, a.fext);
    else
        k_explicit_sources_fext<false><<<grid_for(a.loaded, kBlock), kBlock, 0, st>>>(a.loaded, a.node, f, a.fext);
}

void explicit_operator_input(uint32_t N, const float *u, const float *v, double beta, float *w, hipStream_t st)
{
    if (N)
        k_explicit_input<<<grid_for(N, kBlock), kBlock, 0, st>>>(N, u, v, beta, w);
}

void explicit_power_start(uint32_t N, const uint32_t *mask, float *x, hipStream_t st)
{
    if (N)
        k_power_start<<<grid_for(N, kBlock), kBlock, 0, st>>>(N, mask, x);
}

void explicit_power_z(uint32_t N, const float *mass, const uint32_t *mask, const float *y, float *z, hipStream_t st)
{
    if (N)
        k_power_z<<<grid_for(N, kBlock), kBlock, 0, st>>>(N, mass, mask, y, z);
}

void explicit_power_scale(uint32_t D, const float *z, const double *num_den, float *x, double *lam, hipStream_t st)
{
    if (D)
        k_power_scale<<<grid_for(D, kBlock), kBlock, 0, st>>>(D, z, num_den, x, lam);
}

}  // namespace cwf
