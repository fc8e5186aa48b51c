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
template <bool FOLD, bool PATTERN, bool DAMP, bool DASH>
__global__ __launch_bounds__(kBlock) void k_explicit_update(DevSys s, ExplicitPass a)
{
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= s.N)
        return;
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
            g[k] = ((double)f.c[k] - (double)y.c[k]) / m;
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
    store3(a.u, n, un);
    store3(a.v, n, vn);
    if constexpr (DAMP)
        store3(a.w, n, wn);
    if (bad)
        atomicOr(a.non_finite, 1u);
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

template <bool FOLD, bool PATTERN>
void launch_update(const DevSys &s, const ExplicitPass &a, hipStream_t st)
{
    // a stepper without dashpots launches the instantiations it always did
    if (a.dslot)
    {
        if (a.w != a.u)
            k_explicit_update<FOLD, PATTERN, true, true><<<grid_for(s.N, kBlock), kBlock, 0, st>>>(s, a);
        else
            k_explicit_update<FOLD, PATTERN, false, true><<<grid_for(s.N, kBlock), kBlock, 0, st>>>(s, a);
    }
    else if (a.w != a.u)
        k_explicit_update<FOLD, PATTERN, true, false><<<grid_for(s.N, kBlock), kBlock, 0, st>>>(s, a);
    else
        k_explicit_update<FOLD, PATTERN, false, false><<<grid_for(s.N, kBlock), kBlock, 0, st>>>(s, a);
}
}  // namespace

void explicit_update(const DevSys &s, const ExplicitPass &a, hipStream_t st)
{
    if (!s.N)
        return;
    const bool pattern = a.lbase != nullptr;
    if (!a.y)
        pattern ? launch_update<true, true>(s, a, st) : launch_update<true, false>(s, a, st);
    else
        pattern ? launch_update<false, true>(s, a, st) : launch_update<false, false>(s, a, st);
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
