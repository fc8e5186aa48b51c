// pcg_update.hip -- the update pass of the two-kernel FAST PCG iteration and the scalar hand-offs around it.
//
// k_pcg_update_tiles (256-thread workgroups, resident grid-stride): Ap from the node-major partials the element pass
//   left (never stored), the same p expression, x += alpha p (lazily: every x_lag() iterations, k_x_flush after the
//   solve), r -= alpha Ap, Dirichlet, z = M^-1 r, store x r z p, fp64 r.r / r.z shares.
// k_pcg_check: the residual step of a batch's last iteration. k_fold_pair and fast_fold_*: a shard's per-rank folds of
//   the shares a single handle's consumers fold themselves (fast_direct_fold).
#include <algorithm>

#include "blockinv_pack.hpp"
#include "fast_common.hpp"

namespace cwf
{
namespace
{
constexpr int kUpdThreads = 256;  // update-pass workgroup size (its per-workgroup shares are refolded by every consumer workgroup)
constexpr unsigned kMaxUpdateBlocks = 2048;  // 8 resident per CU (grid-stride beyond); <= 2048 shares to fold

// pcg.cpp:862-895 for the last iteration of a batch (the next batch's tiles kernel repeats it
// idempotently): one workgroup
__global__ __launch_bounds__(256) void k_pcg_check(Ctl *ctl, const double *__restrict__ prr,
                                                   const double *__restrict__ prz, unsigned nparts, unsigned stride,
                                                   unsigned it, double *__restrict__ hist)
{
    __shared__ double red[8];
    if (!ctl->active)
        return;
    float beta;
    (void)residual_step<256>(ctl, prr, prz, nparts, stride, it, hist, red, &beta);
}

// one workgroup: out[0] = fold(a[0..n)), out[1] = fold(b[0..n)) (b may be NULL), fixed order
__global__ __launch_bounds__(1024) void k_fold_pair(const double *__restrict__ a, const double *__restrict__ b,
                                                    unsigned n, double *__restrict__ out)
{
    __shared__ double red[16];
    const double ta = fold_all<1024>(a, n, red);
    const double tb = b ? fold_all<1024>(b, n, red) : 0.0;
    if (threadIdx.x == 0)
    {
        out[0] = ta;
        if (b)
            out[1] = tb;
    }
}

// The four rotating search-direction buffers: p_j lives in p[(j + 1) % 4] (fast_p_buf)
struct PBufs
{
    const float *p[4];
};

// Per-node state of the update pass, loaded in phases so that U nodes per thread have their loads in
// flight together (the pass is latency-bound: node_part_off -> partial run is a dependent chain)
struct UpdNode
{
    uint32_t n, q0, q1, mk;
    bool ok;
    float rv0[3], pa[3], pb[3], pv[3], m;
    uint4 iw;
    float xv[3], pj[kXLag][3];
};

// pcg.cpp:840-895 per owned node: Ap from the node-major partials (folded in ascending tile order),
// r -= alpha Ap, Dirichlet, z = M^-1 r (16-B Jacobi-scaled block, blockinv_pack.hpp), r.r / r.z shares;
// x += alpha_j p_j for the last `lag` iterations every lag-th iteration (lazy x, 1 = every iteration; the
// FMA chain in iteration order is bitwise the eager update), fast_flush_x applies the rest after the solve.
template <int U, bool XF, bool LAT, bool NOZ = false>
__global__ __launch_bounds__(kUpdThreads) void k_pcg_update_tiles(
    DevSys s, const float *__restrict__ rhs, const float *__restrict__ inv, const float *__restrict__ inv9,
    float *__restrict__ x, float *__restrict__ r, float *__restrict__ z, const float *__restrict__ pold,
    float *__restrict__ pnew, Ctl *__restrict__ ctl, const double *__restrict__ part_dot, unsigned ntp,
    double *__restrict__ prr, double *__restrict__ prz, unsigned it, int wt, PBufs pbuf, unsigned lag)
{
    __shared__ double red[2 * (kUpdThreads / 64)];
    __shared__ uint4 cinv[LAT ? kLatClasses : 1];
    const DevTiles &T = s.t;
    const __amdgpu_buffer_rsrc_t rctl = ctl_rsrc(ctl);
    // this iteration's beta (the K_eff kernel's residual step wrote it), as a vector load like every control word here
    const float beta = (float)ctl_f64(rctl, (uint32_t)offsetof(Ctl, beta));
    const float sM = (float)s.sM;
    const __amdgpu_buffer_rsrc_t rpart = whole_rsrc(T.part);
    // XF: this iteration applies the lazy x update (a separate instantiation, so the three iterations in four
    // that do not keep the registers of the update pass's occupancy)
    constexpr bool xflush = XF;
    const uint32_t step = gridDim.x * kUpdThreads * U;
    uint32_t base = blockIdx.x * kUpdThreads * U + threadIdx.x;
    UpdNode v[U];
    // (1) + (2): every load of the U nodes that does not need alpha (issued for the first trip before the
    // p.Ap fold below, so its latency hides under the fold's)
    const auto load_nodes = [&](uint32_t b0) {
#pragma unroll
        for (int u = 0; u < U; ++u)  // the partial-run bounds (and the Dirichlet mask in their top bits)
        {
            v[u].n = b0 + u * kUpdThreads;
            v[u].ok = v[u].n < s.Nown;
            const uint32_t n = v[u].ok ? v[u].n : 0u;
            if constexpr (LAT)  // one row value per node; the mask and the block inverse from the node's class
            {
                v[u].q0 = n;
                v[u].q1 = n + 1u;
                v[u].mk = T.lcls[n];  // class << 3 | mask
            }
            else
            {
                const uint32_t o0 = T.node_part_off[n], o1 = T.node_part_off[n + 1];
                v[u].q0 = o0 & kPartOffBits;
                v[u].q1 = o1 & kPartOffBits;
                v[u].mk = T.off_mask ? o0 >> 29 : s.mask[n];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
        {
            UpdNode &w = v[u];
            const uint32_t n = w.ok ? w.n : 0u;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                w.rv0[k] = r[3u * n + k];
            if constexpr (LAT)
                load3(rpart, n, w.pa);
            else
            {
                w.iw = reinterpret_cast<const uint4 *>(inv)[n];
                // first two partials unconditionally (the part buffer carries 2 padding slots)
                if (T.node_major)
                {
                    load3(rpart, w.q0, w.pa);
                    load3(rpart, w.q0 + 1, w.pb);
                }
            }
            // a node of no element forms p_it here (Ap = m s_M p); the tiles kernel folded the mass term
            // into every other node's owner partial
            w.m = 0.f;
            w.pv[0] = w.pv[1] = w.pv[2] = 0.f;
            if (!LAT && w.q0 == w.q1)
            {
                w.m = s.mass[n] * sM;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    w.pv[k] = fmaf(beta, pold[3u * n + k], z[3u * n + k]);
            }
            if (xflush)
            {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    w.xv[k] = x[3u * n + k];
#pragma unroll
                for (unsigned j = 0; j < kXLag; ++j)
                    if (j < lag)
                    {
                        const float *pj = pbuf.p[(it + 2u - lag + j) % 4u];
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            w.pj[j][k] = pj[3u * n + k];
                    }
            }
        }
    };
    if (base < s.Nown)
        load_nodes(base);
    // LAT (structured block): the packed block inverse of each (boundary class, mask), lattice.cpp; thread c loads
    // class c's with the node loads in flight (one prologue round trip for the nodes, the class table, the control
    // block and the p.Ap shares, instead of three)
    static_assert(!LAT || kLatClasses <= kUpdThreads, "one class per thread");
    uint4 cw = {0u, 0u, 0u, 0u};
    if constexpr (LAT)
        cw = T.lcinv6[min((uint32_t)threadIdx.x, kLatClasses - 1u)];
    // control words (ctl_rsrc): the flag, rho and the lazy-x alphas, in flight with the node loads and the fold's
    const int active = (int)__builtin_amdgcn_raw_buffer_load_b32(rctl, (uint32_t)offsetof(Ctl, active), 0, 0);
    const double rho = ctl_f64(rctl, (uint32_t)(offsetof(Ctl, rho2) + 8u * (it & 1u)));
    double ah[kXLag];
#pragma unroll
    for (unsigned j = 0; j < kXLag; ++j)
        ah[j] = xflush ? ctl_f64(rctl, (uint32_t)(offsetof(Ctl, alpha_h) + 8u * j)) : 0.0;
    // pcg.cpp:840-852: alpha = rho / (p . Ap)
    const double denom = fold_all<kUpdThreads, 12>(part_dot, ntp, red);  // <= 3,072 K_eff shares in one trip
    if (!active)
        return;
    if constexpr (LAT)
    {
        if (threadIdx.x < kLatClasses)
            cinv[threadIdx.x] = cw;
        __syncthreads();
    }
    if (fabs(denom) < 1.0e-18)
    {
        if (blockIdx.x == 0 && threadIdx.x == 0)
        {
            ctl->denom = denom;
            ctl->error = CWF_ERR_DENOM_ZERO;
            ctl->error_iter = (int)it;
            ctl->active = 0;
        }
        return;
    }
    const double alpha_d = rho / denom;
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
        ctl->denom = denom;
        ctl->alpha = alpha_d;
        ctl->alpha_last = alpha_d;
        ctl->alpha_h[it % kXLag] = alpha_d;
    }
    float aj[kXLag];  // alpha of iteration it + 1 - lag + j
#pragma unroll
    for (unsigned j = 0; j < kXLag; ++j)
    {
        const unsigned ij = it + 1u - lag + j;
        aj[j] = j < lag ? (float)(ij == it ? alpha_d : ah[ij % kXLag]) : 0.f;
    }
    const float alpha = (float)alpha_d;
    double rr = 0.0, rz = 0.0;
    for (; base < s.Nown; base += step)
    {
        if (base != blockIdx.x * kUpdThreads * U + threadIdx.x)
            load_nodes(base);
        // (3) fold, update, precondition, store
#pragma unroll
        for (int u = 0; u < U; ++u)
        {
            UpdNode &w = v[u];
            if (!w.ok)
                continue;
            const uint32_t n = w.n, mk = LAT ? w.mk & 7u : w.mk;
            if constexpr (LAT)
                w.iw = cinv[w.mk];
            if (!LAT && w.q0 == w.q1)
                store3(pnew, whole_rsrc(pnew), n, w.pv[0], w.pv[1], w.pv[2], false);
            if (xflush)  // x and the lag p_j were loaded with the rest; the FMA chain in iteration order
            {
#pragma unroll
                for (unsigned j = 0; j < kXLag; ++j)
                    if (j < lag)
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            w.xv[k] = fmaf(aj[j], w.pj[j][k], w.xv[k]);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (mk & (1u << k))
                        w.xv[k] = rhs[3u * n + k];
                store3(x, whole_rsrc(x), n, w.xv[0], w.xv[1], w.xv[2], wt);
            }
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            const uint32_t cnt = w.q1 - w.q0;
            if (LAT)
            {
                a0 = w.pa[0];
                a1 = w.pa[1];
                a2 = w.pa[2];
            }
            else if (T.node_major)
            {
                if (cnt > 0)
                {
                    a0 = w.pa[0];
                    a1 = w.pa[1];
                    a2 = w.pa[2];
                }
                if (cnt > 1)
                {
                    a0 += w.pb[0];
                    a1 += w.pb[1];
                    a2 += w.pb[2];
                }
                for (uint32_t q = 2; q < cnt; ++q)
                {
                    float d[3];
                    load3(rpart, w.q0 + q, d);
                    a0 += d[0];
                    a1 += d[1];
                    a2 += d[2];
                }
            }
            else
                for (uint32_t q = w.q0; q < w.q1; ++q)
                {
                    const float *pp = T.part + 3ull * T.part_slot[q];
                    a0 += pp[0];
                    a1 += pp[1];
                    a2 += pp[2];
                }
            const float av[3] = {a0, a1, a2};
            float rv[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
            {
                const float apk = cnt == 0 ? w.m * w.pv[k] : av[k];
                rv[k] = (mk & (1u << k)) ? 0.0f : fmaf(-alpha, apk, w.rv0[k]);
            }
            store3(r, whole_rsrc(r), n, rv[0], rv[1], rv[2], wt);
            // symmetric block inverse {a00 a01 a02 a11 a12 a22}; a flagged block (negative scale) reads its
            // fp32 copy instead
            float bv[6];
            if ((int)w.iw.x >= 0)
                unpack_block_inverse(w.iw.y, w.iw.z, w.iw.w, __uint_as_float(w.iw.x), bv);
            else
            {
                const float *a9 = LAT ? T.lcinv9 + 9u * w.mk : inv9 + 9ull * n;
                bv[0] = a9[0];
                bv[1] = a9[1];
                bv[2] = a9[2];
                bv[3] = a9[4];
                bv[4] = a9[5];
                bv[5] = a9[8];
            }
            const float iv[9] = {bv[0], bv[1], bv[2], bv[1], bv[3], bv[4], bv[2], bv[4], bv[5]};
            float zs[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
            {
                float zk = fmaf(iv[3 * k + 2], rv[2], fmaf(iv[3 * k + 1], rv[1], iv[3 * k] * rv[0]));
                zk = (mk & (1u << k)) ? 0.0f : zk;
                zs[k] = zk;
                rr += (double)rv[k] * (double)rv[k];
                rz += (double)rv[k] * (double)zk;
            }
            if constexpr (!NOZ)  // NOZ (lattice lzr): the K_eff pass forms z from r itself
                store3(z, whole_rsrc(z), n, zs[0], zs[1], zs[2], wt);
        }
    }
    // ghost nodes of a shard: only the search direction (the tiles kernel's p) is kept
    for (uint32_t n = s.Nown + blockIdx.x * kUpdThreads + threadIdx.x; n < s.N; n += gridDim.x * kUpdThreads)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            pnew[3u * n + k] = fmaf(beta, pold[3u * n + k], z[3u * n + k]);
    }
    double t0, t1;
    block_sum2<kUpdThreads>(rr, rz, red, t0, t1);
    if (threadIdx.x == 0)
    {
        prr[blockIdx.x] = t0;
        prz[blockIdx.x] = t1;
    }
}

using UpdateFn = decltype(&k_pcg_update_tiles<1, false, false>);

// U (nodes per thread) is 1 at every use. It stays a parameter: without it and its one-trip loops the compiler orders
// its passes differently and four of the six instantiations come out as other instruction streams (954 -> 943
// instructions for <false, false>), which is a change to measure, not to make in passing
template <bool XF, bool LAT, bool NOZ> Pick<UpdateFn> update_pick()
{
    static const std::string name = kernel_name("k_pcg_update_tiles", 1, XF, LAT, NOZ);
    return {k_pcg_update_tiles<1, XF, LAT, NOZ>, name.c_str()};
}

// xf: the iteration applies the lazy x terms; lat: a structured block (the class table); noz: its K_eff pass forms z
// from r (lzr), so none is stored
Pick<UpdateFn> pick_update(bool xf, bool lat, bool noz)
{
    return with_bools([](auto x, auto l, auto n) { return update_pick<x(), l(), l() && n()>(); }, xf, lat, noz);
}

// the update pass is grid-stride: at most one resident wave of workgroups (occupancy x CUs), so no
// workgroup waits for a slot behind the others' whole node ranges. The occupancy is the non-lattice instantiation's
// on every handle, lattice ones included: it fixes the grid and with it the number of r.r / r.z shares, so taking the
// lattice instantiation's would change results
unsigned update_resident(bool xf)
{
    return std::min(resident_blocks(pick_update(xf, false, false).fn, kUpdThreads, 0), kMaxUpdateBlocks);
}
}  // namespace

// flush: the grid of the lazy-x instantiation (its own occupancy); the consumers of the update's r.r / r.z
// shares ask with the flag of the iteration that produced them
unsigned fast_update_blocks(const DevSys &s, bool flush)
{
    static const unsigned resident[2] = {update_resident(false), update_resident(true)};
    constexpr unsigned cap = kMaxUpdateBlocks;
    const unsigned res = std::min(resident[flush ? 1 : 0], cap);
    const unsigned g = grid_for(s.N, kUpdThreads);
    return g < res ? (g ? g : 1u) : res;
}

// CWF_XLAG=1..4 (diagnostic): iterations per lazy x update (default kXLag)
static unsigned x_lag()
{
    static const unsigned v = [] {
        const char *e = knob("CWF_XLAG");
        const int k = e ? atoi(e) : (int)kXLag;
        return (unsigned)(k < 1 ? 1 : k > (int)kXLag ? (int)kXLag : k);
    }();
    return v;
}

// iteration j's update applies the lazy x terms
bool x_flush_iter(unsigned j) { return (j + 1u) % x_lag() == 0u; }

// the lazy x terms of the iterations after the last flush: j = n - n % lag .. n - 1, n = completed
// iterations (the device control block's count, so the host needs no iteration count)
__global__ __launch_bounds__(256) void k_x_flush(DevSys s, const float *__restrict__ rhs, float *__restrict__ x,
                                                 const Ctl *__restrict__ ctl, PBufs pb, unsigned lag)
{
    const unsigned n_it = (unsigned)ctl->iterations, j0 = n_it - n_it % lag;
    if (j0 == n_it)
        return;
    for (uint32_t n = blockIdx.x * 256 + threadIdx.x; n < s.Nown; n += gridDim.x * 256)
    {
        float xv[3] = {x[3u * n + 0], x[3u * n + 1], x[3u * n + 2]};
        for (unsigned j = j0; j < n_it; ++j)
        {
            const float *pj = pb.p[(j + 1u) % 4u];
            const float a = (float)ctl->alpha_h[j % kXLag];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                xv[k] = fmaf(a, pj[3u * n + k], xv[k]);
        }
        const uint32_t mk = s.mask[n];
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            if (mk & (1u << k))
                xv[k] = rhs[3u * n + k];
            x[3u * n + k] = xv[k];
        }
    }
}

inline PBufs fast_p_bufs(cwf_hip_system *h) { return PBufs{{h->p, h->p2, h->p3, h->p4}}; }

// x / r / z of the update pass are stored write-through (store3; C2 +2.7% PCG it/s, C3 neutral)
static bool update_write_through() { return true; }

void fast_update_pcg(cwf_hip_system *h, const float *rhs, unsigned it, hipStream_t st)
{
    const DevSys &s = h->ds;
    const bool direct = fast_direct_fold(h);
    const bool xf = x_flush_iter(it);
    const UpdateFn k = pick_update(xf, s.t.lcls != nullptr, s.t.lzr != 0).fn;
    k<<<fast_update_blocks(s, xf), kUpdThreads, 0, st>>>(
        s, rhs, h->inv6, h->inv, h->x, h->r, h->z, fast_p_old(h, it), fast_p_new(h, it), h->ctl,
        direct ? h->part0 : h->g_pap, direct ? fast_tile_blocks(s) : (unsigned)h->nranks, h->part1, h->part2, it,
        update_write_through(), fast_p_bufs(h), x_lag());
}

void fast_flush_x(cwf_hip_system *h, const float *rhs, hipStream_t st)
{
    const DevSys &s = h->ds;
    if (!s.Nown)
        return;
    const unsigned g = std::min<unsigned>(grid_for(s.Nown, 256), 2048u);
    k_x_flush<<<g, 256, 0, st>>>(s, rhs, h->x, h->ctl, fast_p_bufs(h), x_lag());
}

void fast_check_pcg(cwf_hip_system *h, unsigned it, hipStream_t st)
{
    if (fast_direct_fold(h))
        k_pcg_check<<<1, 256, 0, st>>>(h->ctl, h->part1, h->part2,
                                       fast_update_blocks(h->ds, it && x_flush_iter(it - 1u)), 1u, it, h->hist);
    else
        k_pcg_check<<<1, 256, 0, st>>>(h->ctl, h->g_rrz, h->g_rrz + 1, (unsigned)h->nranks, 2u, it, h->hist);
}

void fold_pair(const double *a, const double *b, uint32_t n, double *out, hipStream_t st)
{
    k_fold_pair<<<1, 1024, 0, st>>>(a, b, n, out);
}

// a single (unsharded) handle skips the per-rank fold kernels: every consumer workgroup refolds the
// producer's per-workgroup shares itself (<= 2048 doubles, L2-served), two launches fewer per iteration
// (C2 +11% PCG it/s against fold kernels, same-box A/B, round 2)
bool fast_direct_fold(const cwf_hip_system *h) { return !h->sharded(); }

void fast_fold_pap(cwf_hip_system *h, hipStream_t st)
{
    if (fast_direct_fold(h))
        return;
    fold_pair(h->part0, nullptr, fast_tile_blocks(h->ds), h->g_pap + h->rank, st);
}

unsigned fast_rrz_shares(const DevSys &s, unsigned it) { return fast_update_blocks(s, x_flush_iter(it)); }

void fast_fold_rrz(cwf_hip_system *h, unsigned it, hipStream_t st)
{
    if (fast_direct_fold(h))
        return;
    fold_pair(h->part1, h->part2, fast_update_blocks(h->ds, x_flush_iter(it)), h->g_rrz + 2 * h->rank, st);
}
}  // namespace cwf
