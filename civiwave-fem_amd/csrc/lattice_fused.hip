// lattice_fused.hip -- k_pcg_lattice: the FAST PCG iteration of a structured block in ONE launch (the brick scheme of
// lattice.hip's k_keff_lattice), with its host driver (fast_fused_*, pcg_lattice_*), the diagnostic launch trace of the
// ablation build and a shard's class-byte exchange.
//
// The reference's loop (pcg.cpp:840-901) has two dependent global reductions per iteration: p.Ap for alpha, then
// r.z for beta, hence two kernels (k_keff_lattice, k_pcg_update_tiles) and two scalar hand-offs. Here launch j
// forms iteration j's vectors itself, for every LDS entry of its brick (halo included):
//   r_j = r_(j-1) - alpha_(j-1) Ap_(j-1)  (Dirichlet components 0),  z_j = M^-1 r_j  (the node class's block),
//   p_j = z_j + beta_j p_(j-1),  x_j = x_(j-1) + alpha_(j-1) p_(j-1)  (owned entries),
// then Ap_j = K_eff p_j by the brick stencil, and leaves five fp64 shares per workgroup: r_j.z_j, r_j.r_j, p_j.Ap_j,
// z_j.Ap_j and Ap_j.M^-1 Ap_j (Ap with its Dirichlet components 0). Launch j + 1 folds them and has
//   alpha_j = rho_j / p_j.Ap_j                                       (the direct rho_j = r_j.z_j: the reference's alpha)
//   rho_(j+1) ~ rho_j - 2 alpha_j z_j.Ap_j + alpha_j^2 Ap_j.M^-1 Ap_j  (r_(j+1).z_(j+1) expanded through r_(j+1) =
//                                                                    r_j - alpha_j Ap_j and M^-1 symmetric)
//   beta_(j+1) = rho_(j+1) / rho_j, and the convergence test on the direct |r_j|.
// Only beta's numerator is a one-step recurrence, re-based every iteration on the direct dots of the vectors actually
// stored, so the iteration counts stay within a few percent of the reference loop's, not equal to them
// (tools/cg_variants.py emulates both in FAST arithmetic: 273 / 273 on C1, 418 / 432 and 411 / 412 on a 33 x 9 x 5
// block at tol 3e-4; on C2 the Newmark steps take the PARITY loop's count to +-3; the round-4 Chronopoulos-Gear form,
// whose A u and A p recurrences run in fp32, needed 45-55% more). Per-iteration rates (PCG it/s) of the two schedules
// are therefore compared next to their iteration counts (bench.py reports both). The convergence of r_j is
// decided at launch j + 1's start, where the two-kernel loop's K_eff kernel decides it too.
//
// Buffers: r and Ap by launch parity (a brick reads halo entries of r_(j-1) / Ap_(j-1) that another workgroup's
// owned stores of r_j / Ap_j would overwrite), p over the four rotating buffers (p_j in [(j + 1) % 4]), x in place
// (owned rows only). Per node and iteration: r, Ap, p_old, the class byte and x read; r, p, Ap and x written (97 B),
// against 49 B for k_keff_lattice plus 52 B for the update pass; one launch and one scalar hand-off fewer.
//
// Entry mapping: thread t forms the interior entry of its own column (the node whose row it computes) and threads
// 0 .. 83 the 84 entries of the brick's one-node halo ring, so the thread that forms a node's z and class is the
// one that needs them for the dots of its row (three planes of them in registers).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "fast_common.hpp"

namespace cwf
{
namespace
{
struct FusedArgs
{
    Ctl *ctl;
    const double *sin;  // launch j - 1's shares, [kFusedShares][sstride] (a shard: the all-gathered rank totals,
                        // [nranks][kFusedSlot], sstride_in 1, sis kFusedSlot)
    unsigned nin;       // workgroups of launch j - 1 (a shard: ranks)
    unsigned sin_stride, sis;  // element i of array q at sin[q sin_stride + i sis]
    double *sout;       // this launch's shares, [kFusedShares][sstride]
    unsigned sstride;
    unsigned j;  // launch index; 0: the prologue's (alpha = beta = 0: r_0, z_0, p_0 = z_0, Ap_0)
    unsigned last;  // the solve's last check: max_iterations updates are made, no update follows (fused_decide)
    unsigned grid;  // workgroups (host side: the launch's grid; <= the work items, a multiple of 8 below them)
    double *hist;
    const float *rin;
    float *rout;
    const float *ain;
    float *aout;
    const float *pin;
    float *pout;
    float *x;
    unsigned px;       // a PEER shard's in-kernel exchange (pe; SHARD instantiations only)
    FusedPeerArgs pe;
    uint64_t *trace;   // diagnostic (ablation build, CWF_FUSED_TRACE): per workgroup 8 words of wall-clock stamps
};

// ---- the in-kernel PEER exchange of a shard (px): the protocol of peer.hip's k_peer_step, inside the launch ----
constexpr uint64_t kFusedPeerTimeoutTicks = 10ull * 100000000ull;  // 10 s of s_memrealtime (100 MHz)

// launch j's prologue: the solve still running, every peer's launch j - 1 arrived (its flag at epoch - 1; bounded),
// then acquire at system scope (the received Ap rows and rank totals in the uncached mailbox). False: return now
// (the solve is over, or a peer is gone: CWF_ERR_COMM, sticky)
__device__ bool fused_peer_wait(const FusedPeerArgs &pe, unsigned j, Ctl *ctl)
{
    __shared__ int ok_s;
    if (threadIdx.x < 64)
    {
        const uint32_t p = threadIdx.x;
        const bool run = __hip_atomic_load(&ctl->active, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        const bool dead = __hip_atomic_load(pe.sticky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
        bool ok = run && !dead;
        if (ok && j > 0 && p < pe.nranks && p != pe.rank)
        {
            const uint32_t *f = pe.flags + 16u * p;
            uint32_t spins = 0;
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < pe.epoch - 1u)
            {
                __builtin_amdgcn_s_sleep(2);
                if ((++spins & 63u) == 0u && __builtin_amdgcn_s_memrealtime() - t0 > kFusedPeerTimeoutTicks)
                {
                    ok = false;
                    break;
                }
            }
        }
        const bool all = __all(ok);
        if (threadIdx.x == 0)
            ok_s = all ? 1 : run && !dead ? 2 : run ? 3 : 0;  // 1 go, 2 timed out, 3 dead before, 0 solve over
    }
    __syncthreads();
    const int v = ok_s;
    if (v == 1)
    {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope: an invalidate
        return true;
    }
    if (v >= 2 && threadIdx.x == 0)
    {
        if (v == 2)
            __hip_atomic_store(pe.sticky, (uint32_t)CWF_ERR_COMM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (blockIdx.x == 0)
        {
            ctl->error = CWF_ERR_COMM;
            ctl->error_iter = (int)j;
            ctl->active = 0;
        }
    }
    return false;
}

// launch j's end, every workgroup: its write-through stores (send rows, shares) acknowledged, a ticket; the last one
// folds the launch's shares in k_fused_rank_totals' order, stores the totals into every rank's gather area and,
// after a system-scope release, this launch's epoch into every peer's flag for this rank
template <int NT>
__device__ void fused_peer_publish(const FusedArgs &fa, double *red)
{
    const FusedPeerArgs &pe = fa.pe;
    __shared__ int last_s;
    // relaxed: every store it hands off is write-through (sc0 sc1) and acknowledged (each wave's vmcnt(0) behind the
    // barrier), the hand-off form MI355X_MICROARCH.md measures valid; an acq_rel add (agent-scope L2 write-back +
    // invalidate per workgroup) cost 14 us per launch: 2 PEER ranks on one GPU, C2 strong, 34.8 ->
    // 49.0 us, 26.3k -> 19.1k PCG it/s (profiles/r06s_ticket_acq_rel.txt)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
        last_s = __hip_atomic_fetch_add(pe.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == gridDim.x;
    __syncthreads();
    if (!last_s)
        return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope: the other workgroups' shares
    double v[kFusedShares];
    fold_k<NT, kFusedShares>(fa.sout, gridDim.x, fa.sstride, red, v);
    if (threadIdx.x < kFusedSlot)
    {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < kFusedShares; ++q)
            t = threadIdx.x == (unsigned)q ? v[q] : t;
        for (uint32_t p = 0; p < pe.nranks; ++p)
            __hip_atomic_store(pe.gdst[p] + threadIdx.x, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope
        for (uint32_t p = 0; p < pe.nranks; ++p)
            if (p != pe.rank)
                __hip_atomic_store(pe.flag[p], pe.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(pe.done, pe.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(pe.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one row's write-through push into the neighbour's receive area (an address past the range: dropped)
__device__ __forceinline__ void st3_sys(__amdgpu_buffer_rsrc_t rs, uint32_t byteoff, const float v[3])
{
    const u32x3 w = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2])};
    __builtin_amdgcn_raw_buffer_store_b96(w, rs, byteoff, 0, 17);  // sc0 sc1: system scope, write-through
}

// pcg.cpp:840-895 across the launch boundary: from launch j - 1's shares, alpha_(j-1), beta_j and the convergence
// of r_(j-1); the same values in every workgroup (one fixed-order fold). Returns false when the solve is over.
template <int NT>
__device__ __forceinline__ bool fused_scalars(const FusedArgs &fa, const CtlPre &pre, double *red, float *alpha_out,
                                              float *beta_out)
{
    if (fa.j == 0)
    {
        *alpha_out = 0.f;
        *beta_out = 0.f;
        return pre.active != 0;
    }
    double v[kFusedShares];
    fold_k<NT, kFusedShares>(fa.sin, fa.nin, fa.sin_stride, red, v, fa.sis);
    if (!pre.active)
        return false;
    return fused_decide(fa.ctl, fa.hist, fa.j, pre, blockIdx.x == 0 && threadIdx.x == 0, v, alpha_out, beta_out,
                        fa.last != 0u);
}

// one LDS entry's raw values: r, Ap, p_old of iteration j - 1 and the class byte; the own column's entry also x
// (and its mass unless MU)
struct FusedFill
{
    float r[2][3], a[2][3], p[2][3];
    uint32_t c[2];
    float x[3], m;
};

// what the thread keeps of its own column's node of a formed plane until that plane's row: z_j, the class and mass
struct FusedKeep
{
    float z[3], m;
    uint32_t c;
};

// a surface node of the block (lattice_shell_node's cell form), fused: its own r_j / z_j / p_j / x_j / Ap_j and its
// dots, from gathers of its neighbours' r, Ap, p_old and classes (each neighbour's p_j formed as in the bricks)
template <class E, bool AFF, bool SHARD>
__device__ __forceinline__ void fused_shell_node(const DevSys &s, const FusedArgs &fa, const float *__restrict__ coef,
                                                 const uint32_t *__restrict__ plane, uint32_t q, float alpha,
                                                 float beta, const float4 *czA, const float2 *czB,
                                                 double d[kFusedShares])
{
    const DevTiles &T = s.t;
    const int nx = (int)T.lnx, ny = (int)T.lny, nz = (int)T.lnz;
    int i, j, k;
    uint32_t rq = q;
    const uint32_t full = (uint32_t)(nx * ny), per = (uint32_t)(2 * nx + 2 * (ny - 2));
    const uint32_t nlo = T.lk0 == 0 ? full : 0u, nmid = (T.lkI1 - T.lkI0) * per;
    if (rq < nlo)
    {
        k = 0;
        i = (int)(rq % (uint32_t)nx);
        j = (int)(rq / (uint32_t)nx);
    }
    else if ((rq -= nlo) < nmid)
    {
        k = (int)(T.lkI0 + rq / per);
        rq %= per;
        if (rq < (uint32_t)nx)
            i = (int)rq, j = 0;
        else if (rq < 2u * nx)
            i = (int)rq - nx, j = ny - 1;
        else if (rq < 2u * nx + (uint32_t)(ny - 2))
            i = 0, j = 1 + (int)rq - 2 * nx;
        else
            i = nx - 1, j = 1 + (int)rq - 2 * nx - (ny - 2);
    }
    else
    {
        rq -= nmid;
        k = nz - 1;
        i = (int)(rq % (uint32_t)nx);
        j = (int)(rq / (uint32_t)nx);
    }
    const uint32_t pk[3] = {lat_plane<AFF>(T, plane, max(k - 1, 0)), lat_plane<AFF>(T, plane, k),
                            lat_plane<AFF>(T, plane, min(k + 1, nz - 1))};
    const uint32_t n = pk[1] + (uint32_t)(j * nx + i);
    if (n >= s.Nown)
        return;
    const uint32_t vbytes = 12u * s.N;
    const __amdgpu_buffer_rsrc_t rr = sized_rsrc(fa.rin, vbytes), ra = sized_rsrc(fa.ain, vbytes),
                                 rp = sized_rsrc(fa.pin, vbytes), rcls = sized_rsrc(T.lcls, s.N);
    // px: a ghost neighbour's Ap_(j-1) is in the mailbox's receive area (ghost order), not in ain
    const bool gx = SHARD && fa.px && fa.j > 0;
    const __amdgpu_buffer_rsrc_t rg = sized_rsrc(gx ? fa.pe.arecv : nullptr, gx ? 12u * (s.N - s.Nown) : 0u);
    const auto node_at = [&](int o) {
        const int ii = min(max(i + E::off[o][0], 0), nx - 1), jj = min(max(j + E::off[o][1], 0), ny - 1),
                  kk = min(max(k + E::off[o][2], 0), nz - 1);
        return pk[kk - k + 1] + (uint32_t)(jj * nx + ii);
    };
    float w8[8];
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8)
    {
        const int cx = c8 & 1, cy = (c8 >> 1) & 1, cz = (c8 >> 2) & 1;
        w8[c8] = (cx ? i >= 1 : i + 1 < nx) && (cy ? j >= 1 : j + 1 < ny) && (cz ? k >= 1 : k + 1 < nz) ? 1.f : 0.f;
    }
    // the node itself
    float r0[3], a0[3], p0[3], x0[3], rn0[3], z0[3], u0[3];
    load3(rr, n, r0);
    load3(ra, n, a0);
    load3(rp, n, p0);
    load3(sized_rsrc(fa.x, vbytes), n, x0);
    const uint32_t c0 = __builtin_amdgcn_raw_buffer_load_b8(rcls, n, 0, 0);
    const float mass = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(sized_rsrc(s.mass, 4u * s.N), 4u * n, 0, 0));
    // 7 neighbours' r, Ap, p_old and class per batch: the kernel runs 2 waves per SIMD at its brick path's 168-170
    // VGPRs anyway, so the shell may hold up to 256 (two round trips for the 14 Kuhn neighbours instead of four)
    constexpr int BATCH = 7;
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int bt = 0; bt < (E::nOff - 1 + BATCH - 1) / BATCH; ++bt)
    {
        uint32_t mo[BATCH], mc[BATCH];
        float ra_[BATCH][3], aa_[BATCH][3], pa_[BATCH][3];
#pragma unroll
        for (int q7 = 0; q7 < BATCH; ++q7)
        {
            if (1 + BATCH * bt + q7 >= E::nOff)
                continue;
            mo[q7] = node_at(1 + BATCH * bt + q7);
            load3(rr, mo[q7], ra_[q7]);
            if constexpr (SHARD)
            {
                const bool g = gx && mo[q7] >= s.Nown;  // (without px the ghost rows of ain hold the halo)
                float ga[3];
                load3(ra, g ? kLatOob3 : mo[q7], aa_[q7]);
                load3(rg, g ? mo[q7] - s.Nown : kLatOob3, ga);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    aa_[q7][c] = g ? ga[c] : aa_[q7][c];
            }
            else
                load3(ra, mo[q7], aa_[q7]);
            load3(rp, mo[q7], pa_[q7]);
            mc[q7] = __builtin_amdgcn_raw_buffer_load_b8(rcls, mo[q7], 0, 0);
        }
        if (bt == 0)
            fused_form(czA, czB, c0, alpha, beta, r0, a0, p0, rn0, z0, u0);
#pragma unroll
        for (int q7 = 0; q7 < BATCH; ++q7)
        {
            const int o = 1 + BATCH * bt + q7;
            if (o >= E::nOff)
                continue;
            float rn[3], zz[3], dd[3];
            fused_form(czA, czB, mc[q7], alpha, beta, ra_[q7], aa_[q7], pa_[q7], rn, zz, dd);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                dd[c] -= u0[c];
#pragma unroll
            for (int p = 0; p < E::nPairs; ++p)
            {
                if (E::pairOff[p] != o)
                    continue;
                float t[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int r3 = 0; r3 < 3; ++r3)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        t[r3] = fmaf(coef[E::coefPairs + 9 * p + 3 * r3 + c], dd[c], t[r3]);
#pragma unroll
                for (int r3 = 0; r3 < 3; ++r3)
                    acc[r3] = fmaf(w8[E::pair[p][0]], t[r3], acc[r3]);
            }
        }
    }
    const float sK = (float)s.sK, m = mass * (float)s.sM;
    float a[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        a[c] = fmaf(m, u0[c], sK * acc[c]);
    const __amdgpu_buffer_rsrc_t wa = sized_rsrc(fa.aout, vbytes), wr = sized_rsrc(fa.rout, vbytes),
                                 wp = sized_rsrc(fa.pout, vbytes), wx = sized_rsrc(fa.x, vbytes);
    const auto st3 = [](__amdgpu_buffer_rsrc_t rs, uint32_t node, const float v[3]) {
        const u32x3 w = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2])};
        __builtin_amdgcn_raw_buffer_store_b96(w, rs, 12u * node, 0, 0);
    };
    float xn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        xn[c] = fmaf(alpha, p0[c], x0[c]);
    st3(wa, n, a);
    st3(wr, n, rn0);
    st3(wp, n, u0);
    st3(wx, n, xn);
    if constexpr (SHARD)  // px: a send plane's row into the neighbour's receive area (else past the range: dropped)
    {
#pragma unroll
        for (int e = 0; e < 2; ++e)
        {
            const __amdgpu_buffer_rsrc_t rd = sized_rsrc(fa.pe.dst[e], fa.pe.dst_bytes[e]);
            st3_sys(rd, k == fa.pe.send_k[e] ? 12u * (uint32_t)(j * nx + i) : 12u * kLatOob3, a);
        }
    }
    fused_entry_dots(rn0, z0, d);
    fused_row_dots(czA, czB, c0, u0, z0, a, d);
}

template <bool SYM, class E, bool MU, bool AFF, bool SHARD, bool PERSIST>
__global__ __launch_bounds__(kLatNT) void k_pcg_lattice(DevSys s, FusedArgs fa, const float *__restrict__ coef,
                                                        const uint32_t *__restrict__ plane)
{
    constexpr int BX = kLatBX, BY = kLatNT / BX, PX = BX + 2, PLANE = PX * (BY + 2), NH = PLANE - kLatNT;
    static_assert(NH <= kLatNT, "one halo-ring entry per thread at most");
    __shared__ float4 pl[kLatRing][PLANE];
    __shared__ double red[kFusedShares * (kLatNT / 64)];
    __shared__ float4 czA[kLatClasses];
    __shared__ float2 czB[kLatClasses];
    const DevTiles &T = s.t;
    // Persistent: workgroup b takes the work items (virtual block indices) b, b + grid, b + 2 grid, ... of the
    // non-persistent numbering (grid a multiple of 8, so every item keeps its XCD), one fold per workgroup and one
    // share per workgroup however many items the grid covers (the next launch folds 5 x grid values, not 5 x items)
    struct Item
    {
        bool shell;
        uint32_t ib, jb, kc, qs, qn;
    };
    const uint32_t cols = max(T.lnbx * T.lnby, 1u);
    const auto decode = [&](uint32_t vb) {
        Item it{false, 0u, 0u, 0u, 0u, 0u};
        if (T.lshl == 2)
        {
            const uint32_t nw = T.lnwork, xcd = vb & 7u;
            const uint32_t w = xcd * (nw >> 3) + min(xcd, nw & 7u) + (vb >> 3);
            const uint32_t cw = cols + T.lnsc, nchunk = (T.lkI1 - T.lkI0 + T.lL - 1) / T.lL;
            const uint32_t nx = T.lnx, ny = T.lny, full = nx * ny, per = 2 * nx + 2 * (ny - 2);
            const uint32_t nlo = T.lk0 == 0 ? full : 0u, nmid = (T.lkI1 - T.lkI0) * per;
            if (w < nchunk * cw)
            {
                it.kc = w / cw;
                const uint32_t r = w % cw;
                it.shell = r >= cols;
                it.ib = r % max(T.lnbx, 1u);
                it.jb = r / max(T.lnbx, 1u);
                const uint32_t k0c = it.kc * T.lL, np = min(T.lL, T.lkI1 - T.lkI0 - k0c) * per,
                               ql = (r - cols) * kLatNT;
                it.qs = nlo + k0c * per + ql;
                it.qn = it.shell && ql < np ? min(np - ql, (uint32_t)kLatNT) : 0u;
            }
            else
            {
                it.shell = true;
                const uint32_t f = w - nchunk * cw, flo = (nlo + kLatNT - 1) / kLatNT;
                it.qs = f < flo ? f * kLatNT : nlo + nmid + (f - flo) * kLatNT;
                it.qn = f < flo ? min(nlo - it.qs, (uint32_t)kLatNT) : min(T.lnshell - it.qs, (uint32_t)kLatNT);
            }
        }
        else
        {
            const uint32_t sb0 = T.lshl ? T.lnwm : 0u, bb0 = T.lshl ? 0u : T.lnsb;
            it.shell = vb >= sb0 && vb < sb0 + T.lnsb;
            if (it.shell)
            {
                it.qs = (vb - sb0) * kLatNT;
                it.qn = it.qs < T.lnshell ? min(T.lnshell - it.qs, (uint32_t)kLatNT) : 0u;
            }
            const uint32_t nw = T.lnwm, bb = it.shell ? 0u : vb - bb0, xcd = bb & 7u;
            const uint32_t w = xcd * (nw >> 3) + min(xcd, nw & 7u) + (bb >> 3);
            it.ib = w % max(T.lnbx, 1u);
            it.jb = (w / max(T.lnbx, 1u)) % max(T.lnby, 1u);
            it.kc = w / cols;
        }
        return it;
    };
    const int nx = (int)T.lnx, ny = (int)T.lny, nz = (int)T.lnz;
    const int ti = (int)(threadIdx.x & (BX - 1)), tj = (int)(threadIdx.x / BX);
    // entry u = 0: the own column (interior position); u = 1: halo-ring entry t (t < NH): the top row, the bottom
    // row, the left column, the right column of the (BX + 2) x (BY + 2) plane
    int epos[2], eii[2], ejj[2];
    bool evalid[2];
    {
        const int t = (int)threadIdx.x;
        eii[0] = ti, ejj[0] = tj;
        if (t < PX)
            eii[1] = t - 1, ejj[1] = -1;
        else if (t < 2 * PX)
            eii[1] = t - PX - 1, ejj[1] = BY;
        else if (t < 2 * PX + BY)
            eii[1] = -1, ejj[1] = t - 2 * PX;
        else
            eii[1] = BX, ejj[1] = t - 2 * PX - BY;
        evalid[0] = true;
        evalid[1] = t < NH;
#pragma unroll
        for (int u = 0; u < 2; ++u)
            epos[u] = (ejj[u] + 1) * PX + eii[u] + 1;
    }
    // diagnostic stamps (the ablation build only): s_memrealtime at the phase boundaries, the item kind, HW_ID
    const auto stamp = [&](int i, uint64_t v) {
        if constexpr (CWF_ABLATION)
        {
            if (fa.trace && threadIdx.x == 0)
                __hip_atomic_store(fa.trace + 16ull * blockIdx.x + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    stamp(0, __builtin_amdgcn_s_memrealtime());
    // the current item's geometry (set by `setup`)
    Item cur = decode(blockIdx.x);
    int kb = 0, ke = 0, gi = 0, gj = 0;
    bool active = false;
    int eoff[2] = {0, 0};
    uint32_t eoff12[2] = {0u, 0u}, gidx12 = 0u;
    const auto setup = [&](const Item &it) {
        const int i0 = 1 + (int)it.ib * BX, j0 = 1 + (int)it.jb * BY;
        kb = (int)T.lkI0 + (int)(it.kc * T.lL);
        ke = min(kb + (int)T.lL, (int)T.lkI1);
        gi = i0 + ti;
        gj = j0 + tj;
        active = gi < nx - 1 && gj < ny - 1;
#pragma unroll
        for (int u = 0; u < 2; ++u)
        {
            eoff[u] = min(j0 + ejj[u], ny - 1) * nx + min(i0 + eii[u], nx - 1);
            eoff12[u] = 12u * (uint32_t)eoff[u];
        }
        gidx12 = 12u * (uint32_t)(gj * nx + gi);
    };
    setup(cur);
    const auto ld3 = [](__amdgpu_buffer_rsrc_t rs, uint32_t byteoff, float v[3]) {
        const u32x3 w = __builtin_amdgcn_raw_buffer_load_b96(rs, byteoff, 0, 0);
        v[0] = __uint_as_float(w.x);
        v[1] = __uint_as_float(w.y);
        v[2] = __uint_as_float(w.z);
    };
    const auto st3 = [](__amdgpu_buffer_rsrc_t rs, uint32_t byteoff, const float v[3]) {
        const u32x3 w = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2])};
        __builtin_amdgcn_raw_buffer_store_b96(w, rs, byteoff, 0, 0);
    };
    constexpr uint32_t kOob12 = 12u * kLatOob3;
    const uint32_t vbytes = 12u * s.N, sbytes = 4u * s.N;
    const __amdgpu_buffer_rsrc_t rr = sized_rsrc(fa.rin, vbytes), ra = sized_rsrc(fa.ain, vbytes),
                                 rp = sized_rsrc(fa.pin, vbytes), rx = sized_rsrc(fa.x, vbytes),
                                 rmass = sized_rsrc(s.mass, sbytes), rcls = sized_rsrc(T.lcls, s.N),
                                 wr = sized_rsrc(fa.rout, vbytes), wp = sized_rsrc(fa.pout, vbytes),
                                 wa = sized_rsrc(fa.aout, vbytes);
    // px (SHARD only): a ghost plane's Ap_(j-1) from the mailbox's receive area (ghost order: node - Nown), and the
    // send planes' rows pushed into the neighbours' (ranges 0 without px: every access past the range)
    const bool gx = SHARD && fa.px && fa.j > 0;
    const __amdgpu_buffer_rsrc_t rg = sized_rsrc(gx ? fa.pe.arecv : nullptr, gx ? 12u * (s.N - s.Nown) : 0u),
                                 rd0 = sized_rsrc(SHARD ? fa.pe.dst[0] : nullptr, SHARD ? fa.pe.dst_bytes[0] : 0u),
                                 rd1 = sized_rsrc(SHARD ? fa.pe.dst[1] : nullptr, SHARD ? fa.pe.dst_bytes[1] : 0u);
    // planes owned by this work item: [kb, ke); the own entry of an active column is an owned node there
    const auto load = [&](int k, FusedFill &f) {
        const uint32_t base = lat_plane<AFF>(T, plane, min(k, nz - 1));
        const bool ownk = k >= kb && k < ke;
#pragma unroll
        for (int u = 0; u < 2; ++u)
        {
            const bool go = evalid[u] && k <= ke;
            const uint32_t n = base + (uint32_t)eoff[u], nb = go ? 12u * base + eoff12[u] : kOob12;
            ld3(rr, nb, f.r[u]);
            if constexpr (SHARD)
            {
                const bool gpl = gx && base >= s.Nown;  // workgroup-uniform: a ghost plane
                ld3(gpl ? rg : ra, gpl ? (go ? 12u * (base - s.Nown) + eoff12[u] : kOob12) : nb, f.a[u]);
            }
            else
                ld3(ra, nb, f.a[u]);
            ld3(rp, nb, f.p[u]);
            f.c[u] = __builtin_amdgcn_raw_buffer_load_b8(rcls, go ? n : 0xFFFFFFFFu, 0, 0);
            if (u == 0)
            {
                const bool own = ownk && active && n < s.Nown;
                ld3(rx, own ? nb : kOob12, f.x);
                if constexpr (MU)
                    f.m = 0.f;
                else
                    f.m = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rmass, 4u * (own ? n : kLatOob1), 0, 0));
            }
        }
    };
    // DEEP (the 27-point hex stencil): planes in flight two steps ahead, FA / FB and FC / FD alternating (the step
    // at k forms k + 1, k + 2 from one pair and reloads it with k + 5, k + 6; 240 VGPRs, still 2 waves per SIMD):
    // C2 hex8 +8%. The Kuhn rows are short enough that their steps do not wait on the loads, and the two extra
    // planes issued before the prologue's share fold delay it: C2 -4.8% (profiles/ab_history.md r05n)
    constexpr bool DEEP = E::nOff > kLatOffsets;
    FusedFill P0, P1, FA, FB, FC, FD;
    const auto prologue_loads = [&]() {
        load(kb - 1, P0);
        load(kb, P1);
        load(kb + 1, FA);
        load(kb + 2, FB);
        if constexpr (DEEP)
        {
            load(kb + 3, FC);
            load(kb + 4, FD);
        }
    };
    if constexpr (SHARD)  // px: every peer's previous launch first (the ghost Ap rows the prologue loads)
    {
        if (fa.px && !fused_peer_wait(fa.pe, fa.j, fa.ctl))
            return;
    }
    if (!cur.shell)
        prologue_loads();
    // the class table (thread c: class c), in flight with the planes and the scalar fold
    const uint32_t cthr = min((uint32_t)threadIdx.x, kLatClasses - 1u);
    const float4 zA = T.lcz[2u * cthr], zB = T.lcz[2u * cthr + 1u];
    float alpha = 0.f, beta = 0.f;
    {
        const CtlPre pre = ctl_prefetch(fa.ctl, max(fa.j, 1u));
        if (!fused_scalars<kLatNT>(fa, pre, red, &alpha, &beta))
            return;
    }
    stamp(1, __builtin_amdgcn_s_memrealtime());
    if (threadIdx.x < kLatClasses)
    {
        czA[threadIdx.x] = zA;
        czB[threadIdx.x] = float2{zB.x, zB.y};
    }
    __syncthreads();
    double d[kFusedShares] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // form a plane into ring slot `slot`: every entry's p_j to LDS; the own (owned) entry's r_j, p_j, x_j stores and
    // dots, and what its row needs later into `keep`
    const auto write = [&](int k, int slot, const FusedFill &f, FusedKeep &keep) {
        float4 *dst = pl[slot];
        const uint32_t base = lat_plane<AFF>(T, plane, min(k, nz - 1));
        const bool ownk = k >= kb && k < ke;
#pragma unroll
        for (int u = 0; u < 2; ++u)
        {
            float rn[3], z[3], pn[3];
            fused_form(czA, czB, f.c[u], alpha, beta, f.r[u], f.a[u], f.p[u], rn, z, pn);
            if (evalid[u])
                dst[epos[u]] = float4{pn[0], pn[1], pn[2], 0.f};
            if constexpr (SHARD)
            {
                // a ghost plane (every node of it a ghost, stored after the owned ones): its r_j and p_j are formed
                // here exactly as the owner forms them (the same r_(j-1), Ap_(j-1) -- received --, p_(j-1), global
                // class and scalars), so they are stored for the next launch and only Ap crosses ranks; entries in
                // several bricks' halos are stored by each, with the same bits
                const bool gh = evalid[u] && base >= s.Nown && k <= ke;
                const uint32_t gb = gh ? 12u * base + eoff12[u] : kOob12;
                st3(wr, gb, rn);
                st3(wp, gb, pn);
            }
            if (u == 0)
            {
                const uint32_t n = base + (uint32_t)eoff[0];
                const bool own = ownk && active && n < s.Nown;
                const uint32_t ob = own ? 12u * base + eoff12[0] : kOob12;
                float xn[3];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    xn[c] = fmaf(alpha, f.p[0][c], f.x[c]);
                st3(wr, ob, rn);
                st3(wp, ob, pn);
                st3(rx, ob, xn);
                if (own)
                    fused_entry_dots(rn, z, d);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    keep.z[c] = z[c];
                keep.c = f.c[0];
                keep.m = f.m;
            }
        }
    };
    const float sK = (float)s.sK, sM = (float)s.sM;
    const int c0 = (tj + 1) * PX + ti + 1;
    const auto rows1 = [&](int k, int sm, int s0c, int sp, bool last, const FusedKeep &keep) {
        int zoff;
        asm volatile("s_mov_b32 %0, 0" : "=s"(zoff));
        const float *__restrict__ cf = coef + zoff;
        const float4 q0 = pl[s0c][c0];
        const float u0[3] = {q0.x, q0.y, q0.z};
        const f2 u0xy = {q0.x, q0.y};
        f2 acc01 = {0.f, 0.f};
        float acc2 = 0.f;
#pragma unroll
        for (int o = 1; o < E::nOff; o += (SYM ? 2 : 1))
        {
            f2 wxy;
            float wz;
            const auto dv = [&](int oo, f2 &dxy, float &dz3) {
                const int dz = E::off[oo][2];
                const float4 q = pl[dz < 0 ? sm : dz > 0 ? sp : s0c][c0 + E::off[oo][1] * PX + E::off[oo][0]];
                dxy = f2{q.x, q.y} - u0xy;
                dz3 = q.z - u0[2];
            };
            dv(o, wxy, wz);
            if constexpr (SYM)
            {
                f2 vxy;
                float vz;
                dv(o + 1, vxy, vz);
                wxy += vxy;
                wz += vz;
            }
            const float *b = cf + 9 * o;
            acc01 = __builtin_elementwise_fma(f2{b[0], b[1]}, f2{wxy.x, wxy.x}, acc01);
            acc01 = __builtin_elementwise_fma(f2{b[2], b[3]}, f2{wxy.y, wxy.y}, acc01);
            acc01 = __builtin_elementwise_fma(f2{b[4], b[5]}, f2{wz, wz}, acc01);
            acc2 = fmaf(b[6], wxy.x, acc2);
            acc2 = fmaf(b[7], wxy.y, acc2);
            acc2 = fmaf(b[8], wz, acc2);
        }
        const float acc[3] = {acc01.x, acc01.y, acc2};
        const float m = (MU ? T.lmass : keep.m) * sM;
        float a[3];
#pragma unroll
        for (int r3 = 0; r3 < 3; ++r3)
            a[r3] = fmaf(m, u0[r3], sK * acc[r3]);
        const uint32_t pb = lat_plane<AFF>(T, plane, min(k, nz - 1)), n = pb + (uint32_t)(gj * nx + gi);
        const bool mine = active && !last && n < s.Nown;
        st3(wa, mine ? 12u * pb + gidx12 : kOob12, a);
        if constexpr (SHARD)
        {
            const uint32_t io = 12u * (uint32_t)(gj * nx + gi);
            st3_sys(rd0, mine && k == fa.pe.send_k[0] ? io : kOob12, a);
            st3_sys(rd1, mine && k == fa.pe.send_k[1] ? io : kOob12, a);
        }
        if (mine)
            fused_row_dots(czA, czB, keep.c, u0, keep.z, a, d);
    };
    // step at plane k = kb + 2 m: forms planes k + 1, k + 2 (slots, keeps by relative index), rows k and k + 1
    FusedKeep K0, K1, K2, Kx;  // planes kb + 3 m + {0, 1, 2} (relative index mod 3); Kx: the halo plane kb - 1
    const auto step = [&](int k, int s0, int s1, int s2, int s3, FusedKeep &ka, FusedKeep &kb1, FusedKeep &kb2,
                          FusedFill &W0, FusedFill &W1) {
        // diagnostic stamps of the first step (ablation build): its phases 8 .. 13
        const bool st1 = CWF_ABLATION && k == kb;
        write(k + 1, s2, W0, kb1);
        if (st1)
            stamp(8, __builtin_amdgcn_s_memrealtime());
        write(k + 2, s3, W1, kb2);
        if (st1)
            stamp(9, __builtin_amdgcn_s_memrealtime());
        __syncthreads();
        if (st1)
            stamp(10, __builtin_amdgcn_s_memrealtime());
        load(k + (DEEP ? 5 : 3), W0);
        load(k + (DEEP ? 6 : 4), W1);
        if (st1)
            stamp(11, __builtin_amdgcn_s_memrealtime());
        rows1(k, s0, s1, s2, false, ka);
        if (st1)
            stamp(12, __builtin_amdgcn_s_memrealtime());
        rows1(k + 1, s1, s2, s3, k + 1 >= ke, kb1);
        if (st1)
            stamp(13, __builtin_amdgcn_s_memrealtime());
    };
    for (uint32_t vb = blockIdx.x;;)
    {
        if (cur.shell)
        {
            if (threadIdx.x < cur.qn)
                fused_shell_node<E, AFF, SHARD>(s, fa, coef, plane, cur.qs + threadIdx.x, alpha, beta, czA, czB, d);
        }
        else
        {
            write(kb - 1, 0, P0, Kx);
            write(kb, 1, P1, K0);
            stamp(2, __builtin_amdgcn_s_memrealtime());
            // period 6 steps: the LDS ring's 3 (six slots) times the fill pairs' 2
            for (int k = kb; k < ke; k += 12)
            {
                step(k, 0, 1, 2, 3, K0, K1, K2, FA, FB);
                if (k + 2 < ke)
                    step(k + 2, 2, 3, 4, 5, K2, K0, K1, DEEP ? FC : FA, DEEP ? FD : FB);
                if (k + 4 < ke)
                    step(k + 4, 4, 5, 0, 1, K1, K2, K0, FA, FB);
                if (k + 6 < ke)
                    step(k + 6, 0, 1, 2, 3, K0, K1, K2, DEEP ? FC : FA, DEEP ? FD : FB);
                if (k + 8 < ke)
                    step(k + 8, 2, 3, 4, 5, K2, K0, K1, FA, FB);
                if (k + 10 < ke)
                    step(k + 10, 4, 5, 0, 1, K1, K2, K0, DEEP ? FC : FA, DEEP ? FD : FB);
            }
        }
        if constexpr (!PERSIST)  // one work item per workgroup (the grid covers them): no loop-carried state
            break;
        vb += gridDim.x;
        if (vb >= T.lnwork)
            break;
        cur = decode(vb);
        setup(cur);
        __syncthreads();  // the ring is refilled by the next item
        if (!cur.shell)
            prologue_loads();
    }
    stamp(3, __builtin_amdgcn_s_memrealtime());
    block_sum_k<kLatNT, kFusedShares>(d, red);
    if constexpr (CWF_ABLATION)
    {
        stamp(5, (uint64_t)cur.shell | ((uint64_t)(ke - kb) << 8));
        stamp(6, (uint64_t)__builtin_amdgcn_s_getreg(4 | (31 << 11)));   // HW_ID
        stamp(7, (uint64_t)__builtin_amdgcn_s_getreg(20 | (31 << 11)));  // XCC_ID
    }
    if (threadIdx.x < kFusedShares)
    {
        double v = d[0];
#pragma unroll
        for (int q = 1; q < kFusedShares; ++q)
            v = threadIdx.x == (unsigned)q ? d[q] : v;
        double *o = fa.sout + (size_t)threadIdx.x * fa.sstride + blockIdx.x;
        if (SHARD && fa.px)  // write-through: the launch's last workgroup (any XCD) folds them
            __hip_atomic_store(o, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else
            *o = v;
    }
    stamp(4, __builtin_amdgcn_s_memrealtime());
    if constexpr (SHARD)
    {
        if (fa.px)
            fused_peer_publish<kLatNT>(fa, red);
    }
}

// the end of a batch of fused launches: launch j's shares -> the convergence of r_j (idempotent with launch j + 1's
// start, which repeats it)
__global__ __launch_bounds__(256) void k_fused_check(FusedArgs fa)
{
    __shared__ double red[kFusedShares * 4];
    if (fa.px && !fused_peer_wait(fa.pe, fa.j, fa.ctl))  // px: the peers' totals of launch j - 1 first
        return;
    const CtlPre pre = ctl_prefetch(fa.ctl, max(fa.j, 1u));
    float alpha, beta;
    (void)fused_scalars<256>(fa, pre, red, &alpha, &beta);
}

// a shard's rank totals of its launch's shares, in the fold order every consumer of them uses (fold_k, 256 threads;
// the PEER step folds them itself, the same way): out[q], q < kFusedShares
__global__ __launch_bounds__(256) void k_fused_rank_totals(const double *__restrict__ sh, unsigned n, unsigned stride,
                                                           double *__restrict__ out)
{
    __shared__ double red[kFusedShares * 4];
    double v[kFusedShares];
    fold_k<256, kFusedShares>(sh, n, stride, red, v);
    if (threadIdx.x < kFusedShares)
    {
        double t = v[0];
#pragma unroll
        for (int q = 1; q < kFusedShares; ++q)
            t = threadIdx.x == (unsigned)q ? v[q] : t;
        out[threadIdx.x] = t;
    }
}

// the final residual vector (the solve's r output): r_n is in {r2, r}[n & 1]; r1 = r2, r0 = r
__global__ __launch_bounds__(256) void k_fused_finish(const Ctl *__restrict__ ctl, const float *__restrict__ r1,
                                                      float *__restrict__ r0, uint32_t D)
{
    if (ctl->iterations == 0ull || (ctl->iterations & 1ull) != 0ull)  // r_n in r2 for even n > 0
        return;
    for (uint32_t d = blockIdx.x * 256u + threadIdx.x; d < D; d += gridDim.x * 256u)
        r0[d] = r1[d];
}

using FusedFn = void (*)(DevSys, FusedArgs, const float *, const uint32_t *);

template <bool SYM, class E, bool MU, bool AFF, bool SHARD, bool PERSIST> Pick<FusedFn> pcg_lattice_pick()
{
    static const std::string name = kernel_name("k_pcg_lattice", SYM, lat_kind<E>(), MU, AFF, SHARD, PERSIST);
    return {k_pcg_lattice<SYM, E, MU, AFF, SHARD, PERSIST>, name.c_str()};
}

// a shard (the plane table, never affine): ghost planes store their r_j / p_j; persist (a grid below the work items)
// walks them persistently
Pick<FusedFn> pick_pcg_lattice(const DevSys &s, bool persist)
{
    return with_bools(
        [](auto sym, auto hex, auto mu, auto aff, auto shard, auto per) {
            return pcg_lattice_pick<sym(), LatE<hex()>, mu(), aff(), !aff() && shard(), per()>();
        },
        s.t.lsym != 0, s.t.lhex != 0, s.t.lmu != 0, s.t.lpstride != 0, s.Nown < s.N, persist);
}

// resident workgroups of the one-item instantiation (168-170 VGPRs: 3 per CU) or of the persistent one (234-248
// VGPRs: 2 per CU)
unsigned lattice_resident_count(const DevSys &s, bool persist = false)
{
    return resident_blocks(pick_pcg_lattice(s, persist).fn, kLatNT, 0);
}

// the fused launch's grid: every work item when they fit in one round of resident workgroups of the one-item
// instantiation, else one round of the persistent one (a multiple of 8, so an item keeps its XCD) walking the items;
// at most `cap`
unsigned pcg_lattice_grid(const DevSys &s, unsigned cap)
{
    if (s.t.lnwork <= std::min(lattice_resident_count(s), cap))
        return std::max(s.t.lnwork, 1u);
    // never above the items: a grid past lnwork would decode items that do not exist and store their shares past
    // the W = lnwork columns of fsh (a cap below 8 with fewer than 8 items)
    const unsigned lim = std::min(lattice_resident_count(s, true), cap);
    return std::min(std::max(lim - lim % 8u, 8u), std::max(s.t.lnwork, 1u));
}

void launch_pcg_lattice(const DevSys &s, const FusedArgs &fa, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    launch_kernel(pick_pcg_lattice(s, fa.grid < s.t.lnwork).fn, fa.grid, kLatNT, 0, st, e0, e1, s, fa, s.t.lcoef,
                  s.t.lplane);
}
}  // namespace

// ---- the host driver ----------------------------------------------------------------------------------------
unsigned pcg_lattice_resident_count(const DevSys &s) { return lattice_resident_count(s); }

unsigned pcg_lattice_launch_grid(const DevSys &s, unsigned cap) { return pcg_lattice_grid(s, cap); }

const char *pcg_lattice_kernel_name(const DevSys &s, unsigned grid) { return pick_pcg_lattice(s, grid < s.t.lnwork).name; }

namespace
{
#if CWF_ABLATION
// diagnostic (ablation build): CWF_FUSED_TRACE=path appends the stamps of one launch (CWF_FUSED_TRACE_IT, default
// 50) of every solve: one line per workgroup "wg kind|planes<<8 hw_id xcc_id t0 t1 t2 t3 t4" (s_memrealtime, 100 MHz)
uint64_t *g_ftrace = nullptr;
unsigned g_ftrace_n = 0;
uint64_t *fused_trace_buffer(const cwf_hip_system *h)
{
    if (!knob("CWF_FUSED_TRACE"))
        return nullptr;
    if (g_ftrace_n < h->sched.grid)
    {
        if (g_ftrace)
            (void)hipFree(g_ftrace);
        g_ftrace = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&g_ftrace), 128ull * h->sched.grid) != hipSuccess)
            return nullptr;
        g_ftrace_n = h->sched.grid;
    }
    return g_ftrace;
}
void fused_trace_dump(cwf_hip_system *h, unsigned it, hipStream_t st)
{
    const char *path = knob("CWF_FUSED_TRACE"), *at = knob("CWF_FUSED_TRACE_IT");
    if (!path || !g_ftrace || it != (unsigned)(at ? atoi(at) : 50))
        return;
    std::vector<uint64_t> v(16ull * h->sched.grid);
    if (hipStreamSynchronize(st) != hipSuccess ||
        hipMemcpy(v.data(), g_ftrace, v.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
        return;
    if (FILE *f = std::fopen(path, "a"))
    {
        std::fprintf(f, "# launch %u grid %u\n", it + 1u, h->sched.grid);
        for (unsigned b = 0; b < h->sched.grid; ++b)
        {
            const uint64_t *w = &v[16ull * b];
            std::fprintf(f, "%u %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", b,
                         (unsigned long long)w[5], (unsigned long long)w[6], (unsigned long long)w[7],
                         (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2],
                         (unsigned long long)w[3], (unsigned long long)w[4], (unsigned long long)w[8],
                         (unsigned long long)w[9], (unsigned long long)w[10], (unsigned long long)w[11],
                         (unsigned long long)w[12], (unsigned long long)w[13]);
        }
        std::fclose(f);
    }
}
#endif
// launch j of the fused iteration: r_j -> {r2, r}[j & 1], Ap_j -> {Ap, ap2}[j & 1], p_j -> p[(j + 1) % 4], shares
// -> fsh[j & 1]; launch j reads launch j - 1's (launch 0 reads r from r and Ap from ap2, zeroed at init)
FusedArgs fused_args(cwf_hip_system *h, unsigned j)
{
    const unsigned W = h->ds.t.lnwork;
    float *const R[2] = {h->r2, h->r}, *const A[2] = {h->Ap, h->ap2};
    FusedArgs fa{};
    fa.ctl = h->ctl;
    fa.sstride = W;
    fa.grid = h->sched.grid;
    if (h->sharded())  // every rank folds the all-gathered rank totals, in rank order
    {
        fa.sin = h->g_fsh;
        if (h->sched.launch == PcgSchedule::FusedPeer)  // PEER in-kernel: the totals land in the mailbox's gather area (previous epoch)
        {
            const double *gp = nullptr;
            peer_fused_args(h, j, fa.pe, &gp);
            fa.px = 1;
            fa.sin = gp;
        }
        fa.nin = (unsigned)h->nranks;
        fa.sin_stride = 1;
        fa.sis = kFusedSlot;
    }
    else
    {
        fa.sin = h->fsh + (size_t)((j + 1u) & 1u) * 5 * W;
        fa.nin = h->sched.grid;
        fa.sin_stride = W;
        fa.sis = 1;
    }
    fa.sout = h->fsh + (size_t)(j & 1u) * 5 * W;
    fa.j = j;
    fa.hist = h->hist;
    fa.rin = R[(j + 1u) & 1u];
    fa.rout = R[j & 1u];
    fa.ain = A[(j + 1u) & 1u];
    fa.aout = A[j & 1u];
    fa.pin = fast_p_buf(h, j);
    fa.pout = fast_p_buf(h, j + 1u);
    fa.x = h->x;
    fa.trace = nullptr;
#if CWF_ABLATION
    fa.trace = fused_trace_buffer(h);
#endif
    return fa;
}
}  // namespace

void fast_fused_init(cwf_hip_system *h, const float *rhs, double rel_tol, hipStream_t st, bool launch0)
{
    const DevSys &s = h->ds;
    const uint32_t nbD = fast_dot_blocks(s.D);
    fast_block_inverse(h, st);
    fast_keff(h, h->x, h->Ap, true, nullptr, nullptr, st);
    launch_init_residual(h, rhs, st);  // r_0 = rhs - A x (Dirichlet: x = rhs, r = 0) into h->r
    fast_dot(rhs, rhs, nullptr, s.D, h->part0, nullptr, st);
    fast_dot(h->r, h->r, nullptr, s.D, h->part1, nullptr, st);
    fast_init_scalars_strided(h, h->part0, h->part1, nbD, 1u, rel_tol, st);
    // launch 0 reads p_(-1) and Ap_(-1) (times beta = alpha = 0): zero, so no stale non-finite value enters
    if (launch0)  // (the resident solve runs its phase 0 itself)
        fast_fused_launch0(h, st);
}

void fast_fused_iteration(cwf_hip_system *h, unsigned it, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    launch_pcg_lattice(h->ds, fused_args(h, it + 1u), st, e0, e1);
#if CWF_ABLATION
    fused_trace_dump(h, it, st);
#endif
}

void fast_fused_launch0(cwf_hip_system *h, hipStream_t st)
{
    (void)hipMemsetAsync(h->p, 0, sizeof(float) * h->ds.D, st);
    (void)hipMemsetAsync(h->ap2, 0, sizeof(float) * h->ds.D, st);
    launch_pcg_lattice(h->ds, fused_args(h, 0), st, nullptr, nullptr);
}

// a shard's ghost class bytes from their owners (once per handle, before its first fused solve): the owned classes
// as floats in tmp's x components, a halo, and the ghosts' back into lcls (a ghost's local class is a boundary type
// of the shard's sub-lattice; its owner's is the node's class in the whole block, the one its z_j is formed with)
__global__ __launch_bounds__(256) void k_cls_out(const uint8_t *__restrict__ cls, uint32_t n, float *__restrict__ t)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
        t[3u * i] = (float)cls[i];
}
__global__ __launch_bounds__(256) void k_cls_in(const float *__restrict__ t, uint32_t n0, uint32_t n1,
                                                uint8_t *__restrict__ cls)
{
    for (uint32_t i = n0 + blockIdx.x * 256u + threadIdx.x; i < n1; i += gridDim.x * 256u)
        cls[i] = (uint8_t)t[3u * i];
}
void fast_fused_cls_out(cwf_hip_system *h, hipStream_t st)
{
    if (h->ds.Nown)
        k_cls_out<<<std::min<unsigned>(grid_for(h->ds.Nown, 256), 1024u), 256, 0, st>>>(h->ds.t.lcls, h->ds.Nown, h->tmp);
}
void fast_fused_cls_in(cwf_hip_system *h, hipStream_t st)
{
    if (h->ds.N > h->ds.Nown)
        k_cls_in<<<std::min<unsigned>(grid_for(h->ds.N - h->ds.Nown, 256), 1024u), 256, 0, st>>>(
            h->tmp, h->ds.Nown, h->ds.N, const_cast<uint8_t *>(h->ds.t.lcls));
}

// a shard's launch j: its Ap_j (the vector the exchange after it carries) and its rank totals into g_fsh[rank]
float *fast_fused_ap(cwf_hip_system *h, unsigned j) { return (j & 1u) ? h->ap2 : h->Ap; }
void fast_fused_rank_totals(cwf_hip_system *h, unsigned j, hipStream_t st)
{
    const unsigned W = h->ds.t.lnwork;
    k_fused_rank_totals<<<1, 256, 0, st>>>(h->fsh + (size_t)(j & 1u) * 5 * W, h->sched.grid, W,
                                           h->g_fsh + (size_t)kFusedSlot * h->rank);
}
const double *fast_fused_shares(const cwf_hip_system *h, unsigned j, unsigned *stride, unsigned *count)
{
    *stride = h->ds.t.lnwork;
    *count = h->sched.grid;
    return h->fsh + (size_t)(j & 1u) * 5 * h->ds.t.lnwork;
}

// the convergence of the batch's last launch (it iterations enqueued: launch it's r); last: it is the solve's
// max_iterations, so no launch follows
void fast_fused_check(cwf_hip_system *h, unsigned it, hipStream_t st, bool last)
{
    FusedArgs fa = fused_args(h, it + 1u);
    fa.last = last ? 1u : 0u;
    k_fused_check<<<1, 256, 0, st>>>(fa);
}

void fast_fused_finish(cwf_hip_system *h, hipStream_t st)
{
    const uint32_t D = h->ds.D;
    if (D)
        k_fused_finish<<<std::min<unsigned>(grid_for(D, 256), 1024u), 256, 0, st>>>(h->ctl, h->r2, h->r, D);
}
}  // namespace cwf
