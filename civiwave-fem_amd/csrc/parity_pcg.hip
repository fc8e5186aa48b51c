// parity_pcg.hip -- the bit-exact PCG (pcg.cpp:744-915): the ordered reductions and the scalar kernels, the node-wise
// vector passes, and the driver that runs them for a single handle or a shard group. The reductions and the passes
// are one unit because the streamed passes (k_dot_alpha_stream, k_update<true>) fold the partials themselves, with
// the fold code of the scalar kernels. The rounding contract: parity_common.hpp.
#include "knobs.hpp"
#include "parity_common.hpp"

#include <algorithm>

namespace cwf
{
namespace
{

// ---- reductions (pcg.cpp:170-207): sequential fp64 fold inside each reduction_block chunk ----

// generic chunk size: one thread per chunk, sequential loads
template <int NV>
__global__ __launch_bounds__(kBlock) void k_dot_chunks_generic(const float *__restrict__ a,
                                                               const float *__restrict__ b,
                                                               const float *__restrict__ c, uint32_t D,
                                                               uint32_t B, uint32_t chunks, double *__restrict__ pab,
                                                               double *__restrict__ pac, const Ctl *__restrict__ ctl)
{
    if (ctl && !ctl->active)
        return;
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= chunks)
        return;
    const uint32_t beg = k * B, end = min(beg + B, D);
    double s0 = 0.0, s1 = 0.0;
    for (uint32_t i = beg; i < end; ++i)
    {
        const double av = (double)a[i];
        s0 += av * (double)b[i];
        if constexpr (NV == 2)
            s1 += av * (double)c[i];
    }
    pab[k] = s0;
    if constexpr (NV == 2)
        pac[k] = s1;
}

// chunk = 256 DOFs: a 256-thread workgroup per 32 chunks. The workgroup stages the 32 x 256 values of every
// operand through LDS with coalesced loads (rows padded to 257 floats, so the 32 folding lanes hit 32 different
// banks), then lane c of wave 0 folds chunk c sequentially, in DOF order (pcg.cpp:189-199); the fp32 x fp32
// products are exact in fp64. Values past D are staged as 0: +0.0 * +0.0 added to a fold that started at +0.0 is
// exact (such a fold is never -0.0), so the tail chunk equals the reference's shorter loop.
constexpr int kDotChunksPerBlock = 32;
constexpr int kDotRow = 257;
// (CPB chunks per block; no early return, so a persistent caller can loop over blocks with a barrier in between)
template <int NV, int CPB = kDotChunksPerBlock>
__device__ __forceinline__ void dot_chunks256(const float *__restrict__ a, const float *__restrict__ b,
                                              const float *__restrict__ c, uint32_t D, uint32_t chunks,
                                              double *__restrict__ pab, double *__restrict__ pac, uint32_t bx,
                                              const double *gran, uint32_t tag)
{
    __shared__ float sa[CPB * kDotRow];
    __shared__ float sb[CPB * kDotRow];
    __shared__ float sc[NV == 2 ? CPB * kDotRow : 1];
    const uint64_t base = (uint64_t)bx * CPB * 256u;
    // 16-B loads (4 DOFs per lane and step) when the operands are 16-B aligned (a caller's device pointer need
    // not be); a block's range starts 32 KB into the vector, the tail past D goes scalar
    const bool al = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
                      reinterpret_cast<uintptr_t>(NV == 2 ? c : a)) & 15u) == 0;
    for (uint32_t i = 4u * threadIdx.x; i < CPB * 256u; i += 1024u)
    {
        const uint64_t gi = base + i;
        const uint32_t l = (i >> 8) * kDotRow + (i & 255u);  // 4 consecutive DOFs stay in one row
        if (al && gi + 4u <= D)
        {
            const float4 va = *reinterpret_cast<const float4 *>(a + gi);
            const float4 vb = *reinterpret_cast<const float4 *>(b + gi);
            sa[l] = va.x, sa[l + 1] = va.y, sa[l + 2] = va.z, sa[l + 3] = va.w;
            sb[l] = vb.x, sb[l + 1] = vb.y, sb[l + 2] = vb.z, sb[l + 3] = vb.w;
            if constexpr (NV == 2)
            {
                const float4 vc = *reinterpret_cast<const float4 *>(c + gi);
                sc[l] = vc.x, sc[l + 1] = vc.y, sc[l + 2] = vc.z, sc[l + 3] = vc.w;
            }
        }
        else
            for (uint32_t u = 0; u < 4u; ++u)
            {
                const bool ok = gi + u < D;
                sa[l + u] = ok ? a[gi + u] : 0.0f;
                sb[l + u] = ok ? b[gi + u] : 0.0f;
                if constexpr (NV == 2)
                    sc[l + u] = ok ? c[gi + u] : 0.0f;
            }
    }
    __syncthreads();
    const uint32_t k = bx * CPB + threadIdx.x;
    if (threadIdx.x >= (uint32_t)CPB || k >= chunks)
        return;
    const float *ra = sa + threadIdx.x * kDotRow, *rb = sb + threadIdx.x * kDotRow;
    const float *rc = sc + (NV == 2 ? threadIdx.x * kDotRow : 0u);
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 16
    for (uint32_t i = 0; i < 256u; ++i)
    {
        const double av = (double)ra[i];
        s0 += av * (double)rb[i];
        if constexpr (NV == 2)
            s1 += av * (double)rc[i];
    }
    if (gran)
    {
        const __amdgpu_buffer_rsrc_t rs = gran_rsrc(gran);
        gran_store(rs, NV * k, s0, tag);
        if constexpr (NV == 2)
            gran_store(rs, NV * k + 1u, s1, tag);
    }
    else
    {
        pab[k] = s0;
        if constexpr (NV == 2)
            pac[k] = s1;
    }
}

template <int NV>
__global__ __launch_bounds__(256) void k_dot_chunks256(const float *__restrict__ a, const float *__restrict__ b,
                                                       const float *__restrict__ c, uint32_t D, uint32_t chunks,
                                                       double *__restrict__ pab, double *__restrict__ pac,
                                                       const Ctl *__restrict__ ctl)
{
    if (ctl && !ctl->active)
        return;
    dot_chunks256<NV>(a, b, c, D, chunks, pab, pac, blockIdx.x, nullptr, 0u);
}

// The ordered chain over one block of NB partials in LDS, fully unrolled with scheduling barriers. A loop of two
// alternating register sets is rotated by LLVM so that both sets load at the top of each trip: every 32 adds then
// wait a full LDS round trip (C2's 4,020-partial folds took 28-30 us in the streamed kernels, ~6 ns per add). Here
// the next set's eight 16-B reads are pinned in front of the current set's 16 dependent adds.
template <uint32_t NB, uint32_t H = 8>  // H: double2 per register set (2 sets: 4 H VGPRs)
__device__ __forceinline__ void fold_block(const double2 *v, double &acc)
{
    double2 A[H], B[H];
#pragma unroll
    for (uint32_t u = 0; u < H; ++u)
        A[u] = v[u];
#pragma unroll
    for (uint32_t i = 0; i < NB / 2u; i += 2u * H)
    {
#pragma unroll
        for (uint32_t u = 0; u < H; ++u)
            B[u] = v[i + H + u];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (uint32_t u = 0; u < H; ++u)
        {
            acc += A[u].x;
            acc += A[u].y;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (i + 2u * H < NB / 2u)
        {
#pragma unroll
            for (uint32_t u = 0; u < H; ++u)
                A[u] = v[i + 2u * H + u];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (uint32_t u = 0; u < H; ++u)
        {
            acc += B[u].x;
            acc += B[u].y;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

constexpr int kFoldThreads = 256;
constexpr uint32_t kFoldBlock = 4096;  // partials per staged block and operand (one block: C2's 4,030 chunks)
constexpr uint32_t kFoldSub = 256;     // partials per fold_block (a staged block is padded with +0.0 to a multiple)
template <int NC>
__device__ void fold_seq(const double *__restrict__ p0, const double *__restrict__ p1, uint32_t count, double &t0,
                         double &t1)
{
    // a staged block is padded with +0.0 to a multiple of kFoldSub (a sequential sum from +0.0 is never -0.0, so
    // adding +0.0 is exact) and folded by fold_block, branch-free. Two operands (NC = 2) are two independent chains,
    // run by thread 0 (operand 0) and thread 64 (operand 1) in different waves: interleaved in one thread they
    // measured no faster than back to back (C2 beta 39 us; a ping-pong of both 42-45).
    constexpr uint32_t W = 16, kRow = kFoldBlock + W;
    constexpr uint32_t kStage = NC == 2 ? 128u : 64u;  // the first thread of the staging waves
    __shared__ double2 buf[2][NC][kRow / 2];
    __shared__ double other;
    const uint32_t nb = (count + kFoldBlock - 1u) / kFoldBlock;
    const auto stage = [&](uint32_t blk, uint32_t first, uint32_t step) {
        const uint32_t b0 = blk * kFoldBlock, n = min(kFoldBlock, count - b0);
        const uint32_t npad = (n + kFoldSub - 1u) / kFoldSub * kFoldSub;
        double *d0 = reinterpret_cast<double *>(buf[blk & 1u][0]);
        double *d1 = reinterpret_cast<double *>(buf[blk & 1u][NC - 1]);
        for (uint32_t i = first; i < npad; i += step)
        {
            d0[i] = i < n ? p0[b0 + i] : 0.0;
            if constexpr (NC == 2)
                d1[i] = i < n ? p1[b0 + i] : 0.0;
        }
    };
    // whole kFoldSub-partial sub-blocks through fold_block (its next reads pinned ahead of the adds)
    const auto chain = [](const double2 *v, uint32_t npad, double &acc) {
        for (uint32_t i = 0; i < npad; i += kFoldSub)
            fold_block<kFoldSub>(v + i / 2u, acc);
    };
    double acc = 0.0;
    if (nb)
        stage(0, threadIdx.x, kFoldThreads);
    __syncthreads();
    for (uint32_t blk = 0; blk < nb; ++blk)
    {
        const uint32_t n = min(kFoldBlock, count - blk * kFoldBlock);
        const uint32_t npad = (n + kFoldSub - 1u) / kFoldSub * kFoldSub;
        if (threadIdx.x >= kStage)  // the staging waves; the folding threads' waves do nothing else
        {
            if (blk + 1u < nb)
                stage(blk + 1u, threadIdx.x - kStage, kFoldThreads - kStage);
        }
        else if (threadIdx.x == 0)
            chain(buf[blk & 1u][0], npad, acc);
        else if (NC == 2 && threadIdx.x == 64)
            chain(buf[blk & 1u][NC - 1], npad, acc);
        __syncthreads();
    }
    if (NC == 2 && threadIdx.x == 64)
        other = acc;
    __syncthreads();
    t0 = acc;
    t1 = NC == 2 ? other : 0.0;
}

__global__ __launch_bounds__(kFoldThreads) void k_fold1(const double *__restrict__ p, uint32_t count,
                                                        double *__restrict__ out)
{
    double t0, t1;
    fold_seq<1>(p, nullptr, count, t0, t1);
    if (threadIdx.x == 0)
        out[0] = t0;
}

// ---- PCG scalar phases (one workgroup; thread 0 decides), pcg.cpp:768-895 ----

__global__ __launch_bounds__(kFoldThreads) void k_pcg_init_scalars(Ctl *ctl, const double *__restrict__ p_rhs,
                                                                   const double *__restrict__ p_rr, uint32_t count,
                                                                   double rel_tol, double *__restrict__ hist)
{
    double rhs_sq, rr;
    fold_seq<2>(p_rhs, p_rr, count, rhs_sq, rr);
    if (threadIdx.x)
        return;
    double rhs_norm = sqrt(rhs_sq);
    if (rhs_norm < 1.0e-12)
        rhs_norm = 1.0;
    const double res = sqrt(rr);
    Ctl c{};
    c.res = res;
    c.rhs_norm = rhs_norm;
    c.rhs_norm_raw = sqrt(rhs_sq);
    c.tol = rel_tol * rhs_norm;
    c.iterations = 0;
    c.converged = res <= c.tol ? 1 : 0;
    c.active = c.converged ? 0 : 1;
    c.error = 0;
    c.error_iter = 0;
    hist[0] = res;
    *ctl = c;
}

__global__ __launch_bounds__(kFoldThreads) void k_pcg_init_rho(Ctl *ctl, const double *__restrict__ p_rz,
                                                               uint32_t count)
{
    if (!ctl->active)
        return;
    double rho, unused;
    fold_seq<1>(p_rz, nullptr, count, rho, unused);
    if (threadIdx.x)
        return;
    ctl->rho = rho;
    if (fabs(rho) < 1.0e-18)
    {
        ctl->error = CWF_ERR_RHO_ZERO;
        ctl->error_iter = -1;
        ctl->active = 0;
    }
}

// alpha from the folded p . Ap (pcg.cpp:840-853), thread 0
__device__ __forceinline__ void alpha_decide(Ctl *ctl, double denom)
{
    ctl->denom = denom;
    if (fabs(denom) < 1.0e-18)
    {
        ctl->error = CWF_ERR_DENOM_ZERO;
        ctl->error_iter = (int)ctl->iterations;
        ctl->active = 0;
        return;
    }
    const double alpha = ctl->rho / denom;
    ctl->alpha = alpha;
    ctl->alpha_last = alpha;
}

// residual, convergence and beta from the folded r . r and r . z (pcg.cpp:862-895), thread 0
__device__ __forceinline__ void beta_decide(Ctl *ctl, double rr, double rz, double *__restrict__ hist)
{
    const double res = sqrt(rr);
    const unsigned long long it = ctl->iterations;
    ctl->res = res;
    ctl->iterations = it + 1;
    hist[it + 1] = res;
    if (res <= ctl->tol)
    {
        ctl->converged = 1;
        ctl->active = 0;
        return;
    }
    if (fabs(ctl->rho) < 1.0e-18)
    {
        ctl->error = CWF_ERR_RHO_ZERO;
        ctl->error_iter = (int)it;
        ctl->active = 0;
        return;
    }
    const double beta = rz / ctl->rho;
    ctl->beta = beta;
    ctl->beta_last = beta;
    ctl->rho = rz;
}

__global__ __launch_bounds__(kFoldThreads) void k_pcg_alpha(Ctl *ctl, const double *__restrict__ p_pAp, uint32_t count)
{
    if (!ctl->active)
        return;
    double denom, unused;
    fold_seq<1>(p_pAp, nullptr, count, denom, unused);
    if (threadIdx.x == 0)
        alpha_decide(ctl, denom);
}

__global__ __launch_bounds__(kFoldThreads) void k_pcg_beta(Ctl *ctl, const double *__restrict__ p_rr,
                                                           const double *__restrict__ p_rz, uint32_t count,
                                                           double *__restrict__ hist)
{
    if (!ctl->active)
        return;
    double rr, rz;
    fold_seq<2>(p_rr, p_rz, count, rr, rz);
    if (threadIdx.x == 0)
        beta_decide(ctl, rr, rz, hist);
}

// The streamed form of fold_seq, run by workgroup 0 of the producing pass. Wave c < NC folds operand c (its lane 0,
// wave-uniform LDS addresses). The S = 4 - NC other waves stage: staging wave w polls the granules of blocks w,
// w + S, ... (kStreamBlock chunks each; a block's slot is claimed first, then every lane polls its NC kStreamBlock / 64
// granules at once, re-polling only those that do not carry the launch's tag yet, and stores each landed value to
// LDS) into a ring of kStreamRing LDS slots, and publishes the block with an LDS flag; the folding waves wait on the
// flag and count the block folded when done. So S blocks' polls are in flight while the chains run, decoupled by
// LDS flags instead of workgroup barriers. The chain is fold_block, in chunk order: bitwise fold_seq over the
// partial arrays. Bounded: a granule that never arrives ends the poll (the block is published anyway, the fold
// returns false and the solve fails).
#ifndef CWF_ALPHA_FOLD_H
#define CWF_ALPHA_FOLD_H 16
#endif
constexpr uint32_t kAlphaFoldH = CWF_ALPHA_FOLD_H;  // (a build macro for the same-box A/B of the register sets)
constexpr uint32_t kStreamBlock = 256;
constexpr uint32_t kStreamCPB = 8;         // chunks per block of the streamed p.Ap pass
// the producing workgroups of the streamed p.Ap / update passes (persistent, in block order). Production, not the
// chain, bounds both passes (C2, rocprofv3 means, same box: p.Ap + alpha 25.5 / 21.9 / 24.0 us at 128 / 256 / 512;
// update + beta 31.9 / 28.1 / 29.4 us at 256 / 512 / 768, 29.5 with one workgroup per node block)
constexpr uint32_t kStreamDotWG = 256;
constexpr uint32_t kStreamUpdWG = 512;
// (kStreamBlock: chunks per fold block; C2's 4,020 chunks in 16 blocks)
constexpr uint32_t kStreamRing = 6;              // LDS slots
constexpr uint32_t kStreamRow = kStreamBlock + 16u;  // + the chain's W spare slots
constexpr uint32_t kStreamMaxRounds = 4000000u;  // poll rounds per block before giving up (>= 4 s)
template <int NC>
constexpr uint32_t fold_stream_lds()  // double2 entries of the caller's staging buffer
{
    return kStreamRing * NC * (kStreamRow / 2u);
}
// bufp: fold_stream_lds<NC>() double2 of LDS (the caller's, so a producing workgroup reuses it for its own staging);
// t0 (operand 0) and t1 (operand 1) are valid in thread 0
template <int NC>
__device__ bool fold_stream(const double *gran, uint32_t count, uint32_t tag, double2 *bufp, double &t0, double &t1)
{
    constexpr uint32_t W = 16, kRow = kStreamRow, kStagers = kFoldThreads / 64 - NC;
    constexpr uint32_t P = kStreamBlock * NC / 64u;  // granules per staging lane and block
    static_assert(P <= 32u && kStreamBlock % (2u * W) == 0u, "stream block");
    double *buf = reinterpret_cast<double *>(bufp);  // slot s, operand c: buf + (s NC + c) kRow
    __shared__ uint32_t ready[kStreamRing], consumed[NC], fail;
    __shared__ double other;
    const __amdgpu_buffer_rsrc_t rs = gran_rsrc(gran);
    const uint32_t nb = (count + kStreamBlock - 1u) / kStreamBlock, lane = threadIdx.x % 64u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64u);  // wave-uniform (scalar LDS addresses)
    if (threadIdx.x < kStreamRing)
        ready[threadIdx.x] = 0u;
    if (threadIdx.x < (uint32_t)NC)
        consumed[threadIdx.x] = 0u;
    if (threadIdx.x == 0)
        fail = 0u;
    __syncthreads();
    // the producing workgroups' waves share these SIMDs: the chain's dependent adds (and the polls feeding it) issue
    // first
    if (wave < (uint32_t)NC)
        __builtin_amdgcn_s_setprio(3);
    else
        __builtin_amdgcn_s_setprio(2);
    if (wave >= (uint32_t)NC)
    {
        for (uint32_t blk = wave - NC; blk < nb; blk += kStagers)
        {
            const uint32_t b0 = blk * kStreamBlock, n = min(kStreamBlock, count - b0), slot = blk % kStreamRing;
            // the slot is free once the chain has folded block blk - kStreamRing (the polls of the next slots are
            // still ahead of the chain: kStreamRing / kStagers blocks per staging wave)
            const auto folded = [&]() {  // blocks both chains have folded
                uint32_t c = __hip_atomic_load(&consumed[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                if constexpr (NC == 2)
                    c = min(c, __hip_atomic_load(&consumed[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
                return c;
            };
            while (blk >= kStreamRing && folded() + kStreamRing <= blk)
                __builtin_amdgcn_s_sleep(1);
            double *row = buf + slot * NC * kRow;
            uint32_t pending = 0;
#pragma unroll
            for (uint32_t u = 0; u < P; ++u)
            {
                const uint32_t q = lane + 64u * u;
                if (q / NC < n)
                    pending |= 1u << u;
                else
                    row[(q % NC) * kRow + q / NC] = 0.0;  // +0.0 pads: the chain always folds kStreamBlock terms
            }
            for (uint32_t round = 0; pending; ++round)
            {
                u32x4 g[P];
#pragma unroll
                for (uint32_t u = 0; u < P; ++u)
                    if ((pending >> u) & 1u)
                        g[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, 16u * (NC * b0 + lane + 64u * u), 0, 16);
#pragma unroll
                for (uint32_t u = 0; u < P; ++u)
                    if (((pending >> u) & 1u) && g[u].z == tag)
                    {
                        const uint32_t q = lane + 64u * u;
                        row[(q % NC) * kRow + q / NC] = __hiloint2double((int)g[u].y, (int)g[u].x);
                        pending &= ~(1u << u);
                    }
                if (!pending)
                    break;
                if (round >= kStreamMaxRounds)
                {
                    __hip_atomic_store(&fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0)
                __hip_atomic_store(&ready[slot], blk + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    else if (lane == 0)
    {
        double acc = 0.0;
        for (uint32_t blk = 0; blk < nb; ++blk)
        {
            const uint32_t slot = blk % kStreamRing;
            while (__hip_atomic_load(&ready[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != blk + 1u)
                __builtin_amdgcn_s_sleep(1);
            // the alpha pass (NC = 1) runs at 2 waves / SIMD (its LDS): 32-partial register sets; the update pass
            // keeps 16 (its VGPRs set its occupancy)
            fold_block<kStreamBlock, NC == 1 ? kAlphaFoldH : 8u>(
                reinterpret_cast<const double2 *>(buf + (slot * NC + wave) * kRow), acc);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __hip_atomic_store(&consumed[wave], blk + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (wave == 1)
            other = acc;
        t0 = acc;
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    t1 = NC == 2 ? other : 0.0;
    return fail == 0u;
}

__device__ __forceinline__ void stream_fail(Ctl *ctl)
{
    ctl->error = CWF_ERR_HIP;
    ctl->error_iter = (int)ctl->iterations;
    ctl->active = 0;
}

// the p . Ap chunk partials (k_dot_chunks256, workgroups 1..) streamed into alpha (k_pcg_alpha, workgroup 0)
__global__ __launch_bounds__(256) void k_dot_alpha_stream(const float *__restrict__ p, const float *__restrict__ Ap,
                                                          uint32_t D, uint32_t chunks, Ctl *ctl,
                                                          const double *gran, uint32_t tag)
{
    if (!ctl->active)
        return;
    if (blockIdx.x == 0)
    {
        __shared__ double2 fbuf[fold_stream_lds<1>()];
        double denom = 0.0, unused;
        const bool ok = fold_stream<1>(gran, chunks, tag, fbuf, denom, unused);
        if (threadIdx.x == 0)
            ok ? alpha_decide(ctl, denom) : stream_fail(ctl);
        return;
    }
    // workgroups 1..G walk the blocks in order (block j G + b - 1 in their j-th step), so the partials land roughly in
    // chunk order while workgroup 0 folds: 8 chunks per block, the first step's land after one round trip
    const uint32_t nblk = (chunks + kStreamCPB - 1u) / kStreamCPB, G = gridDim.x - 1u;
    for (uint32_t bx = blockIdx.x - 1u; bx < nblk; bx += G)
    {
        dot_chunks256<1, kStreamCPB>(p, Ap, nullptr, D, chunks, nullptr, nullptr, bx, gran, tag);
        __syncthreads();  // the staging rows are refilled by the next block
    }
}

// ---- node-wise vector phases ----

// r = rhs - Ap (f32), then enforce_dirichlet_solution (pcg.cpp:761-766, 458-475)
__global__ __launch_bounds__(kBlock) void k_init_residual(DevSys s, const float *__restrict__ rhs,
                                                          const float *__restrict__ Ap, float *__restrict__ x,
                                                          float *__restrict__ r)
{
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= s.N)
        return;
    const uint32_t mk = s.mask[n];
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        const uint32_t d = 3u * n + k;
        float rv = rhs[d] - Ap[d];
        if (mk & (1u << k))
        {
            x[d] = rhs[d];
            rv = 0.0f;
        }
        r[d] = rv;
    }
}

__device__ __forceinline__ void precond_node(const float *__restrict__ inv, uint32_t n, uint32_t mk, const float rv[3],
                                             float z[3])
{
    // pcg.cpp:426-453
    const double r0 = (double)rv[0], r1 = (double)rv[1], r2 = (double)rv[2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        double sum = 0.0;
        sum += (double)inv[9u * n + 3 * k + 0] * r0;
        sum += (double)inv[9u * n + 3 * k + 1] * r1;
        sum += (double)inv[9u * n + 3 * k + 2] * r2;
        z[k] = (mk & (1u << k)) ? 0.0f : (float)sum;
    }
}

__global__ __launch_bounds__(kBlock) void k_precond(DevSys s, const float *__restrict__ inv,
                                                    const float *__restrict__ r, float *__restrict__ z,
                                                    const Ctl *__restrict__ ctl)
{
    if (ctl && !ctl->active)
        return;
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= s.N)
        return;
    const float rv[3] = {r[3u * n], r[3u * n + 1], r[3u * n + 2]};
    float zv[3];
    precond_node(inv, n, s.mask[n], rv, zv);
    z[3u * n] = zv[0];
    z[3u * n + 1] = zv[1];
    z[3u * n + 2] = zv[2];
}

// p = z, constrained -> 0 (pcg.cpp:815-828)
__global__ __launch_bounds__(kBlock) void k_p_init(DevSys s, const float *__restrict__ z, float *__restrict__ p,
                                                   const Ctl *__restrict__ ctl)
{
    if (!ctl->active)
        return;
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= s.N)
        return;
    const uint32_t mk = s.mask[n];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        p[3u * n + k] = (mk & (1u << k)) ? 0.0f : z[3u * n + k];
}

// x += f32(alpha p); r -= f32(alpha Ap); enforce; z = M^-1 r  (pcg.cpp:854-860, 877), and the chunk partials of
// r . r and r . z (pcg.cpp:862, 883) from the workgroup's own DOFs (wg_chunk_partials)
// STREAM: workgroup 0 folds the r . r and r . z granules of workgroups 1.. (their nodes: blockIdx - 1) into the
// residual check and beta (k_pcg_beta's work, fold_stream), gran / tag / hist its arguments
template <bool STREAM>
__global__ __launch_bounds__(kBlock) void k_update(DevSys s, const float *__restrict__ rhs,
                                                   const float *__restrict__ inv, const float *__restrict__ p,
                                                   const float *__restrict__ Ap, float *__restrict__ x,
                                                   float *__restrict__ r, float *__restrict__ z,
                                                   Ctl *__restrict__ ctl, double *__restrict__ prr,
                                                   double *__restrict__ prz, uint32_t nlim, uint32_t chunks,
                                                   const double *gran, uint32_t tag, double *__restrict__ hist)
{
    constexpr uint32_t kSh = STREAM ? std::max<uint32_t>(6u * kChunkRow, fold_stream_lds<2>()) : 3u * kChunkRow;
    __shared__ double2 srz[kSh];
    if (!ctl->active)
        return;
    if constexpr (STREAM)
        if (blockIdx.x == 0)
        {
            double rr = 0.0, rz;
            const bool ok = fold_stream<2>(gran, chunks, tag, srz, rr, rz);
            if (threadIdx.x == 0)
                ok ? beta_decide(ctl, rr, rz, hist) : stream_fail(ctl);
            return;
        }
    // one node block: x, r, z and (prr) the staged fp64 products of its DOFs in st
    const auto nodes = [&](uint32_t bx, double2 *st) {
        const uint32_t n = bx * kBlock + threadIdx.x;
        float rv[3] = {0.f, 0.f, 0.f}, zv[3] = {0.f, 0.f, 0.f};
        if (n < s.N)
        {
            const double alpha = ctl->alpha;
            const uint32_t mk = s.mask[n];
#pragma unroll
            for (int k = 0; k < 3; ++k)
            {
                const uint32_t d = 3u * n + k;
                float xv = x[d] + (float)(alpha * (double)p[d]);
                float rr = r[d] - (float)(alpha * (double)Ap[d]);
                if (mk & (1u << k))
                {
                    xv = rhs[d];
                    rr = 0.0f;
                }
                x[d] = xv;
                r[d] = rr;
                rv[k] = rr;
            }
            precond_node(inv, n, mk, rv, zv);
            z[3u * n] = zv[0];
            z[3u * n + 1] = zv[1];
            z[3u * n + 2] = zv[2];
        }
        if (!prr)  // a reduction chunk other than 256 DOFs: the partials are a separate pass
            return;
        const bool own = n < nlim;
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            const double r = (double)rv[k];
            st[chunk_slot(3u * threadIdx.x + k)] = own ? double2{r * r, r * (double)zv[k]} : double2{0.0, 0.0};
        }
    };
    if constexpr (STREAM)
    {
        // workgroups 1..G walk the node blocks in order (block j G + b - 1 in their j-th step), so the partials
        // land roughly in chunk order while workgroup 0 folds them. The staging rows alternate by step: wave 0's
        // lanes 0-2 fold block j's chunks while waves 1-3 already load and form block j + G (wave 0 reaches step
        // j + 1's barrier only after its chains, so block j + 2 G never restages rows still being folded)
        const uint32_t nblk = (s.N + kBlock - 1u) / kBlock, G = gridDim.x - 1u;
        uint32_t j = 0;
        for (uint32_t bx = blockIdx.x - 1u; bx < nblk; bx += G, ++j)
        {
            double2 *st = srz + (j & 1u) * (3u * kChunkRow);
            nodes(bx, st);
            __syncthreads();
            wg_chunk_partials<2>(st, chunks, prr, prz, bx, gran, tag);
        }
    }
    else
    {
        nodes(blockIdx.x, srz);
        if (!prr)
            return;
        __syncthreads();
        wg_chunk_partials<2>(srz, chunks, prr, prz, blockIdx.x);
    }
}

// p = f32(double(z) + beta double(p)), constrained -> 0 (pcg.cpp:897-914)
__global__ __launch_bounds__(kBlock) void k_p_update(DevSys s, const float *__restrict__ z, float *__restrict__ p,
                                                     const Ctl *__restrict__ ctl)
{
    if (!ctl->active)
        return;
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= s.N)
        return;
    const double beta = ctl->beta;
    const uint32_t mk = s.mask[n];
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        const uint32_t d = 3u * n + k;
        const float pv = (float)((double)z[d] + beta * (double)p[d]);
        p[d] = (mk & (1u << k)) ? 0.0f : pv;
    }
}

inline bool knob_off(const char *name)
{
    const char *v = knob(name);
    return v && v[0] == '0';
}

}  // namespace

uint32_t parity_chunk_count(const cwf_hip_system *h)
{
    const uint64_t B = h->reduction_block ? h->reduction_block : 1;
    return (uint32_t)((h->ds.D + B - 1) / B);
}

// the chunk partials of a . b (and a . c) over the first D DOFs, B per chunk. An unsharded handle's D = 3 Nown = ds.D:
// abi.cpp sets Nown = N and D = 3 N at create, and only an attach (comm.cpp) lowers Nown
void parity_dot_partials(uint32_t D, uint32_t B, const float *a, const float *b, const float *c, double *pab,
                         double *pac, const Ctl *ctl, hipStream_t st)
{
    B = B ? B : 1;
    const uint32_t chunks = (uint32_t)(((uint64_t)D + B - 1) / B);
    if (chunks == 0)
        return;
    if (B == 256)
    {
        if (c)
            k_dot_chunks256<2><<<grid_for(chunks, kDotChunksPerBlock), 256, 0, st>>>(a, b, c, D, chunks, pab, pac, ctl);
        else
            k_dot_chunks256<1><<<grid_for(chunks, kDotChunksPerBlock), 256, 0, st>>>(a, b, c, D, chunks, pab, pac, ctl);
    }
    else
    {
        if (c)
            k_dot_chunks_generic<2><<<grid_for(chunks, kBlock), kBlock, 0, st>>>(a, b, c, D, B, chunks, pab, pac,
                                                                                ctl);
        else
            k_dot_chunks_generic<1><<<grid_for(chunks, kBlock), kBlock, 0, st>>>(a, b, c, D, B, chunks, pab, pac,
                                                                                ctl);
    }
}

void parity_fold(const double *part, uint32_t count, double *out, hipStream_t st)
{
    k_fold1<<<1, kFoldThreads, 0, st>>>(part, count, out);
}

void launch_init_residual(const cwf_hip_system *h, const float *rhs, hipStream_t st)
{
    k_init_residual<<<grid_for(h->ds.N, kBlock), kBlock, 0, st>>>(h->ds, rhs, h->Ap, h->x, h->r);
}

void launch_precond(const cwf_hip_system *h, const Ctl *ctl, hipStream_t st)
{
    k_precond<<<grid_for(h->ds.N, kBlock), kBlock, 0, st>>>(h->ds, h->inv, h->r, h->z, ctl);
}

void launch_p_init(const cwf_hip_system *h, hipStream_t st)
{
    k_p_init<<<grid_for(h->ds.N, kBlock), kBlock, 0, st>>>(h->ds, h->z, h->p, h->ctl);
}

namespace
{
using Group = std::vector<cwf_hip_system *>;

// where a member's chunk partials go and how many entries its scalar kernels fold. A single handle folds its own
// chunks. A shard writes its chunks to its rank's slot of the all-gathered block (pstride entries per rank, +0.0 past
// the rank's own chunks: comm.cpp sharded_parity_setup) and folds every rank's, which is the global chunk order
struct Partials
{
    double *p0, *p1;  // the two arrays the scalar kernels fold, from their first entry
    size_t own;       // the member's own slot in them
    uint32_t count;   // entries folded
};

Partials partials_of(const cwf_hip_system *h)
{
    if (!h->sharded())
        return {h->part0, h->part1, 0, parity_chunk_count(h)};
    return {h->gp0, h->gp1, (size_t)h->rank * h->pstride, (uint32_t)h->nranks * h->pstride};
}

inline uint32_t owned_dofs(const cwf_hip_system *h) { return 3u * h->ds.Nown; }

// the exchanges between the phases, a shard group's only: every rank's slot of gp0 (both: and of gp1) to every rank
int gather_partials(const Group &g, bool both)
{
    if (!g[0]->sharded())
        return 0;
    const size_t S = g[0]->pstride;
    if (!both)
        return comm_allgather(g, &cwf_hip_system::gp0, S);
    return comm_exchange(g, {Gather{&cwf_hip_system::gp0, S}, Gather{&cwf_hip_system::gp1, S}}, nullptr);
}

int ghost_rows(const Group &g, float *cwf_hip_system::*vec) { return g[0]->sharded() ? comm_halo(g, vec) : 0; }

// x, r, z of every node and the chunk partials of r . r and r . z over the owned ones (fused for 256-DOF chunks)
void update_pass(cwf_hip_system *h, const float *rhs, double *prr, double *prz)
{
    const uint32_t nlim = h->ds.Nown;
    const bool fused = h->reduction_block == 256;
    k_update<false><<<grid_for(h->ds.N, kBlock), kBlock, 0, h->stream>>>(
        h->ds, rhs, h->inv, h->p, h->Ap, h->x, h->r, h->z, h->ctl, fused ? prr : nullptr, prz, nlim,
        grid_for(3u * nlim, 256u), nullptr, 0u, nullptr);
    if (!fused)
        parity_dot_partials(3u * nlim, (uint32_t)h->reduction_block, h->r, h->r, h->z, prr, prz, h->ctl, h->stream);
}
}  // namespace

// solve_pcg prologue (pcg.cpp:744-828) of every member (a single unsharded handle is the group {h}: no exchange).
// Requires x (warm start or zeroed) on device.
int parity_pcg_init_group(const Group &g, const std::vector<const float *> &rhs, double rel_tol)
{
    if (g[0]->sharded())
        if (int st = sharded_parity_setup(g))
            return st;
    for (cwf_hip_system *h : g)
    {
        if (!h->sharded() && !h->fgran && h->reduction_block == 256 && !knob_off("CWF_PARITY_STREAM"))
        {
            // the streamed folds' granules: 2 per chunk, tag 0 (the first streamed launch's tag is 1)
            const size_t count = 4ull * parity_chunk_count(h) + 8u;  // doubles: 32 B per chunk and 64 B
            if ((h->fgran = h->mem.alloc<double>(count)) != nullptr)
            {
                h->fgran_tag = 0;
                (void)hipMemsetAsync(h->fgran, 0, count * sizeof(double), h->stream);
            }
        }
        parity_block_jacobi(h, h->inv, h->stream);
        h->inv_fast = false;  // inv now holds the PARITY inverse (not symmetrised, no inv6)
    }
    if (int st = ghost_rows(g, &cwf_hip_system::x))  // warm start: ghost x from the owners
        return st;
    for (size_t i = 0; i < g.size(); ++i)
    {
        cwf_hip_system *h = g[i];
        const Partials q = partials_of(h);
        const uint32_t B = (uint32_t)h->reduction_block;
        parity_keff(h, h->x, h->Ap, true, nullptr, h->stream);
        launch_init_residual(h, rhs[i], h->stream);
        parity_dot_partials(owned_dofs(h), B, rhs[i], rhs[i], nullptr, q.p0 + q.own, nullptr, nullptr, h->stream);
        parity_dot_partials(owned_dofs(h), B, h->r, h->r, nullptr, q.p1 + q.own, nullptr, nullptr, h->stream);
    }
    if (int st = gather_partials(g, true))
        return st;
    for (cwf_hip_system *h : g)
    {
        const Partials q = partials_of(h);
        k_pcg_init_scalars<<<1, kFoldThreads, 0, h->stream>>>(h->ctl, q.p0, q.p1, q.count, rel_tol, h->hist);
        launch_precond(h, h->ctl, h->stream);
        parity_dot_partials(owned_dofs(h), (uint32_t)h->reduction_block, h->r, h->z, nullptr, q.p0 + q.own, nullptr,
                            h->ctl, h->stream);
    }
    if (int st = gather_partials(g, false))
        return st;
    for (cwf_hip_system *h : g)
    {
        k_pcg_init_rho<<<1, kFoldThreads, 0, h->stream>>>(h->ctl, partials_of(h).p0, partials_of(h).count);
        launch_p_init(h, h->stream);
    }
    return ghost_rows(g, &cwf_hip_system::p);
}

// one PCG iteration (pcg.cpp:830-915) of every member; no-op once ctl->active == 0. Member 0's K_eff carries the
// timing events
int parity_pcg_iteration_group(const Group &g, const std::vector<const float *> &rhs, hipEvent_t e0, hipEvent_t e1)
{
    cwf_hip_system *h0 = g[0];
    if (!h0->sharded() && h0->fgran && h0->reduction_block == 256 && h0->ds.ptile_nodes && h0->ds.Nown == h0->ds.N)
    {
        // streamed folds: alpha folded by the p . Ap pass's workgroup 0, beta by the update pass's (the same
        // partials in the same order as below: bitwise the same scalars), two launches fewer per iteration
        const DevSys &s = h0->ds;
        const hipStream_t st = h0->stream;
        const uint32_t chunks = parity_chunk_count(h0);
        if (e0)
            (void)hipEventRecord(e0, st);
        parity_keff_ds(s, h0->p, h0->Ap, false, h0->ctl, st);
        if (e1)
            (void)hipEventRecord(e1, st);
        const uint32_t t1 = ++h0->fgran_tag, t2 = ++h0->fgran_tag;
        const uint32_t gd = std::min(grid_for(chunks, kStreamCPB), kStreamDotWG);
        const uint32_t gu = std::min(grid_for(s.N, kBlock), kStreamUpdWG);
        k_dot_alpha_stream<<<1u + gd, 256, 0, st>>>(h0->p, h0->Ap, 3u * s.N, chunks, h0->ctl, h0->fgran, t1);
        k_update<true><<<1u + gu, kBlock, 0, st>>>(s, rhs[0], h0->inv, h0->p, h0->Ap, h0->x, h0->r, h0->z, h0->ctl,
                                                   h0->part0, h0->part1, s.N, chunks, h0->fgran, t2, h0->hist);
        k_p_update<<<grid_for(s.N, kBlock), kBlock, 0, st>>>(s, h0->z, h0->p, h0->ctl);
        return 0;
    }
    for (size_t i = 0; i < g.size(); ++i)
    {
        cwf_hip_system *h = g[i];
        const Partials q = partials_of(h);
        if (i == 0 && e0)
            (void)hipEventRecord(e0, h->stream);
        parity_keff_dot(h, h->p, h->Ap, h->ctl, q.p0 + q.own, h->stream);  // + the p . Ap chunk partials
        if (i == 0 && e1)
            (void)hipEventRecord(e1, h->stream);
    }
    if (int st = gather_partials(g, false))
        return st;
    for (size_t i = 0; i < g.size(); ++i)
    {
        cwf_hip_system *h = g[i];
        const Partials q = partials_of(h);
        k_pcg_alpha<<<1, kFoldThreads, 0, h->stream>>>(h->ctl, q.p0, q.count);
        update_pass(h, rhs[i], q.p0 + q.own, q.p1 + q.own);  // + the r . r and r . z chunk partials
    }
    if (int st = gather_partials(g, true))
        return st;
    for (cwf_hip_system *h : g)
    {
        const Partials q = partials_of(h);
        k_pcg_beta<<<1, kFoldThreads, 0, h->stream>>>(h->ctl, q.p0, q.p1, q.count, h->hist);
        k_p_update<<<grid_for(h->ds.N, kBlock), kBlock, 0, h->stream>>>(h->ds, h->z, h->p, h->ctl);
    }
    return ghost_rows(g, &cwf_hip_system::p);  // p on the ghosts, for the next K_eff p
}

}  // namespace cwf
