// resident.hip -- k_pcg_resident: a whole FAST PCG solve of a structured block in ONE launch, with every vector on chip
// (lattice_common.hpp: the fused iteration's per-node arithmetic, run unchanged).
//
// Why: the fused one-launch iteration (lattice_fused.hip) is bound by a per-workgroup chain, not by bytes -- every
// launch re-reads r, Ap, p, x and the class of every node from L2 / MALL (97 B per node), every workgroup refolds the
// previous launch's 436 x 5 shares, and a kernel boundary separates the iterations (C2: 18 us per iteration for 33 MB,
// 0.23 of HBM; VERDICT r5 items 2 and the C3 / 8 strong-scaling bound). A block of up to ~0.5M nodes fits on chip:
// 256 CUs x 160 KB of LDS and 512 KB of VGPRs hold C2's 16.5 MB of r, Ap, p, x many times over. So the solve becomes
// one persistent launch of one 512-thread workgroup per CU, each owning a box of the lattice:
//   - its nodes' r, Ap, p, x, class and mass live on chip (registers, or LDS in the 4-node instantiation) for the
//     whole solve;
//   - per iteration (phase j) it forms r_j, z_j, p_j, x_j exactly as lattice_fused.hip's launch j does (fused_form),
//     writes p_j into an LDS image of the box plus its one-node ring, applies the stencil rows (interior nodes: the
//     brick rows' difference form; block-surface nodes: the shell's cell form), and leaves the five fp64 dots. The
//     image's strides are the box's own (ResArgs::hdr), padded by the plan so that the rows' ds_read_b128 and the
//     form's ds_write_b128 spread over the LDS banks: with dense strides 14 lanes in a line and the next line 16 slots
//     on put two lanes of a read group on one bank quad, and a block x-face row (x fixed, lanes stepping y by 16
//     slots) all sixteen (resident_image.hpp; CWF_RESIDENT_IMAGE=0 keeps the dense strides, same bits).
// The hand-off between boxes is tagged 16-B granules, one synchronisation per iteration, no counter:
//   - published: per box-surface node that another box reads, ONE granule {Ap_j.xyz, tag} per phase (pub, by phase
//     parity), and per workgroup five share granules {dot lo, hi, tag, -} (sh). The tag is tag0 + j + 1: a granule of
//     another phase or of an earlier solve never matches. Every granule is one write-through (sc1) 16-B store; the
//     node granules are stored in the rows, the shares last;
//   - kept by the consumer: r_(j-1) and p_(j-1) of each ring entry, in the registers of the thread that has the entry
//     (hr, hp), for the whole solve. Phase 0 takes r_0 from fast_fused_init's r vector and p = Ap = 0, as the owner
//     does; phase j forms r_j = r_(j-1) - alpha Ap_(j-1), z_j, p_j = z_j + beta p_(j-1) with fused_form from the kept
//     values, the loaded Ap_(j-1) and the node's class. The owner runs the same function on the same bits with the same
//     alpha and beta (every workgroup folds the same shares in the same order, fused_decide), so both sides hold the
//     same r_j and p_j bit for bit and neither ever has to be sent. A shard's ghost entries are ring entries like any
//     other: only the source of their Ap granule differs (the PEER mailbox, system scope);
//   - who folds the shares is decided per launch (launch_pcg_resident, CWF_RESIDENT_REDUCER):
//     * the reducer role (an unsharded plan of >= kResReducerMinBoxes boxes that leaves a CU spare: C2's 245 boxes on
//       256 CUs): the grid is G + 1 workgroups and workgroup G owns no box (resident_reduce). Per phase its thread
//       t < G polls box t's five shares (each wave on its own), it folds them with block_sum_lds in the boxes' order,
//       runs fused_decide ONCE, records ctl and the history, and stores one decision granule {alpha f32, beta f32,
//       state, tag0 + j} (two of them, by phase parity, 128 B apart in the part of pub behind the Ap granules). A box
//       polls that one granule (every lane the same address, under the workgroup's vote) and meanwhile requests its
//       ring's Ap granules, each until it carries the tag; it takes alpha and beta from the granule and neither sweeps
//       the G x 5 shares nor folds nor decides. state: continue / stop (write x, r) / failed (the reducer gave up:
//       leave without writing). The decision granule needs no ordering against any other granule: alpha, beta, state
//       and tag travel in the one 16-B store, and the Ap granules a box reads beside it carry their own tags. Same
//       bits as the other path: the same shares, the same fold, the same fused_decide, and the float alpha and beta
//       every box would have computed (tests/test_gpu_resident_reducer.py);
//     * otherwise (and always on a PEER shard) every box polls the G x 5 shares itself, as below;
//   - a phase polls (sc1 loads, served past the non-coherent L1 / per-XCD L2) the G x 5 shares until all carry phase
//     j - 1's tag, requests its ring's Ap granules, folds the shares, forms its own nodes, then checks each ring
//     granule's tag under a workgroup vote; granules that had not landed are requested again. The vote can fail, so
//     the ring check can run more than once per phase: every pass forms from the OLD kept values into temporaries
//     (hrn, hpn), and they replace the kept ones only after the vote has passed. Updating in place would apply alpha
//     twice to the entries that had landed on a pass another entry failed (CWF_RESIDENT_REREAD forces a second pass:
//     tests/test_gpu_resident_handoff.py);
//   - this rests on a 16-B store being seen whole or not at all by a 16-B load of the same aligned address (value and
//     tag travel in one granule, so no ordering between granules is needed): observed on gfx950 for the dwordx4
//     buffer accesses used here, not an architectural guarantee (DESIGN.md section 7 states the same for the mailboxes).
// Every wait is bounded (kResMaxRounds poll rounds, then give_up): a workgroup that is never scheduled (the grid must be
// co-resident, one per CU; resident_blocks_per_cu checks the occupancy, and the reducer role runs only where G + 1
// workgroups fit) ends the solve with CWF_ERR_HIP instead of hanging the GPU. With the role a reducer that gives up
// publishes "failed", so every box leaves at its next poll; a box that gives up stores no shares, so the reducer gives
// up one bound later and releases the rest. Every exit is workgroup-uniform (the votes; the reducer's timeout flag is
// read behind its fold's barrier).
//
// Results: the per-node arithmetic is lattice_fused.hip's; only the grouping of the fp64 dot sums differs (boxes
// instead of bricks), so alpha / beta differ in their last bits and the solve is tolerance-equal, not bit-equal, to the
// fused schedule (tests/test_gpu_resident.py). Deterministic run to run: no atomics touch a value, the folds' order is
// fixed.
#include <hip/hip_ext.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lattice_common.hpp"

namespace cwf
{
namespace
{
constexpr int kResNT = 512;
constexpr uint32_t kResMaxRounds = 4000000u;  // poll rounds before a phase gives up (>= 4 s: a round is >= 1 us)
constexpr uint32_t kResNone = 0xFFFFFFFFu;
constexpr uint32_t kResOob = 0xFFFFFF00u;  // a byte offset past every range-checked buffer here, +32 included (no wrap)
constexpr uint32_t kResGhost = 0x80000000u;  // a halo entry's source: a shard's ghost record (resident.cpp)
// boxes from which the reducer role runs by default (the same-box A/B by box count)
constexpr unsigned kResReducerMinBoxes = 56;
constexpr int kResTypes = 12;  // boundary types one box's own nodes touch, at most (resident.cpp kResTypesHost)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct ResArgs
{
    Ctl *ctl;
    double *hist;
    const uint4 *hdr;   // [G] {LDS slots, - (the plan's first ghost halo entry: unused here), PX, PXY}: the box's
                        // (sx + 2)(sy + 2)(sz + 2) image and its strides PX >= sx + 2, PXY >= PX (sy + 2), padded per
                        // box against LDS bank conflicts (resident_image.hpp); slots = PXY (sz + 2)
    const uint4 *own;   // [G][own_stride] {node, image slot, publication index or kResNone, -}
    const uint4 *halo;  // [G][halo_stride] {node, slot, publication index of its owner's record, -}
    const float4 *tcoef;  // the stencil of each boundary type (the block-surface rows), padded blocks: [27][nOff][3]
                          // for the register-state instantiation; for the LDS-state one [G][kResTypes][nOff][3], per
                          // box only the types its nodes have (the own entry's y >> 24 is the node's index there)
    uint32_t own_stride, halo_stride;
    float *pub;         // [2][npub][4] by phase parity: one granule {Ap.xyz, tag} per published node
    uint32_t npub;
    double *sh;         // [2][G][5] granules {share lo, hi, tag, -} by phase parity
    uint32_t tag0;      // this solve's tag base: phase j's granules carry tag0 + j + 1 (a previous solve's never match)
    float *x, *r;       // in: x_0 (the warm start) and r_0 (fast_fused_init); out: x and r at the stop
    uint32_t max_it;
    uint64_t *trace;    // diagnostic (CWF_RESIDENT_TRACE): per workgroup 8 s_memrealtime stamps of phase trace_j
    uint32_t trace_j;
    uint32_t reread;    // test (CWF_RESIDENT_REREAD): every phase j > 0 takes its first ring vote as failed once
    uint32_t G;         // the plan's boxes (the grid has one workgroup more when the reducer role is on)
    uint32_t reducer;   // 1: workgroup G is the reducer, the boxes poll its decision granule (never with MR)
    uint32_t dec_off;   // byte offset in pub of the decision granules {alpha, beta, state, tag}, 128 B apart by phase parity
    // a PEER slab shard (nranks > 1): the send planes' Ap_(j-1) granules stored into the neighbours' mailboxes too (a
    // ghost is a ring entry like any other, only its granule's source differs), the ghosts' granules read from this
    // rank's, the rank totals stored to every rank and polled from this rank's
    ResPeerArgs pa;
};

__device__ __forceinline__ void st4_sc1(__amdgpu_buffer_rsrc_t rs, uint32_t off, u32x4 w)
{
    __builtin_amdgcn_raw_buffer_store_b128(w, rs, off, 0, 16);  // sc1: write-through, past the XCD's L2
}
__device__ __forceinline__ u32x4 pk4(float a, float b, float c, float d)
{
    return u32x4{__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d)};
}
__device__ __forceinline__ u32x4 ld4_sc1(__amdgpu_buffer_rsrc_t rs, uint32_t off)
{
    return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16);  // sc1: served past L1
}
// the PEER mailboxes (uncached IPC memory, written by other devices over xGMI): system scope both ways
__device__ __forceinline__ void st4_sys(__amdgpu_buffer_rsrc_t rs, uint32_t off, u32x4 w)
{
    __builtin_amdgcn_raw_buffer_store_b128(w, rs, off, 0, 17);  // sc0 sc1
}
__device__ __forceinline__ u32x4 ld4_sys(__amdgpu_buffer_rsrc_t rs, uint32_t off)
{
    return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 17);
}

// a workgroup barrier that orders LDS only: no vmcnt wait, so the write-through stores and the polls in flight stay in
// flight across it (__syncthreads' workgroup fence would wait for every store to be acknowledged)
__device__ __forceinline__ void lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// block_sum_k's fixed order (wave sums, then the waves in order) over lds_sync. No trailing barrier: each caller's next
// write of `red` is behind other workgroup barriers of the phase (the halo vote / image barrier, the next phase's polls)
template <int NT, int K>
__device__ __forceinline__ void block_sum_lds(double v[K], double *red)
{
#pragma unroll
    for (int q = 0; q < K; ++q)
    {
        v[q] = wave_sum(v[q]);
        if ((threadIdx.x & 63) == 0)
            red[K * (threadIdx.x >> 6) + q] = v[q];
    }
    lds_sync();
#pragma unroll
    for (int q = 0; q < K; ++q)
    {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w)
            t += red[K * w + q];
        v[q] = t;
    }
}

// the decision granule's state word
constexpr uint32_t kDecGo = 1u, kDecStop = 2u, kDecFailed = 3u;  // continue; stop and write x, r; leave without writing

// The reducer role: workgroup G of a G + 1 grid owns no box. Per phase j >= 1 thread t < G polls workgroup t's five
// share granules of phase j - 1 (each wave on its own: it runs its wave_sum as soon as its 64 workgroups' tags match;
// the workgroup meets once, at block_sum_lds' barrier), the shares are folded in block_sum_lds' order, fused_decide
// runs once, and one lane stores the decision granule every box polls. Thread 0 records ctl and the history. `red2` is
// two fold buffers by phase parity (a wave may poll phase j + 1 while another still reads phase j's wave sums: the
// reducer has no other barrier in its phase); `flag` three words by phase mod 3, a wave's timeout of that phase.
__device__ __forceinline__ void resident_reduce(const ResArgs &ra, double *red2, int *flag)
{
    const uint32_t G = ra.G, tid = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rsh = sized_rsrc(ra.sh, 160u * G),
                                 rdec = sized_rsrc(reinterpret_cast<const char *>(ra.pub) + ra.dec_off, 256u);
    const CtlPre pre = ctl_prefetch(ra.ctl, 1u);
    const bool tr = ra.trace != nullptr;
    if (tid == 0)
        flag[1] = 0;
    lds_sync();
    if (pre.active == 0)
        return;
    for (unsigned j = 1;; ++j)
    {
        const uint32_t par = (j - 1u) & 1u, want = ra.tag0 + j;
        const bool st = tr && j == ra.trace_j;
        uint64_t t0 = 0;
        if (st)
            t0 = __builtin_amdgcn_s_memrealtime();
        if (tid == 0)
            flag[(j + 1u) % 3u] = 0;
        u32x4 g[kFusedShares];
        uint32_t rounds = 0;
        for (;; ++rounds)
        {
#pragma unroll
            for (int q = 0; q < kFusedShares; ++q)
                g[q] = ld4_sc1(rsh, tid < G ? 16u * ((par * G + tid) * kFusedShares + (uint32_t)q) : kResOob);
            bool ok = true;
#pragma unroll
            for (int q = 0; q < kFusedShares; ++q)
                ok = ok && (tid >= G || g[q].z == want);
            if (__builtin_amdgcn_ballot_w64(!ok) == 0ull)
                break;
            if (rounds >= kResMaxRounds)
            {
                flag[j % 3u] = 1;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        double *red = red2 + (j & 1u) * (kFusedShares * (kResNT / 64));
        if (st && (tid & 63u) == 0u)  // when this wave had seen its shares: the latest of the eight is stamp 1
            reinterpret_cast<uint64_t *>(red2 + 2 * kFusedShares * (kResNT / 64))[tid >> 6] = __builtin_amdgcn_s_memrealtime();
        double v[kFusedShares];
#pragma unroll
        for (int q = 0; q < kFusedShares; ++q)
            v[q] = tid < G ? __hiloint2double((int)g[q].y, (int)g[q].x) : 0.0;
        block_sum_lds<kResNT, kFusedShares>(v, red);  // the boxes' fold: the same totals, bit for bit
        const bool failed = flag[j % 3u] != 0;
        uint64_t t2 = 0;
        if (st)
            t2 = __builtin_amdgcn_s_memrealtime();
        float alpha = 0.f, beta = 0.f;
        bool go = false;
        if (failed)
        {
            if (tid == 0)
            {
                ra.ctl->error = CWF_ERR_HIP;
                ra.ctl->error_iter = (int)j;
                ra.ctl->active = 0;
            }
        }
        else
        {
            go = fused_decide(ra.ctl, ra.hist, j, pre, tid == 0, v, &alpha, &beta, j - 1u == ra.max_it);
            if (go && j - 1u == ra.max_it)  // max_iterations updates made
                go = false;
        }
        // the publishing lane is wave 1's first: wave 0 has thread 0's ctl and history stores in front of it
        if (tid == 64u)
            st4_sc1(rdec, 128u * (j & 1u),
                    u32x4{__float_as_uint(alpha), __float_as_uint(beta), failed ? kDecFailed : go ? kDecGo : kDecStop, want});
        if (st && tid == 64u)
            __hip_atomic_store(ra.trace + 8ull * G + 3, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        if (st && tid == 0)
        {
            const uint64_t *ws = reinterpret_cast<const uint64_t *>(red2 + 2 * kFusedShares * (kResNT / 64));
            uint64_t t1 = 0;
            for (int w = 0; w < kResNT / 64; ++w)
                t1 = ws[w] > t1 ? ws[w] : t1;
            uint64_t *row = ra.trace + 8ull * G;
            __hip_atomic_store(row + 0, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(row + 1, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(row + 2, t2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(row + 4, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!go)
            return;
    }
}

template <bool SYM, class E, int NPT, int NPH, bool MR>
__global__ __launch_bounds__(kResNT) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_pcg_resident(DevSys s, ResArgs ra, const float *__restrict__ coef)
{
    extern __shared__ float4 pl[];  // the box + one-node halo image of p_j (out-of-block entries stay 0)
    __shared__ double red[kFusedShares * (kResNT / 64)];
    __shared__ float4 czA[kLatClasses];
    __shared__ float2 czB[kLatClasses];
    constexpr bool LST = NPT > 3;
    constexpr int kTT = LST ? kResTypes : 27;  // the box's boundary types (LST: the LDS the image needs) or all 27
    __shared__ float4 tcf[kTT * E::nOff * 3];  // the boundary types' stencils (not the interior's)
    __shared__ int vote[3];  // the poll rounds' workgroup vote, by round mod 3
    __shared__ double rt[MR ? kFusedShares * kMaxPeers : 1];  // a shard: the ranks' totals, folded in rank order
    // the own entries' r, Ap, x and p: in registers for boxes of <= 3 nodes per thread (C2's 14 x 10 x 10), else
    // (LST) r, Ap, x in LDS (lane-linear: conflict-free) and p in the image (each slot formed by one thread), so 4
    // nodes per thread fit without spilling (the C3 / 8 slab's 19 x 19 x 5; LDS state cost C2 0.9 us per phase)
    __shared__ float st[LST ? 9 : 1][LST ? NPT * kResNT : 1];
    float sreg[LST ? 1 : NPT][LST ? 1 : 12];  // r, Ap, x, p
    const auto S = [&](int u, int q) -> float & {  // q: 0-2 r, 3-5 Ap, 6-8 x (9-11 p: registers only)
        if constexpr (LST)
            return st[q][threadIdx.x + (uint32_t)u * kResNT];
        else
            return sreg[u][q];
    };
    const DevTiles &T = s.t;
    const uint32_t G = ra.G, b = blockIdx.x, tid = threadIdx.x;
    if constexpr (!MR)
        if (ra.reducer != 0u && b == G)  // the reducer: no box, no image; its fold buffers in the stencil table's LDS
        {
            resident_reduce(ra, reinterpret_cast<double *>(tcf), vote);
            return;
        }
    const uint4 hd = ra.hdr[b];
    const int PX = (int)hd.z, PXY = (int)hd.w;
    // diagnostic phase stamps (a uniform branch; no store unless CWF_RESIDENT_TRACE asked for them)
    const auto stamp = [&](unsigned j, int i) {
        if (ra.trace && j == ra.trace_j && tid == 0)
            __hip_atomic_store(ra.trace + 8ull * b + i, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    };
    for (uint32_t i = tid; i < hd.x; i += kResNT)
        pl[i] = float4{0.f, 0.f, 0.f, 0.f};
    for (uint32_t i = tid; i < (uint32_t)(kTT * E::nOff * 3); i += kResNT)
        tcf[i] = ra.tcoef[(LST ? (size_t)b * (kTT * E::nOff * 3) : 0) + i];

    if (tid < kLatClasses)
    {
        const float4 zA = T.lcz[2u * tid], zB = T.lcz[2u * tid + 1u];
        czA[tid] = zA;
        czB[tid] = float2{zB.x, zB.y};
    }
    const uint32_t vbytes = 12u * s.N;
    constexpr bool multi = MR;  // a PEER slab shard (its own instantiation: the one-block kernel stays as it was)
    const __amdgpu_buffer_rsrc_t rx = sized_rsrc(ra.x, vbytes), rr = sized_rsrc(ra.r, vbytes),
                                 rcls = sized_rsrc(T.lcls, s.N), rmass = sized_rsrc(s.mass, 4u * s.N),
                                 rpub = sized_rsrc(ra.pub, 32u * ra.npub), rsh = sized_rsrc(ra.sh, 160u * G);
    // own nodes: their r, Ap, x in LDS (st), p in the image, for the whole solve; in registers only the node, its
    // image slot and class, publication index and mass (4 per node: 4 nodes per thread fit without spilling)
    uint32_t on[NPT], osc[NPT], opub[NPT];  // node; image slot | class << 16; publication index
    float m[NPT];
#pragma unroll
    for (int u = 0; u < NPT; ++u)
    {
        const uint32_t e0 = tid + (uint32_t)u * kResNT;
        const uint4 e = ra.own[(size_t)b * ra.own_stride + e0];
        on[u] = e.x;
        opub[u] = e.z;
        const bool v = e.x != kResNone;
        const uint32_t nb = v ? 12u * e.x : 12u * kLatOob3;
        const u32x3 wr = __builtin_amdgcn_raw_buffer_load_b96(rr, nb, 0, 0),
                    wx = __builtin_amdgcn_raw_buffer_load_b96(rx, nb, 0, 0);
        S(u, 0) = __uint_as_float(wr.x), S(u, 1) = __uint_as_float(wr.y), S(u, 2) = __uint_as_float(wr.z);
        S(u, 3) = S(u, 4) = S(u, 5) = 0.f;
        S(u, 6) = __uint_as_float(wx.x), S(u, 7) = __uint_as_float(wx.y), S(u, 8) = __uint_as_float(wx.z);
        if constexpr (!LST)
            sreg[u][9] = sreg[u][10] = sreg[u][11] = 0.f;
        // image slot | class << 16 (| LST: the box's index of the node's boundary type << 24)
        osc[u] = (e.y & (LST ? 0xFF00FFFFu : 0xFFFFu)) |
                 (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rcls, v ? e.x : kResNone, 0, 0) << 16;
        m[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rmass, v ? 4u * e.x : 4u * kLatOob1, 0, 0));
    }
    // halo (ring) entries: their owners' records; r_(j-1) and p_(j-1) of each as this thread formed them in phase
    // j - 1, kept for the whole solve (fused_form on the owner's inputs: the owner's bits)
    uint32_t hn[NPH], hsc[NPH], hpub[NPH];  // node; image slot | class << 16; the owner's publication index
    float hr[NPH][3], hp[NPH][3];
#pragma unroll
    for (int h = 0; h < NPH; ++h)
    {
        const uint4 e = ra.halo[(size_t)b * ra.halo_stride + tid + (uint32_t)h * kResNT];
        hn[h] = e.x;
        hpub[h] = e.z;
        hsc[h] = e.y | (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rcls, e.x != kResNone ? e.x : kResNone, 0, 0)
                           << 16;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            hr[h][c] = hp[h][c] = 0.f;
    }
    const CtlPre pre = ctl_prefetch(ra.ctl, 1u);  // tol and active (set by fast_fused_init)
    // the node's neighbours in the image (workgroup-uniform)
    int soff[E::nOff];
#pragma unroll
    for (int o = 0; o < E::nOff; ++o)
        soff[o] = E::off[o][0] + E::off[o][1] * PX + E::off[o][2] * PXY;
    // halo entry h's Ap granule of the phase of parity par: another box's (pub), or a ghost's in the mailbox (a
    // shard; the out-of-range load of the other source returns 0, so the two combine by OR)
    const auto request = [&](int h, uint32_t par, u32x4 &c, bool need = true) {
        const bool gh = (hpub[h] & kResGhost) != 0u, v = need && hn[h] != kResNone;
        c = ld4_sc1(rpub, v && !gh ? 16u * (par * ra.npub + hpub[h]) : kResOob);
        if constexpr (multi)
        {
            const __amdgpu_buffer_rsrc_t rg = sized_rsrc(par ? ra.pa.grecv[1] : ra.pa.grecv[0], ra.pa.grecv_bytes);
            c |= ld4_sys(rg, v && gh ? 16u * (hpub[h] & ~kResGhost) : kResOob);
        }
    };
    __syncthreads();
    const float sK = (float)s.sK, sM = (float)s.sM;
    bool go = pre.active != 0;
    unsigned j = 0;
    for (; go; ++j)
    {
        float alpha = 0.f, beta = 0.f;
        float ha[NPH][3], hrn[NPH][3], hpn[NPH][3];  // Ap_(j-1); r_j, p_j as formed (kept once the vote has passed)
        u32x4 w1[NPH];  // phase j - 1's halo granules {Ap, tag}
        const uint32_t par = (j - 1u) & 1u, want = ra.tag0 + j;
        // the workgroup's vote on `ok` (slot round mod 3; the next round's slot is reset before this round's
        // barrier: its last readers passed a barrier since). Every thread counts the same rounds: uniform
        uint32_t round = 0;
        const auto all_ok = [&](bool ok) {
            if (tid == 0)
                vote[(round + 1u) % 3u] = 1;
            if (!ok)
                vote[round % 3u] = 0;
            lds_sync();
            return vote[round % 3u] != 0;
        };
        const auto give_up = [&]() {
            if (tid == 0)
            {
                ra.ctl->error = CWF_ERR_HIP;
                ra.ctl->error_iter = (int)j;
                ra.ctl->active = 0;
            }
        };
        if (j == 0)  // phase 0 (alpha = beta = 0; Ap_(-1) = p_(-1) = 0, hp as initialised): the halo's r_0 from
                     // fast_fused_init's r
        {
#pragma unroll
            for (int h = 0; h < NPH; ++h)
            {
                const u32x3 w = __builtin_amdgcn_raw_buffer_load_b96(rr, hn[h] != kResNone ? 12u * hn[h] : 12u * kLatOob3,
                                                                     0, 0);
                hr[h][0] = __uint_as_float(w.x), hr[h][1] = __uint_as_float(w.y), hr[h][2] = __uint_as_float(w.z);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    ha[h][c] = 0.f;
            }
        }
        else if (!MR && ra.reducer != 0u)
        {
            stamp(j, 0);
            // the reducer's decision of phase j (it folded phase j - 1's shares of every workgroup): one granule
            // {alpha, beta, state, tag}, every lane loading the same address, polled until it carries this phase's
            // tag under the workgroup's vote (so the exit stays uniform). Bounded like every wait here
            const __amdgpu_buffer_rsrc_t rdec = sized_rsrc(reinterpret_cast<const char *>(ra.pub) + ra.dec_off, 256u);
            // Every round also requests the ring's Ap granules that have not landed yet (a lane whose granule carries
            // the tag asks for nothing more): their owners stored them in their rows, before their shares, so they
            // are here by the time the decision is, and the ring vote below passes without a load in its way
            u32x4 dg;
#pragma unroll
            for (int h = 0; h < NPH; ++h)
                w1[h] = u32x4{0u, 0u, 0u, ~want};
            for (;; ++round)
            {
#pragma unroll
                for (int h = 0; h < NPH; ++h)
                {
                    const bool need = w1[h].w != want;
                    u32x4 c;
                    request(h, par, c, need);
                    w1[h] = need ? c : w1[h];
                }
                dg = ld4_sc1(rdec, 128u * (j & 1u));
                if (all_ok(dg.w == want))
                    break;
                if (round >= kResMaxRounds)
                {
                    give_up();
                    return;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            stamp(j, 1);  // "decision seen": no fold and no decide span on a box (stamps 7 and 2 keep the old layout)
            stamp(j, 7);
            stamp(j, 2);
            const uint32_t state = __builtin_amdgcn_readfirstlane(dg.z);
            if (state == kDecFailed)  // the reducer gave up (it recorded the error): x, r are not written
                return;
            alpha = __uint_as_float(__builtin_amdgcn_readfirstlane(dg.x));
            beta = __uint_as_float(__builtin_amdgcn_readfirstlane(dg.y));
            if (state != kDecGo)
            {
                go = false;
                break;
            }
        }
        else
        {
            stamp(j, 0);
            // phase j - 1's five shares of every workgroup and this box's halo granules, polled until every granule
            // carries phase j - 1's tag (each 16-B granule is one write-through store with its own tag: no counter,
            // no ordering between granules needed). Bounded: a workgroup that never publishes ends the solve
            u32x4 g[kFusedShares];
            // the five share granules of every workgroup (thread t < G: workgroup t's), polled until all carry
            // phase j - 1's tag; then this box's halo granules are requested and arrive while the shares are folded
            // and the own nodes formed (a producer stores its Ap granules before its shares, so they have nearly
            // always landed by then; a granule with another tag is read again below)
            for (;; ++round)
            {
#pragma unroll
                for (int q = 0; q < kFusedShares; ++q)
                    g[q] = ld4_sc1(rsh, tid < G ? 16u * ((par * G + tid) * kFusedShares + (uint32_t)q) : kResOob);
                bool ok = true;
#pragma unroll
                for (int q = 0; q < kFusedShares; ++q)
                    ok = ok && (tid >= G || g[q].z == want);
                if (all_ok(ok))
                    break;
                if (round >= kResMaxRounds)
                {
                    give_up();
                    return;  // x, r are not written: the solve fails
                }
                __builtin_amdgcn_s_sleep(2);
            }
#pragma unroll
            for (int h = 0; h < NPH; ++h)
                request(h, par, w1[h]);
            stamp(j, 1);
            double v[kFusedShares];
#pragma unroll
            for (int q = 0; q < kFusedShares; ++q)
                v[q] = tid < G ? __hiloint2double((int)g[q].y, (int)g[q].x) : 0.0;
            block_sum_lds<kResNT, kFusedShares>(v, red);  // fixed order: every workgroup the same totals
            if constexpr (multi)  // the rank's totals to every rank (workgroup 0), then every rank's, folded in rank order
            {
                const uint32_t nr = ra.pa.nranks, jp = j & 1u;
                if (b == 0 && tid < (uint32_t)kFusedShares)
                {
                    double t = v[0];
#pragma unroll
                    for (int q = 1; q < kFusedShares; ++q)
                        t = tid == (uint32_t)q ? v[q] : t;
                    const u32x4 w = {(uint32_t)__double2loint(t), (uint32_t)__double2hiint(t), want, 0u};
#pragma unroll
                    for (int p = 0; p < kMaxPeers; ++p)
                        if ((uint32_t)p < nr)
                            st4_sys(sized_rsrc(jp ? ra.pa.tot[p][1] : ra.pa.tot[p][0], 80u * nr),
                                    16u * (kFusedShares * ra.pa.rank + tid), w);
                }
                const __amdgpu_buffer_rsrc_t rtm = sized_rsrc(jp ? ra.pa.tot_mine[1] : ra.pa.tot_mine[0], 80u * nr);
                u32x4 gt;
                for (;; ++round)
                {
                    gt = ld4_sys(rtm, tid < kFusedShares * nr ? 16u * tid : kResOob);
                    if (all_ok(tid >= kFusedShares * nr || gt.z == want))
                        break;
                    if (round >= kResMaxRounds)
                    {
                        give_up();
                        return;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                if (tid < kFusedShares * nr)
                    rt[tid] = __hiloint2double((int)gt.y, (int)gt.x);
                lds_sync();
#pragma unroll
                for (int q = 0; q < kFusedShares; ++q)
                {
                    double t = 0.0;
                    for (uint32_t p = 0; p < nr; ++p)
                        t += rt[kFusedShares * p + q];
                    v[q] = t;
                }
            }
            stamp(j, 7);
            go = fused_decide(ra.ctl, ra.hist, j, pre, b == 0 && tid == 0, v, &alpha, &beta, j - 1u == ra.max_it);
            if (go && j - 1u == ra.max_it)  // max_iterations updates made (the host loop's last launch)
                go = false;
            if (!go)
                break;
            stamp(j, 2);
        }
        // form r_j, z_j, p_j (x_j) of the own nodes and p_j of the halo into the image. The per-node indices are
        // opaque per phase, so no address derived from them is hoisted out of the phase loop into a VGPR
#pragma unroll
        for (int u = 0; u < NPT; ++u)
            asm volatile("" : "+v"(osc[u]), "+v"(opub[u]), "+v"(on[u]));
#pragma unroll
        for (int h = 0; h < NPH; ++h)
            asm volatile("" : "+v"(hsc[h]), "+v"(hpub[h]), "+v"(hn[h]));
        double d[kFusedShares] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < NPT; ++u)
        {
            __builtin_amdgcn_sched_barrier(0);  // one node's working set at a time (no cross-node hoisting)
            if (on[u] == kResNone)
                continue;
            const uint32_t slot = osc[u] & 0xFFFFu;
            // p_(j-1): this thread formed it last phase (0 at phase 0)
            const float4 po = LST ? pl[slot] : float4{S(u, 9), S(u, 10), S(u, 11), 0.f};
            const float rr0[3] = {S(u, 0), S(u, 1), S(u, 2)}, aa0[3] = {S(u, 3), S(u, 4), S(u, 5)},
                        pp0[3] = {po.x, po.y, po.z};
            float rn[3], zz[3], pn[3];
            fused_form(czA, czB, LST ? (osc[u] >> 16) & 0xFFu : osc[u] >> 16, alpha, beta, rr0, aa0, pp0, rn, zz, pn);
#pragma unroll
            for (int c = 0; c < 3; ++c)
            {
                S(u, 6 + c) = fmaf(alpha, pp0[c], S(u, 6 + c));  // x_j = x_(j-1) + alpha_(j-1) p_(j-1)
                S(u, c) = rn[c];
                if constexpr (!LST)
                    S(u, 9 + c) = pn[c];
            }
            pl[slot] = float4{pn[0], pn[1], pn[2], 0.f};
            fused_entry_dots(rn, zz, d);
        }
        // the halo's r_j, p_j from the kept r_(j-1), p_(j-1) (phase 0: fast_fused_init's r and 0) and the Ap_(j-1)
        // granules requested above, each checked for its tag (one that had not landed is read again: a bounded, voted
        // re-read). Every pass forms from the kept values into hrn / hpn; they replace the kept ones only once the vote
        // has passed, so an entry formed on two passes takes alpha once
        bool again = ra.reread != 0u && j > 0;  // (the test knob: the first vote of the phase counts as failed)
        for (;; ++round)
        {
            bool hok = true;
#pragma unroll
            for (int h = 0; h < NPH; ++h)
            {
                if (hn[h] == kResNone)
                    continue;
                if (j > 0)
                {
                    if (w1[h].w != want)
                    {
                        hok = false;
                        continue;
                    }
                    ha[h][0] = __uint_as_float(w1[h].x), ha[h][1] = __uint_as_float(w1[h].y);
                    ha[h][2] = __uint_as_float(w1[h].z);
                }
                float zz[3];
                fused_form(czA, czB, hsc[h] >> 16, alpha, beta, hr[h], ha[h], hp[h], hrn[h], zz, hpn[h]);
                pl[hsc[h] & 0xFFFFu] = float4{hpn[h][0], hpn[h][1], hpn[h][2], 0.f};
            }
            if (j == 0)
            {
                lds_sync();  // the image complete before the rows
                break;
            }
            const bool pass = all_ok(hok);  // (its barrier also completes the image: the own entries were written before it)
            if (pass && !again)
                break;
            again = false;
            if (round >= kResMaxRounds)
            {
                give_up();
                return;
            }
#pragma unroll
            for (int h = 0; h < NPH; ++h)
                request(h, par, w1[h]);
        }
#pragma unroll
        for (int h = 0; h < NPH; ++h)
            if (hn[h] != kResNone)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    hr[h][c] = hrn[h][c], hp[h][c] = hpn[h][c];
        stamp(j, 3);
        // rows: Ap_j = K_eff p_j, the dots of the row, the box-surface nodes' Ap_j granules for the neighbours' next phase
#pragma unroll
        for (int u = 0; u < NPT; ++u)
        {
            __builtin_amdgcn_sched_barrier(0);  // one row's LDS reads in flight at a time (VGPRs)
            if (on[u] == kResNone)
                continue;
            int c0 = (int)(osc[u] & 0xFFFFu);
            asm volatile("" : "+v"(c0));  // opaque per phase: the rows' image addresses are not hoisted out of the phase
                                          // loop (56 loop-invariant addresses would pin as many VGPRs)
            const uint32_t e0 = tid + (uint32_t)u * kResNT;
            const uint32_t rw = multi ? ra.own[(size_t)b * ra.own_stride + e0].w : kResNone;  // a shard's send position
            const float4 q0 = LST ? pl[c0] : float4{S(u, 9), S(u, 10), S(u, 11), 0.f};
            const float u0[3] = {q0.x, q0.y, q0.z};
            float acc[3];
            const uint32_t cls = LST ? (osc[u] >> 16) & 0xFFu : osc[u] >> 16, ty = cls >> 3;  // boundary type
            if (ty != 13u)  // a block-surface node: its type's stencil (the cell form's pair blocks of the cells that
            {               // exist, summed per offset at plan time), every offset on its own
                const float4 *tb = tcf + (LST ? osc[u] >> 24 : ty) * (uint32_t)(E::nOff * 3);
                f2 acc01 = {0.f, 0.f};
                float acc2 = 0.f;
                const f2 u0xy = {u0[0], u0[1]};
#pragma unroll
                for (int o = 1; o < E::nOff; ++o)
                {
                    const float4 q = pl[c0 + soff[o]];
                    const f2 wxy = f2{q.x, q.y} - u0xy;
                    const float wz = q.z - u0[2];
                    const float4 b0 = tb[3 * o], b1 = tb[3 * o + 1], b2 = tb[3 * o + 2];
                    acc01 = __builtin_elementwise_fma(f2{b0.x, b0.y}, f2{wxy.x, wxy.x}, acc01);
                    acc01 = __builtin_elementwise_fma(f2{b0.z, b0.w}, f2{wxy.y, wxy.y}, acc01);
                    acc01 = __builtin_elementwise_fma(f2{b1.x, b1.y}, f2{wz, wz}, acc01);
                    acc2 = fmaf(b1.z, wxy.x, acc2);
                    acc2 = fmaf(b1.w, wxy.y, acc2);
                    acc2 = fmaf(b2.x, wz, acc2);
                }
                acc[0] = acc01.x;
                acc[1] = acc01.y;
                acc[2] = acc2;
            }
            else  // the brick rows' difference form (lattice_fused.hip rows1); the blocks as scalar loads (from LDS
            {     // as well: rows 3.5 -> 4.7 us per phase on C2)
                int zoff;
                asm volatile("s_mov_b32 %0, 0" : "=s"(zoff));
                const float *__restrict__ cf = coef + zoff;
                const f2 u0xy = {u0[0], u0[1]};
                f2 acc01 = {0.f, 0.f};
                float acc2 = 0.f;
#pragma unroll
                for (int o = 1; o < E::nOff; o += (SYM ? 2 : 1))
                {
                    f2 wxy;
                    float wz;
                    {
                        const float4 q = pl[c0 + soff[o]];
                        wxy = f2{q.x, q.y} - u0xy;
                        wz = q.z - u0[2];
                    }
                    if constexpr (SYM)
                    {
                        const float4 q = pl[c0 + soff[o + 1]];
                        wxy += f2{q.x, q.y} - u0xy;
                        wz += q.z - u0[2];
                    }
                    const float *bq = cf + 9 * o;
                    acc01 = __builtin_elementwise_fma(f2{bq[0], bq[1]}, f2{wxy.x, wxy.x}, acc01);
                    acc01 = __builtin_elementwise_fma(f2{bq[2], bq[3]}, f2{wxy.y, wxy.y}, acc01);
                    acc01 = __builtin_elementwise_fma(f2{bq[4], bq[5]}, f2{wz, wz}, acc01);
                    acc2 = fmaf(bq[6], wxy.x, acc2);
                    acc2 = fmaf(bq[7], wxy.y, acc2);
                    acc2 = fmaf(bq[8], wz, acc2);
                }
                acc[0] = acc01.x;
                acc[1] = acc01.y;
                acc[2] = acc2;
            }
            const float mm = m[u] * sM;
            float an[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                an[c] = fmaf(mm, u0[c], sK * acc[c]);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                S(u, 3 + c) = an[c];
            const float rj[3] = {S(u, 0), S(u, 1), S(u, 2)};
            float zz[3];  // z_j again from r_j (the form's arithmetic: the same bits)
            lat_z(czA[cls], czB[cls], cls, rj, zz);
            fused_row_dots(czA, czB, cls, u0, zz, an, d);
            // (r_j and p_j are not published: every reader formed them itself, from the same inputs)
            const uint32_t po = opub[u] != kResNone ? 16u * ((j & 1u) * ra.npub + opub[u]) : kResOob;
            const u32x4 g1 = {__float_as_uint(an[0]), __float_as_uint(an[1]), __float_as_uint(an[2]), ra.tag0 + j + 1u};
            st4_sc1(rpub, po, g1);
            if constexpr (multi)  // a send-plane node: its Ap_j granule into the neighbour's mailbox, at its ghost position
            {
                const uint32_t jp = j & 1u, e = rw >> 24, pos = 16u * (rw & 0xFFFFFFu);
                const __amdgpu_buffer_rsrc_t d0 = sized_rsrc(jp ? ra.pa.rdst[0][1] : ra.pa.rdst[0][0], ra.pa.rdst_bytes[0]),
                                             d1 = sized_rsrc(jp ? ra.pa.rdst[1][1] : ra.pa.rdst[1][0], ra.pa.rdst_bytes[1]);
                const uint32_t o0 = rw != kResNone && e == 0u ? pos : kResOob, o1 = rw != kResNone && e == 1u ? pos : kResOob;
                st4_sys(d0, o0, g1);
                st4_sys(d1, o1, g1);
            }
        }
        stamp(j, 4);
        block_sum_lds<kResNT, kFusedShares>(d, red);
        stamp(j, 5);
        if (tid < (uint32_t)kFusedShares)  // one tagged granule per share: {lo, hi, tag, -}
        {
            double v = d[0];
#pragma unroll
            for (int q = 1; q < kFusedShares; ++q)
                v = tid == (uint32_t)q ? d[q] : v;
            st4_sc1(rsh, 16u * (((j & 1u) * G + b) * kFusedShares + tid),
                    u32x4{(uint32_t)__double2loint(v), (uint32_t)__double2hiint(v), ra.tag0 + j + 1u, 0u});
        }
        stamp(j, 6);
    }
    // the stop at phase j: x_(j-1) and r_(j-1) (phase j made no update)
    const __amdgpu_buffer_rsrc_t wx = sized_rsrc(ra.x, vbytes), wr = sized_rsrc(ra.r, vbytes);
#pragma unroll
    for (int u = 0; u < NPT; ++u)
    {
        const uint32_t nb = on[u] != kResNone ? 12u * on[u] : 12u * kLatOob3;
        const u32x3 vx = {__float_as_uint(S(u, 6)), __float_as_uint(S(u, 7)), __float_as_uint(S(u, 8))},
                    vr = {__float_as_uint(S(u, 0)), __float_as_uint(S(u, 1)), __float_as_uint(S(u, 2))};
        __builtin_amdgcn_raw_buffer_store_b96(vx, wx, nb, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b96(vr, wr, nb, 0, 0);
    }
}

using ResidentFn = void (*)(DevSys, ResArgs, const float *);

template <bool SYM, class E, int NPT, int NPH, bool MR> Pick<ResidentFn> resident_pick()
{
    static const std::string name = kernel_name("k_pcg_resident", SYM, lat_kind<E>(), NPT, NPH, MR);
    return {k_pcg_resident<SYM, E, NPT, NPH, MR>, name.c_str()};
}

// the instantiations: <= 3 own + 2 halo entries per thread, state in registers (small: boxes of <= 1,536 nodes and
// <= 1,024 ring entries: C2's 14 x 10 x 10), or <= 4 + 3 with the state in LDS (<= 2,048 nodes, <= 1,536 entries: the
// C3 / 8 slab's 19 x 19 x 5); 2 waves per SIMD, one workgroup per CU, no scratch
Pick<ResidentFn> pick_resident(const DevSys &s, bool small, bool shard)
{
    // (the bools in this order: the code object keeps the kernels in the order it always had them)
    return with_bools(
        [](auto sm, auto mr, auto hex, auto sym) {
            return resident_pick<sym(), LatE<hex()>, sm() ? 3 : 4, sm() ? 2 : 3, mr()>();
        },
        small, shard, s.t.lhex != 0, s.t.lsym != 0);
}
inline bool resident_small(unsigned npt, unsigned nph) { return npt <= 3 && nph <= 2; }
}  // namespace

// ---- the resident solve (the kernel above): one launch per PCG solve ------------------------------------------------
size_t resident_static_lds(const DevSys &s, bool small, bool shard)
{
    hipFuncAttributes a{};
    const void *k = reinterpret_cast<const void *>(pick_resident(s, small, shard).fn);
    return hipFuncGetAttributes(&a, k) == hipSuccess ? a.sharedSizeBytes : 0;
}

int resident_blocks_per_cu(const DevSys &s, unsigned npt, unsigned nph, size_t lds, bool shard)
{
    if (npt > 4 || nph > 3)
        return 0;
    int bpc = 0;
    const ResidentFn k = pick_resident(s, resident_small(npt, nph), shard).fn;
    // the image is dynamic LDS beside ~100 KB of static arrays: allow the workgroup its size (gfx950: 160 KB)
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, k, kResNT, lds) != hipSuccess)
        return 0;
    return bpc;
}

const char *resident_kernel_name(const DevSys &s, const ResidentPlan &rp)
{
    return pick_resident(s, resident_small(rp.npt, rp.nph), rp.shard).name;
}

void launch_pcg_resident(cwf_hip_system *h, uint32_t max_it, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    ResidentPlan &rp = h->res;
    ResArgs ra{};
    ra.ctl = h->ctl;
    ra.hist = h->hist;
    ra.hdr = rp.hdr;
    ra.own = rp.own;
    ra.halo = rp.halo;
    ra.tcoef = rp.tcoef;
    ra.own_stride = rp.own_stride;
    ra.halo_stride = rp.halo_stride;
    ra.pub = rp.pub;
    ra.npub = rp.npub;
    ra.sh = rp.sh;
    ra.tag0 = h->res.tag;  // (resident.cpp advances it past this solve's phases)
    ra.x = h->x;
    ra.r = h->r;
    ra.max_it = max_it;
    if (rp.shard)
        peer_resident_args(h, ra.pa);
    else
        ra.pa = ResPeerArgs{};
    // the reducer role: CWF_RESIDENT_REDUCER 0 never, 1 wherever eligible, unset from kResReducerMinBoxes boxes
    const bool eligible = !rp.shard && rp.G >= 2u && rp.G + 1u <= rp.capacity && rp.dec_off != 0u;
    const char *rdk = knob("CWF_RESIDENT_REDUCER");
    ra.G = rp.G;
    ra.reducer = eligible && (rdk ? rdk[0] == '1' : rp.G >= kResReducerMinBoxes) ? 1u : 0u;
    ra.dec_off = rp.dec_off;
    const unsigned grid = rp.G + ra.reducer;
    // diagnostic: CWF_RESIDENT_TRACE=path appends phase CWF_FUSED_TRACE_IT's stamps, one row per workgroup (the
    // reducer's last); the buffer is the handle's, on the handle's device
    const char *tp = knob("CWF_RESIDENT_TRACE");
    if (tp && rp.trace_n < grid)
        rp.trace_n = rp.trace.alloc(8ull * grid) == hipSuccess ? grid : 0u;
    uint64_t *trace = tp && rp.trace_n >= grid ? rp.trace.get() : nullptr;
    if (trace)
    {
        const char *at = knob("CWF_FUSED_TRACE_IT");
        ra.trace = trace;
        ra.trace_j = at ? (uint32_t)atoi(at) : 50u;
        (void)hipMemsetAsync(trace, 0, 64ull * grid, st);
    }
    const char *rk = knob("CWF_RESIDENT_REREAD");  // tests/test_gpu_resident_handoff.py
    ra.reread = rk && rk[0] == '1' ? 1u : 0u;
    launch_kernel(pick_resident(h->ds, resident_small(rp.npt, rp.nph), rp.shard).fn, grid, kResNT, rp.lds, st, e0, e1,
                  h->ds, ra, h->ds.t.lcoef);
    if (trace)
    {
        std::vector<uint64_t> v(8ull * grid);
        if (hipStreamSynchronize(st) == hipSuccess &&
            hipMemcpy(v.data(), trace, v.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess)
            if (FILE *f = std::fopen(tp, "a"))
            {
                // ("reducer 1": the last row is the reducer's five stamps, the boxes' stamps 1, 7, 2 "decision seen")
                // (the box grid stays the line's last field: tools/resident_trace.py reads it there)
                std::fprintf(f, "# resident phase %u grid %u reducer %u image %u,%u lds %zu boxes %ux%ux%u\n", ra.trace_j, grid,
                             ra.reducer, rp.image[0], rp.image[1], rp.lds, rp.dims[0], rp.dims[1], rp.dims[2]);
                for (unsigned b = 0; b < grid; ++b)
                {
                    std::fprintf(f, "%u", b);
                    for (int i = 0; i < 8; ++i)
                        std::fprintf(f, " %llu", (unsigned long long)v[8ull * b + i]);
                    std::fprintf(f, "\n");
                }
                std::fclose(f);
            }
    }
}

}  // namespace cwf
