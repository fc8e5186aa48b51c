// lattice.hip -- k_keff_lattice and k_keff_lattice_layered, the FAST K_eff of a structured Kuhn block (lattice.cpp).
// They share residual_step, block_sum, load3 and the PcgArgs contract of the tiles kernels (fast_common.hpp).
//
// Node-centric and HBM-streaming: every owned node's row is the Kuhn stencil of its neighbours, so no element
// record, partial run or fold exists; per node the kernel reads z and p_old (PCG; x for apply_keff) and the mass,
// and writes the new p and one 12-B row value Ap (the "partial" of a run of length one: the update pass and
// k_keff_finalize read it through node_part_off[n] = n).
//
// Rows, in difference form (lattice.cpp): the rows of K annihilate rigid translations, so
//   (K u)_n = sum_(d != 0) S_d (u_(n+d) - u_n),
// each fp32 term strain-sized as in the element loop (pcg.cpp:622-651 forms B u), never a near-cancelling sum
// of |S_0 u_n|-sized terms (which costs the low modes their accuracy in fp32). When S_(-d) = S_d (an isotropic
// block; SYM) the 14 off-centre blocks pair up: sum over the 7 directions of S_d ((u_(n+d) - u_n) + (u_(n-d) -
// u_n)). Nodes on the block's surface (which miss cells) are not in any brick: the first lnsb workgroups form their
// rows one node per thread in the cell form (lattice_shell_node), so the bricks carry no boundary branch at all
// (surface corrections inside the bricks cost C3 31 of 68 us: every brick at i = 0 or nx - 1 has them in every
// wave).
//
// Work item = a BX x BY = 32 x 8 (i, j) column brick of the strict interior times L consecutive k planes (16 x 16
// bricks load 5% fewer halo entries on C3 and 12% fewer on C2, but ran C3 15% and C2 3% slower, same box). A 256-thread workgroup
// (one thread per column) marches k two planes per step: each thread forms the rows of its column's nodes in
// planes k and k + 1, one plane at a time, from LDS planes k - 1 .. k + 2 of (BX + 2) x (BY + 2) nodes (the brick
// plus its one-node halo, float4 {u_x, u_y, u_z, mass}) in a ring of 6; planes k + 1 and k + 2 are formed in LDS
// at the step's start (p = z + beta p_old: the p-update pass fused as in the tiles kernels; or the sanitised x),
// planes k + 3 and k + 4 are loaded into registers during the step. One barrier per step. The blocks are
// workgroup-uniform (scalar loads). When every strict-interior node has the same lumped mass (MU, checked at
// create) no mass is read: the rows take it from the kernel argument. Work items are numbered i-brick fastest,
// then j-brick, then k-chunk, and workgroup b runs on XCD b mod 8 and takes that XCD's contiguous share of the
// items, so bricks that share halo rows share an L2.
//
// Every global load and store is unconditional: a load or store in a branch makes the waitcnt pass merge its
// counters pessimistically, and the vmcnt(0) it then emits drains the prefetched planes. Lanes with nothing to
// move address past the end of a range-checked buffer descriptor instead: such a load returns 0 and such a store
// is dropped, without memory traffic. coef and plane are restrict kernel arguments (scalar loads): a vector load
// issued after the prefetch and consumed before it would drain it too (vmcnt retires in order).
#include "fast_common.hpp"

namespace cwf
{
namespace
{
// one plane of the brick's halo region in registers: entries e = threadIdx.x + kLatNT u (u = 0, 1; e < PLANE)
struct LatFill
{
    float a[2][3];  // z (PCG; r with ZR) or x (apply)
    float b[2][3];  // p_old (PCG)
    float m[2];     // mass (PCG: rides in the LDS entry's w)
    uint32_t c[2];  // ZR: the node's class byte
};

// The surface shell (lattice_plan): one node per thread, its row in the cell form (each existing cell's blocks on
// the differences to the node's own value; cells outside the block do not exist), from direct gathers of its
// neighbours' z / p_old (p formed as in the bricks) or x. Only ~4% of C3's nodes (11% of C2's).
//
// LAY (a layered block, lattice.cpp): each existing cell's pair blocks come from the table of that cell's material,
// the layer above the node's plane for corner positions with z-bit 0 and the layer below for z-bit 1 (lay[k] >> 16 is
// the material slot of the layer above plane k). The tables depend on the node's plane, which differs between the
// lanes of a shell workgroup, but only over the few planes [ka, kb] the workgroup's nodes lie in (workgroup-uniform,
// from its first and last node). So after the batch's gathers are issued, the rows are accumulated in a uniform loop
// over those planes, each pass with its plane's two tables as scalar loads and only that plane's lanes taking part:
// the blocks stay in SGPRs as in the one-material form (as per-lane vector loads, 342 to 504 of them per node, they
// took the kernel to 256 VGPRs and one wave per SIMD, bricks included). A lane's arithmetic and its order are the
// one-material form's.
__device__ __forceinline__ int lattice_shell_plane(const DevTiles &T, uint32_t q)
{
    const uint32_t full = T.lnx * T.lny, per = 2u * T.lnx + 2u * (T.lny - 2u);
    const uint32_t nlo = T.lk0 == 0 ? full : 0u, nmid = (T.lkI1 - T.lkI0) * per;
    return q < nlo ? 0 : q - nlo < nmid ? (int)(T.lkI0 + (q - nlo) / per) : (int)T.lnz - 1;
}

template <int MODE, bool SANITIZE, class E, bool ZR, bool AFF, bool LAY = false>
__device__ __forceinline__ double lattice_shell_node(const DevSys &s, const float *__restrict__ x, const PcgArgs &pa,
                                                     const float *__restrict__ coef,
                                                     const uint32_t *__restrict__ plane, uint32_t q, float beta,
                                                     const float4 *czA, const float2 *czB,
                                                     const uint32_t *__restrict__ lay = nullptr, int ka = 0, int kb = 0)
{
    const DevTiles &T = s.t;
    const int nx = (int)T.lnx, ny = (int)T.lny, nz = (int)T.lnz;
    // q -> (i, j, k): a full plane k = 0 (when computed), the perimeters of the interior planes, a full plane nz - 1
    int i, j, k;
    uint32_t r = q;
    const uint32_t full = (uint32_t)(nx * ny), per = (uint32_t)(2 * nx + 2 * (ny - 2));
    const uint32_t nlo = T.lk0 == 0 ? full : 0u, nmid = (T.lkI1 - T.lkI0) * per;
    if (r < nlo)
    {
        k = 0;
        i = (int)(r % (uint32_t)nx);
        j = (int)(r / (uint32_t)nx);
    }
    else if ((r -= nlo) < nmid)
    {
        k = (int)(T.lkI0 + r / per);
        r %= per;
        if (r < (uint32_t)nx)
            i = (int)r, j = 0;
        else if (r < 2u * nx)
            i = (int)r - nx, j = ny - 1;
        else if (r < 2u * nx + (uint32_t)(ny - 2))
            i = 0, j = 1 + (int)r - 2 * nx;
        else
            i = nx - 1, j = 1 + (int)r - 2 * nx - (ny - 2);
    }
    else
    {
        r -= nmid;
        k = nz - 1;
        i = (int)(r % (uint32_t)nx);
        j = (int)(r / (uint32_t)nx);
    }
    // the three plane bases the node's offsets reach, loaded together (one round trip; plane[] is a per-lane
    // vector load here)
    const uint32_t pk[3] = {lat_plane<AFF>(T, plane, max(k - 1, 0)), lat_plane<AFF>(T, plane, k),
                            lat_plane<AFF>(T, plane, min(k + 1, nz - 1))};
    const uint32_t n = pk[1] + (uint32_t)(j * nx + i);
    if (n >= s.Nown)
        return 0.0;
    // raw gathers (12-B buffer loads; z and p_old, or x) of a batch of offsets are all issued before any is used:
    // one batch of all 14 Kuhn offsets with the node's own values (one round trip), two of 13 for hex8 (VGPRs)
    const uint32_t vbytes = 12u * s.N;
    const __amdgpu_buffer_rsrc_t rz = sized_rsrc(MODE == 1 ? pa.z : x, vbytes), rx = sized_rsrc(x, vbytes),
                                 rcls = sized_rsrc(T.lcls, ZR ? s.N : 0u);
    const auto node_at = [&](int o) {
        const int ii = min(max(i + E::off[o][0], 0), nx - 1), jj = min(max(j + E::off[o][1], 0), ny - 1),
                  kk = min(max(k + E::off[o][2], 0), nz - 1);
        return pk[kk - k + 1] + (uint32_t)(jj * nx + ii);
    };
    const auto cls_at = [&](uint32_t m) {
        return ZR ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rcls, m, 0, 0) : 0u;
    };
    const auto form = [&](uint32_t m, uint32_t cl, const float a[3], const float b[3], float u[3]) {
        float zz[3] = {a[0], a[1], a[2]};
        if constexpr (ZR)
            lat_z(czA[cl], czB[cl], cl, a, zz);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            u[c] = MODE == 1 ? fmaf(beta, b[c], zz[c]) : zz[c];
        if constexpr (MODE == 0 && SANITIZE)
        {
            const uint32_t mk = s.mask[m];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                u[c] = (mk >> c) & 1u ? 0.f : u[c];
        }
    };
    float w8[8];
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8)
    {
        const int cx = c8 & 1, cy = (c8 >> 1) & 1, cz = (c8 >> 2) & 1;
        // the cell at corner position c8 (cell index (i - cx, j - cy, k - cz)) exists inside the block
        w8[c8] = (cx ? i >= 1 : i + 1 < nx) && (cy ? j >= 1 : j + 1 < ny) && (cz ? k >= 1 : k + 1 < nz) ? 1.f : 0.f;
    }
    constexpr int BATCH = ZR ? 7 : E::nOff <= 15 ? E::nOff - 1 : (E::nOff - 1) / 2;
    float a0[3], b0[3] = {0.f, 0.f, 0.f};
    load3(rz, n, a0);
    if constexpr (MODE == 1)
        load3(rx, n, b0);
    const uint32_t c0 = cls_at(n);
    const float mass = MODE == 1 ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                                       sized_rsrc(s.mass, 4u * s.N), 4u * n, 0, 0))
                                 : 0.f;
    float u0[3];
    float acc[3] = {0.f, 0.f, 0.f};
    // offset-major (for each offset, the blocks of the existing cells that pair the node with it, each weighted
    // 0 / 1), in batches
#pragma unroll
    for (int bt = 0; bt < (E::nOff - 1 + BATCH - 1) / BATCH; ++bt)
    {
        uint32_t mo[BATCH], mc[BATCH];
        float ra[BATCH][3], rb[BATCH][3];
#pragma unroll
        for (int q7 = 0; q7 < BATCH; ++q7)
        {
            if (1 + BATCH * bt + q7 >= E::nOff)
                continue;
            mo[q7] = node_at(1 + BATCH * bt + q7);
            load3(rz, mo[q7], ra[q7]);
            if constexpr (MODE == 1)
                load3(rx, mo[q7], rb[q7]);
            mc[q7] = cls_at(mo[q7]);
        }
        if (bt == 0)
            form(n, c0, a0, b0, u0);
        if constexpr (!LAY)
        {
#pragma unroll
        for (int q7 = 0; q7 < BATCH; ++q7)
        {
            const int o = 1 + BATCH * bt + q7;
            if (o >= E::nOff)
                continue;
            float d[3];
            form(mo[q7], mc[q7], ra[q7], MODE == 1 ? rb[q7] : ra[q7], d);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                d[c] -= u0[c];
#pragma unroll
            for (int p = 0; p < E::nPairs; ++p)
            {
                if (E::pairOff[p] != o)
                    continue;
                float t[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        t[rr] = fmaf(coef[E::coefPairs + 9 * p + 3 * rr + c], d[c], t[rr]);
#pragma unroll
                for (int rr = 0; rr < 3; ++rr)
                    acc[rr] = fmaf(w8[E::pair[p][0]], t[rr], acc[rr]);
            }
        }
        }
        else
        {
            // the same rows, plane by plane: pass kk takes the tables of the cells above (pb0) and below (pb1) plane
            // kk, as scalars, and the lanes of that plane accumulate
            float dd[BATCH][3];
#pragma unroll
            for (int q7 = 0; q7 < BATCH; ++q7)
            {
                if (1 + BATCH * bt + q7 >= E::nOff)
                    continue;
                form(mo[q7], mc[q7], ra[q7], MODE == 1 ? rb[q7] : ra[q7], dd[q7]);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    dd[q7][c] -= u0[c];
            }
            const uint32_t tb = (T.llayers & 0xFFFFu) * (9u * E::nOff), ts = 9u * E::nPairs, mm = (T.llayers >> 16) - 1u;
            for (int kk = ka; kk <= kb; ++kk)
            {
                const uint32_t pb0 = tb + __builtin_amdgcn_readfirstlane(min(lay[kk] >> 16, mm)) * ts,
                               pb1 = tb + __builtin_amdgcn_readfirstlane(min(lay[max(kk - 1, 0)] >> 16, mm)) * ts;
                if (k != kk)
                    continue;
#pragma unroll
                for (int q7 = 0; q7 < BATCH; ++q7)
                {
                    const int o = 1 + BATCH * bt + q7;
                    if (o >= E::nOff)
                        continue;
#pragma unroll
                    for (int p = 0; p < E::nPairs; ++p)
                    {
                        if (E::pairOff[p] != o)
                            continue;
                        const float *__restrict__ blk = coef + ((E::pair[p][0] >> 2) & 1 ? pb1 : pb0) + 9 * p;
                        float t[3] = {0.f, 0.f, 0.f};
#pragma unroll
                        for (int rr = 0; rr < 3; ++rr)
#pragma unroll
                            for (int c = 0; c < 3; ++c)
                                t[rr] = fmaf(blk[3 * rr + c], dd[q7][c], t[rr]);
#pragma unroll
                        for (int rr = 0; rr < 3; ++rr)
                            acc[rr] = fmaf(w8[E::pair[p][0]], t[rr], acc[rr]);
                    }
                }
            }
        }
    }
    const float sK = (float)s.sK, m = mass * (float)s.sM;
    float a[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        a[c] = fmaf(m, u0[c], sK * acc[c]);
    T.part[3u * n + 0] = a[0];
    T.part[3u * n + 1] = a[1];
    T.part[3u * n + 2] = a[2];
    if constexpr (MODE == 1)
    {
        if (pa.pnew)
        {
            pa.pnew[3u * n + 0] = u0[0];
            pa.pnew[3u * n + 1] = u0[1];
            pa.pnew[3u * n + 2] = u0[2];
        }
        return (double)fmaf(u0[2], a[2], fmaf(u0[1], a[1], u0[0] * a[0]));
    }
    return 0.0;
}

// The kernel's statements are in lattice_body.inc, shared with k_keff_lattice_layered below by inclusion: this
// kernel compiles from the statements it always had (a shared __device__ function took its instantiations to other
// register allocations: VGPRs +-1..3, other SGPR spills).
template <int MODE, bool SANITIZE, bool SYM, class E, bool MU, bool ZR, bool AFF>
__global__ __launch_bounds__(kLatNT) void k_keff_lattice(DevSys s, const float *__restrict__ x, PcgArgs pa,
                                                         const float *__restrict__ coef,
                                                         const uint32_t *__restrict__ plane)
{
    constexpr bool LAY = false;
    constexpr const uint32_t *lay = nullptr;
#include "lattice_body.inc"
}

// layered blocks (one material per k-layer of cells): coef holds a stencil table per plane class and a cell-pair
// table per material, lay[k] (the words behind those tables, as an argument of its own so that it is a restrict
// pointer) the class of plane k and the material of the layer above it
template <int MODE, bool SANITIZE, class E, bool AFF>
__global__ __launch_bounds__(kLatNT) void k_keff_lattice_layered(DevSys s, const float *__restrict__ x, PcgArgs pa,
                                                                 const float *__restrict__ coef,
                                                                 const uint32_t *__restrict__ plane,
                                                                 const uint32_t *__restrict__ lay)
{
    // unpaired rows (SYM needs S_(-d) = S_d), per-node mass, z stored by the update pass
    constexpr bool LAY = true, SYM = false, MU = false, ZR = false;
#include "lattice_body.inc"
}

using LatticeFn = void (*)(DevSys, const float *, PcgArgs, const float *, const uint32_t *);
using LayeredFn = void (*)(DevSys, const float *, PcgArgs, const float *, const uint32_t *, const uint32_t *);

template <int MODE, bool SAN, bool SYM, class E, bool MU, bool ZR, bool AFF>
Pick<LatticeFn> lattice_pick()
{
    static const std::string name = kernel_name("k_keff_lattice", MODE, SAN, SYM, lat_kind<E>(), MU, ZR, AFF);
    return {k_keff_lattice<MODE, SAN, SYM, E, MU, ZR, AFF>, name.c_str()};
}

// The PCG loop (pcg) takes z from r when lzr (then pa.z is r) and the strict interior's one mass when lmu; the apply
// path keeps the per-node mass and reads x. The affine instantiations only for the PCG loop (apply_keff is not a hot
// path); only the apply path sanitises
Pick<LatticeFn> pick_lattice(const DevSys &s, bool pcg, bool sanitize)
{
    return with_bools(
        [](auto pc, auto san, auto sym, auto hex, auto mu, auto zr, auto aff) {
            return lattice_pick<pc() ? 1 : 0, !pc() && san(), sym(), LatE<hex()>, pc() && mu(), pc() && mu() && zr(),
                                pc() && aff()>();
        },
        pcg, sanitize, s.t.lsym != 0, s.t.lhex != 0, s.t.lmu != 0, s.t.lzr != 0, s.t.lpstride != 0);
}

template <int MODE, bool SAN, class E, bool AFF> Pick<LayeredFn> layered_pick()
{
    static const std::string name = kernel_name("k_keff_lattice_layered", MODE, SAN, lat_kind<E>(), AFF);
    return {k_keff_lattice_layered<MODE, SAN, E, AFF>, name.c_str()};
}

Pick<LayeredFn> pick_lattice_layered(const DevSys &s, bool pcg, bool sanitize)
{
    return with_bools(
        [](auto pc, auto san, auto hex, auto aff) {
            return layered_pick<pc() ? 1 : 0, !pc() && san(), LatE<hex()>, pc() && aff()>();
        },
        pcg, sanitize, s.t.lhex != 0, s.t.lpstride != 0);
}
}  // namespace

void launch_lattice(const DevSys &s, const float *x, const PcgPassArgs &pa, bool pcg, bool sanitize, hipStream_t st,
                    hipEvent_t e0, hipEvent_t e1)
{
    const DevTiles &t = s.t;
    if (t.llayers)
        launch_kernel(pick_lattice_layered(s, pcg, sanitize).fn, t.lnwork, kLatNT, 0, st, e0, e1, s, x, PcgArgs{pa},
                      t.lcoef, t.lplane, lattice_layers(t));
    else
        launch_kernel(pick_lattice(s, pcg, sanitize).fn, t.lnwork, kLatNT, 0, st, e0, e1, s, x, PcgArgs{pa}, t.lcoef,
                      t.lplane);
}

const char *lattice_kernel_name(const DevSys &s)
{
    return s.t.llayers ? pick_lattice_layered(s, true, false).name : pick_lattice(s, true, false).name;
}

}  // namespace cwf
