// fast_dispatch.hip -- the FAST operator of a handle: which element-pass family runs (launch_tiles over spmv_tiles.hip,
// tiles_groups.hip, tiles_hex.hip and lattice.hip; its grid and name queries), the apply path around it, and the small
// kernels of no family.
//
// k_keff_finalize (apply_keff): y = node's partials (ascending tile) + m s_M x, Dirichlet identity rows.
// k_sym_inverse, k_lat_class_inverse (fast_block_inverse): the block-Jacobi inverse packed for the update pass.
// k_halo_pack: a shard's send rows.
#include <algorithm>

#include "blockinv_pack.hpp"
#include "cwf_internal.hpp"

namespace cwf
{
namespace
{
// FAST: symmetrise the block inverse (upper triangle wins, so k_precond and the update agree) and pack
// it to 16 B per node for the update pass in the Jacobi-scaled form of blockinv_pack.hpp (fp32 scale,
// fp16 row scales and correlations; a flagged fp32 fallback for blocks that form does not hold). The
// operator the solve applies is written back to the 9-float copy, so the prologue's z (k_precond) and
// the update's z use the same symmetric preconditioner.
__global__ __launch_bounds__(256) void k_sym_inverse(uint32_t N, const uint32_t *__restrict__ mask,
                                                     float *__restrict__ inv9, float *__restrict__ inv6)
{
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= N)
        return;
    float *a = inv9 + 9ull * n;
    const float v[6] = {a[0], a[1], a[2], a[4], a[5], a[8]};  // a00 a01 a02 a11 a12 a22
    uint32_t w[4];
    float d[6];
    (void)pack_block_inverse(v, mask[n], w, d);
    a[0] = d[0];
    a[1] = a[3] = d[1];
    a[2] = a[6] = d[2];
    a[4] = d[3];
    a[5] = a[7] = d[4];
    a[8] = d[5];
    reinterpret_cast<uint4 *>(inv6)[n] = make_uint4(w[0], w[1], w[2], w[3]);
}

// a lattice handle's per-class block inverse (packed record and the 9-float operator) from one representative node
// of each class (every node of a class has the same diagonal blocks and mass: lattice.cpp)
__global__ __launch_bounds__(256) void k_lat_class_inverse(const uint32_t *__restrict__ rep,
                                                           const float *__restrict__ inv6, const float *__restrict__ inv9,
                                                           uint4 *__restrict__ cinv6, float *__restrict__ cinv9,
                                                           float4 *__restrict__ cz)
{
    for (uint32_t c = threadIdx.x; c < kLatClasses; c += 256)
    {
        const uint32_t n = rep[c];
        if (n == 0xFFFFFFFFu)
            continue;
        const uint4 iw = reinterpret_cast<const uint4 *>(inv6)[n];
        float a9[9];
        for (int q = 0; q < 9; ++q)
            a9[q] = inv9[9ull * n + q];
        cinv6[c] = iw;
        for (int q = 0; q < 9; ++q)
            cinv9[9 * c + q] = a9[q];
        // the operator k_pcg_update_tiles applies (its unpack, or the flagged block's fp32 copy)
        float bv[6];
        if ((int)iw.x >= 0)
            unpack_block_inverse(iw.y, iw.z, iw.w, __uint_as_float(iw.x), bv);
        else
        {
            bv[0] = a9[0];
            bv[1] = a9[1];
            bv[2] = a9[2];
            bv[3] = a9[4];
            bv[4] = a9[5];
            bv[5] = a9[8];
        }
        if (cz)
        {
            cz[2 * c] = float4{bv[0], bv[1], bv[2], bv[3]};
            cz[2 * c + 1] = float4{bv[4], bv[5], 0.f, 0.f};
        }
    }
}

__global__ __launch_bounds__(256) void k_halo_pack(const uint32_t *__restrict__ idx, uint64_t n,
                                                   const float *__restrict__ v, float *__restrict__ out)
{
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256ull)
    {
        const uint32_t q = idx[i];
        out[3 * i + 0] = v[3ull * q + 0];
        out[3 * i + 1] = v[3ull * q + 1];
        out[3 * i + 2] = v[3ull * q + 2];
    }
}

template <bool SANITIZE>
__global__ __launch_bounds__(256) void k_keff_finalize(DevSys s, const float *__restrict__ x, float *__restrict__ y)
{
    const DevTiles &T = s.t;
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n >= s.N)
        return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (uint32_t q = T.node_part_off[n] & kPartOffBits; q < (T.node_part_off[n + 1] & kPartOffBits); ++q)
    {
        const float *pp = T.part + 3ull * (T.node_major ? q : T.part_slot[q]);
        a0 += pp[0];
        a1 += pp[1];
        a2 += pp[2];
    }
    const uint32_t mk = s.mask[n];
    const float m = s.mass[n] * (float)s.sM;
    const float x0 = x[3u * n + 0], x1 = x[3u * n + 1], x2 = x[3u * n + 2];
    float y0 = fmaf(m, (SANITIZE && (mk & 1u)) ? 0.f : x0, a0);
    float y1 = fmaf(m, (SANITIZE && (mk & 2u)) ? 0.f : x1, a1);
    float y2 = fmaf(m, (SANITIZE && (mk & 4u)) ? 0.f : x2, a2);
    y[3u * n + 0] = (mk & 1u) ? x0 : y0;
    y[3u * n + 1] = (mk & 2u) ? x1 : y1;
    y[3u * n + 2] = (mk & 4u) ? x2 : y2;
}

// the element pass of a FAST handle with tiles: the PCG loop's (pcg) or the apply path's, by the handle's family
// (a structured block, else fan groups, else hex tiles, else tets)
void launch_tiles(const DevSys &s, const float *x, const PcgPassArgs &pa, bool pcg, bool sanitize, hipStream_t st,
                  hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr)
{
    const DevTiles &t = s.t;
    if (t.lat)
        launch_lattice(s, x, pa, pcg, sanitize, st, e0, e1);
    else if (t.grp)
        launch_groups(s, x, pa, pcg, sanitize, st, e0, e1);
    else if (t.hex)
        launch_hex_tiles(s, x, pa, pcg, sanitize, st, e0, e1);
    else
        launch_tet_tiles(s, x, pa, pcg, sanitize, st, e0, e1);
}
}  // namespace

unsigned fast_tile_blocks(const DevSys &s)
{
    return s.t.lat ? s.t.lnwork : (s.t.pipe || s.t.hex) ? s.t.pipe_grid : s.t.ntiles;
}

unsigned fast_pipe_grid(const DevSys &s)
{
    return s.t.grp ? groups_pipe_grid(s) : s.t.hex ? hex_tiles_pipe_grid(s) : tet_tiles_pipe_grid(s);
}

// the PCG loop's instantiation of the two-kernel element pass, by name (cwf_hip_system_keff_kernel)
const char *fast_tiles_kernel_name(const DevSys &s)
{
    const DevTiles &t = s.t;
    return t.lat   ? lattice_kernel_name(s)
           : t.grp ? groups_kernel_name(s)
           : t.hex ? hex_tiles_kernel_name(s)
                   : tet_tiles_kernel_name(s);
}

void fast_keff_ds(const DevSys &s, const float *x, float *y, bool sanitize, hipStream_t st)
{
    if (s.N == 0)
        return;
    fast_keff_partials_ds(s, x, sanitize, st);
    const unsigned g = grid_for(s.N, 256);
    if (sanitize)
        k_keff_finalize<true><<<g, 256, 0, st>>>(s, x, y);
    else
        k_keff_finalize<false><<<g, 256, 0, st>>>(s, x, y);
}

void fast_keff_partials_ds(const DevSys &s, const float *x, bool sanitize, hipStream_t st)
{
    if (s.N == 0 || !s.t.ntiles)
        return;
    launch_tiles(s, x, PcgPassArgs{}, false, sanitize, st);
}

// iteration `it`: residual step of it-1's update (beta, convergence) + p_new + tile partials + p.Ap shares
void fast_tiles_pcg(cwf_hip_system *h, unsigned it, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    const DevSys &s = h->ds;
    if (!s.t.ntiles)
        return;
    const unsigned abl = 0u;
    // beta / convergence: a single handle folds the update kernel's per-workgroup {r.r, r.z} shares
    // directly; a shard reads the all-gathered per-rank pairs
    // lzr: the lattice kernel forms z from r (pa.z carries r)
    const float *pz = s.t.lzr ? h->r : h->z;
    const PcgPassArgs pa = fast_direct_fold(h)
                               ? PcgPassArgs{pz, h->ctl, h->part0, h->part1, h->part2,
                                             fast_update_blocks(s, it && x_flush_iter(it - 1u)), 1u, it, h->hist, abl,
                                             fast_p_new(h, it)}
                               : PcgPassArgs{pz, h->ctl, h->part0, h->g_rrz, h->g_rrz + 1,
                                             (unsigned)h->nranks, 2u, it, h->hist, abl, fast_p_new(h, it)};
    launch_tiles(s, fast_p_old(h, it), pa, true, false, st, e0, e1);
}

// diagnostic: `reps` PCG-mode tiles launches with side-effect-free preambles (ablation bits | 32)
void fast_tiles_pcg_dry(cwf_hip_system *h, unsigned abl, int reps, hipStream_t st)
{
    const DevSys &s = h->ds;
    const PcgPassArgs pa{s.t.lzr ? h->r : h->z, h->ctl, h->part0, h->g_rrz, h->g_rrz + 1, (unsigned)h->nranks, 2u, 1u,
                         h->hist, abl | 32u};
    for (int i = 0; i < reps; ++i)
        launch_tiles(s, h->p, pa, true, false, st);
}

void fast_block_inverse(cwf_hip_system *h, hipStream_t st)
{
    if (h->inv_fast && h->inv_sK == h->ds.sK && h->inv_sM == h->ds.sM)
        return;  // built for these scalars (C2: one 350-us fp64 setup per Newmark step saved)
    h->inv_fast = true;
    h->inv_sK = h->ds.sK;
    h->inv_sM = h->ds.sM;
    if (h->ds.hex)
        hex_block_jacobi(h, h->inv, st);
    else
        parity_block_jacobi(h, h->inv, st);
    if (h->ds.N)
        k_sym_inverse<<<grid_for(h->ds.N, 256), 256, 0, st>>>(h->ds.N, h->ds.mask, h->inv, h->inv6);
    if (h->ds.t.lcls)  // structured block: one representative node per (boundary class, mask)
        k_lat_class_inverse<<<1, 256, 0, st>>>(h->ds.t.lrep, h->inv6, h->inv, h->ds.t.lcinv6, h->ds.t.lcinv9,
                                               h->ds.t.lcz);
}

void halo_pack(cwf_hip_system *h, const float *v, hipStream_t st, float *dst)
{
    if (!h->nsend)
        return;
    const uint64_t g = std::min<uint64_t>((h->nsend + 255) / 256, 1024);
    k_halo_pack<<<(unsigned)g, 256, 0, st>>>(h->send_idx, h->nsend, v, dst ? dst : h->sendbuf);
}
}  // namespace cwf
