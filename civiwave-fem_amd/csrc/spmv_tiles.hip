// spmv_tiles.hip -- the FAST K_eff element pass over tiles of linear tets, one tet per lane.
//
// k_keff_tiles_pipe (persistent, XCD-aware, software-pipelined; tiles of <= 2 NT Morton-ordered tets and <= NT
// nodes; the per-tet path of a mesh without fan groups):
//   a) tile-node phase: the node's coordinates and value go to LDS: x (apply_keff) or, inside PCG, the new
//      search direction p = z + beta p_old formed on the fly (the p-update pass of pcg.cpp:897-914 is
//      fused here); the next tile's records are already in flight;
//   b) element phase: 8-B corner-id records, gradients and volume recomputed from the tile-relative
//      coordinates (cofactor rows, one stress scale), fp32 strain -> stress -> 12 nodal forces, each
//      corner's 3 forces pushed to its position in the tile's local CSR (epos);
//   c) fold phase: every tile node sums its contiguous run (ascending element, deterministic, no atomics)
//      and stores a 12-B partial at its node-major slot; PCG adds the tile's fp64 share of p.Ap.
// k_keff_tiles: one workgroup per tile, 48-B gradient records and a local-CSR fold; the path for meshes
//   without coordinates that reproduce their gradients.
// The pickers of both and what fast_dispatch.hip needs of them (launch, name, grid) are at the end.
#include "fast_common.hpp"

namespace cwf
{
namespace
{
// value of one tile node: x (apply, optionally sanitised) or p_new = z + beta p_old (PCG)
template <bool SANITIZE, int MODE>
__device__ __forceinline__ void gather_node(const DevSys &s, const float *__restrict__ x, const float *__restrict__ z,
                                            float beta, uint32_t g, float u[3])
{
    if constexpr (MODE == 1)
    {
        // constrained dofs stay 0 (z_c = 0, p_c = 0)
        u[0] = fmaf(beta, x[3u * g + 0], z[3u * g + 0]);
        u[1] = fmaf(beta, x[3u * g + 1], z[3u * g + 1]);
        u[2] = fmaf(beta, x[3u * g + 2], z[3u * g + 2]);
    }
    else
    {
        u[0] = x[3u * g + 0];
        u[1] = x[3u * g + 1];
        u[2] = x[3u * g + 2];
        if constexpr (SANITIZE)
        {
            const uint32_t mk = s.mask[g];
            u[0] = (mk & 1u) ? 0.f : u[0];
            u[1] = (mk & 2u) ? 0.f : u[1];
            u[2] = (mk & 4u) ? 0.f : u[2];
        }
    }
}

// strain -> stress -> 12 nodal forces of one tet from its corner gradients g[12] (corner-major xyz), its
// local corner ids and V s_K; corner values from LDS, forces stored to LDS as f[12][kTileElems]
// (fp32 counterpart of pcg.cpp:140-220)
template <bool ISO>
__device__ __forceinline__ void element_force_values(const DevSys &s, const float g[12], const uint32_t li[4], float vol,
                                                     uint32_t mi, const float *sp, uint32_t ms, const float *dtab,
                                                     float f[12])
{
    constexpr int kTab = ISO ? 12 : 36;
    float eps[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 4; ++a)
    {
        const float u0 = sp[li[a]], u1 = sp[ms + li[a]], u2 = sp[2 * ms + li[a]];
        const float gx = g[3 * a], gy = g[3 * a + 1], gz = g[3 * a + 2];
        eps[0] = fmaf(gx, u0, eps[0]);
        eps[1] = fmaf(gy, u1, eps[1]);
        eps[2] = fmaf(gz, u2, eps[2]);
        eps[3] = fmaf(gx, u1, fmaf(gy, u0, eps[3]));
        eps[4] = fmaf(gy, u2, fmaf(gz, u1, eps[4]));
        eps[5] = fmaf(gx, u2, fmaf(gz, u0, eps[5]));
    }
    float sig[6];
    if (mi < (uint32_t)kMaxM)
        stress_f32<ISO>(dtab + kTab * mi, eps, sig);
    else
    {
        float tab[36];
        for (int t = 0; t < kTab; ++t)
            tab[t] = (float)s.dmat[36u * mi + dsrc(ISO, t)];
        stress_f32<ISO>(tab, eps, sig);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
    {
        const float ax = g[3 * a], ay = g[3 * a + 1], az = g[3 * a + 2];
        f[3 * a + 0] = vol * fmaf(az, sig[5], fmaf(ay, sig[3], ax * sig[0]));
        f[3 * a + 1] = vol * fmaf(az, sig[4], fmaf(ax, sig[3], ay * sig[1]));
        f[3 * a + 2] = vol * fmaf(ax, sig[5], fmaf(ay, sig[4], az * sig[2]));
    }
}

template <bool ISO>
__device__ __forceinline__ void element_forces(const DevSys &s, const float g[12], const uint32_t li[4], float vol,
                                               uint32_t mi, uint32_t j, const float *sp, uint32_t ms,
                                               const float *dtab, float *sf)
{
    float f[12];
    element_force_values<ISO>(s, g, li, vol, mi, sp, ms, dtab, f);
#pragma unroll
    for (int c = 0; c < 12; ++c)
        sf[c * kTileElems + j] = f[c];
}

// 48-B record {idx01, idx23, g0x, g0y}{g0z g1x g1y g1z}{g2x g2y g2z vol}: gradients as stored
__device__ __forceinline__ void record_geometry(uint4 q0, uint4 q1, uint4 q2, float g[12], uint32_t li[4], float *vol)
{
    g[0] = __uint_as_float(q0.z);
    g[1] = __uint_as_float(q0.w);
    g[2] = __uint_as_float(q1.x);
    g[3] = __uint_as_float(q1.y);
    g[4] = __uint_as_float(q1.z);
    g[5] = __uint_as_float(q1.w);
    g[6] = __uint_as_float(q2.x);
    g[7] = __uint_as_float(q2.y);
    g[8] = __uint_as_float(q2.z);
    g[9] = -(g[0] + g[3] + g[6]);
    g[10] = -(g[1] + g[4] + g[7]);
    g[11] = -(g[2] + g[5] + g[8]);
    li[0] = q0.x & 0xffffu;
    li[1] = q0.x >> 16;
    li[2] = q0.y & 0xffffu;
    li[3] = q0.y >> 16;
    *vol = __uint_as_float(q2.w);
}

// on-the-fly geometry of a linear tet from its corner coordinates (tile-relative f32, staged in LDS):
// with edge columns c_k = x_k - x_0, the rows of [c1 c2 c3]^-1 are the gradients of N_1..N_3
// (r1 = c2 x c3 / det, r2 = c3 x c1 / det, r3 = c1 x c2 / det), grad N_0 = -(r1 + r2 + r3) and
// V = |det| / 6 -- the quantities preprocess.cpp:284-379 tabulates, recomputed instead of streamed
__device__ __forceinline__ void coord_geometry(uint2 id, const float *sx, uint32_t ms, float g[12], uint32_t li[4],
                                               float *vol)
{
    li[0] = id.x & 0xffffu;
    li[1] = id.x >> 16;
    li[2] = id.y & 0xffffu;
    li[3] = id.y >> 16;
    float c[3][3];  // c[k] = x_{k+1} - x_0
    const float x0 = sx[li[0]], y0 = sx[ms + li[0]], z0 = sx[2 * ms + li[0]];
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        c[k][0] = sx[li[k + 1]] - x0;
        c[k][1] = sx[ms + li[k + 1]] - y0;
        c[k][2] = sx[2 * ms + li[k + 1]] - z0;
    }
    float r[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        const float *u = c[(k + 1) % 3], *v = c[(k + 2) % 3];
        r[k][0] = u[1] * v[2] - u[2] * v[1];
        r[k][1] = u[2] * v[0] - u[0] * v[2];
        r[k][2] = u[0] * v[1] - u[1] * v[0];
    }
    const float det = c[0][0] * r[0][0] + c[0][1] * r[0][1] + c[0][2] * r[0][2];
    const float inv = 1.0f / det;
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        g[3 * (k + 1) + 0] = r[k][0] * inv;
        g[3 * (k + 1) + 1] = r[k][1] * inv;
        g[3 * (k + 1) + 2] = r[k][2] * inv;
    }
    g[0] = -(g[3] + g[6] + g[9]);
    g[1] = -(g[4] + g[7] + g[10]);
    g[2] = -(g[5] + g[8] + g[11]);
    *vol = fabsf(det) * (1.0f / 6.0f);
}

// Pipelined-kernel element body (GEO). With edge columns c_k = x_k - x_0 and r_k their cofactor rows
// (r_1 = c_2 x c_3, ...), the gradients are g_a = r_a / det and V = |det| / 6, so
//   f_a = V B(g_a)^T D B(g) u = B(r_a)^T D (sum_b B(r_b) u_b) * s_K / (6 |det|):
// the strain is built from the unscaled r_a and ONE scale lands on the 6 stresses (no per-gradient
// division, no per-force volume multiply). FAST arithmetic: FMA contractions and the hardware
// reciprocal (1 ulp), tolerance-checked against the oracle.
// the element body from register operands: corners X[a] = {x, y, z, p_x}, Q[a] = {p_y, p_z}
template <bool ISO>
__device__ __forceinline__ void tet_forces_reg(const DevSys &s, const float4 X[4], const float2 Q[4], float sK6,
                                               uint32_t mi, const float *dtab, float f[12])
{
    constexpr int kTab = ISO ? 12 : 36;
    float c[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        c[k][0] = X[k + 1].x - X[0].x;
        c[k][1] = X[k + 1].y - X[0].y;
        c[k][2] = X[k + 1].z - X[0].z;
    }
    float g[4][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        const float *u = c[(k + 1) % 3], *v = c[(k + 2) % 3];
        g[k + 1][0] = fmaf(u[1], v[2], -u[2] * v[1]);
        g[k + 1][1] = fmaf(u[2], v[0], -u[0] * v[2]);
        g[k + 1][2] = fmaf(u[0], v[1], -u[1] * v[0]);
    }
    const float det = fmaf(c[0][0], g[1][0], fmaf(c[0][1], g[1][1], c[0][2] * g[1][2]));
    const float scale = sK6 * __builtin_amdgcn_rcpf(fabsf(det));
#pragma unroll
    for (int q = 0; q < 3; ++q)
        g[0][q] = -(g[1][q] + g[2][q] + g[3][q]);
    float eps[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 4; ++a)
    {
        const float u0 = X[a].w, u1 = Q[a].x, u2 = Q[a].y;
        const float gx = g[a][0], gy = g[a][1], gz = g[a][2];
        eps[0] = fmaf(gx, u0, eps[0]);
        eps[1] = fmaf(gy, u1, eps[1]);
        eps[2] = fmaf(gz, u2, eps[2]);
        eps[3] = fmaf(gx, u1, fmaf(gy, u0, eps[3]));
        eps[4] = fmaf(gy, u2, fmaf(gz, u1, eps[4]));
        eps[5] = fmaf(gx, u2, fmaf(gz, u0, eps[5]));
    }
    float sig[6];
    if (s.M == 1)  // uniform branch: D from the kernel arguments (SGPR operands, no LDS reads)
        stress_f32<ISO>(s.d1, eps, sig);
    else if (mi < (uint32_t)kMaxM)
        stress_f32<ISO>(dtab + kTab * mi, eps, sig);
    else
    {
        float tab[36];
        for (int t = 0; t < kTab; ++t)
            tab[t] = (float)s.dmat[36u * mi + dsrc(ISO, t)];
        stress_f32<ISO>(tab, eps, sig);
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
        sig[r] *= scale;
#pragma unroll
    for (int a = 0; a < 4; ++a)
    {
        const float ax = g[a][0], ay = g[a][1], az = g[a][2];
        f[3 * a + 0] = fmaf(az, sig[5], fmaf(ay, sig[3], ax * sig[0]));
        f[3 * a + 1] = fmaf(az, sig[4], fmaf(ax, sig[3], ay * sig[1]));
        f[3 * a + 2] = fmaf(ax, sig[5], fmaf(ay, sig[4], az * sig[2]));
    }
}

template <bool ISO>
__device__ __forceinline__ void geo_element_forces(const DevSys &s, uint2 id, const float4 *sxp, const float2 *sq,
                                                   float sK6, uint32_t mi, const float *dtab, float f[12])
{
    const uint32_t li[4] = {id.x & 0xffffu, id.x >> 16, id.y & 0xffffu, id.y >> 16};
    // one ds_read_b128 {x, y, z, p_x} + one ds_read_b64 {p_y, p_z} per corner
    float4 X[4];
    float2 Q[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
    {
        X[a] = sxp[li[a]];
        Q[a] = sq[li[a]];
    }
    tet_forces_reg<ISO>(s, X, Q, sK6, mi, dtab, f);
}

// MODE 0: apply (gather x, optional sanitize); MODE 1: PCG (gather z, p_old -> p_new).
// GEO: 8-B element records + per-tile-node coordinates (geometry recomputed); else 48-B records.
template <bool ISO, bool SANITIZE, int MODE, int NT, bool GEO>
__global__ __launch_bounds__(NT) void k_keff_tiles(DevSys s, const float *__restrict__ x, PcgArgs pa)
{
    constexpr int kTab = ISO ? 12 : 36;
    extern __shared__ float lds[];
    const DevTiles &T = s.t;
    const uint32_t ms = T.max_tile_nodes;
    float *sf = lds;                                                     // [12][kTileElems]
    uint16_t *sc = reinterpret_cast<uint16_t *>(lds + 12 * kTileElems);  // [4*kTileElems] local CSR
    float *sp = lds + 14 * kTileElems;                                   // [3][ms] node values
    float *sx = sp + 3 * ms;                                             // [3][ms] node coordinates (GEO)
    __shared__ float dtab[kMaxM * kTab];
    __shared__ double red[2 * (NT / 64)];
    if constexpr (MODE == 1)
    {
        if (!pa.ctl->active)
            return;
    }
    const uint4 hd = T.hdr[blockIdx.x];
    const uint32_t e0 = hd.x, ne = hd.y, nb = hd.z, nn = hd.w;
    const float sK = (float)s.sK;
    // (a) issue every load that does not depend on beta: the first tile-node record, its coordinates
    //     and value(s), the thread's element records and the tile's local CSR (staged into LDS)
    const uint32_t i0 = threadIdx.x;
    uint2 tn0 = uint2{0u, 0u};
    float v0[3] = {0.f, 0.f, 0.f}, w0[3] = {0.f, 0.f, 0.f};
    if (i0 < nn)
    {
        tn0 = T.tnode[nb + i0];
        const uint32_t g = tn0.x & 0x7fffffffu;
        v0[0] = x[3u * g + 0];
        v0[1] = x[3u * g + 1];
        v0[2] = x[3u * g + 2];
        if constexpr (MODE == 1)
        {
            w0[0] = pa.z[3u * g + 0];
            w0[1] = pa.z[3u * g + 1];
            w0[2] = pa.z[3u * g + 2];
        }
        else if constexpr (SANITIZE)
        {
            const uint32_t mk = s.mask[g];
            v0[0] = (mk & 1u) ? 0.f : v0[0];
            v0[1] = (mk & 2u) ? 0.f : v0[1];
            v0[2] = (mk & 4u) ? 0.f : v0[2];
        }
    }
    if constexpr (GEO)
    {
        const uint32_t T3 = T.total_tile_nodes;
        for (uint32_t i = threadIdx.x; i < nn; i += NT)
        {
            sx[i] = T.tcoord[nb + i];
            sx[ms + i] = T.tcoord[T3 + nb + i];
            sx[2 * ms + i] = T.tcoord[2 * T3 + nb + i];
        }
    }
    constexpr int kPer = kTileElems / NT;
    uint4 pq[kPer][GEO ? 1 : 3];
    uint2 pid[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k)
    {
        const uint32_t j = threadIdx.x + k * NT;
        const uint32_t e = e0 + (j < ne ? j : 0u);
        if constexpr (GEO)
            pid[k] = T.eid[e];
        else
        {
            const uint4 *P = T.planes;
            pq[k][0] = P[e];
            pq[k][GEO ? 0 : 1] = P[T.E + e];
            pq[k][GEO ? 0 : 2] = P[2u * T.E + e];
        }
    }
    {
        const uint2 *src = reinterpret_cast<const uint2 *>(T.csr_ent + 4ull * e0);  // 8-B aligned
        uint2 *dst = reinterpret_cast<uint2 *>(sc);
        for (uint32_t k = threadIdx.x; k < ne; k += NT)
            dst[k] = src[k];
    }
    const uint32_t nm = s.M < kMaxM ? s.M : kMaxM;
    for (uint32_t i = threadIdx.x; i < nm * kTab; i += NT)
        dtab[i] = (float)s.dmat[36u * (i / kTab) + dsrc(ISO, i % kTab)];
    float beta = 0.f;
    if constexpr (MODE == 1)
    {
        // pcg.cpp:862-895 of the previous update; its fold latency overlaps the loads above
        if (ablate(pa, 1u))
            beta = (float)pa.ctl->beta;
        else if (!residual_step<NT>(pa.ctl, pa.prr, pa.prz, pa.nupd, pa.stride, pa.it, pa.hist, red, &beta,
                                    pa.abl & 32u))
            return;
    }
    if (i0 < nn)
    {
        if constexpr (MODE == 1)
        {
            // p_new = z + beta p_old; constrained dofs stay 0 (z_c = 0, p_c = 0)
            v0[0] = fmaf(beta, v0[0], w0[0]);
            v0[1] = fmaf(beta, v0[1], w0[1]);
            v0[2] = fmaf(beta, v0[2], w0[2]);
        }
        sp[i0] = v0[0];
        sp[ms + i0] = v0[1];
        sp[2 * ms + i0] = v0[2];
    }
    for (uint32_t i = i0 + NT; i < nn; i += NT)
    {
        const uint2 tn = T.tnode[nb + i];
        float u[3];
        gather_node<SANITIZE, MODE>(s, x, pa.z, beta, tn.x & 0x7fffffffu, u);
        sp[i] = u[0];
        sp[ms + i] = u[1];
        sp[2 * ms + i] = u[2];
    }
    __syncthreads();
    // (b) elements
    if (!ablate(pa, 16u))
    {
#pragma unroll
        for (int k = 0; k < kPer; ++k)
        {
            const uint32_t j = threadIdx.x + k * NT;
            if (j < ne)
            {
                float g[12], vol;
                uint32_t li[4];
                if constexpr (GEO)
                    coord_geometry(pid[k], sx, ms, g, li, &vol);
                else
                    record_geometry(pq[k][0], pq[k][GEO ? 0 : 1], pq[k][GEO ? 0 : 2], g, li, &vol);
                element_forces<ISO>(s, g, li, vol * sK, T.mat ? T.mat[e0 + j] : 0u, j, sp, ms, dtab, sf);
            }
        }
    }
    __syncthreads();
    // (c) fold per tile node (tile-major partials: the tile's block is one contiguous store)
    double pap = 0.0;
    const float sM = (float)s.sM;
    for (uint32_t i = threadIdx.x; i < (ablate(pa, 8u) ? 0u : nn); i += NT)
    {
        const uint2 tn = i == threadIdx.x ? tn0 : T.tnode[nb + i];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        const uint32_t qe = tn.y >> 16;
        uint32_t q = tn.y & 0xffffu;
        // 4 independent (entry, force) LDS chains in flight; the sums stay in ascending-entry order
        for (; q + 4 <= qe; q += 4)
        {
            uint32_t ent[4];
            float f[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                ent[u] = sc[q + u];
#pragma unroll
            for (int u = 0; u < 4; ++u)
            {
                const uint32_t el = ent[u] >> 2, c = 3u * (ent[u] & 3u);
                f[u][0] = sf[(c + 0) * kTileElems + el];
                f[u][1] = sf[(c + 1) * kTileElems + el];
                f[u][2] = sf[(c + 2) * kTileElems + el];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
            {
                a0 += f[u][0];
                a1 += f[u][1];
                a2 += f[u][2];
            }
        }
        for (; q < qe; ++q)
        {
            const uint32_t ent = sc[q];
            const uint32_t el = ent >> 2, c = 3u * (ent & 3u);
            a0 += sf[(c + 0) * kTileElems + el];
            a1 += sf[(c + 1) * kTileElems + el];
            a2 += sf[(c + 2) * kTileElems + el];
        }
        if constexpr (MODE == 1)
        {
            const float p0 = sp[i], p1 = sp[ms + i], p2 = sp[2 * ms + i];
            // the node's owner slot carries its mass term m s_M p (once), as k_keff_tiles_pipe's does: the update
            // pass forms r -= alpha Ap from the partials alone (k_pcg_update_tiles adds no mass term of its own)
            if (tn.x & 0x80000000u)
            {
                const float m = s.mass[tn.x & 0x7fffffffu] * sM;
                a0 = fmaf(m, p0, a0);
                a1 = fmaf(m, p1, a1);
                a2 = fmaf(m, p2, a2);
                if (pa.pnew)  // and stores the new p for the update pass
                {
                    float *q = pa.pnew + 3ull * (tn.x & 0x7fffffffu);
                    q[0] = p0;
                    q[1] = p1;
                    q[2] = p2;
                }
            }
            if (!ablate(pa, 4u) && (tn.x & 0x7fffffffu) < s.Nown)  // ghosts: another rank's row
                pap += (double)fmaf(p2, a2, fmaf(p1, a1, p0 * a0));  // fp32 per node, fp64 across nodes
        }
        float *o = T.part + 3ull * (nb + i);
        o[0] = a0;
        o[1] = a1;
        o[2] = a2;
    }
    if constexpr (MODE == 1)
    {
        const double t = block_sum<NT>(pap, red);
        if (threadIdx.x == 0)
            pa.part_dot[blockIdx.x] = t;
    }
}

// Persistent, software-pipelined form of k_keff_tiles (GEO records, push fold; the default FAST path).
// A resident grid (occupancy x CUs) walks the tiles; while a workgroup computes tile t from LDS, the
// loads of its next tile t' (tile-node records, coordinates, corner ids, local CSR, then the z/p
// gathers) are already in flight in registers, so each tile's memory chain overlaps the previous
// tile's element and fold work instead of being exposed. Tiles are dealt XCD-contiguously (workgroup
// b runs on XCD b % 8 and walks that XCD's eighth of the Morton-ordered tiles) so neighbouring tiles,
// which share nodes, share an L2. beta (the residual step) and the material table are set up once
// per workgroup; the p.Ap share is one per workgroup.

struct PipeNext
{
    uint2 tn;          // record of tile node threadIdx.x
    float c[3];        // its coordinates
    float v[3], w[3];  // x / p_old and z (MODE 1) at that node
    float m;           // its lumped mass (MODE 1: the owner slot's m s_M |p|^2 share of p.Ap)
    uint2 id[2];       // corner ids of elements threadIdx.x, threadIdx.x + 256
    uint2 pos[2];      // local-CSR positions of the corners of elements threadIdx.x, + NT
    uint32_t slot;     // node-major partial slot of tile node threadIdx.x
    uint32_t mat[2];   // material of elements threadIdx.x, threadIdx.x + 256 (0 when M == 1)
};

template <int NT, bool SANITIZE, int MODE>
__device__ __forceinline__ void pipe_issue_records(const DevSys &s, uint4 hd, PipeNext &n)
{
    const DevTiles &T = s.t;
    const uint32_t e0 = hd.x, ne = hd.y, nb = hd.z, nn = hd.w;
    const uint32_t i = threadIdx.x;
    n.tn = i < nn ? T.tnode[nb + i] : uint2{0u, 0u};
    n.slot = i < nn ? T.tslot[nb + i] : 0u;
    const uint32_t T3 = T.total_tile_nodes;
    const uint32_t q = nb + (i < nn ? i : 0u);
    n.c[0] = T.tcoord[q];
    n.c[1] = T.tcoord[T3 + q];
    n.c[2] = T.tcoord[2 * T3 + q];
#pragma unroll
    for (int k = 0; k < 2; ++k)
    {
        const uint32_t j = i + k * (uint32_t)NT;
        n.id[k] = T.eid[e0 + (j < ne ? j : 0u)];
        // prefetched with the records: a load inside the element phase would make its wait drain
        // every record load in flight for the next tile
        n.mat[k] = T.mat ? T.mat[e0 + (j < ne ? j : 0u)] : 0u;
        n.pos[k] = T.epos[e0 + (j < ne ? j : 0u)];
    }
}

template <bool SANITIZE, int MODE>
__device__ __forceinline__ void pipe_issue_gather(const DevSys &s, const float *__restrict__ x,
                                                  const float *__restrict__ z, uint32_t nn, PipeNext &n)
{
    const uint32_t g = n.tn.x & 0x7fffffffu;  // node 0 for idle lanes (harmless, in range)
    n.m = 0.f;
    (void)nn;
    n.v[0] = x[3u * g + 0];
    n.v[1] = x[3u * g + 1];
    n.v[2] = x[3u * g + 2];
    if constexpr (MODE == 1)
    {
        n.w[0] = z[3u * g + 0];
        n.w[1] = z[3u * g + 1];
        n.w[2] = z[3u * g + 2];
        n.m = s.mass[g];
    }
    else if constexpr (SANITIZE)
    {
        const uint32_t mk = s.mask[g];
        n.v[0] = (mk & 1u) ? 0.f : n.v[0];
        n.v[1] = (mk & 2u) ? 0.f : n.v[1];
        n.v[2] = (mk & 4u) ? 0.f : n.v[2];
    }
}

// NT threads per workgroup, tiles of <= TE = 2 NT elements and <= NT nodes (one node per lane)
// Push fold: each element stores its 4 corner forces at their tile-relative local-CSR positions (epos),
// so a node's forces sit contiguously in ascending element order and the fold reads them without a
// dependent CSR-entry lookup (the order of a local-CSR fold, without its index stream).
template <bool ISO, bool SANITIZE, int MODE, int NT>
__global__ __launch_bounds__(NT) void k_keff_tiles_pipe(DevSys s, const float *__restrict__ x, PcgArgs pa,
                                                        const uint4 *__restrict__ hdr)
{
    constexpr int TE = 2 * NT;
    constexpr int SP = 4 * TE + 2 * NT;  // slots per component plane: (element, corner) pairs + run pads
    constexpr int kTab = ISO ? 12 : 36;
    extern __shared__ float lds[];
    const DevTiles &T = s.t;
    const uint32_t ms = T.max_tile_nodes;
    // pushed corner forces: {f_x, f_y} pairs (one ds_write_b64 / ds_read2_b64 per two, summed with
    // v_pk_add_f32 without repacking) and an f_z plane
    float2 *sfxy = reinterpret_cast<float2 *>(lds);           // [SP]
    float *sfz = lds + 2 * SP;                                // [SP]
    float4 *sxp = reinterpret_cast<float4 *>(lds + 3 * SP);  // [ms] {x, y, z, v_x}
    float2 *sq = reinterpret_cast<float2 *>(sxp + ms);                   // [ms] {v_y, v_z}
    __shared__ float dtab[kMaxM * kTab];
    __shared__ double red[2 * (NT / 64)];
    if constexpr (MODE == 1)
    {
        if (!pa.ctl->active)
            return;
    }
    // this workgroup's tiles: XCD-contiguous ranges, stride = workgroups per XCD
    const TileRange tr = xcd_tile_range(T.ntiles);
    const uint32_t nbx = tr.nbx, t_end = tr.t_end;
    uint32_t t = tr.t;
    PipeNext cur;
    uint4 hd = t < t_end ? hdr[t] : uint4{0u, 0u, 0u, 0u};
    // header of the tile after next, loaded one tile early so phase (b) never waits on it
    uint4 hd2 = t + nbx < t_end ? hdr[t + nbx] : uint4{0u, 0u, 0u, 0u};
    if (t < t_end)
    {
        pipe_issue_records<NT, SANITIZE, MODE>(s, hd, cur);
        pipe_issue_gather<SANITIZE, MODE>(s, x, pa.z, hd.w, cur);
    }
    const uint32_t nm = s.M < kMaxM ? s.M : kMaxM;
    for (uint32_t i = threadIdx.x; i < nm * kTab; i += NT)
        dtab[i] = (float)s.dmat[36u * (i / kTab) + dsrc(ISO, i % kTab)];
    float beta = 0.f;
    if constexpr (MODE == 1)
    {
        // pcg.cpp:862-895 of the previous update, once per workgroup
        if (!residual_step<NT>(pa.ctl, pa.prr, pa.prz, pa.nupd, pa.stride, pa.it, pa.hist, red, &beta, pa.abl & 32u))
            return;
    }
    const float sK6 = (float)(s.sK / 6.0), sM = (float)s.sM;
    double pap = 0.0;
    for (; t < t_end; t += nbx)
    {
        const uint32_t ne = hd.y, nn = hd.w;
        // (a) LDS fill of tile t from the prefetched registers (second node slot, if any, loads directly)
        const uint32_t i0 = threadIdx.x;
        if (i0 < nn)
        {
            float v0 = cur.v[0], v1 = cur.v[1], v2 = cur.v[2];
            if constexpr (MODE == 1)
            {
                v0 = fmaf(beta, v0, cur.w[0]);
                v1 = fmaf(beta, v1, cur.w[1]);
                v2 = fmaf(beta, v2, cur.w[2]);
            }
            sxp[i0] = float4{cur.c[0], cur.c[1], cur.c[2], v0};
            sq[i0] = float2{v1, v2};
        }
        const uint2 id0 = cur.id[0], id1 = cur.id[1];
        const uint2 pos0 = cur.pos[0], pos1 = cur.pos[1];
        const uint32_t mat0 = cur.mat[0], mat1 = cur.mat[1];
        const uint2 tn_own = cur.tn;
        const uint32_t slot_own = cur.slot;
        const float m_own = cur.m;
        __syncthreads();
        // (b) next tile's records in flight during this tile's element and fold work
        const uint32_t tn_next = t + nbx;
        const uint4 hdn = hd2;
        if (tn_next < t_end)
            pipe_issue_records<NT, SANITIZE, MODE>(s, hdn, cur);
        hd2 = tn_next + nbx < t_end ? hdr[tn_next + nbx] : uint4{0u, 0u, 0u, 0u};
        // (c) elements of tile t (ablation bit 64: skipped, diagnostic timing only)
#pragma unroll
        for (int k = 0; k < 2; ++k)
        {
            const uint32_t j = threadIdx.x + k * NT;
            if (j < ne && !ablate(pa, 64u))
            {
                float f[12];
                geo_element_forces<ISO>(s, k ? id1 : id0, sxp, sq, sK6, k ? mat1 : mat0, dtab, f);
                const uint2 ps = k ? pos1 : pos0;
                const uint32_t pq[4] = {ps.x & 0xffffu, ps.x >> 16, ps.y & 0xffffu, ps.y >> 16};
#pragma unroll
                for (int a = 0; a < 4; ++a)
                {
                    sfxy[pq[a]] = float2{f[3 * a], f[3 * a + 1]};
                    sfz[pq[a]] = f[3 * a + 2];
                }
            }
        }
        __syncthreads();
        // (d) next tile's gathers (its node records have arrived by now; ablation bit 256: skipped)
        if (tn_next < t_end && !ablate(pa, 256u))
            pipe_issue_gather<SANITIZE, MODE>(s, x, pa.z, hdn.w, cur);
        // (e) fold per tile node -> node-major partials (+ p.Ap) (ablation bit 128: skipped)
        if (threadIdx.x < (ablate(pa, 128u) ? 0u : nn))  // nn <= 256: one tile node per lane
        {
            const uint32_t i = threadIdx.x;
            const uint2 tn = tn_own;
            float a0, a1, a2;
            fold_run(sfxy, sfz, tn.y & 0xffffu, tn.y >> 16, a0, a1, a2);
            float p0 = 0.f, p1 = 0.f, p2 = 0.f;
            if constexpr (MODE == 1)
            {
                p0 = sxp[i].w;
                p1 = sq[i].x;
                p2 = sq[i].y;
                if (tn.x & 0x80000000u)  // the node's owner slot carries its mass term m s_M p (once)
                {
                    const float m = m_own * sM;
                    a0 = fmaf(m, p0, a0);
                    a1 = fmaf(m, p1, a1);
                    a2 = fmaf(m, p2, a2);
                    if (pa.pnew)  // and stores the new p for the update pass (no z / p_old re-read there)
                    {
                        float *q = pa.pnew + 3ull * (tn.x & 0x7fffffffu);
                        q[0] = p0;
                        q[1] = p1;
                        q[2] = p2;
                    }
                }
            }
            // ablation (diagnostic timing only): 512 = no partial store, 1024 = tile-major store position
            if (!ablate(pa, 512u))
            {
                float *o = T.part + 3ull * (ablate(pa, 1024u) ? hd.z + i : slot_own);
                o[0] = a0;
                o[1] = a1;
                o[2] = a2;
            }
            if (MODE == 1 && (tn.x & 0x7fffffffu) < s.Nown)  // ghosts: another rank's row
                pap += (double)fmaf(p2, a2, fmaf(p1, a1, p0 * a0));  // fp32 per node, fp64 across nodes
        }
        __syncthreads();  // LDS is refilled by the next tile
        hd = hdn;
    }
    if constexpr (MODE == 1)
    {
        const double tt = block_sum<NT>(pap, red);
        if (threadIdx.x == 0)
            pa.part_dot[blockIdx.x] = tt;
    }
}

inline size_t tiles_lds(const DevSys &s)
{
    // element forces [12][kTileElems] f32 + local CSR [4*kTileElems] u16 + node values [3][ms]
    // (+ node coordinates [3][ms] with GEO records)
    return sizeof(float) * (14 * kTileElems + (s.t.geo ? 6 : 3) * (size_t)s.t.max_tile_nodes);
}

using TileFn = void (*)(DevSys, const float *, PcgArgs);

template <bool ISO, bool SAN, int MODE, bool GEO> Pick<TileFn> tiles_pick()
{
    static const std::string name = kernel_name("k_keff_tiles", ISO, SAN, MODE, 256, GEO);
    return {k_keff_tiles<ISO, SAN, MODE, 256, GEO>, name.c_str()};
}

// Every FAST element pass has three uses: the PCG loop (pcg: MODE 1, never sanitised) and the apply path (MODE 0)
// with or without the Dirichlet sanitise. The pickers spell them <!pcg && sanitize, pcg ? 1 : 0>
Pick<TileFn> pick_tiles(const DevSys &s, bool pcg, bool sanitize)
{
    return with_bools(
        [](auto iso, auto pc, auto san, auto geo) { return tiles_pick<iso(), !pc() && san(), pc() ? 1 : 0, geo()>(); },
        s.iso != 0, pcg, sanitize, s.t.geo != 0);
}

// pipelined kernel: element forces + local CSR + per tile node {x y z v_x}{v_y v_z}
inline size_t pipe_lds(const DevSys &s)
{
    const size_t ms = s.t.max_tile_nodes, te = 2 * (size_t)s.t.pipe_nt;
    // 3 component planes of 4 te (element, corner) slots + one pad per tile node (odd runs), then the tile
    // nodes {x y z v_x}{v_y v_z}
    return sizeof(float) * 3 * (4 * te + 2 * (size_t)s.t.pipe_nt) + ms * (16 + 8);
}

template <bool ISO, bool SAN, int MODE, int NT> Pick<HdrTileFn> pipe_pick()
{
    static const std::string name = kernel_name("k_keff_tiles_pipe", ISO, SAN, MODE, NT);
    return {k_keff_tiles_pipe<ISO, SAN, MODE, NT>, name.c_str()};
}

HdrTilePick pick_pipe(const DevSys &s, bool pcg, bool sanitize)
{
    const int nt = s.t.pipe_nt == 128 ? 128 : 256;
    return {with_bools(
                [](auto iso, auto pc, auto san, auto wide) {
                    return pipe_pick<iso(), !pc() && san(), pc() ? 1 : 0, wide() ? 256 : 128>();
                },
                s.iso != 0, pcg, sanitize, nt == 256),
            nt, pipe_lds(s)};
}
}  // namespace

void launch_tet_tiles(const DevSys &s, const float *x, const PcgPassArgs &pa, bool pcg, bool sanitize, hipStream_t st,
                      hipEvent_t e0, hipEvent_t e1)
{
    const DevTiles &t = s.t;
    if (t.pipe)
    {
        const HdrTilePick p = pick_pipe(s, pcg, sanitize);
        launch_kernel(p.k.fn, t.pipe_grid, p.nt, p.lds, st, e0, e1, s, x, PcgArgs{pa}, t.hdr);
    }
    else
    {
        if (e0)
            (void)hipEventRecord(e0, st);
        launch_kernel(pick_tiles(s, pcg, sanitize).fn, t.ntiles, 256, tiles_lds(s), st, nullptr, nullptr, s, x,
                      PcgArgs{pa});
        if (e1)
            (void)hipEventRecord(e1, st);
    }
}

const char *tet_tiles_kernel_name(const DevSys &s)
{
    return s.t.pipe ? pick_pipe(s, true, false).k.name : pick_tiles(s, true, false).name;
}

unsigned tet_tiles_pipe_grid(const DevSys &s)
{
    const HdrTilePick p = pick_pipe(s, true, false);
    return xcd_grid(p.k.fn, p.nt, p.lds, s.t.ntiles);
}

}  // namespace cwf
