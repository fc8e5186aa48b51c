// tiles_hex.hip -- k_keff_hex_tiles: the native trilinear hex8 K_eff on the tile machinery of the tet
// kernels (fast_common.hpp: PcgArgs, residual_step, stress_f32, load3 / store3).
//
// PARITY UNPINNED: the reference rejects hex8 ("only tetrahedron elements supported in Phase 3",
// src/mesh/preprocess.cpp:326-330). The element is the textbook isoparametric hex (Gmsh/VTK corner
// order, full 2x2x2 Gauss) restated in fp64 by oracle/hex8_oracle.c, which the tests compare against.
//
// Arithmetic (fp32, FMA), per hex and with corners in lexicographic order L = i + 2 j + 4 k:
//   * reference gradients by sum factorisation. With B = [[a, b], [b, a]] (the two 1-D linear shape
//     functions at the Gauss points +-1/sqrt 3) and d = half the differences along one axis, the
//     derivative along that axis at all 4 point pairs is B d B^T (interp2); it does not depend on the
//     Gauss coordinate along the axis itself. 20 flops per axis per field instead of 8 x 8 x 2.
//   * J[m][l] = dx_m / dxi_l from the tile-relative corner coordinates, A = adj(J), det = det J;
//     H^ = G A (G[c][l] = du_c / dxi_l), eps = sym(H^) (engineering Voigt), sig^ = D eps * s_K / |det|,
//     Q[c][l] = sum_m sig^_cm A[l][m]; then f_L,c = sum_gp sum_l Q[c][l] dN_L / dxi_l, the adjoint of
//     the gradient evaluation (B is symmetric, so the adjoint of interp2 is interp2).
//   * one hardware reciprocal per Gauss point, no divisions.
// The tile machinery is the tet kernel's push fold: each hex stores its 8 corner forces at their
// local-CSR positions (epos8), every tile node sums its contiguous run in ascending element order and
// stores one node-major partial; the update / finalize passes are shared with the tet path.
#include "fast_common.hpp"

namespace cwf
{
namespace
{
constexpr float kGa = 0.78867513459481288f;  // (1 + 1/sqrt 3) / 2
constexpr float kGb = 0.21132486540518712f;  // (1 - 1/sqrt 3) / 2
constexpr int kHexLex[8] = {0, 1, 3, 2, 4, 5, 7, 6};  // Gmsh corner a -> lexicographic corner (self-inverse)

// T = B d B^T for a 2 x 2 array (B = [[a, b], [b, a]] symmetric: also the adjoint map)
__device__ __forceinline__ void interp2(const float d[2][2], float T[2][2])
{
    float e[2][2];
#pragma unroll
    for (int k = 0; k < 2; ++k)
    {
        e[0][k] = fmaf(kGa, d[0][k], kGb * d[1][k]);
        e[1][k] = fmaf(kGb, d[0][k], kGa * d[1][k]);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
    {
        T[r][0] = fmaf(kGa, e[r][0], kGb * e[r][1]);
        T[r][1] = fmaf(kGb, e[r][0], kGa * e[r][1]);
    }
}

// gradients of a lexicographic corner field at the Gauss points (q, r, s):
// d/dxi = gx[r][s], d/deta = gy[q][s], d/dzeta = gz[q][r]
__device__ __forceinline__ void hex_ref_grad(const float v[8], float gx[2][2], float gy[2][2], float gz[2][2])
{
    float d[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k)
            d[j][k] = 0.5f * (v[1 + 2 * j + 4 * k] - v[2 * j + 4 * k]);
    interp2(d, gx);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k)
            d[i][k] = 0.5f * (v[i + 2 + 4 * k] - v[i + 4 * k]);
    interp2(d, gy);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            d[i][j] = 0.5f * (v[i + 2 * j + 4] - v[i + 2 * j]);
    interp2(d, gz);
}

// adjoint of hex_ref_grad: f[L] = sum over the Gauss points of sx dN_L/dxi + sy dN_L/deta + sz dN_L/dzeta,
// with sx[r][s] = sum_q (.), sy[q][s] = sum_r (.), sz[q][r] = sum_s (.) already summed over the free axis
__device__ __forceinline__ void hex_ref_grad_adj(const float sx[2][2], const float sy[2][2], const float sz[2][2],
                                                 float f[8])
{
    float w[2][2];
    interp2(sx, w);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k)
        {
            f[1 + 2 * j + 4 * k] = 0.5f * w[j][k];
            f[2 * j + 4 * k] = -0.5f * w[j][k];
        }
    interp2(sy, w);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k)
        {
            f[i + 2 + 4 * k] = fmaf(0.5f, w[i][k], f[i + 2 + 4 * k]);
            f[i + 4 * k] = fmaf(-0.5f, w[i][k], f[i + 4 * k]);
        }
    interp2(sz, w);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
        {
            f[i + 2 * j + 4] = fmaf(0.5f, w[i][j], f[i + 2 * j + 4]);
            f[i + 2 * j] = fmaf(-0.5f, w[i][j], f[i + 2 * j]);
        }
}

// F[c][L] = (K_e u)_{L,c} * s_K for one hex: X[m][L] corner coordinates, U[c][L] corner values (lexicographic)
template <bool ISO>
__device__ __forceinline__ void hex_element_forces(const float X[3][8], const float U[3][8], float sK, const float *Dm,
                                                   float F[3][8])
{
    float Jx[3][2][2], Jy[3][2][2], Jz[3][2][2];  // J[m][0] at (q,r,s) = Jx[m][r][s], J[m][1] = Jy[m][q][s], ...
    float Gx[3][2][2], Gy[3][2][2], Gz[3][2][2];
#pragma unroll
    for (int m = 0; m < 3; ++m)
    {
        hex_ref_grad(X[m], Jx[m], Jy[m], Jz[m]);
        hex_ref_grad(U[m], Gx[m], Gy[m], Gz[m]);
    }
    float Sx[3][2][2], Sy[3][2][2], Sz[3][2][2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                Sx[c][i][j] = Sy[c][i][j] = Sz[c][i][j] = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int s = 0; s < 2; ++s)
            {
                float J[3][3], G[3][3];
#pragma unroll
                for (int m = 0; m < 3; ++m)
                {
                    J[m][0] = Jx[m][r][s];
                    J[m][1] = Jy[m][q][s];
                    J[m][2] = Jz[m][q][r];
                    G[m][0] = Gx[m][r][s];
                    G[m][1] = Gy[m][q][s];
                    G[m][2] = Gz[m][q][r];
                }
                float A[3][3];  // adj(J) = det J^-1
                A[0][0] = fmaf(J[1][1], J[2][2], -J[1][2] * J[2][1]);
                A[0][1] = fmaf(J[0][2], J[2][1], -J[0][1] * J[2][2]);
                A[0][2] = fmaf(J[0][1], J[1][2], -J[0][2] * J[1][1]);
                A[1][0] = fmaf(J[1][2], J[2][0], -J[1][0] * J[2][2]);
                A[1][1] = fmaf(J[0][0], J[2][2], -J[0][2] * J[2][0]);
                A[1][2] = fmaf(J[0][2], J[1][0], -J[0][0] * J[1][2]);
                A[2][0] = fmaf(J[1][0], J[2][1], -J[1][1] * J[2][0]);
                A[2][1] = fmaf(J[0][1], J[2][0], -J[0][0] * J[2][1]);
                A[2][2] = fmaf(J[0][0], J[1][1], -J[0][1] * J[1][0]);
                const float det = fmaf(J[0][0], A[0][0], fmaf(J[0][1], A[1][0], J[0][2] * A[2][0]));
                const float scale = sK * __builtin_amdgcn_rcpf(fabsf(det));
                float H[3][3];  // det * du_c / dx_m
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int m = 0; m < 3; ++m)
                        H[c][m] = fmaf(G[c][2], A[2][m], fmaf(G[c][1], A[1][m], G[c][0] * A[0][m]));
                const float eps[6] = {H[0][0], H[1][1], H[2][2], H[0][1] + H[1][0], H[1][2] + H[2][1],
                                      H[0][2] + H[2][0]};
                float sg[6];
                stress_f32<ISO>(Dm, eps, sg);
#pragma unroll
                for (int t = 0; t < 6; ++t)
                    sg[t] *= scale;
                // Cauchy tensor rows: c0 {s0 s3 s5}, c1 {s3 s1 s4}, c2 {s5 s4 s2}
                const float S[3][3] = {{sg[0], sg[3], sg[5]}, {sg[3], sg[1], sg[4]}, {sg[5], sg[4], sg[2]}};
#pragma unroll
                for (int c = 0; c < 3; ++c)
                {
                    const float Q0 = fmaf(S[c][2], A[0][2], fmaf(S[c][1], A[0][1], S[c][0] * A[0][0]));
                    const float Q1 = fmaf(S[c][2], A[1][2], fmaf(S[c][1], A[1][1], S[c][0] * A[1][0]));
                    const float Q2 = fmaf(S[c][2], A[2][2], fmaf(S[c][1], A[2][1], S[c][0] * A[2][0]));
                    Sx[c][r][s] += Q0;
                    Sy[c][q][s] += Q1;
                    Sz[c][q][r] += Q2;
                }
            }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        hex_ref_grad_adj(Sx[c], Sy[c], Sz[c], F[c]);
}

// Parallelepiped hex (tile flag from tiles.cpp): J, adj(J), det J and the stress scale are constant, so
// they are formed once from the element-centre derivatives instead of at each Gauss point; the per-point
// work is the strain / stress / Q contraction only. Same integrals as hex_element_forces.
template <bool ISO>
__device__ __forceinline__ void hex_element_forces_affine(const float X[3][8], const float U[3][8], float sK,
                                                          const float *Dm, float F[3][8])
{
    float J[3][3];
#pragma unroll
    for (int m = 0; m < 3; ++m)
    {
        const float *v = X[m];
        // centre derivatives: mean of the axis differences (equal for every point of a parallelepiped)
        J[m][0] = 0.125f * ((v[1] - v[0]) + (v[3] - v[2]) + (v[5] - v[4]) + (v[7] - v[6]));
        J[m][1] = 0.125f * ((v[2] - v[0]) + (v[3] - v[1]) + (v[6] - v[4]) + (v[7] - v[5]));
        J[m][2] = 0.125f * ((v[4] - v[0]) + (v[5] - v[1]) + (v[6] - v[2]) + (v[7] - v[3]));
    }
    float A[3][3];
    A[0][0] = fmaf(J[1][1], J[2][2], -J[1][2] * J[2][1]);
    A[0][1] = fmaf(J[0][2], J[2][1], -J[0][1] * J[2][2]);
    A[0][2] = fmaf(J[0][1], J[1][2], -J[0][2] * J[1][1]);
    A[1][0] = fmaf(J[1][2], J[2][0], -J[1][0] * J[2][2]);
    A[1][1] = fmaf(J[0][0], J[2][2], -J[0][2] * J[2][0]);
    A[1][2] = fmaf(J[0][2], J[1][0], -J[0][0] * J[1][2]);
    A[2][0] = fmaf(J[1][0], J[2][1], -J[1][1] * J[2][0]);
    A[2][1] = fmaf(J[0][1], J[2][0], -J[0][0] * J[2][1]);
    A[2][2] = fmaf(J[0][0], J[1][1], -J[0][1] * J[1][0]);
    const float det = fmaf(J[0][0], A[0][0], fmaf(J[0][1], A[1][0], J[0][2] * A[2][0]));
    const float scale = sK * __builtin_amdgcn_rcpf(fabsf(det));
    float Gx[3][2][2], Gy[3][2][2], Gz[3][2][2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        hex_ref_grad(U[c], Gx[c], Gy[c], Gz[c]);
    float Sx[3][2][2], Sy[3][2][2], Sz[3][2][2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                Sx[c][i][j] = Sy[c][i][j] = Sz[c][i][j] = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int s = 0; s < 2; ++s)
            {
                float H[3][3];
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int m = 0; m < 3; ++m)
                        H[c][m] = fmaf(Gz[c][q][r], A[2][m], fmaf(Gy[c][q][s], A[1][m], Gx[c][r][s] * A[0][m]));
                const float eps[6] = {H[0][0], H[1][1], H[2][2], H[0][1] + H[1][0], H[1][2] + H[2][1],
                                      H[0][2] + H[2][0]};
                float sg[6];
                stress_f32<ISO>(Dm, eps, sg);
#pragma unroll
                for (int t = 0; t < 6; ++t)
                    sg[t] *= scale;
                const float S[3][3] = {{sg[0], sg[3], sg[5]}, {sg[3], sg[1], sg[4]}, {sg[5], sg[4], sg[2]}};
#pragma unroll
                for (int c = 0; c < 3; ++c)
                {
                    Sx[c][r][s] += fmaf(S[c][2], A[0][2], fmaf(S[c][1], A[0][1], S[c][0] * A[0][0]));
                    Sy[c][q][s] += fmaf(S[c][2], A[1][2], fmaf(S[c][1], A[1][1], S[c][0] * A[1][0]));
                    Sz[c][q][r] += fmaf(S[c][2], A[2][2], fmaf(S[c][1], A[2][1], S[c][0] * A[2][0]));
                }
            }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        hex_ref_grad_adj(Sx[c], Sy[c], Sz[c], F[c]);
}

// NT threads, tiles of <= NT hexes (one per lane) and <= 2 NT nodes (two per lane). Persistent grid over
// XCD-contiguous tile ranges like k_keff_tiles_pipe; MODE 0 = apply (x, optional sanitise), 1 = PCG.
// AFF: every tile of the handle is a parallelepiped tile, so the general path is not compiled in (its
// per-point Jacobians hold ~100 more VGPRs: 216 -> the affine-only kernel's budget)
template <bool ISO, bool SANITIZE, int MODE, int NT, bool AFF>
__global__ __launch_bounds__(NT) void k_keff_hex_tiles(DevSys s, const float *__restrict__ x, PcgArgs pa,
                                                       const uint4 *__restrict__ hdr)
{
    constexpr int SP = 8 * NT;  // (hex, corner) slots per component plane
    constexpr int MN = 2 * NT;  // tile nodes
    constexpr int kTab = ISO ? 12 : 36;
    extern __shared__ float lds[];
    const DevTiles &T = s.t;
    float *sf = lds;                                         // [3][SP] pushed corner forces
    float4 *sxp = reinterpret_cast<float4 *>(lds + 3 * SP);  // [MN] {x, y, z, v_x}
    float2 *sq = reinterpret_cast<float2 *>(sxp + MN);       // [MN] {v_y, v_z}
    __shared__ float dtab[kMaxM * kTab];
    __shared__ double red[2 * (NT / 64)];
    if constexpr (MODE == 1)
    {
        if (!pa.ctl->active)
            return;
    }
    const TileRange tr = xcd_tile_range(T.ntiles);
    const uint32_t nbx = tr.nbx, t_end = tr.t_end;
    uint32_t t = tr.t;
    const uint32_t nm = s.M < kMaxM ? s.M : kMaxM;
    for (uint32_t i = threadIdx.x; i < nm * kTab; i += NT)
        dtab[i] = (float)s.dmat[36u * (i / kTab) + dsrc(ISO, i % kTab)];
    float beta = 0.f;
    if constexpr (MODE == 1)
    {
        if (!residual_step<NT>(pa.ctl, pa.prr, pa.prz, pa.nupd, pa.stride, pa.it, pa.hist, red, &beta, pa.abl & 32u))
            return;
    }
    __syncthreads();  // dtab
    const float sK = (float)s.sK, sM = (float)s.sM;
    const uint32_t T3 = T.total_tile_nodes;
    double pap = 0.0;
    for (; t < t_end; t += nbx)
    {
        const uint4 hd = hdr[t];
        const uint32_t e0 = hd.x & 0x7fffffffu, ne = hd.y, nb = hd.z, nn = hd.w;
        const bool affine = (hd.x >> 31) != 0u;  // uniform: every hex of the tile is a parallelepiped
        const uint32_t j = threadIdx.x;
        // the hex's records are in flight while the node phase gathers
        uint4 id = uint4{0u, 0u, 0u, 0u}, ps = uint4{0u, 0u, 0u, 0u};
        uint32_t mi = 0;
        if (j < ne)
        {
            id = T.eid8[e0 + j];
            ps = T.epos8[e0 + j];
            mi = T.mat ? T.mat[e0 + j] : 0u;
        }
        uint2 tn[2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
        {
            const uint32_t i = threadIdx.x + h * NT;
            tn[h] = uint2{0u, 0u};
            if (i < nn)
            {
                tn[h] = T.tnode[nb + i];
                const uint32_t g = tn[h].x & 0x7fffffffu;
                float u[3];
                load3(whole_rsrc(x), g, u);  // one 12-B buffer load per node and vector
                if constexpr (MODE == 1)
                {
                    float zv[3];
                    load3(whole_rsrc(pa.z), g, zv);
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        u[c] = fmaf(beta, u[c], zv[c]);
                }
                else if constexpr (SANITIZE)
                {
                    const uint32_t mk = s.mask[g];
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        u[c] = (mk & (1u << c)) ? 0.f : u[c];
                }
                sxp[i] = float4{T.tcoord[nb + i], T.tcoord[T3 + nb + i], T.tcoord[2 * T3 + nb + i], u[0]};
                sq[i] = float2{u[1], u[2]};
            }
        }
        __syncthreads();
        if (j < ne)
        {
            const uint32_t li[8] = {id.x & 0xffffu, id.x >> 16, id.y & 0xffffu, id.y >> 16,
                                    id.z & 0xffffu, id.z >> 16, id.w & 0xffffu, id.w >> 16};
            float X[3][8], U[3][8];
#pragma unroll
            for (int a = 0; a < 8; ++a)
            {
                const float4 xp = sxp[li[a]];
                const float2 qv = sq[li[a]];
                const int L = kHexLex[a];
                X[0][L] = xp.x;
                X[1][L] = xp.y;
                X[2][L] = xp.z;
                U[0][L] = xp.w;
                U[1][L] = qv.x;
                U[2][L] = qv.y;
            }
            float F[3][8];
            float tab[36];
            const float *Dm = dtab + kTab * mi;
            if (mi >= (uint32_t)kMaxM)
            {
                for (int q = 0; q < kTab; ++q)
                    tab[q] = (float)s.dmat[36u * mi + dsrc(ISO, q)];
                Dm = tab;
            }
            if (AFF || affine)
                hex_element_forces_affine<ISO>(X, U, sK, Dm, F);
            else
                hex_element_forces<ISO>(X, U, sK, Dm, F);
            const uint32_t pq[8] = {ps.x & 0xffffu, ps.x >> 16, ps.y & 0xffffu, ps.y >> 16,
                                    ps.z & 0xffffu, ps.z >> 16, ps.w & 0xffffu, ps.w >> 16};
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    sf[c * SP + pq[a]] = F[c][kHexLex[a]];
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h)
        {
            const uint32_t i = threadIdx.x + h * NT;
            if (i >= nn)
                continue;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            const uint32_t qe = tn[h].y >> 16;
            uint32_t q = tn[h].y & 0xffffu;
            for (; q + 4 <= qe; q += 4)
            {
                float f[4][3];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        f[u][c] = sf[c * SP + q + u];
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
                a0 += sf[q];
                a1 += sf[SP + q];
                a2 += sf[2 * SP + q];
            }
            const uint32_t g = tn[h].x & 0x7fffffffu;
            float p0 = 0.f, p1 = 0.f, p2 = 0.f;
            if constexpr (MODE == 1)
            {
                p0 = sxp[i].w;
                p1 = sq[i].x;
                p2 = sq[i].y;
                if (tn[h].x & 0x80000000u)  // owner slot: the node's mass term m s_M p (once)
                {
                    const float m = s.mass[g] * sM;
                    a0 = fmaf(m, p0, a0);
                    a1 = fmaf(m, p1, a1);
                    a2 = fmaf(m, p2, a2);
                    if (pa.pnew)  // and the new p for the update pass
                        store3(pa.pnew, whole_rsrc(pa.pnew), g, p0, p1, p2, false);
                }
            }
            store3(T.part, whole_rsrc(T.part), T.tslot[nb + i], a0, a1, a2, T.wt_part != 0);
            if (MODE == 1 && g < s.Nown)
                pap += (double)fmaf(p2, a2, fmaf(p1, a1, p0 * a0));  // fp32 per node, fp64 across nodes
        }
        __syncthreads();  // LDS is refilled by the next tile
    }
    if constexpr (MODE == 1)
    {
        const double tt = block_sum<NT>(pap, red);
        if (threadIdx.x == 0)
            pa.part_dot[blockIdx.x] = tt;
    }
}

inline size_t hex_lds(int nt) { return sizeof(float) * 3 * 8 * nt + 2 * (size_t)nt * (16 + 8); }

template <bool ISO, bool SAN, int MODE, int NT, bool AFF> Pick<HdrTileFn> hex_pick()
{
    static const std::string name = kernel_name("k_keff_hex_tiles", ISO, SAN, MODE, NT, AFF);
    return {k_keff_hex_tiles<ISO, SAN, MODE, NT, AFF>, name.c_str()};
}

HdrTilePick pick_hex(const DevSys &s, bool pcg, bool sanitize)
{
    const int nt = s.t.hex_nt == 256 ? 256 : 128;
    return {with_bools(
                [](auto iso, auto pc, auto san, auto wide, auto aff) {
                    return hex_pick<iso(), !pc() && san(), pc() ? 1 : 0, wide() ? 256 : 128, aff()>();
                },
                s.iso != 0, pcg, sanitize, nt == 256, s.t.hex_all_affine != 0),
            nt, hex_lds(nt)};
}
}  // namespace

void launch_hex_tiles(const DevSys &s, const float *x, const PcgPassArgs &pa, bool pcg, bool sanitize, hipStream_t st,
                      hipEvent_t e0, hipEvent_t e1)
{
    const HdrTilePick p = pick_hex(s, pcg, sanitize);
    launch_kernel(p.k.fn, s.t.pipe_grid, p.nt, p.lds, st, e0, e1, s, x, PcgArgs{pa}, s.t.hdr);
}

const char *hex_tiles_kernel_name(const DevSys &s) { return pick_hex(s, true, false).k.name; }

unsigned hex_tiles_pipe_grid(const DevSys &s)
{
    const HdrTilePick p = pick_hex(s, true, false);
    return xcd_grid(p.k.fn, p.nt, p.lds, s.t.ntiles);
}

}  // namespace cwf
