// parity_keff.hip -- the bit-exact K_eff operator over node tiles (k_keff_parity_tile) and the two block-Jacobi
// builders, which share its element gradient records. The rounding contract: parity_common.hpp.
#include "keff_pick.hpp"
#include "parity_common.hpp"

namespace cwf
{
namespace
{

constexpr int kMaxLdsMaterials = 16;

struct Grad
{
    float g[12];  // g[3a+k]
    uint32_t c[4];
};

__device__ __forceinline__ void load_erec(const uint4 *__restrict__ erec, uint32_t e, Grad &r)
{
    const uint4 q0 = erec[4u * e + 0u];
    const uint4 q1 = erec[4u * e + 1u];
    const uint4 q2 = erec[4u * e + 2u];
    const uint4 q3 = erec[4u * e + 3u];
    r.c[0] = q0.x;
    r.c[1] = q0.y;
    r.c[2] = q0.z;
    r.c[3] = q0.w;
    r.g[0] = __uint_as_float(q1.x);
    r.g[1] = __uint_as_float(q1.y);
    r.g[2] = __uint_as_float(q1.z);
    r.g[3] = __uint_as_float(q1.w);
    r.g[4] = __uint_as_float(q2.x);
    r.g[5] = __uint_as_float(q2.y);
    r.g[6] = __uint_as_float(q2.z);
    r.g[7] = __uint_as_float(q2.w);
    r.g[8] = __uint_as_float(q3.x);
    r.g[9] = __uint_as_float(q3.y);
    r.g[10] = __uint_as_float(q3.z);
    r.g[11] = __uint_as_float(q3.w);
}

// stress = D strain (pcg.cpp:632-640). ISO: 12-entry table [D00 D01 D02 D10 D11 D12 D20 D21 D22 D33 D44 D55].
template <bool ISO>
__device__ __forceinline__ void stress_fp64(const double *Dm, const double e[6], double s[6])
{
    if constexpr (ISO)
    {
#pragma unroll
        for (int r = 0; r < 3; ++r)
        {
            double sum = 0.0;
            sum += Dm[3 * r + 0] * e[0];
            sum += Dm[3 * r + 1] * e[1];
            sum += Dm[3 * r + 2] * e[2];
            s[r] = sum;
        }
#pragma unroll
        for (int r = 3; r < 6; ++r)
        {
            double sum = 0.0;
            sum += Dm[6 + r] * e[r];
            s[r] = sum;
        }
    }
    else
    {
#pragma unroll
        for (int r = 0; r < 6; ++r)
        {
            double sum = 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c)
                sum += Dm[6 * r + c] * e[c];
            s[r] = sum;
        }
    }
}

// f[col] = (sum_r B[r][col] sigma_r) * vol for one corner (pcg.cpp:643-651), the term the scatter adds
__device__ __forceinline__ void corner_force(double ax, double ay, double az, const double sig[6], double vol,
                                             double f[3])
{
    double fx = 0.0, fy = 0.0, fz = 0.0;
    fx += ax * sig[0];
    fx += ay * sig[3];
    fx += az * sig[5];
    fy += ay * sig[1];
    fy += ax * sig[3];
    fy += az * sig[4];
    fz += az * sig[2];
    fz += ay * sig[4];
    fz += ax * sig[5];
    f[0] = fx * vol;
    f[1] = fy * vol;
    f[2] = fz * vol;
}

// a tet's operands: its record (corner ids, f32 gradients), the f32 corner values and (SANITIZE) the corners'
// Dirichlet masks, its volume and material. Gathered first so a pipelined kernel can have them in flight while it
// works on the previous tet (k_keff_parity_tile).
template <bool SANITIZE>
struct TetIn
{
    Grad G;
    float u[12];
    uint32_t mk[SANITIZE ? 4 : 1];
    float vol;
    uint32_t mat;
};

// the loads of the corner values (needs G.c) and of the volume and material
template <bool SANITIZE>
__device__ __forceinline__ void tet_gather(const DevSys &s, const float *__restrict__ x, uint32_t e, TetIn<SANITIZE> &t)
{
#pragma unroll
    for (int q = 0; q < 4; ++q)
    {
        const uint32_t m = t.G.c[q];
        const float *xp = x + 3u * m;
        t.u[3 * q + 0] = xp[0];
        t.u[3 * q + 1] = xp[1];
        t.u[3 * q + 2] = xp[2];
        if constexpr (SANITIZE)
            t.mk[q] = s.mask[m];
    }
    t.vol = s.vol[e];
    t.mat = s.mat[e];
}

// strain / stress of a tet from its operands (pcg.cpp:574-640): gradients g{x,y,z}[4] in fp64, stress sig[6]
template <bool ISO, bool SANITIZE>
__device__ __forceinline__ void tet_stress_in(const DevSys &s, const TetIn<SANITIZE> &t, const double *dtab,
                                              double gx[4], double gy[4], double gz[4], double sig[6])
{
    constexpr int kTab = ISO ? 12 : 36;
    const uint32_t mi = t.mat;
    double u[12];
#pragma unroll
    for (int q = 0; q < 4; ++q)
    {
        double u0 = (double)t.u[3 * q + 0], u1 = (double)t.u[3 * q + 1], u2 = (double)t.u[3 * q + 2];
        if constexpr (SANITIZE)
        {
            const uint32_t mk = t.mk[q];
            if (mk & 1u)
                u0 = 0.0;
            if (mk & 2u)
                u1 = 0.0;
            if (mk & 4u)
                u2 = 0.0;
        }
        u[3 * q + 0] = u0;
        u[3 * q + 1] = u1;
        u[3 * q + 2] = u2;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
    {
        gx[q] = (double)t.G.g[3 * q + 0];
        gy[q] = (double)t.G.g[3 * q + 1];
        gz[q] = (double)t.G.g[3 * q + 2];
    }
    double eps[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q)
    {
        eps[0] += gx[q] * u[3 * q + 0];
        eps[1] += gy[q] * u[3 * q + 1];
        eps[2] += gz[q] * u[3 * q + 2];
        eps[3] += gy[q] * u[3 * q + 0];
        eps[3] += gx[q] * u[3 * q + 1];
        eps[4] += gz[q] * u[3 * q + 1];
        eps[4] += gy[q] * u[3 * q + 2];
        eps[5] += gz[q] * u[3 * q + 0];
        eps[5] += gx[q] * u[3 * q + 2];
    }
    if (mi < (uint32_t)kMaxLdsMaterials)
        stress_fp64<ISO>(dtab + kTab * mi, eps, sig);
    else
    {
        double tab[36];
        for (int t2 = 0; t2 < kTab; ++t2)
        {
            uint32_t src;
            if constexpr (ISO)
                src = t2 < 9 ? (t2 / 3) * 6 + (t2 % 3) : (t2 - 6) * 7;
            else
                src = t2;
            tab[t2] = s.dmat[36u * mi + src];
        }
        stress_fp64<ISO>(tab, eps, sig);
    }
}

template <bool ISO>
__device__ __forceinline__ void stage_dtab(const DevSys &s, double *dtab)
{
    constexpr int kTab = ISO ? 12 : 36;
    const uint32_t nm = s.M < kMaxLdsMaterials ? s.M : kMaxLdsMaterials;
    for (uint32_t i = threadIdx.x; i < nm * kTab; i += kBlock)
    {
        const uint32_t m = i / kTab, t = i % kTab;
        uint32_t src;
        if constexpr (ISO)
            src = t < 9 ? (t / 3) * 6 + (t % 3) : (t - 6) * 7;  // (3,3) (4,4) (5,5)
        else
            src = t;
        dtab[i] = s.dmat[36u * m + src];
    }
}

// K_eff x (pcg.cpp:505-694) over node tiles: workgroup b owns nodes [256 b, 256 b + 256) (thread t node 256 b + t)
// and walks the tile's incident tets in ascending element order, 256 at a time. In each batch thread t computes one
// tet's strain and stress in fp64 (the reference's operand order) and the corner forces of its corners inside the
// tile, each the exact fp64 term pcg.cpp:643-661 adds, into LDS; then every node thread adds its incidences that
// fall in the batch, in ascending element order, to its fp64 accumulators (started at +0.0). Batches run in
// element order, so each node's sum is the reference's left fold over its incident elements: y is bit-identical.
// Then the mass term, the Dirichlet identity rows and the cast (pcg.cpp:664-691); DOT (the PCG loop): the chunk
// partials of x . y (the p . Ap of pcg.cpp:840), three whole 256-DOF chunks per workgroup (wg_chunk_partials).
// Halo tets (those with corners in two tiles) are computed once per tile that needs them (~2.4 tets per tet on a
// Kuhn block); nothing but y leaves the workgroup. Round 3 stored every corner force to HBM (96 B per tet written
// and read back by a node pass: 76 + 36 us on C2); round 2 gathered every incident tet per node (4x the element
// work, 293 us).
constexpr int kTileTets = 256;
constexpr int kIncAhead = 4;  // a node's next incidence entries held in registers
// The PCG loop's compact-tile instantiation (ISO, no sanitize, SET) is held to 128 VGPRs: 4 waves per SIMD instead
// of 3 at 132, no spill (C3 PARITY K_eff 1,260 -> 1,124 us, C2 121 -> 124 us, same box: profiles/r04zg_*); the
// others spill at 128 and keep their registers.
template <bool ISO, bool SANITIZE, bool DOT, bool SET>
__global__ __launch_bounds__(kBlock, ISO && !SANITIZE && SET ? 4 : 1) void k_keff_parity_tile(DevSys s, const float *__restrict__ x,
                                                             float *__restrict__ y, const Ctl *__restrict__ ctl,
                                                             double *__restrict__ pdot, uint32_t nlim,
                                                             uint32_t chunks)
{
    __shared__ double dtab[kMaxLdsMaterials * 36];
    __shared__ double fs[3][4 * kTileTets];  // [component][batch tet * 4 + corner]
    __shared__ double sxy[DOT ? 3 * kChunkRow : 1];
    if (ctl && !ctl->active)
        return;
    stage_dtab<ISO>(s, dtab);
    // XCD-aware tile order: consecutive tiles (which share halo tets) on one XCD
    const uint32_t ntile = gridDim.x, xcd = blockIdx.x & 7u, per = ntile >> 3, rem = ntile & 7u;
    const uint32_t tile = xcd * per + min(xcd, rem) + (blockIdx.x >> 3);
    // SET (compact tiles): the tile's nodes from ptile_nodes (pads are ~0 >= N); else 256 consecutive nodes
    const uint32_t n0 = tile * kBlock, n = SET ? s.ptile_nodes[n0 + threadIdx.x] : n0 + threadIdx.x;
    static_assert(!(SET && DOT), "compact tiles are not runs of consecutive DOFs");
    const uint32_t t0 = s.ptile_off[tile], nt = s.ptile_off[tile + 1] - t0;
    uint32_t j = 0, jend = 0;
    if (n < s.N)
    {
        j = s.off[n];
        jend = s.off[n + 1];
    }
    // the node's next kIncAhead incidence entries (tile-local tet << 2 | corner; ~0 past its last), refilled after
    // each batch's fold so their loads are in flight during the next batch's element work
    uint32_t qa[kIncAhead];
#pragma unroll
    for (int i = 0; i < kIncAhead; ++i)
        qa[i] = j + i < jend ? s.pinc[j + i] : 0xFFFFFFFFu;
    // software pipeline over batches: batch b's operands were gathered during batch b - 1; the next batch's record
    // is issued before this batch's math and its corner gathers before the fold
    const uint32_t tid = threadIdx.x;
    TetIn<SANITIZE> cur;
    uint32_t e_cur = tid < nt ? s.ptile_tets[t0 + tid] : 0u;
    if (tid < nt)
    {
        load_erec(s.erec, e_cur, cur.G);
        tet_gather<SANITIZE>(s, x, e_cur, cur);
    }
    uint32_t e_nxt = kTileTets + tid < nt ? s.ptile_tets[t0 + kTileTets + tid] : 0u;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    __syncthreads();  // dtab
    for (uint32_t base = 0; base < nt; base += kTileTets)
    {
        const bool has_nxt = base + kTileTets + tid < nt;
        TetIn<SANITIZE> nxt;
        if (has_nxt)
            load_erec(s.erec, e_nxt, nxt.G);
        const uint32_t e_nn = base + 2 * kTileTets + tid < nt ? s.ptile_tets[t0 + base + 2 * kTileTets + tid] : 0u;
        if (base + tid < nt)
        {
            double gx[4], gy[4], gz[4], sig[6];
            tet_stress_in<ISO, SANITIZE>(s, cur, dtab, gx, gy, gz, sig);
            const double vol = (double)cur.vol * s.sK;  // pcg.cpp:642
#pragma unroll
            for (int a = 0; a < 4; ++a)
                if (SET || cur.G.c[a] - n0 < (uint32_t)kBlock)  // a corner of this tile (SET: every corner)
                {
                    double f[3];
                    corner_force(gx[a], gy[a], gz[a], sig, vol, f);
                    const uint32_t sl = 4u * tid + (uint32_t)a;
                    fs[0][sl] = f[0];
                    fs[1][sl] = f[1];
                    fs[2][sl] = f[2];
                }
        }
        if (has_nxt)
            tet_gather<SANITIZE>(s, x, e_nxt, nxt);
        __syncthreads();
        // incidences are ascending in element order, so in tile-local tet order: the node's entries below lim are
        // this batch's, consumed in order
        const uint32_t lim = (base + kTileTets) << 2;
        int used = 0;
#pragma unroll
        for (int i = 0; i < kIncAhead; ++i)
            if (qa[i] < lim && used == i)
            {
                const uint32_t sl = qa[i] - (base << 2);
                acc0 += fs[0][sl];
                acc1 += fs[1][sl];
                acc2 += fs[2][sl];
                ++used;
            }
        j += (uint32_t)used;
        if (used == kIncAhead)  // more in this batch than the register window holds (rare): straight from memory
        {
            uint32_t q = j < jend ? s.pinc[j] : 0xFFFFFFFFu;
            while (q < lim)
            {
                const uint32_t sl = q - (base << 2);
                acc0 += fs[0][sl];
                acc1 += fs[1][sl];
                acc2 += fs[2][sl];
                ++j;
                q = j < jend ? s.pinc[j] : 0xFFFFFFFFu;
            }
        }
#pragma unroll
        for (int i = 0; i < kIncAhead; ++i)
            qa[i] = j + i < jend ? s.pinc[j + i] : 0xFFFFFFFFu;
        __syncthreads();
        cur = nxt;
        e_nxt = e_nn;
    }
    float yv[3] = {0.f, 0.f, 0.f}, xv[3] = {0.f, 0.f, 0.f};
    if (n < s.N)
    {
        const uint32_t mk = s.mask[n];
        const double m = (double)s.mass[n] * s.sM;
        const float x0 = x[3u * n + 0], x1 = x[3u * n + 1], x2 = x[3u * n + 2];
        const double s0 = (SANITIZE && (mk & 1u)) ? 0.0 : (double)x0;
        const double s1 = (SANITIZE && (mk & 2u)) ? 0.0 : (double)x1;
        const double s2 = (SANITIZE && (mk & 4u)) ? 0.0 : (double)x2;
        acc0 += m * s0;
        acc1 += m * s1;
        acc2 += m * s2;
        if (mk & 1u)
            acc0 = (double)x0;
        if (mk & 2u)
            acc1 = (double)x1;
        if (mk & 4u)
            acc2 = (double)x2;
        yv[0] = (float)acc0;
        yv[1] = (float)acc1;
        yv[2] = (float)acc2;
        y[3u * n + 0] = yv[0];
        y[3u * n + 1] = yv[1];
        y[3u * n + 2] = yv[2];
        xv[0] = x0;
        xv[1] = x1;
        xv[2] = x2;
    }
    if constexpr (DOT)
    {
        // the tile's chunks are 3 tile, 3 tile + 1, 3 tile + 2
        const bool own = n < nlim;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            sxy[chunk_slot(3u * threadIdx.x + k)] = own ? (double)xv[k] * (double)yv[k] : 0.0;
        __syncthreads();
        wg_chunk_partials<1>(sxy, chunks, pdot, nullptr, tile);
    }
}

__device__ void invert_spd_3x3(double m[9], double inv[9])
{
    // pcg.cpp:215-268
    const double kDetTol = 1.0e-12;
    auto det3 = [&]() {
        return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
               m[2] * (m[3] * m[7] - m[4] * m[6]);
    };
    double det = det3();
    if (fabs(det) < kDetTol)
    {
        const double md = fmax(fmax(m[0], m[4]), m[8]);
        const double eps = fmax(1.0e-6, md * 1.0e-6 + 1.0e-12);
        m[0] += eps;
        m[4] += eps;
        m[8] += eps;
        det = det3();
    }
    if (fabs(det) < kDetTol)
    {
        for (int i = 0; i < 9; ++i)
            inv[i] = 0.0;
        inv[0] = 1.0 / fmax(m[0], 1.0e-6);
        inv[4] = 1.0 / fmax(m[4], 1.0e-6);
        inv[8] = 1.0 / fmax(m[8], 1.0e-6);
        return;
    }
    const double id = 1.0 / det;
    inv[0] = (m[4] * m[8] - m[5] * m[7]) * id;
    inv[1] = (m[2] * m[7] - m[1] * m[8]) * id;
    inv[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    inv[3] = (m[5] * m[6] - m[3] * m[8]) * id;
    inv[4] = (m[0] * m[8] - m[2] * m[6]) * id;
    inv[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    inv[6] = (m[3] * m[7] - m[4] * m[6]) * id;
    inv[7] = (m[1] * m[6] - m[0] * m[7]) * id;
    inv[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// Block-Jacobi inverse, one thread per node (pcg.cpp:270-408): the node's diagonal 3x3 block of
// every incident K_e in ascending element order, + m*s_M, fp64 inverse, constrained rows -> identity.
__global__ __launch_bounds__(kBlock) void k_block_jacobi_parity(DevSys s, float *__restrict__ inv_out)
{
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= s.N)
        return;
    double blk[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t j = s.off[n]; j < s.off[n + 1]; ++j)
    {
        const uint32_t inc = s.inc[j];
        const uint32_t e = inc >> 2, a = inc & 3u;
        const uint4 *rec = s.erec + 4u * e;
        const float *gf = reinterpret_cast<const float *>(rec + 1);
        const double gx = (double)gf[3 * a + 0], gy = (double)gf[3 * a + 1], gz = (double)gf[3 * a + 2];
        const double *Dm = s.dmat + 36u * s.mat[e];
        // nonzero rows of B column 3a+k, ascending: k=0 {0:gx,3:gy,5:gz} k=1 {1:gy,3:gx,4:gz} k=2 {2:gz,4:gy,5:gx}
        const int rows[3][3] = {{0, 3, 5}, {1, 3, 4}, {2, 4, 5}};
        const double vals[3][3] = {{gx, gy, gz}, {gy, gx, gz}, {gz, gy, gx}};
        double DB[6][3];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k)
            {
                double sum = 0.0;
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    sum += Dm[6 * r + rows[k][t]] * vals[k][t];
                DB[r][k] = sum;
            }
        const double sv = (double)s.vol[e] * s.sK;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k)
            {
                double sum = 0.0;
#pragma unroll
                for (int t = 0; t < 3; ++t)
                    sum += vals[i][t] * DB[rows[i][t]][k];
                blk[3 * i + k] += sum * sv;
            }
    }
    const double m = (double)s.mass[n] * s.sM;
    blk[0] += m;
    blk[4] += m;
    blk[8] += m;
    double iv[9];
    invert_spd_3x3(blk, iv);
    const uint32_t mk = s.mask[n];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (mk & (1u << k))
            for (int c = 0; c < 3; ++c)
                iv[3 * k + c] = (k == c) ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
        inv_out[9u * n + i] = (float)iv[i];
}

// Native hex8 block-Jacobi (FAST only; parity unpinned: the reference rejects hex8). One
// thread per node, incident hexes in ascending element order (inc = element << 3 | corner): the
// corner's diagonal 3x3 block of K_e = sum_gp |det J| B_a^T D B_a s_K in fp64 (2x2x2 Gauss), then the
// same m s_M diagonal, regularised fp64 inverse and constrained-row identity as the tet path.
__global__ __launch_bounds__(kBlock) void k_block_jacobi_hex(DevSys s, float *__restrict__ inv_out)
{
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= s.N)
        return;
    const double sg[8][3] = {{-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1},
                             {-1, -1, 1},  {1, -1, 1},  {1, 1, 1},  {-1, 1, 1}};
    const double r3 = 0.57735026918962576;  // 1 / sqrt(3)
    double blk[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t j = s.off[n]; j < s.off[n + 1]; ++j)
    {
        const uint32_t inc = s.inc[j];
        const uint32_t e = inc >> 3, a = inc & 7u;
        double X[8][3];
        for (int c = 0; c < 8; ++c)
        {
            const uint32_t v = s.hconn[8ull * e + c];
            X[c][0] = s.hcoord[3ull * v + 0];
            X[c][1] = s.hcoord[3ull * v + 1];
            X[c][2] = s.hcoord[3ull * v + 2];
        }
        const double *Dm = s.dmat + 36u * s.mat[e];
        for (int p = 0; p < 8; ++p)
        {
            const double q[3] = {(p & 1) ? r3 : -r3, (p & 2) ? r3 : -r3, (p & 4) ? r3 : -r3};
            double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, dNa[3] = {0, 0, 0};
            for (int c = 0; c < 8; ++c)
            {
                const double f0 = 1.0 + sg[c][0] * q[0], f1 = 1.0 + sg[c][1] * q[1], f2 = 1.0 + sg[c][2] * q[2];
                const double d0 = 0.125 * sg[c][0] * f1 * f2, d1 = 0.125 * f0 * sg[c][1] * f2,
                             d2 = 0.125 * f0 * f1 * sg[c][2];
                for (int m = 0; m < 3; ++m)
                {
                    J[m][0] += X[c][m] * d0;
                    J[m][1] += X[c][m] * d1;
                    J[m][2] += X[c][m] * d2;
                }
                if ((uint32_t)c == a)
                {
                    dNa[0] = d0;
                    dNa[1] = d1;
                    dNa[2] = d2;
                }
            }
            double A[3][3];
            A[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
            A[0][1] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
            A[0][2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
            A[1][0] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
            A[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
            A[1][2] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
            A[2][0] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
            A[2][1] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
            A[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
            const double det = J[0][0] * A[0][0] + J[0][1] * A[1][0] + J[0][2] * A[2][0];
            double g[3];
            for (int m = 0; m < 3; ++m)
                g[m] = (dNa[0] * A[0][m] + dNa[1] * A[1][m] + dNa[2] * A[2][m]) / det;
            // B_a (6x3), rows xx yy zz xy yz xz
            const double B[6][3] = {{g[0], 0, 0}, {0, g[1], 0}, {0, 0, g[2]},
                                    {g[1], g[0], 0}, {0, g[2], g[1]}, {g[2], 0, g[0]}};
            const double w = fabs(det) * s.sK;
            for (int i = 0; i < 3; ++i)
                for (int k = 0; k < 3; ++k)
                {
                    double sum = 0.0;
                    for (int r = 0; r < 6; ++r)
                    {
                        double db = 0.0;
                        for (int c = 0; c < 6; ++c)
                            db += Dm[6 * r + c] * B[c][k];
                        sum += B[r][i] * db;
                    }
                    blk[3 * i + k] += sum * w;
                }
        }
    }
    const double m = (double)s.mass[n] * s.sM;
    blk[0] += m;
    blk[4] += m;
    blk[8] += m;
    double iv[9];
    invert_spd_3x3(blk, iv);
    const uint32_t mk = s.mask[n];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (mk & (1u << k))
            for (int c = 0; c < 3; ++c)
                iv[3 * k + c] = (k == c) ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
        inv_out[9u * n + i] = (float)iv[i];
}

using ParityTileFn = void (*)(DevSys, const float *, float *, const Ctl *, double *, uint32_t, uint32_t);

template <bool ISO, bool SAN, bool DOT, bool SET> Pick<ParityTileFn> parity_tile_pick()
{
    static const std::string name = kernel_name("k_keff_parity_tile", ISO, SAN, DOT, SET);
    return {k_keff_parity_tile<ISO, SAN, DOT, SET>, name.c_str()};
}

// dot: the PCG loop's fused p . Ap chunk partials, which need strip tiles (SET: compact tiles) and never sanitise
Pick<ParityTileFn> pick_parity_tile(const DevSys &s, bool sanitize, bool dot, bool compact)
{
    // (plain = !dot first, then the bools in this order: the code object keeps the kernels in the order it always had them)
    return with_bools(
        [](auto plain, auto san, auto set, auto iso) {
            return parity_tile_pick<iso(), plain() && san(), !plain(), plain() && set()>();
        },
        !dot, sanitize, compact, s.iso != 0);
}

// the PCG loop fuses the partials into the node fold when the reduction chunk is 256 DOFs (every workgroup then owns
// three whole chunks) and the tiles are strips
inline bool parity_fused_dot(const cwf_hip_system *h, bool compact) { return h->reduction_block == 256 && !compact; }

// the node-tile K_eff (the handle builds its tiles whenever it runs PARITY: abi.cpp parity_force_buffer)
void launch_parity_tile(const DevSys &s, const float *x, float *y, bool sanitize, bool dot, const Ctl *ctl, double *pdot,
                        uint32_t nlim, uint32_t chunks, hipStream_t st)
{
    const bool compact = s.ptile_nodes && !dot;
    launch_kernel(pick_parity_tile(s, sanitize, dot, compact).fn, compact ? s.pntile : grid_for(s.N, kBlock), kBlock, 0,
                  st, nullptr, nullptr, s, x, y, ctl, pdot, nlim, chunks);
}
}  // namespace

// compact: the handle's tiles are, or will be, the compact ones (abi.cpp parity_compact_tiles_wanted)
const char *parity_keff_kernel_name(const cwf_hip_system *h, bool compact)
{
    return pick_parity_tile(h->ds, false, parity_fused_dot(h, compact), compact).name;
}

void parity_keff_ds(const DevSys &s, const float *x, float *y, bool sanitize, const Ctl *ctl, hipStream_t st)
{
    if (s.N == 0)
        return;
    launch_parity_tile(s, x, y, sanitize, false, ctl, nullptr, 0u, 0u, st);
}

// the PCG loop's K_eff p with the chunk partials of p . Ap over nodes [0, Nown) into pdot: fused, or a separate pass
void parity_keff_dot(const cwf_hip_system *h, const float *p, float *Ap, const Ctl *ctl, double *pdot, hipStream_t st)
{
    const DevSys &s = h->ds;
    if (!parity_fused_dot(h, s.ptile_nodes != nullptr))
    {
        parity_keff_ds(s, p, Ap, false, ctl, st);
        parity_dot_partials(3u * s.Nown, (uint32_t)h->reduction_block, p, Ap, nullptr, pdot, nullptr, ctl, st);
        return;
    }
    if (s.N == 0)
        return;
    launch_parity_tile(s, p, Ap, false, true, ctl, pdot, s.Nown, grid_for(3u * s.Nown, 256u), st);
}

void parity_keff(const cwf_hip_system *h, const float *x, float *y, bool sanitize, const Ctl *ctl, hipStream_t st)
{
    parity_keff_ds(h->ds, x, y, sanitize, ctl, st);
}

void hex_block_jacobi(const cwf_hip_system *h, float *inv, hipStream_t st)
{
    if (h->ds.N == 0)
        return;
    k_block_jacobi_hex<<<grid_for(h->ds.N, kBlock), kBlock, 0, st>>>(h->ds, inv);
}

void parity_block_jacobi(const cwf_hip_system *h, float *inv, hipStream_t st)
{
    if (h->ds.N == 0)
        return;
    k_block_jacobi_parity<<<grid_for(h->ds.N, kBlock), kBlock, 0, st>>>(h->ds, inv);
}

}  // namespace cwf
