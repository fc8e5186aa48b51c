// modal.hip -- the block linear algebra of the modal analysis (modal.cpp) for gfx950: tall-skinny Gram matrices
// G = A^T W B with fp64 products and sums on v_mfma_f64_16x16x4_f64, their ordered fold, and the basis rotation
// X' = X Q, Y' = M X'. A block is q <= kModalMaxBlock contiguous f32 [D] columns (column j at base + j D), so every
// column is directly a PCG right-hand side or solution.
#include <algorithm>

#include "cwf_internal.hpp"
#include "modal.hpp"

namespace cwf
{

namespace
{

typedef double double4_t __attribute__((ext_vector_type(4)));

// W's diagonal entry of DOF row r: the node's lumped mass, 0 on a constrained DOF
__device__ inline double row_weight(const float *mass, const uint32_t *mask, uint32_t r)
{
    const uint32_t n = r / 3u, k = r - 3u * n;
    return (mask[n] >> k) & 1u ? 0.0 : (double)mass[n];
}

// rows r0 .. r0 + 3 of one column: one 16-B load when the four rows exist and the address allows it (a column
// starts at base + 4 j D bytes, which is 16-B aligned only for some j when D % 4 != 0), else row by row; rows past
// D and columns past q (live == false) read nothing and give zeros
__device__ inline void load_rows4(const float *col, uint32_t r0, uint32_t D, bool live, float v[4])
{
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (!live || r0 >= D)
        return;
    const float *p = col + r0;
    if (r0 + 4u <= D && (reinterpret_cast<uintptr_t>(p) & 15u) == 0)
    {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if (r0 + j < D)
            v[j] = p[j];
}

// One workgroup per chunk of kGramChunkRows rows; each of its 4 waves takes every 4th 16-row slab. Lane l loads
// four consecutive rows (offset 4 (l >> 4) in the slab) of column l & 15 of each 16-column tile, and feeds register j
// to MFMA k-step j: the instruction's A operand is A[row l & 15][k = l >> 4] and its B operand B[k = l >> 4][col
// l & 15], so with the same row -> (step, lane group) map on both sides the four steps sum over all 16 rows, and a
// wave load touches 16 full 64-B lines. C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg.
// SYM (A == B): the columns are loaded once and tile (1, 0) is left to the fold (the transpose of (0, 1)).
template <bool SYM>
__global__ __launch_bounds__(256) void k_block_gram(const float *__restrict__ A, uint32_t qa,
                                                    const float *__restrict__ B, uint32_t qb, uint32_t D,
                                                    const float *__restrict__ mass, const uint32_t *__restrict__ mask,
                                                    double *__restrict__ part)
{
    __shared__ double red[3][2][2][4][64];  // waves 1..3: [ta][tb][reg][lane]
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = lane & 15u, g = lane >> 4;
    const uint32_t row_lo = blockIdx.x * kGramChunkRows;
    const uint32_t row_hi = D - row_lo < kGramChunkRows ? D : row_lo + kGramChunkRows;
    const uint32_t nta = (qa + 15u) >> 4, ntb = (qb + 15u) >> 4;
    double4_t acc[2][2];
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
            acc[ta][tb] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (uint32_t slab = row_lo + 16u * wave; slab < row_hi; slab += 64u)
    {
        const uint32_t r0 = slab + 4u * g;
        float a[2][4], b[2][4];
#pragma unroll
        for (uint32_t t = 0; t < 2; ++t)
            load_rows4(A + (size_t)(16u * t + c) * D, r0, D, 16u * t + c < qa, a[t]);
        if (!SYM)
        {
#pragma unroll
            for (uint32_t t = 0; t < 2; ++t)
                load_rows4(B + (size_t)(16u * t + c) * D, r0, D, 16u * t + c < qb, b[t]);
        }
        double w[4] = {1.0, 1.0, 1.0, 1.0};
        if (mass)
        {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                w[j] = r0 + j < D ? row_weight(mass, mask, r0 + j) : 0.0;
        }
#pragma unroll
        for (uint32_t ta = 0; ta < 2; ++ta)
#pragma unroll
            for (uint32_t tb = 0; tb < 2; ++tb)
                if (ta < nta && tb < ntb && (!SYM || tb >= ta))
                {
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j)
                    {
                        // f32 x f32 is exact in fp64; the weight's product rounds once
                        const double bv = (double)(SYM ? a[tb][j] : b[tb][j]) * w[j];
                        acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[ta][j], bv, acc[ta][tb], 0, 0, 0);
                    }
                }
    }
    // the chunk's partial = wave 0 + wave 1 + wave 2 + wave 3, in that order
    if (wave)
    {
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
            for (int tb = 0; tb < 2; ++tb)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    red[wave - 1][ta][tb][v][lane] = acc[ta][tb][v];
    }
    __syncthreads();
    if (wave)
        return;
    double *out = part + (size_t)blockIdx.x * qa * qb;
#pragma unroll
    for (uint32_t ta = 0; ta < 2; ++ta)
#pragma unroll
        for (uint32_t tb = 0; tb < 2; ++tb)
            if (ta < nta && tb < ntb && (!SYM || tb >= ta))
            {
#pragma unroll
                for (uint32_t v = 0; v < 4; ++v)
                {
                    const uint32_t i = 16u * ta + g + 4u * v, j = 16u * tb + c;
                    double s = acc[ta][tb][v];
                    s += red[0][ta][tb][v][lane];
                    s += red[1][ta][tb][v][lane];
                    s += red[2][ta][tb][v][lane];
                    if (i < qa && j < qb)
                        out[(size_t)i * qb + j] = s;
                }
            }
}

// G[i][j] = the chunk partials of (i, j) added in ascending chunk order; sym: a pair of tile (1, 0) is the
// transposed pair of tile (0, 1), which k_block_gram<true> computed in its place
__global__ __launch_bounds__(256) void k_gram_fold(const double *__restrict__ part, uint32_t chunks, uint32_t qa,
                                                   uint32_t qb, int sym, double *__restrict__ G)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= qa * qb)
        return;
    uint32_t i = e / qb, j = e - i * qb;
    if (sym && (i >> 4) > (j >> 4))
    {
        const uint32_t t = i;
        i = j, j = t;
    }
    const size_t src = (size_t)i * qb + j, stride = (size_t)qa * qb;
    double s = 0.0;
    for (uint32_t ch = 0; ch < chunks; ++ch)
        s += part[ch * stride + src];
    G[e] = s;
}

// X'[:, o] = sum_i X[:, i] Q[i][o] (fp64 products and sums, i ascending, rounded to f32 once) and, when wanted,
// Y'[:, o] = W X'[:, o] from the rounded value, so Y' is the mass times the stored X' exactly rounded. One thread per
// row keeps the row's q_in entries in registers; Q sits in LDS padded with zero rows to kModalMaxBlock, every lane of
// a wave reading the same entry (a broadcast). Out of place.
__global__ __launch_bounds__(256) void k_block_rotate(const float *__restrict__ X, uint32_t q_in,
                                                      const double *__restrict__ Q, uint32_t q_out, uint32_t D,
                                                      const float *__restrict__ mass,
                                                      const uint32_t *__restrict__ mask, float *__restrict__ Xo,
                                                      float *__restrict__ MXo)
{
    __shared__ double Qs[kModalMaxBlock * kModalMaxBlock];
    for (uint32_t t = threadIdx.x; t < kModalMaxBlock * q_out; t += 256u)
        Qs[t] = t < q_in * q_out ? Q[t] : 0.0;
    __syncthreads();
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < D; r += gridDim.x * 256u)
    {
        double x[kModalMaxBlock];
#pragma unroll
        for (uint32_t i = 0; i < kModalMaxBlock; ++i)
            x[i] = i < q_in ? (double)X[(size_t)i * D + r] : 0.0;
        const double w = MXo ? row_weight(mass, mask, r) : 0.0;
        for (uint32_t o = 0; o < q_out; ++o)
        {
            double s = 0.0;
#pragma unroll
            for (uint32_t i = 0; i < kModalMaxBlock; ++i)
                s = fma(x[i], Qs[i * q_out + o], s);
            const float xf = (float)s;
            Xo[(size_t)o * D + r] = xf;
            if (MXo)
                MXo[(size_t)o * D + r] = (float)(w * (double)xf);
        }
    }
}

__global__ __launch_bounds__(256) void k_modal_start(float *__restrict__ X, uint32_t q, uint32_t D,
                                                     const uint32_t *__restrict__ mask)
{
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < D; r += gridDim.x * 256u)
    {
        const uint32_t n = r / 3u, k = r - 3u * n;
        const bool fixed = (mask[n] >> k) & 1u;
        for (uint32_t j = 0; j < q; ++j)
            X[(size_t)j * D + r] = fixed ? 0.f : modal_start_value(j, r);
    }
}

__global__ __launch_bounds__(256) void k_modal_scale(float *__restrict__ dst, const float *__restrict__ src, double s,
                                                     uint32_t D)
{
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < D; r += gridDim.x * 256u)
        dst[r] = (float)((double)src[r] * s);
}

// One workgroup per column: the component of largest magnitude (ties: the lowest DOF in the caller's numbering,
// perm[internal node] = caller's node) decides the sign; a negative one flips the column.
__global__ __launch_bounds__(1024) void k_modal_sign(float *__restrict__ X, uint32_t D,
                                                     const uint32_t *__restrict__ perm)
{
    __shared__ float smax[1024];
    __shared__ uint32_t sidx[1024];
    __shared__ int sneg[1024];
    float *x = X + (size_t)blockIdx.x * D;
    float best = -1.f;
    uint32_t bidx = 0xFFFFFFFFu;
    int bneg = 0;
    for (uint32_t r = threadIdx.x; r < D; r += 1024u)
    {
        const float v = x[r], m = fabsf(v);
        const uint32_t n = r / 3u, k = r - 3u * n;
        const uint32_t id = perm ? 3u * perm[n] + k : r;
        if (m > best || (m == best && id < bidx))
            best = m, bidx = id, bneg = v < 0.f;
    }
    smax[threadIdx.x] = best, sidx[threadIdx.x] = bidx, sneg[threadIdx.x] = bneg;
    __syncthreads();
    for (uint32_t s = 512u; s; s >>= 1)
    {
        if (threadIdx.x < s)
        {
            const float m = smax[threadIdx.x + s];
            const uint32_t id = sidx[threadIdx.x + s];
            if (m > smax[threadIdx.x] || (m == smax[threadIdx.x] && id < sidx[threadIdx.x]))
                smax[threadIdx.x] = m, sidx[threadIdx.x] = id, sneg[threadIdx.x] = sneg[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (!sneg[0])
        return;
    for (uint32_t r = threadIdx.x; r < D; r += 1024u)
        x[r] = -x[r];
}

inline unsigned stride_grid(uint32_t D) { return std::max(1u, std::min((D + 255u) / 256u, 4096u)); }

}  // namespace

uint32_t modal_gram_chunks(uint32_t D) { return std::max(1u, (D + kGramChunkRows - 1u) / kGramChunkRows); }

void modal_gram(const float *A, uint32_t qa, const float *B, uint32_t qb, uint32_t D, const float *mass,
                const uint32_t *mask, double *part, double *G, hipStream_t st)
{
    const uint32_t chunks = modal_gram_chunks(D);
    const bool sym = A == B && qa == qb;
    if (sym)
        k_block_gram<true><<<chunks, 256, 0, st>>>(A, qa, B, qb, D, mass, mask, part);
    else
        k_block_gram<false><<<chunks, 256, 0, st>>>(A, qa, B, qb, D, mass, mask, part);
    k_gram_fold<<<(qa * qb + 255u) / 256u, 256, 0, st>>>(part, chunks, qa, qb, sym ? 1 : 0, G);
}

void modal_rotate(const float *X, uint32_t q_in, const double *Q, uint32_t q_out, uint32_t D, const float *mass,
                  const uint32_t *mask, float *Xo, float *MXo, hipStream_t st)
{
    k_block_rotate<<<stride_grid(D), 256, 0, st>>>(X, q_in, Q, q_out, D, mass, mask, Xo, MXo);
}

void modal_start(float *X, uint32_t q, uint32_t D, const uint32_t *mask, hipStream_t st)
{
    k_modal_start<<<stride_grid(D), 256, 0, st>>>(X, q, D, mask);
}

void modal_scale(float *dst, const float *src, double s, uint32_t D, hipStream_t st)
{
    k_modal_scale<<<stride_grid(D), 256, 0, st>>>(dst, src, s, D);
}

void modal_sign(float *X, uint32_t columns, uint32_t D, const uint32_t *perm, hipStream_t st)
{
    k_modal_sign<<<columns, 1024, 0, st>>>(X, D, perm);
}

}  // namespace cwf
