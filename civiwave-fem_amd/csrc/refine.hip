// refine.hip -- the fp64 kernels of the refined static solve (refine.cpp) for gfx950: the true residual
// r = b - K_eff x over fp64 vectors, its norm, the scaled f32 right-hand side of the next inner solve and the fp64
// update of x.
//
// The operator is the reference's (pcg.cpp:505-694), the one k_keff_parity_tile applies: fp64 element math on the f32
// records widened, the reference's operand order (this file is built with -ffp-contract=off like that one), each
// node's incident corner forces added in ascending element order from +0.0, then the mass term. Only the vectors
// differ: x is read as fp64 and nothing is cast to f32. The element helpers below restate parity_keff.hip's
// instead of being shared with it: that file's kernels are the bit-exact yardstick, and sharing a __device__ function
// between instantiations has moved register allocation before (the lattice kernels, DESIGN.md section 3 "Layered
// blocks"). Their resource usage is unchanged by this file (profiles/refine_kernel_resources.txt).
#include "cwf_internal.hpp"
#include "refine.hpp"

namespace cwf
{
namespace
{

constexpr int kBlock = 256;
constexpr int kMaxLdsMaterials = 16;
constexpr int kTileTets = 256;

// stress = D strain (pcg.cpp:632-640). ISO: 12-entry table [D00 D01 D02 D10 D11 D12 D20 D21 D22 D33 D44 D55]
template <bool ISO> __device__ __forceinline__ void stress_fp64(const double *Dm, const double e[6], double s[6])
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

// entry t of a material's LDS table -> its index in the 6 x 6 D
template <bool ISO> __device__ __forceinline__ uint32_t dtab_src(uint32_t t)
{
    if constexpr (ISO)
        return t < 9u ? (t / 3u) * 6u + (t % 3u) : (t - 6u) * 7u;  // (3,3) (4,4) (5,5)
    else
        return t;
}

// One workgroup per PARITY node tile (abi.cpp parity_incidence_slots: 256 nodes, compact blobs or strips of
// consecutive nodes; the tile's incident tets ascending; pinc = each incidence's tile-local tet << 2 | corner). The
// tile's tets are walked 256 at a time: thread t computes one tet's fp64 corner forces into LDS, then every node
// thread adds its incidences that fall in the batch, in ascending element order. Constrained input DOFs enter the
// element loop and the mass term as 0; a constrained row's residual is 0. Per node the kernel writes r (3 doubles) and
// the node's share r0^2 + r1^2 + r2^2 of |r|^2 (that order). No atomics, every node in exactly one tile: the bits are
// a function of the inputs alone.
template <bool ISO>
__global__ __launch_bounds__(kBlock) void k_refine_residual(DevSys s, const double *__restrict__ x,
                                                            const double *__restrict__ b, double *__restrict__ r,
                                                            double *__restrict__ share)
{
    constexpr int kTab = ISO ? 12 : 36;
    __shared__ double dtab[kMaxLdsMaterials * kTab];
    __shared__ double fs[3][4 * kTileTets];  // [component][batch tet * 4 + corner]
    const uint32_t tid = threadIdx.x, tile = blockIdx.x;
    const uint32_t nm = s.M < (uint32_t)kMaxLdsMaterials ? s.M : (uint32_t)kMaxLdsMaterials;
    for (uint32_t i = tid; i < nm * kTab; i += kBlock)
        dtab[i] = s.dmat[36u * (i / kTab) + dtab_src<ISO>(i % kTab)];
    const uint32_t n = s.ptile_nodes ? s.ptile_nodes[tile * kBlock + tid] : tile * kBlock + tid;  // pads are ~0 >= N
    const uint32_t t0 = s.ptile_off[tile], nt = s.ptile_off[tile + 1] - t0;
    uint32_t j = 0, jend = 0;
    if (n < s.N)
    {
        j = s.off[n];
        jend = s.off[n + 1];
    }
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    __syncthreads();  // dtab
    for (uint32_t base = 0; base < nt; base += kTileTets)
    {
        if (base + tid < nt)
        {
            const uint32_t e = s.ptile_tets[t0 + base + tid];
            const uint4 q0 = s.erec[4u * e + 0u], q1 = s.erec[4u * e + 1u], q2 = s.erec[4u * e + 2u],
                        q3 = s.erec[4u * e + 3u];
            const uint32_t c[4] = {q0.x, q0.y, q0.z, q0.w};
            const uint32_t gb[12] = {q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
            double u[12], gx[4], gy[4], gz[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
            {
                const uint32_t mk = s.mask[c[q]];
                const double *xp = x + 3u * (size_t)c[q];
                u[3 * q + 0] = (mk & 1u) ? 0.0 : xp[0];
                u[3 * q + 1] = (mk & 2u) ? 0.0 : xp[1];
                u[3 * q + 2] = (mk & 4u) ? 0.0 : xp[2];
                gx[q] = (double)__uint_as_float(gb[3 * q + 0]);
                gy[q] = (double)__uint_as_float(gb[3 * q + 1]);
                gz[q] = (double)__uint_as_float(gb[3 * q + 2]);
            }
            // strain (pcg.cpp:574-630), the reference's term order
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
            double sig[6];
            const uint32_t mi = s.mat[e];
            if (mi < (uint32_t)kMaxLdsMaterials)
                stress_fp64<ISO>(dtab + kTab * mi, eps, sig);
            else
            {
                double tab[kTab];
#pragma unroll
                for (int t2 = 0; t2 < kTab; ++t2)
                    tab[t2] = s.dmat[36u * mi + dtab_src<ISO>((uint32_t)t2)];
                stress_fp64<ISO>(tab, eps, sig);
            }
            const double vol = (double)s.vol[e] * s.sK;  // pcg.cpp:642
            // f[col] = (sum_r B[r][col] sigma_r) * vol per corner (pcg.cpp:643-651), the term the scatter adds
#pragma unroll
            for (int a = 0; a < 4; ++a)
            {
                double fx = 0.0, fy = 0.0, fz = 0.0;
                fx += gx[a] * sig[0];
                fx += gy[a] * sig[3];
                fx += gz[a] * sig[5];
                fy += gy[a] * sig[1];
                fy += gx[a] * sig[3];
                fy += gz[a] * sig[4];
                fz += gz[a] * sig[2];
                fz += gy[a] * sig[4];
                fz += gx[a] * sig[5];
                const uint32_t sl = 4u * tid + (uint32_t)a;
                fs[0][sl] = fx * vol;
                fs[1][sl] = fy * vol;
                fs[2][sl] = fz * vol;
            }
        }
        __syncthreads();
        // a node's incidences ascend in element order, so in tile-local tet order: those below lim are this batch's
        const uint32_t lim = (base + kTileTets) << 2;
        while (j < jend)
        {
            const uint32_t q = s.pinc[j];
            if (q >= lim)
                break;
            const uint32_t sl = q - (base << 2);
            acc0 += fs[0][sl];
            acc1 += fs[1][sl];
            acc2 += fs[2][sl];
            ++j;
        }
        __syncthreads();
    }
    if (n >= s.N)
        return;
    const uint32_t mk = s.mask[n];
    const double m = (double)s.mass[n] * s.sM;
    const double *xp = x + 3u * (size_t)n, *bp = b + 3u * (size_t)n;
    acc0 += m * ((mk & 1u) ? 0.0 : xp[0]);
    acc1 += m * ((mk & 2u) ? 0.0 : xp[1]);
    acc2 += m * ((mk & 4u) ? 0.0 : xp[2]);
    const double r0 = (mk & 1u) ? 0.0 : bp[0] - acc0;
    const double r1 = (mk & 2u) ? 0.0 : bp[1] - acc1;
    const double r2 = (mk & 4u) ? 0.0 : bp[2] - acc2;
    double *rp = r + 3u * (size_t)n;
    rp[0] = r0;
    rp[1] = r1;
    rp[2] = r2;
    double sq = r0 * r0;
    sq += r1 * r1;
    sq += r2 * r2;
    share[n] = sq;
}

// the shares of |b|^2 over the free DOFs (the right-hand side the free rows see), the residual kernel's form
__global__ __launch_bounds__(kBlock) void k_refine_rhs_shares(const double *__restrict__ b,
                                                              const uint32_t *__restrict__ mask, uint32_t N,
                                                              double *__restrict__ share)
{
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= N)
        return;
    const uint32_t mk = mask[n];
    const double *bp = b + 3u * (size_t)n;
    const double b0 = (mk & 1u) ? 0.0 : bp[0], b1 = (mk & 2u) ? 0.0 : bp[1], b2 = (mk & 4u) ? 0.0 : bp[2];
    double sq = b0 * b0;
    sq += b1 * b1;
    sq += b2 * b2;
    share[n] = sq;
}

// One workgroup per chunk of kRefineChunkNodes node shares: thread t adds shares t, t + 256, ... of the chunk in that
// order, then the 256 sums fold pairwise (stride 128, 64, ... 1). The tree depends on N alone.
__global__ __launch_bounds__(kBlock) void k_refine_norm_chunks(const double *__restrict__ share, uint32_t N,
                                                               double *__restrict__ part)
{
    __shared__ double red[kBlock];
    const uint32_t lo = blockIdx.x * kRefineChunkNodes;
    double sum = 0.0;
    for (uint32_t i = threadIdx.x; i < kRefineChunkNodes; i += kBlock)
        if (lo + i < N)
            sum += share[lo + i];
    red[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t w = kBlock / 2; w > 0; w >>= 1)
    {
        if (threadIdx.x < w)
            red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        part[blockIdx.x] = red[0];
}

// the chunk partials in chunk order: out = {|v|^2, |v|}
__global__ void k_refine_norm_fold(const double *__restrict__ part, uint32_t chunks, double *__restrict__ out)
{
    double sum = 0.0;
    for (uint32_t c = 0; c < chunks; ++c)
        sum += part[c];
    out[0] = sum;
    out[1] = sqrt(sum);
}

// x = the start value on free DOFs (0 for a cold start), b on constrained ones
__global__ __launch_bounds__(kBlock) void k_refine_start(double *__restrict__ x, const double *__restrict__ b,
                                                         const uint32_t *__restrict__ mask, uint32_t D, int warm)
{
    const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
    if (d >= D)
        return;
    const uint32_t n = d / 3u, k = d - 3u * n;
    if ((mask[n] >> k) & 1u)
        x[d] = b[d];
    else if (!warm)
        x[d] = 0.0;
}

// rhs32 = f32(2^e r): the scale is exact, the cast rounds once
__global__ __launch_bounds__(kBlock) void k_refine_scale(const double *__restrict__ r, int e, uint32_t D,
                                                         float *__restrict__ rhs)
{
    const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
    if (d < D)
        rhs[d] = (float)ldexp(r[d], e);
}

// x += 2^(-e) d on the free DOFs (constrained ones keep b)
__global__ __launch_bounds__(kBlock) void k_refine_update(double *__restrict__ x, const float *__restrict__ dx, int e,
                                                          const uint32_t *__restrict__ mask, uint32_t D)
{
    const uint32_t d = blockIdx.x * kBlock + threadIdx.x;
    if (d >= D)
        return;
    const uint32_t n = d / 3u, k = d - 3u * n;
    if (!((mask[n] >> k) & 1u))
        x[d] += ldexp((double)dx[d], -e);
}

unsigned blocks_for(uint32_t n) { return (n + kBlock - 1u) / kBlock; }

}  // namespace

uint32_t refine_norm_chunks(uint32_t N) { return (N + kRefineChunkNodes - 1u) / kRefineChunkNodes; }

void refine_norm(const double *share, uint32_t N, double *part, double *out, hipStream_t st)
{
    const uint32_t chunks = refine_norm_chunks(N);
    if (chunks)
        k_refine_norm_chunks<<<chunks, kBlock, 0, st>>>(share, N, part);
    k_refine_norm_fold<<<1, 1, 0, st>>>(part, chunks, out);
}

void refine_residual_tiles(const DevSys &s, const double *x, const double *b, double *r, double *share, hipStream_t st)
{
    if (!s.pntile)
        return;
    if (s.iso)
        k_refine_residual<true><<<s.pntile, kBlock, 0, st>>>(s, x, b, r, share);
    else
        k_refine_residual<false><<<s.pntile, kBlock, 0, st>>>(s, x, b, r, share);
}

void refine_residual(const DevSys &s, const double *x, const double *b, double *r, double *share, double *part,
                     double *out, hipStream_t st)
{
    refine_residual_tiles(s, x, b, r, share, st);
    refine_norm(share, s.N, part, out, st);
}

void refine_rhs_norm(const DevSys &s, const double *b, double *share, double *part, double *out, hipStream_t st)
{
    if (s.N)
        k_refine_rhs_shares<<<blocks_for(s.N), kBlock, 0, st>>>(b, s.mask, s.N, share);
    refine_norm(share, s.N, part, out, st);
}

void refine_start(const DevSys &s, double *x, const double *b, bool warm, hipStream_t st)
{
    if (s.D)
        k_refine_start<<<blocks_for(s.D), kBlock, 0, st>>>(x, b, s.mask, s.D, warm ? 1 : 0);
}

void refine_scale(const DevSys &s, const double *r, int e, float *rhs, hipStream_t st)
{
    if (s.D)
        k_refine_scale<<<blocks_for(s.D), kBlock, 0, st>>>(r, e, s.D, rhs);
}

void refine_update(const DevSys &s, double *x, const float *dx, int e, hipStream_t st)
{
    if (s.D)
        k_refine_update<<<blocks_for(s.D), kBlock, 0, st>>>(x, dx, e, s.mask, s.D);
}

}  // namespace cwf
