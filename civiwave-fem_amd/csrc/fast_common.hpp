// fast_common.hpp -- what the FAST element-pass and update-pass translation units share (spmv_tiles.hip,
// tiles_groups.hip, tiles_hex.hip, lattice.hip, lattice_fused.hip, pcg_update.hip): the 12-B buffer loads and stores,
// the residual step every consumer workgroup runs in its preamble, the fp32 stress, the PCG arguments of an element
// pass with the ablation bits, and the push fold's run sum. Scalars cross kernels without
// atomics or fences: every consumer workgroup folds the producer's partials itself in a fixed order (alpha in the
// update kernel, |r| / convergence / beta in the element pass's preamble, pcg.cpp:840-895); the host passes the
// iteration index and rho is double-buffered by parity, so no device scalar is read after being written inside one
// kernel. Device code (and the names a picker needs of it), in an anonymous namespace per including unit, like
// lattice_common.hpp, which this header includes.
#pragma once

#include "lattice_common.hpp"

namespace cwf
{
namespace
{
constexpr int kMaxM = 16;  // materials whose D sits in a tile kernel's LDS table

// buffer descriptor over a whole allocation (base pointer wave-uniform: a kernel argument)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t whole_rsrc(const void *base)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, -1, 0x00020000);
}

// 12-B store at float index 3 q; wt: write-through (sc1), so the line leaves L2 during the kernel instead of
// in the end-of-kernel write-back the next launch waits for (the update pass's x / r / z: C2 +2.7% PCG it/s,
// C3 neutral, same-box A/B; the tiles kernel's scattered partial / p stores measured 5% slower that way)
// (one buffer_store_dwordx3 either way; base: the buffer the descriptor covers)
__device__ __forceinline__ void store3(float *base, __amdgpu_buffer_rsrc_t rs, uint64_t q, float a, float b, float c,
                                       bool wt)
{
    (void)base;
    const u32x3 v = {__float_as_uint(a), __float_as_uint(b), __float_as_uint(c)};
    if (wt)
        __builtin_amdgcn_raw_buffer_store_b96(v, rs, (uint32_t)(12ull * q), 0, 16);
    else
        __builtin_amdgcn_raw_buffer_store_b96(v, rs, (uint32_t)(12ull * q), 0, 0);
}

// one 12-B node triple per lane in a single buffer_load_dwordx3 (three dword gathers cost three address
// walks of the wave's 64 scattered lines)
__device__ __forceinline__ void load3(__amdgpu_buffer_rsrc_t rs, uint32_t q, float v[3])
{
    const u32x3 w = __builtin_amdgcn_raw_buffer_load_b96(rs, 12u * q, 0, 0);
    v[0] = __uint_as_float(w.x);
    v[1] = __uint_as_float(w.y);
    v[2] = __uint_as_float(w.z);
}

// pcg.cpp:862-895 for iteration `it` >= 1 from the update kernel's r.r / r.z shares (stride 1), or
// from the all-gathered per-rank {r.r, r.z} pairs of a sharded system (stride 2, rank order).
// Returns false when the solve is over (converged or rho breakdown); *beta_out = beta for this iteration. pre: the
// control words prefetched by the caller (ctl_prefetch); then !pre->active (tested after the fold) also returns false.
template <int NT, int B = 4>
__device__ __forceinline__ bool residual_step(Ctl *ctl, const double *__restrict__ prr, const double *__restrict__ prz,
                                              unsigned nparts, unsigned stride, unsigned it,
                                              double *__restrict__ hist, double *red, float *beta_out,
                                              bool dry = false, const CtlPre *pre = nullptr)
{
    if (it == 0)
    {
        *beta_out = 0.f;
        return pre ? pre->active != 0 : true;
    }
    double rr, rz;
    fold_all2<NT, B>(prr, prz, nparts, red, stride, rr, rz);
    if (pre && !pre->active)
        return false;
    const double res = sqrt(rr);
    const double rho_old = pre ? pre->rho_old : ctl->rho2[(it - 1) & 1u];
    const bool conv = res <= (pre ? pre->tol : ctl->tol);
    const bool err = !conv && fabs(rho_old) < 1.0e-18;
    const double beta = (conv || err) ? 0.0 : rz / rho_old;
    if (dry)  // diagnostic timing: full work, no side effects
    {
        *beta_out = (float)beta;
        return true;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
        ctl->res = res;
        ctl->iterations = it;
        hist[it] = res;
        if (conv)
        {
            ctl->converged = 1;
            ctl->active = 0;
        }
        else if (err)
        {
            ctl->error = CWF_ERR_RHO_ZERO;
            ctl->error_iter = (int)it - 1;
            ctl->active = 0;
        }
        else
        {
            ctl->rho2[it & 1u] = rz;
            ctl->beta = beta;
            ctl->beta_last = beta;
        }
    }
    *beta_out = (float)beta;
    return !(conv || err);
}

template <bool ISO>
__device__ __forceinline__ void stress_f32(const float *Dm, const float e[6], float s[6])
{
    if constexpr (ISO)
    {
#pragma unroll
        for (int r = 0; r < 3; ++r)
            s[r] = fmaf(Dm[3 * r + 2], e[2], fmaf(Dm[3 * r + 1], e[1], Dm[3 * r] * e[0]));
#pragma unroll
        for (int r = 3; r < 6; ++r)
            s[r] = Dm[6 + r] * e[r];
    }
    else
    {
#pragma unroll
        for (int r = 0; r < 6; ++r)
        {
            float sum = 0.0f;
#pragma unroll
            for (int c = 0; c < 6; ++c)
                sum = fmaf(Dm[6 * r + c], e[c], sum);
            s[r] = sum;
        }
    }
}

__device__ __forceinline__ uint32_t dsrc(bool iso, uint32_t t)
{
    return iso ? (t < 9 ? (t / 3) * 6 + (t % 3) : (t - 6) * 7) : t;
}

// The PCG arguments as the element-pass kernels take them. The fields are PcgPassArgs (cwf_internal.hpp), the named
// type that can cross translation units; this empty derived type exists only for symbol-name stability: the kernels'
// mangled names carry (anonymous namespace)::PcgArgs, and they stay what they were before the units were split
struct PcgArgs : PcgPassArgs
{
};

// Ablation bits (tools/ablate.py): phases of the tiles kernels skipped for diagnostic timing. They are compiled
// in only by the ablation build (make ABLATION=1, -DCWF_ABLATION=1); release kernels test a constant 0. Bit 32
// (a side-effect-free residual step, the dry timing of cwf_hip_keff_timed) is not a phase and stays live.
#ifndef CWF_ABLATION
#define CWF_ABLATION 0
#endif
__device__ __forceinline__ bool ablate(const PcgArgs &pa, unsigned bit) { return CWF_ABLATION && (pa.abl & bit); }

// Sum of a node's contiguous run [q, qe) of pushed corner forces, in ascending order: {f_x, f_y} pairs
// accumulate with v_pk_add_f32 straight from ds_read2_b64 (component-wise, so the same order and
// bits as three scalar sums), f_z from its own plane.
__device__ __forceinline__ void fold_run(const float2 *sfxy, const float *sfz, uint32_t q, uint32_t qe, float &a0,
                                         float &a1, float &a2)
{
    typedef float pair_t __attribute__((ext_vector_type(2)));
    const pair_t *pxy = reinterpret_cast<const pair_t *>(sfxy);
    // runs start on even slots: two entries per step, {f_x, f_y} x 2 in one ds_read_b128 (4 LDS cycles) and
    // f_z x 2 in one ds_read_b64 (2 cycles) instead of merged ds_read2_b64 / ds_read2_b32 (8 + 4)
    typedef float quad_t __attribute__((ext_vector_type(4)));
    pair_t axy = {0.f, 0.f};
    float az = 0.f;
#pragma unroll 1
    for (; q + 2 <= qe; q += 2)
    {
        const quad_t f2 = *reinterpret_cast<const quad_t *>(pxy + q);
        const pair_t z2 = *reinterpret_cast<const pair_t *>(sfz + q);
        axy += f2.xy;
        az += z2.x;
        axy += f2.zw;
        az += z2.y;
    }
    if (q < qe)
    {
        axy += pxy[q];
        az += sfz[q];
    }
    a0 = axy.x;
    a1 = axy.y;
    a2 = az;
}

// A persistent workgroup's tiles t, t + nbx, ... < t_end: workgroup b runs on XCD b % kXcds and walks that XCD's
// contiguous share of the Morton-ordered tiles (neighbouring tiles, which share nodes, share an L2), stride = the
// workgroups per XCD
constexpr uint32_t kXcds = 8;
struct TileRange
{
    uint32_t t, t_end, nbx;
};
__device__ __forceinline__ TileRange xcd_tile_range(uint32_t ntiles)
{
    const uint32_t xcd = blockIdx.x % kXcds, lb = blockIdx.x / kXcds;
    TileRange r;
    r.nbx = gridDim.x / kXcds;
    r.t_end = (uint32_t)(((uint64_t)(xcd + 1) * ntiles) / kXcds);
    r.t = (uint32_t)(((uint64_t)xcd * ntiles) / kXcds) + lb;
    return r;
}

// the persistent tile kernels (fan groups, hex tiles, pipelined per-tet tiles) share a signature, the tile headers as
// their last argument, and the grid t.pipe_grid; a pick of one comes with its block size and LDS bytes
using HdrTileFn = void (*)(DevSys, const float *, PcgArgs, const uint4 *);
struct HdrTilePick
{
    Pick<HdrTileFn> k;
    int nt;
    size_t lds;
};
}  // namespace
}  // namespace cwf
