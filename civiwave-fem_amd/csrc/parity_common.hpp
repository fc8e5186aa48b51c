// parity_common.hpp -- what the PARITY translation units share (parity_keff.hip, parity_pcg.hip): the reference-order
// (bit-exact) kernels for gfx950.
//
// Every fold of these units reproduces the reference's src/gpu/pcg.cpp in order:
//  * node-centric gather over the ascending node->element CSR reproduces the scatter-add of
//    pcg.cpp:653-661 (an fp64 accumulator per DOF that receives element contributions in
//    ascending element order, starting at +0.0);
//  * element math is fp64 on fp32 inputs with the reference operand order; structural zeros
//    of B (and of an isotropic D) are skipped, which is exact: every fold starts at +0.0, a
//    round-to-nearest sum that starts at +0.0 is never -0.0, so adding a +-0 term is a no-op;
//  * every unit is compiled with -ffp-contract=off (no FMA contraction), IEEE fp64 div/sqrt.
//
// Here: the workgroup size of the node passes and the chunk partials a node pass forms from its own DOFs, which the
// K_eff tile kernel (p . Ap) and the update pass (r . r, r . z) both do. Device code, in an anonymous namespace per
// including unit, like fast_common.hpp.
#pragma once

#include "cwf_internal.hpp"

#include <type_traits>

namespace cwf
{
namespace
{

constexpr int kBlock = 256;

// A 256-thread workgroup of consecutive nodes covers 768 DOFs = three whole 256-DOF reduction chunks (workgroup b:
// chunks 3b .. 3b + 2), so the node kernels that produce a dot's operands also produce its chunk partials. Every
// thread stages the fp64 products of its own DOFs in LDS (chunk k at row 257 k, against bank conflicts); a
// product of two fp32 values is exact in fp64, so staging (double)a * (double)b is bitwise the term
// pcg.cpp:189-199 adds. Lanes 0..2 then fold one chunk each, sequentially in DOF order, adds only (the chains
// are the critical path: staging the fp32 operands and forming the products in the chains measured 22 us for
// the C2 update pass against 14 us without the partials). DOFs of nodes at or past `nlim` (the owned nodes of
// a shard, or N) are staged as +0.0, an exact no-op in a fold from +0.0. NV = 2: two dots per DOF, {ab, ac}.
// Streamed scalar folds (the single-handle PCG loop, 256-DOF chunks; parity_pcg.hip): a producing pass stores each
// chunk partial as a tagged 16-B granule {partial lo, hi, tag, 0} in ONE write-through (sc1) store, and its
// workgroup 0 polls them (sc1 loads, served past L1 and the per-XCD L2) and folds them in chunk order while the other
// workgroups still produce: each granule carries its own tag, so no counter and no ordering between granules is
// needed (the hand-off form of resident.hip / MI355X_MICROARCH.md). Granule of chunk k, operand c: NC k + c.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gran_rsrc(const double *g)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(g), 0, -1, 0x00020000);
}
__device__ __forceinline__ void gran_store(__amdgpu_buffer_rsrc_t rs, uint32_t idx, double v, uint32_t tag)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const u32x4 w = {(uint32_t)b, (uint32_t)(b >> 32), tag, 0u};
    __builtin_amdgcn_raw_buffer_store_b128(w, rs, 16u * idx, 0, 16);  // sc1: write-through
}

constexpr int kChunkRow = 257;
template <int NV>
using ChunkTerm = std::conditional_t<NV == 2, double2, double>;

__device__ __forceinline__ uint32_t chunk_slot(uint32_t d)  // LDS index of the workgroup's d-th DOF
{
    return (d >> 8) * kChunkRow + (d & 255u);
}

template <int NV>
__device__ __forceinline__ void wg_chunk_partials(const ChunkTerm<NV> *st, uint32_t chunks, double *pab, double *pac,
                                                  uint32_t blk, const double *gran = nullptr, uint32_t tag = 0)
{
    if (threadIdx.x >= 3u)
        return;
    const uint32_t k = 3u * blk + threadIdx.x;
    if (k >= chunks)
        return;
    const ChunkTerm<NV> *row = st + threadIdx.x * kChunkRow;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 16
    for (uint32_t i = 0; i < 256u; ++i)
    {
        if constexpr (NV == 2)
        {
            const double2 t = row[i];
            s0 += t.x;
            s1 += t.y;
        }
        else
            s0 += row[i];
    }
    if (gran)  // streamed: the granules the folding workgroup polls
    {
        const __amdgpu_buffer_rsrc_t rs = gran_rsrc(gran);
        gran_store(rs, NV * k, s0, tag);
        if constexpr (NV == 2)
            gran_store(rs, NV * k + 1u, s1, tag);
        return;
    }
    pab[k] = s0;
    if constexpr (NV == 2)
        pac[k] = s1;
}

}  // namespace
}  // namespace cwf
