// refine.hpp -- what refine.cpp (the refined solve's driver) and refine.hip (its fp64 kernels) share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cwf_internal.hpp"

namespace cwf
{

// |v|^2 is folded from one share per node: chunks of this many nodes, each a fixed tree, added in chunk order
constexpr uint32_t kRefineChunkNodes = 4096;
uint32_t refine_norm_chunks(uint32_t N);

// r = b - K_eff x (fp64, internal node order, the handle's PARITY node tiles), share[N] the nodes' shares of |r|^2,
// out = {|r|^2, |r|} on the device (part: refine_norm_chunks(N) doubles of scratch)
void refine_residual(const DevSys &s, const double *x, const double *b, double *r, double *share, double *part,
                     double *out, hipStream_t st);
// the tile kernel of refine_residual alone (cwf_hip_residual_f64_timed)
void refine_residual_tiles(const DevSys &s, const double *x, const double *b, double *r, double *share, hipStream_t st);
// out = {|b|^2, |b|} over the free DOFs, the same fold
void refine_rhs_norm(const DevSys &s, const double *b, double *share, double *part, double *out, hipStream_t st);
// x = b on constrained DOFs; on free ones 0 (cold) or left as it is (warm)
void refine_start(const DevSys &s, double *x, const double *b, bool warm, hipStream_t st);
void refine_scale(const DevSys &s, const double *r, int e, float *rhs, hipStream_t st);   // rhs = f32(2^e r)
void refine_update(const DevSys &s, double *x, const float *dx, int e, hipStream_t st);  // x += 2^(-e) dx, free DOFs

}  // namespace cwf
