// explicit_ties.hip -- the explicit stepper's tie gather (include/cwf_hip.h "Tied boundaries"): per step and tie group
// the shared acceleration g_G = F_G / M_G, from exactly the f, y and p the update pass of the same step reads. The
// tied form of the update pass itself is k_explicit_update<..., TIE> in explicit.hip. Compiled with -ffp-contract=off.
// The small helpers are restated here, not shared with explicit.hip: the update pass's instantiations keep their code.
#include "cwf_internal.hpp"

namespace cwf
{
namespace
{
constexpr int kBlock = 256;
constexpr int kWave = 64;

struct alignas(4) F3
{
    float c[3];
};
__device__ __forceinline__ F3 load3(const float *p, uint32_t n) { return *reinterpret_cast<const F3 *>(p + 3ull * n); }

// explicit.hip's safe_cast
__device__ __forceinline__ float safe_cast(double v)
{
    const double fmax = 3.4028234663852886e38;  // FLT_MAX
    if (!isfinite(v))
        return v > 0.0 ? __int_as_float(0x7f800000) : v < 0.0 ? __int_as_float((int)0xff800000u) : __int_as_float(0x7fc00000);
    if (v > fmax)
        return 3.4028234663852886e38f;
    if (v < -fmax)
        return -3.4028234663852886e38f;
    return (float)v;
}

struct D3
{
    double c[3];
};

// term_k = ((double)f_k - (double)y_k) + (double)p_k of internal node n (without plasticity: no + p; 0 for a constrained
// component), f and y formed as k_explicit_update forms them: y folded from the FAST partials in k_keff_finalize's
// order and arithmetic or read from the PARITY rows, f from the pattern or the force buffer. Which of these runs is
// launch-uniform.
__device__ __forceinline__ D3 member_term(const DevSys &s, const ExplicitPass &a, uint32_t n)
{
    F3 y;
    const uint32_t mk = s.mask[n];
    if (!a.y)
    {
        const DevTiles &T = s.t;
        const float mass = s.mass[n];
        const F3 u = load3(a.u, n);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        for (uint32_t q = T.node_part_off[n] & kPartOffBits; q < (T.node_part_off[n + 1] & kPartOffBits); ++q)
        {
            const F3 pp = load3(T.part, T.node_major ? q : T.part_slot[q]);
            a0 += pp.c[0];
            a1 += pp.c[1];
            a2 += pp.c[2];
        }
        const float m = mass * (float)s.sM;
        F3 x = u;
        if (a.w != a.u)  // beta_R != 0: the operator's input as the last pass stored it
        {
            const F3 v = load3(a.v, n);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                x.c[k] = (float)((double)u.c[k] + a.beta * (double)v.c[k]);
        }
        y.c[0] = fmaf(m, (mk & 1u) ? 0.f : x.c[0], a0);
        y.c[1] = fmaf(m, (mk & 2u) ? 0.f : x.c[1], a1);
        y.c[2] = fmaf(m, (mk & 4u) ? 0.f : x.c[2], a2);
    }
    else
        y = load3(a.y, n);
    F3 f;
    if (a.lbase)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            f.c[k] = safe_cast(a.lbase[3ull * n + k] + a.scale * a.lpat[3ull * n + k]);
    }
    else
        f = load3(a.f, n);
    D3 t;
    if (a.p)
    {
        const F3 pl = load3(a.p, n);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            t.c[k] = ((double)f.c[k] - (double)y.c[k]) + (double)pl.c[k];
    }
    else
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            t.c[k] = (double)f.c[k] - (double)y.c[k];
    }
    // a constrained component adds nothing (a group has one mask): what the operator leaves in a constrained row, which
    // differs between the FAST fold and the PARITY rows, never reaches a free row through Q_G
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (mk & (1u << k))
            t.c[k] = 0.0;
    return t;
}

// One wavefront per group, four groups per workgroup; no atomics, no LDS. The summation order is a function of the
// member count c alone (the header states it): c <= 8: acc = 0, acc = acc + term_j for j = 0 .. c - 1 in list order;
// else lane l of 64 holds L_l = 0, L_l = L_l + term_j for j = l, l + 64, ..., and the lanes fold pairwise,
// L_l = L_l + L_(l + s) for s = 32, 16, 8, 4, 2, 1. Lane 0 divides by M_G and stores three f64.
// A lane's members are taken four at a time: the four members' loads are independent and issued before the first sum.
__global__ __launch_bounds__(kBlock) void k_explicit_tie_gather(DevSys s, ExplicitPass a, ExplicitTies t)
{
    const uint32_t lane = threadIdx.x & (kWave - 1u);
    const uint32_t G = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (G >= t.groups)  // wave-uniform
        return;
    const uint32_t begin = t.toff[G], count = t.toff[G + 1] - begin;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (count <= 8u)
    {
        D3 mine = {{0.0, 0.0, 0.0}};
        if (lane < count)
            mine = member_term(s, a, t.tnode[begin + lane]);
#pragma unroll
        for (int j = 0; j < 8; ++j)
        {
            const double t0 = __shfl(mine.c[0], j, kWave), t1 = __shfl(mine.c[1], j, kWave),
                         t2 = __shfl(mine.c[2], j, kWave);
            if ((uint32_t)j < count)
            {
                x0 = x0 + t0;
                x1 = x1 + t1;
                x2 = x2 + t2;
            }
        }
    }
    else
    {
        for (uint32_t j0 = lane; j0 < count; j0 += 4u * kWave)
        {
            D3 m[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
            {
                const uint32_t j = j0 + (uint32_t)q * kWave;
                if (j < count)
                    m[q] = member_term(s, a, t.tnode[begin + j]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (j0 + (uint32_t)q * kWave < count)
                {
                    x0 = x0 + m[q].c[0];
                    x1 = x1 + m[q].c[1];
                    x2 = x2 + m[q].c[2];
                }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
        {
            x0 = x0 + __shfl_down(x0, off, kWave);
            x1 = x1 + __shfl_down(x1, off, kWave);
            x2 = x2 + __shfl_down(x2, off, kWave);
        }
    }
    if (lane == 0)
    {
        const double M = t.tmass[G];
        double *g = t.tg + 3ull * G;
        g[0] = x0 / M;
        g[1] = x1 / M;
        g[2] = x2 / M;
    }
}
}  // namespace

void explicit_tie_gather(const DevSys &s, const ExplicitPass &a, const ExplicitTies &t, hipStream_t st)
{
    if (!t.groups)
        return;
    const uint32_t per = kBlock / kWave;
    k_explicit_tie_gather<<<(t.groups + per - 1u) / per, kBlock, 0, st>>>(s, a, t);
}

}  // namespace cwf
