// soil_plasticity.hpp -- the element update of the explicit stepper's Drucker-Prager plasticity (include/cwf_hip.h
// "Soil plasticity"): one inline function for the device pass (post.hip k_explicit_dp_elements) and the host-only ABI
// function cwf_explicit_dp_update (soil.cpp). Both translation units are built with -ffp-contract=off and IEEE fp64
// division and square root, so the two give the same bits; the statement order is the header's. Nothing here needs a
// HIP header: a host compiler sees plain inline functions (soil.cpp's stand-alone build).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CWF_SOIL_HD __host__ __device__
#else
#define CWF_SOIL_HD
#endif

namespace cwf
{

// D x by the ISO row fold of element_tensors (post.hip), as the J2 pass: a normal row adds its three normal columns
// from +0.0 in ascending order, a shear row its diagonal entry; D row-major [36]
CWF_SOIL_HD inline void dp_row_fold(const double *D, const double x[6], double out[6])
{
#pragma unroll
    for (int r = 0; r < 6; ++r)
    {
        double acc = 0.0;
        if (r < 3)
        {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                acc += D[6 * r + k] * x[k];
        }
        else
            acc += D[6 * r + r] * x[r];
        out[r] = acc;
    }
}

// One plastic element's return to the cone f = J + 3 alpha pm - (kappa + H abar) at total strain e (Voigt, engineering
// shears) and stress at rest sig0 (NULL: none): updates ep[6], abar and wp where the trial stress sig0 + D (e - ep) lies
// outside, then sp = D ep of the (updated) plastic strain. par = {alpha, kappa, beta, H}; V: the element's volume,
// weighting the plastic work. Returns 0 elastic, 1 returned to the cone, 2 returned to the apex; a NaN never yields.
CWF_SOIL_HD inline int dp_update(const double *D, const double par[4], const double *sig0, double V, const double e[6],
                                 double ep[6], double &abar, double &wp, double sp[6])
{
    const double alpha = par[0], kappa = par[1], beta = par[2], H = par[3];
    double ee[6], st[6], s[6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
        ee[r] = e[r] - ep[r];
    dp_row_fold(D, ee, st);
    if (sig0)
    {
#pragma unroll
        for (int r = 0; r < 6; ++r)
            st[r] = sig0[r] + st[r];
    }
    const double pm = ((st[0] + st[1]) + st[2]) / 3.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
        s[r] = st[r] - pm;
#pragma unroll
    for (int r = 3; r < 6; ++r)
        s[r] = st[r];
    const double j2 = 0.5 * ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) + ((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]);
    const double J = sqrt(j2 < 0.0 ? 0.0 : j2);  // NaN passes through
    const double kc = kappa + H * abar;
    const double f = (J + (3.0 * alpha) * pm) - kc;
    int branch = 0;
    if (f > 0.0)
    {
        const double mu = D[21];  // D[3][3]
        const double Kb = D[1] + (2.0 / 3.0) * mu;
        const double dl = f / ((mu + ((9.0 * Kb) * alpha) * beta) + H);
        const double Jn = J - mu * dl;
        if (Jn >= 0.0 || !(alpha > 0.0))
        {
            branch = 1;
            const double half = (0.5 * dl) / J;
            const double bdl = beta * dl;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                ep[r] = ep[r] + (half * s[r] + bdl);
#pragma unroll
            for (int r = 3; r < 6; ++r)
                ep[r] = ep[r] + (2.0 * half) * s[r];
            abar = abar + dl;
            wp = wp + V * (dl * (Jn + (3.0 * beta) * (pm - ((3.0 * Kb) * beta) * dl)));
        }
        else
        {
            branch = 2;
            const double pa = kc / (3.0 * alpha);
            const double dv = (pm - pa) / Kb;
            const double third = dv / 3.0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                ep[r] = ep[r] + (s[r] / (2.0 * mu) + third);
#pragma unroll
            for (int r = 3; r < 6; ++r)
                ep[r] = ep[r] + s[r] / mu;
            abar = abar + J / mu;
            wp = wp + V * (pa * dv);
        }
    }
    dp_row_fold(D, ep, sp);
    return branch;
}

}  // namespace cwf
