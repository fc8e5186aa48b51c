// plasticity.hpp -- the element update of the explicit stepper's J2 plasticity (include/cwf_hip.h "Plasticity"): one
// inline function for the device pass (post.hip k_explicit_plastic_elements) and the host-only ABI function
// cwf_explicit_j2_update (abi_explicit_plasticity.cpp). Both translation units are built with -ffp-contract=off and
// IEEE fp64 division and square root, so the two give the same bits; the statement order is the header's.
#pragma once

#include <hip/hip_runtime.h>

namespace cwf
{

// derived_fields.cpp:47-63 (post.hip's von Mises stress of a Voigt stress)
__host__ __device__ inline double von_mises(const double s[6])
{
    const double dxy = s[0] - s[1], dyz = s[1] - s[2], dzx = s[2] - s[0];
    const double energy = 0.5 * (dxy * dxy + dyz * dyz + dzx * dzx) + 3.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]);
    return sqrt(energy < 0.0 ? 0.0 : energy);  // std::max(energy, 0.0), NaN passes through
}

// D x by the ISO row fold of element_tensors (post.hip): a normal row adds its three normal columns from +0.0 in
// ascending order, a shear row its diagonal entry; D row-major [36], only the 12 entries of the isotropic pattern read
__host__ __device__ inline void iso_row_fold(const double *D, const double x[6], double out[6])
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

// One plastic element's radial return at total strain e (Voigt, engineering shears): updates ep[6], abar and wp where
// the trial stress D (e - ep) lies outside the yield surface sy + H abar, then sp = D ep of the (updated) plastic
// strain. V: the element's volume, weighting the plastic work. Returns whether the element yielded; a NaN never does.
__host__ __device__ inline bool j2_update(const double *D, double sy, double H, double V, const double e[6],
                                          double ep[6], double &abar, double &wp, double sp[6])
{
    double ee[6], st[6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
        ee[r] = e[r] - ep[r];
    iso_row_fold(D, ee, st);
    const double q = von_mises(st);
    const double Y = sy + H * abar;
    const bool yielded = q > Y;
    if (yielded)
    {
        const double mu = D[21];  // D[3][3]
        const double dg = (q - Y) / (3.0 * mu + H);
        const double pm = ((st[0] + st[1]) + st[2]) / 3.0;
        const double fac = (1.5 * dg) / q;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            ep[r] = ep[r] + fac * (st[r] - pm);
#pragma unroll
        for (int r = 3; r < 6; ++r)
            ep[r] = ep[r] + (2.0 * fac) * st[r];
        abar = abar + dg;
        wp = wp + V * ((sy + H * abar) * dg);
    }
    iso_row_fold(D, ep, sp);
    return yielded;
}

}  // namespace cwf
