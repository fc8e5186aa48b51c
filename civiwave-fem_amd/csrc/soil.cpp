// soil.cpp -- the host-only part of the soil plasticity (include/cwf_hip.h "Soil plasticity"): the element update the
// device pass runs (soil_plasticity.hpp), Drucker-Prager parameters from Mohr-Coulomb ones, and the geostatic stress
// of a horizontally layered deposit. Plain C++, no device code: with CWF_SOIL_STANDALONE it builds without the
// library (tests/cpp/soil_host_test.cpp, also under the host sanitizers) and a refusal is its code alone.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "soil_plasticity.hpp"

#ifdef CWF_SOIL_STANDALONE
#include "cwf_hip.h"
namespace
{
int refuse(int code, const char *, const std::string & = "") { return code; }
}  // namespace
#else
#include "cwf_internal.hpp"
namespace
{
int refuse(int code, const char *msg, const std::string &ctx = "") { return cwf::set_error(nullptr, code, msg, ctx); }
}  // namespace
#endif

extern "C" {

int cwf_explicit_dp_update(const double D[36], const double params[4], const double *sig0, double volume,
                           const double strain[6], double state[8], double sigma_p[6])
{
    if (!D || !params || !strain || !state || !sigma_p)
        return 0;
    return cwf::dp_update(D, params, sig0, volume, strain, state, state[6], state[7], sigma_p);
}

int cwf_soil_dp_from_mohr_coulomb(double cohesion, double phi, double psi, int match, double out[3])
{
    if (!out)
        return refuse(CWF_ERR_ARGUMENT, "null pointer");
    const double half_pi = 1.5707963267948966;  // pi / 2
    if (!(cohesion >= 0.0) || !std::isfinite(cohesion) || !(phi >= 0.0 && phi < half_pi) || !(psi >= 0.0 && psi <= phi))
        return refuse(CWF_ERR_ARGUMENT, "Mohr-Coulomb parameters out of range",
                      "cohesion=" + std::to_string(cohesion) + "\nphi=" + std::to_string(phi) +
                          "\npsi=" + std::to_string(psi));
    if (match < 0 || match > 2)
        return refuse(CWF_ERR_ARGUMENT, "unknown Drucker-Prager match", "match=" + std::to_string(match));
    const double r3 = std::sqrt(3.0);
    // alpha of the angle a, and kappa's factor of the cohesion at the angle a
    auto alpha_of = [&](double a) {
        if (match == 2)
            return std::tan(a) / std::sqrt(9.0 + 12.0 * std::tan(a) * std::tan(a));
        const double den = r3 * (match == 0 ? 3.0 - std::sin(a) : 3.0 + std::sin(a));
        return 2.0 * std::sin(a) / den;
    };
    out[0] = alpha_of(phi);
    if (match == 2)
        out[1] = 3.0 * cohesion / std::sqrt(9.0 + 12.0 * std::tan(phi) * std::tan(phi));
    else
        out[1] = 6.0 * cohesion * std::cos(phi) / (r3 * (match == 0 ? 3.0 - std::sin(phi) : 3.0 + std::sin(phi)));
    out[2] = alpha_of(psi);
    return 0;
}

int cwf_soil_geostatic_stress(uint64_t element_count, const double *centroids, const uint32_t *material,
                              uint64_t material_count, const double *density, const double *k0, double gravity,
                              int axis, const double *surface, uint64_t node_count, const double *coords, double *sig0)
{
    const uint64_t E = element_count, M = material_count;
    if (!centroids || !material || !density || !k0 || !sig0 || (!surface && !coords))
        return refuse(CWF_ERR_ARGUMENT, "null pointer");
    if (axis < 0 || axis > 2)
        return refuse(CWF_ERR_ARGUMENT, "the vertical axis must be 0, 1 or 2", "axis=" + std::to_string(axis));
    if (!std::isfinite(gravity))
        return refuse(CWF_ERR_ARGUMENT, "gravity is not finite");
    for (uint64_t m = 0; m < M; ++m)
        if (!(density[m] >= 0.0) || !std::isfinite(density[m]) || !std::isfinite(k0[m]))
            return refuse(CWF_ERR_ARGUMENT, "density and K0 must be finite, the density non-negative",
                          "material=" + std::to_string(m));
    for (uint64_t e = 0; e < E; ++e)
        if (material[e] >= M)
            return refuse(CWF_ERR_INDEX, "material index out of range",
                          "element=" + std::to_string(e) + "\nmaterial=" + std::to_string(material[e]));
    if (!E)
        return 0;
    double top;
    if (surface)
        top = *surface;
    else
    {
        if (!node_count)
            return refuse(CWF_ERR_ARGUMENT, "no surface elevation and no nodes");
        top = coords[axis];
        for (uint64_t n = 1; n < node_count; ++n)
            top = std::max(top, coords[3 * n + axis]);
    }
    // the elements from the top down; elevations closer than 1e-9 of the deposit's height are one bin
    std::vector<uint64_t> order(E);
    std::iota(order.begin(), order.end(), (uint64_t)0);
    auto z_of = [&](uint64_t e) { return centroids[3 * e + axis]; };
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return z_of(a) > z_of(b); });
    const double zmax = z_of(order.front()), zmin = z_of(order.back());
    if (!std::isfinite(zmax) || !std::isfinite(zmin) || !std::isfinite(top))
        return refuse(CWF_ERR_ARGUMENT, "elevations are not finite");
    if (zmax > top)
        return refuse(CWF_ERR_ARGUMENT, "a centroid lies above the surface", "element=" + std::to_string(order.front()));
    const double tol = 1e-9 * std::max(top - zmin, 1e-300);
    // layers: maximal runs of bins of one material; layer l spans [bottom_l, top_l], its bottom the midpoint between
    // its lowest centroid bin and the next layer's highest. above_l: the integral of rho from the surface to top_l
    struct Layer
    {
        uint32_t mat;
        double top, above;
    };
    std::vector<Layer> layers;
    std::vector<uint32_t> layer_of(E);
    double bin_z = zmax, prev_bin_z = zmax;  // the current bin's elevation, the bin above it
    uint32_t bin_mat = material[order[0]];
    layers.push_back({bin_mat, top, 0.0});
    for (uint64_t i = 0; i < E; ++i)
    {
        const uint64_t e = order[i];
        const double z = z_of(e);
        if (bin_z - z > tol)  // a new bin
        {
            prev_bin_z = bin_z;
            bin_z = z;
            bin_mat = material[e];
            if (bin_mat != layers.back().mat)
            {
                const double cut = 0.5 * (prev_bin_z + bin_z);
                const Layer up = layers.back();
                layers.push_back({bin_mat, cut, up.above + density[up.mat] * (up.top - cut)});
            }
        }
        else if (material[e] != bin_mat)
            return refuse(CWF_ERR_ARGUMENT, "the deposit is not horizontally layered",
                          "element=" + std::to_string(e) + "\nmaterial=" + std::to_string(material[e]) +
                              "\nlayer_material=" + std::to_string(bin_mat));
        layer_of[e] = (uint32_t)(layers.size() - 1);
    }
    for (uint64_t e = 0; e < E; ++e)
    {
        const Layer &l = layers[layer_of[e]];
        const double sv = -gravity * (l.above + density[l.mat] * (l.top - z_of(e)));
        const double sh = k0[l.mat] * sv;
        double *o = sig0 + 6 * e;
        for (int c = 0; c < 3; ++c)
            o[c] = c == axis ? sv : sh;
        o[3] = o[4] = o[5] = 0.0;
    }
    return 0;
}

}  // extern "C"
