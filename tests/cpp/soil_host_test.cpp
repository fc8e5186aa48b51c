// soil_host_test.cpp -- the host-only part of the soil plasticity (csrc/soil.cpp): cwf_explicit_dp_update on the three
// outcomes with and without a stress at rest, cwf_soil_dp_from_mohr_coulomb, and cwf_soil_geostatic_stress on a
// six-element column small enough to state every expected entry, with its refusals. No GPU call. Builds stand-alone
// together with soil.cpp (-DCWF_SOIL_STANDALONE), then also under -fsanitize=address,undefined.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cwf_hip.h"

namespace
{
int failures = 0;

void expect(const char *what, bool ok)
{
    if (!ok)
    {
        std::printf("FAIL %s\n", what);
        ++failures;
    }
}

bool close(double a, double b, double rel) { return std::fabs(a - b) <= rel * std::fmax(std::fabs(a), std::fabs(b)); }

std::vector<double> iso(double E, double nu)
{
    const double lam = nu * E / ((1.0 + nu) * (1.0 - 2.0 * nu)), mu = E / (2.0 * (1.0 + nu));
    std::vector<double> D(36, 0.0);
    for (int r = 0; r < 3; ++r)
    {
        for (int k = 0; k < 3; ++k)
            D[6 * r + k] = r == k ? lam + 2.0 * mu : lam;
        D[7 * (r + 3)] = mu;
    }
    return D;
}

void return_map()
{
    const std::vector<double> D = iso(200.0e6, 0.3);
    const double mu = D[21], Kb = D[1] + (2.0 / 3.0) * mu;
    const double par[4] = {0.25, 5.0e3, 0.1, 0.0};
    const double p0 = 50.0e3, strength = par[1] + 3.0 * par[0] * p0;
    const double sig0[6] = {-p0, -p0, -p0, 0.0, 0.0, 0.0};
    double sp[6];
    {  // elastic under confinement, the same strain yields without it
        const double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.5 * strength / mu};
        std::vector<double> st(8, 0.0);
        expect("confined: elastic", cwf_explicit_dp_update(D.data(), par, sig0, 1.0, e, st.data(), sp) == 0);
        expect("confined: state untouched", st[5] == 0.0 && st[6] == 0.0 && sp[5] == 0.0);
        expect("unconfined: cone", cwf_explicit_dp_update(D.data(), par, nullptr, 1.0, e, st.data(), sp) == 1);
        expect("unconfined: plastic shear", st[5] > 0.0 && st[6] > 0.0 && st[7] > 0.0 && sp[5] == mu * st[5]);
    }
    {  // the cone: dl = f / (mu + 9 Kb alpha beta)
        const double gamma = 2.5 * strength / mu;
        const double e[6] = {0.0, 0.0, 0.0, 0.0, 0.0, gamma};
        std::vector<double> st(8, 0.0);
        expect("cone", cwf_explicit_dp_update(D.data(), par, sig0, 1.0, e, st.data(), sp) == 1);
        const double dl = (mu * gamma - strength) / (mu + 9.0 * Kb * par[0] * par[2]);
        expect("cone: dl", close(st[6], dl, 1e-12) && close(st[5], dl, 1e-12));
        expect("cone: dilation", close(st[0] + st[1] + st[2], 3.0 * par[2] * dl, 1e-12));
    }
    {  // the apex
        const double pa = par[1] / (3.0 * par[0]), eps = 4.0 * pa / (3.0 * Kb);
        const double e[6] = {eps, eps, eps, 0.0, 0.0, 0.0};
        std::vector<double> st(8, 0.0);
        expect("apex", cwf_explicit_dp_update(D.data(), par, nullptr, 1.0, e, st.data(), sp) == 2);
        expect("apex: mean stress", close(3.0 * Kb * (eps - st[0]), pa, 1e-12) && st[0] == st[1] && st[1] == st[2]);
    }
    {  // a NaN never yields; null arguments are answered, not read
        const double e[6] = {std::nan(""), 0.0, 0.0, 0.0, 0.0, 0.0};
        std::vector<double> st(8, 0.0);
        expect("nan", cwf_explicit_dp_update(D.data(), par, sig0, 1.0, e, st.data(), sp) == 0 && st[6] == 0.0);
        expect("null", cwf_explicit_dp_update(nullptr, par, sig0, 1.0, e, st.data(), sp) == 0);
    }
}

void mohr_coulomb()
{
    const double phi = std::asin(0.5);  // 30 degrees
    double out[3];
    expect("mc compression", cwf_soil_dp_from_mohr_coulomb(10.0e3, phi, 0.0, 0, out) == 0);
    expect("mc compression alpha", close(out[0], 2.0 * 0.5 / (std::sqrt(3.0) * 2.5), 1e-12) && out[2] == 0.0);
    expect("mc extension", cwf_soil_dp_from_mohr_coulomb(10.0e3, phi, phi, 1, out) == 0 && out[0] == out[2]);
    expect("mc extension alpha", close(out[0], 2.0 * 0.5 / (std::sqrt(3.0) * 3.5), 1e-12));
    expect("mc plane strain", cwf_soil_dp_from_mohr_coulomb(10.0e3, 0.0, 0.0, 2, out) == 0 && out[0] == 0.0);
    expect("mc plane strain kappa", close(out[1], 10.0e3, 1e-12));
    expect("mc bad match", cwf_soil_dp_from_mohr_coulomb(10.0e3, phi, 0.0, 3, out) == CWF_ERR_ARGUMENT);
    expect("mc psi > phi", cwf_soil_dp_from_mohr_coulomb(10.0e3, 0.1, 0.2, 0, out) == CWF_ERR_ARGUMENT);
    expect("mc null", cwf_soil_dp_from_mohr_coulomb(10.0e3, phi, 0.0, 0, nullptr) == CWF_ERR_ARGUMENT);
}

void geostatic()
{
    // six elements in a column along z, given out of order; the three upper ones are material 1
    const double z[6] = {0.5, 5.5, 2.5, 1.5, 4.5, 3.5};
    const uint32_t mat[6] = {0, 1, 0, 0, 1, 1};
    std::vector<double> cen(18, 0.25);
    for (int e = 0; e < 6; ++e)
        cen[3 * e + 2] = z[e];
    const double rho[2] = {2000.0, 1600.0}, k0[2] = {0.5, 0.4}, g = 9.81, top = 6.0;
    std::vector<double> s(36, -1.0);
    expect("geostatic", cwf_soil_geostatic_stress(6, cen.data(), mat, 2, rho, k0, g, 2, &top, 0, nullptr, s.data()) == 0);
    for (int e = 0; e < 6; ++e)
    {
        const double want = mat[e] ? -g * (rho[1] * (top - z[e])) : -g * (rho[1] * 3.0 + rho[0] * (3.0 - z[e]));
        expect("geostatic: vertical", close(s[6 * e + 2], want, 1e-14));
        expect("geostatic: horizontal", s[6 * e] == k0[mat[e]] * s[6 * e + 2] && s[6 * e + 1] == s[6 * e]);
        expect("geostatic: shears", s[6 * e + 3] == 0.0 && s[6 * e + 4] == 0.0 && s[6 * e + 5] == 0.0);
    }
    // the surface from the nodes
    const double nodes[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 6.0};
    std::vector<double> s2(36, -1.0);
    expect("geostatic from nodes",
           cwf_soil_geostatic_stress(6, cen.data(), mat, 2, rho, k0, g, 2, nullptr, 2, nodes, s2.data()) == 0 && s2 == s);
    // one material: exactly -g (rho depth)
    const uint32_t one[6] = {0, 0, 0, 0, 0, 0};
    expect("geostatic one", cwf_soil_geostatic_stress(6, cen.data(), one, 1, rho, k0, g, 2, &top, 0, nullptr, s.data()) == 0);
    for (int e = 0; e < 6; ++e)
        expect("geostatic one: exact", s[6 * e + 2] == -g * (rho[0] * (top - z[e])));
    // refusals
    const uint32_t side[6] = {0, 1, 0, 0, 1, 1};
    std::vector<double> flat(18, 0.25);  // every centroid at one elevation, two materials
    expect("not layered",
           cwf_soil_geostatic_stress(6, flat.data(), side, 2, rho, k0, g, 2, &top, 0, nullptr, s.data()) == CWF_ERR_ARGUMENT);
    const uint32_t bad[6] = {0, 1, 0, 7, 1, 1};
    expect("material index",
           cwf_soil_geostatic_stress(6, cen.data(), bad, 2, rho, k0, g, 2, &top, 0, nullptr, s.data()) == CWF_ERR_INDEX);
    const double low = 1.0;
    expect("above the surface",
           cwf_soil_geostatic_stress(6, cen.data(), mat, 2, rho, k0, g, 2, &low, 0, nullptr, s.data()) == CWF_ERR_ARGUMENT);
    expect("axis", cwf_soil_geostatic_stress(6, cen.data(), mat, 2, rho, k0, g, 3, &top, 0, nullptr, s.data()) == CWF_ERR_ARGUMENT);
    expect("no surface", cwf_soil_geostatic_stress(6, cen.data(), mat, 2, rho, k0, g, 2, nullptr, 0, nullptr, s.data()) ==
                             CWF_ERR_ARGUMENT);
    expect("no elements", cwf_soil_geostatic_stress(0, cen.data(), mat, 2, rho, k0, g, 2, &top, 0, nullptr, s.data()) == 0);
}
}  // namespace

int main()
{
    return_map();
    mohr_coulomb();
    geostatic();
    if (!failures)
        std::printf("ok\n");
    return failures ? 1 : 0;
}
