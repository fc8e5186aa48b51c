// absorbing.cpp -- host side of the explicit stepper's absorbing (viscous, Lysmer-Kuhlemeyer) boundaries
// (include/cwf_hip.h "Absorbing boundaries"): the dashpot matrices of a face list from the owning elements'
// materials, the per-node update matrices P, Q of the scheme, and the entries of an obliquely incident plane wave.
// No GPU; fp64, compiled with -ffp-contract=off.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "cwf_internal.hpp"

namespace
{
using Key = std::array<uint32_t, 4>;  // a face's nodes, ascending (a triangle's fourth is 0xFFFFFFFF)
struct KeyHash
{
    size_t operator()(const Key &k) const
    {
        uint64_t h = 0x9e3779b97f4a7c15ull;
        for (uint32_t v : k)
            h = (h ^ v) * 0xff51afd7ed558ccdull + (h >> 29);
        return (size_t)h;
    }
};
struct Owner
{
    uint32_t count = 0;
    uint64_t element = 0;
};

Key key_of(const uint32_t *n, uint32_t k)
{
    Key key = {n[0], n[1], n[2], k == 4 ? n[3] : 0xFFFFFFFFu};
    std::sort(key.begin(), key.end());
    return key;
}

constexpr int kTetFaces[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
// hex8 faces in the Gmsh corner order (meshgen.HEX_FACES)
constexpr int kHexFaces[6][4] = {{0, 3, 2, 1}, {4, 5, 6, 7}, {0, 1, 5, 4}, {1, 2, 6, 5}, {2, 3, 7, 6}, {3, 0, 4, 7}};

void tri_cross(const double *X, uint32_t i0, uint32_t i1, uint32_t i2, double *cr)
{
    const double *p0 = X + 3ull * i0, *p1 = X + 3ull * i1, *p2 = X + 3ull * i2;
    const double v1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const double v2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    cr[0] = (v1[1] * v2[2]) - (v1[2] * v2[1]);
    cr[1] = (v1[2] * v2[0]) - (v1[0] * v2[2]);
    cr[2] = (v1[0] * v2[1]) - (v1[1] * v2[0]);
}
double norm3(const double *v) { return std::sqrt((v[0] * v[0]) + (v[1] * v[1]) + (v[2] * v[2])); }
}  // namespace

namespace cwf
{
// P = A ((1 - h) I - B), Q = dt A with h = alpha dt / 2, B = C dt / (2 m), A = ((1 + h) I + B)^-1 (adjugate over
// determinant). -> 0, or the reason C, mass, alpha or dt is refused.
const char *dashpot_update(const double C[9], double mass, double alpha, double dt, double P[9], double Q[9])
{
    if (!std::isfinite(mass) || !(mass > 0.0))
        return "dashpot node mass must be positive";
    if (!std::isfinite(alpha) || !std::isfinite(dt) || alpha < 0.0 || dt < 0.0)
        return "dashpot update coefficients must be finite and non-negative";
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(C[i]))
            return "dashpot matrix is not finite";
    const double tr = C[0] + C[4] + C[8];
    const double tol = 1e-12 * std::fabs(tr);
    if (std::fabs(C[1] - C[3]) > tol || std::fabs(C[2] - C[6]) > tol || std::fabs(C[5] - C[7]) > tol)
        return "dashpot matrix is not symmetric";
    // positive semidefinite: every principal minor is non-negative (to rounding, relative to the trace)
    const double m01 = C[0] * C[4] - C[1] * C[3], m02 = C[0] * C[8] - C[2] * C[6], m12 = C[4] * C[8] - C[5] * C[7];
    const double det = C[0] * m12 - C[1] * (C[3] * C[8] - C[5] * C[6]) + C[2] * (C[3] * C[7] - C[4] * C[6]);
    if (tr < 0.0 || C[0] < -tol || C[4] < -tol || C[8] < -tol || m01 < -tol * tr || m02 < -tol * tr ||
        m12 < -tol * tr || det < -tol * tr * tr)
        return "dashpot matrix is not positive semidefinite";
    const double h = alpha * dt / 2.0, s = dt / (2.0 * mass);
    double M[9], R[9];
    for (int i = 0; i < 9; ++i)
    {
        const double b = C[i] * s, eye = (i % 4 == 0) ? 1.0 : 0.0;
        M[i] = (1.0 + h) * eye + b;
        R[i] = (1.0 - h) * eye - b;
    }
    const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    const double d = M[0] * c00 + M[1] * c01 + M[2] * c02;
    if (!std::isfinite(d) || !(d > 0.0))
        return "dashpot matrix is not positive semidefinite";
    const double A[9] = {c00 / d, (M[2] * M[7] - M[1] * M[8]) / d, (M[1] * M[5] - M[2] * M[4]) / d,
                         c01 / d, (M[0] * M[8] - M[2] * M[6]) / d, (M[2] * M[3] - M[0] * M[5]) / d,
                         c02 / d, (M[1] * M[6] - M[0] * M[7]) / d, (M[0] * M[4] - M[1] * M[3]) / d};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
        {
            P[3 * r + c] = (A[3 * r] * R[c] + A[3 * r + 1] * R[3 + c]) + A[3 * r + 2] * R[6 + c];
            Q[3 * r + c] = dt * A[3 * r + c];
        }
    return nullptr;
}
}  // namespace cwf

extern "C" int cwf_explicit_dashpot_update(const double C[9], double mass, double alpha, double dt, double P[9],
                                           double Q[9])
{
    using cwf::set_error;
    if (!C || !P || !Q)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    if (const char *why = cwf::dashpot_update(C, mass, alpha, dt, P, Q))
        return set_error(nullptr, CWF_ERR_ARGUMENT, why);
    return 0;
}

namespace
{
// what both face-list entry points need of a face: area, unit normal (the winding's), the element that owns it
struct FaceFrames
{
    std::vector<double> area, normal;
    std::vector<uint64_t> element;
};

// the faces' geometry and owners; 0 or the error (set)
int face_frames(uint64_t N, const double *coords, uint64_t E, uint32_t nodes_per_element, const uint32_t *connectivity,
                uint64_t F, uint32_t nodes_per_face, const uint32_t *faces, FaceFrames &out)
{
    using cwf::set_error;
    if (nodes_per_element != 4 && nodes_per_element != 8)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "elements must be tet4 or hex8",
                         "nodes_per_element=" + std::to_string(nodes_per_element));
    if (nodes_per_face != 3 && nodes_per_face != 4)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "absorbing faces must be triangles or quads",
                         "nodes_per_face=" + std::to_string(nodes_per_face));
    const uint32_t k = nodes_per_face;
    // area and unit normal per face; the faces' keys
    std::vector<double> &area = out.area, &normal = out.normal;
    area.assign(F, 0.0);
    normal.assign(3 * F, 0.0);
    std::unordered_map<Key, Owner, KeyHash> owners;
    std::vector<uint8_t> on_face(N, 0);
    for (uint64_t f = 0; f < F; ++f)
    {
        const uint32_t *n = faces + (uint64_t)k * f;
        for (uint32_t a = 0; a < k; ++a)
            if (n[a] >= N)
                return set_error(nullptr, CWF_ERR_NODE_RANGE, "absorbing face references node out of range",
                                 "face=" + std::to_string(f) + "\nnode=" + std::to_string(n[a]));
        double cr[3], c2[3] = {0.0, 0.0, 0.0};
        tri_cross(coords, n[0], n[1], n[2], cr);
        double a2 = 0.5 * norm3(cr);
        if (k == 4)  // the two triangles (0,1,2) + (0,2,3), as the traction loads
        {
            tri_cross(coords, n[0], n[2], n[3], c2);
            a2 = a2 + 0.5 * norm3(c2);
        }
        const double s[3] = {cr[0] + c2[0], cr[1] + c2[1], cr[2] + c2[2]};
        const double len = norm3(s);
        if (!std::isfinite(a2) || !(a2 > 0.0) || !std::isfinite(len) || !(len > 0.0))
            return set_error(nullptr, CWF_ERR_ARGUMENT, "absorbing face has zero area", "face=" + std::to_string(f));
        area[f] = a2;
        for (int c = 0; c < 3; ++c)
            normal[3 * f + c] = s[c] / len;
        owners.emplace(key_of(n, k), Owner{});
        for (uint32_t a = 0; a < k; ++a)
            on_face[n[a]] = 1;
    }
    // the elements that own them: only an element face whose nodes all lie on some listed face is looked up
    const uint32_t nf = nodes_per_element == 4 ? 4u : 6u, fk = nodes_per_element == 4 ? 3u : 4u;
    for (uint64_t e = 0; F && e < E; ++e)
    {
        const uint32_t *en = connectivity + (uint64_t)nodes_per_element * e;
        uint32_t hit = 0;
        for (uint32_t a = 0; a < nodes_per_element; ++a)
        {
            if (en[a] >= N)
                return set_error(nullptr, CWF_ERR_NODE_RANGE, "element references node out of range",
                                 "elements [" + std::to_string(e) + "]");
            hit += on_face[en[a]];
        }
        if (hit < fk || fk != k)
            continue;
        for (uint32_t q = 0; q < nf; ++q)
        {
            uint32_t fn[4];
            for (uint32_t a = 0; a < fk; ++a)
                fn[a] = en[nodes_per_element == 4 ? kTetFaces[q][a] : kHexFaces[q][a]];
            if (!(on_face[fn[0]] && on_face[fn[1]] && on_face[fn[2]] && (fk == 3 || on_face[fn[3]])))
                continue;
            const auto it = owners.find(key_of(fn, fk));
            if (it != owners.end())
            {
                ++it->second.count;
                it->second.element = e;
            }
        }
    }
    out.element.assign(F, 0);
    for (uint64_t f = 0; f < F; ++f)
    {
        const Owner &o = owners[key_of(faces + (uint64_t)k * f, k)];
        if (o.count != 1)
            return set_error(nullptr, CWF_ERR_ARGUMENT, "absorbing face is not a boundary face of the mesh",
                             "face=" + std::to_string(f));
        out.element[f] = o.element;
    }
    return 0;
}

// rho, V_p, V_s of face f's owning element; 0 or the error (set)
int face_speeds(uint64_t f, uint64_t element, const uint32_t *element_material, uint64_t material_count,
                const double *rho, const double *lame_lambda, const double *lame_mu, uint32_t *material, double *r,
                double *vp, double *vs)
{
    using cwf::set_error;
    const uint32_t mi = element_material[element];
    if (mi >= material_count)
        return set_error(nullptr, CWF_ERR_MATERIAL_RANGE, "element physical group missing assignment",
                         "elements [" + std::to_string(element) + "]");
    *material = mi;
    *r = rho[mi];
    *vp = std::sqrt((lame_lambda[mi] + 2.0 * lame_mu[mi]) / *r);
    *vs = std::sqrt(lame_mu[mi] / *r);
    if (!(*r > 0.0) || !std::isfinite(*vp) || !std::isfinite(*vs))
        return set_error(nullptr, CWF_ERR_MATERIALS, "absorbing face's material has no wave speeds",
                         "face=" + std::to_string(f) + "\nmaterial=" + std::to_string(mi));
    return 0;
}
}  // namespace

extern "C" int cwf_absorbing_dashpots(uint64_t N, const double *coords, uint64_t E, uint32_t nodes_per_element,
                                      const uint32_t *connectivity, const uint32_t *element_material,
                                      uint64_t material_count, const double *rho, const double *lame_lambda,
                                      const double *lame_mu, uint64_t F, uint32_t nodes_per_face,
                                      const uint32_t *faces, uint64_t *count, uint32_t *node_ids, double *C)
{
    using cwf::set_error;
    if (!count || (F && (!coords || !connectivity || !element_material || !rho || !lame_lambda || !lame_mu ||
                         !faces || !node_ids || !C)))
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    *count = 0;
    FaceFrames fr;
    if (int st = face_frames(N, coords, E, nodes_per_element, connectivity, F, nodes_per_face, faces, fr))
        return st;
    const uint32_t k = nodes_per_face;
    std::map<uint32_t, std::array<double, 9>> acc;
    for (uint64_t f = 0; f < F; ++f)
    {
        const uint32_t *n = faces + (uint64_t)k * f;
        uint32_t mi;
        double r, vp, vs;
        if (int st = face_speeds(f, fr.element[f], element_material, material_count, rho, lame_lambda, lame_mu, &mi,
                                 &r, &vp, &vs))
            return st;
        const double share = fr.area[f] / (double)k, *nu = fr.normal.data() + 3 * f;
        double Cf[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
            {
                const double nn = nu[i] * nu[j];
                Cf[3 * i + j] = (r * share) * (vp * nn + vs * ((i == j ? 1.0 : 0.0) - nn));
            }
        for (uint32_t a = 0; a < k; ++a)
        {
            auto &dst = acc.try_emplace(n[a], std::array<double, 9>{}).first->second;
            for (int i = 0; i < 9; ++i)
                dst[i] += Cf[i];
        }
    }
    uint64_t c = 0;
    for (const auto &kv : acc)
    {
        node_ids[c] = kv.first;
        std::copy(kv.second.begin(), kv.second.end(), C + 9 * c);
        ++c;
    }
    *count = c;
    return 0;
}

extern "C" int cwf_absorbing_incident_plane(uint64_t N, const double *coords, uint64_t E, uint32_t nodes_per_element,
                                            const uint32_t *connectivity, const uint32_t *element_material,
                                            uint64_t material_count, const double *rho, const double *lame_lambda,
                                            const double *lame_mu, uint64_t F, uint32_t nodes_per_face,
                                            const uint32_t *faces, const double polarisation[3],
                                            const double propagation[3], const double origin[3], uint64_t *count,
                                            uint32_t *node_ids, double *A, double *tau, double *wave_speed)
{
    using cwf::set_error;
    if (!count || !polarisation || !propagation || !origin ||
        (F && (!coords || !connectivity || !element_material || !rho || !lame_lambda || !lame_mu || !faces ||
               !node_ids || !A || !tau)))
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    *count = 0;
    const double klen = norm3(propagation), dlen = norm3(polarisation);
    if (!std::isfinite(klen) || !(klen > 0.0))
        return set_error(nullptr, CWF_ERR_ARGUMENT, "propagation must be a non-zero finite vector");
    if (!std::isfinite(dlen) || !(dlen > 0.0))
        return set_error(nullptr, CWF_ERR_ARGUMENT, "polarisation must be a non-zero finite vector");
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return set_error(nullptr, CWF_ERR_ARGUMENT, "origin must be finite");
    const double kh[3] = {propagation[0] / klen, propagation[1] / klen, propagation[2] / klen};
    const double *d = polarisation;
    const double dk = (d[0] * kh[0] + d[1] * kh[1]) + d[2] * kh[2];
    const double cosine = std::fabs(dk) / dlen;
    const bool pwave = cosine >= 1.0 - CWF_PLANE_WAVE_TOLERANCE;
    if (!pwave && !(cosine <= CWF_PLANE_WAVE_TOLERANCE))
    {
        char b[40];
        std::snprintf(b, sizeof b, "%.17g", cosine);
        return set_error(nullptr, CWF_ERR_ARGUMENT,
                         "polarisation is neither parallel nor perpendicular to the propagation",
                         std::string("cosine=") + b);
    }
    FaceFrames fr;
    if (int st = face_frames(N, coords, E, nodes_per_element, connectivity, F, nodes_per_face, faces, fr))
        return st;
    const uint32_t k = nodes_per_face;
    std::map<uint32_t, std::array<double, 3>> acc;
    uint32_t first_material = 0;
    double c = 0.0;
    for (uint64_t f = 0; f < F; ++f)
    {
        const uint32_t *n = faces + (uint64_t)k * f;
        uint32_t mi;
        double r, vp, vs;
        if (int st = face_speeds(f, fr.element[f], element_material, material_count, rho, lame_lambda, lame_mu, &mi,
                                 &r, &vp, &vs))
            return st;
        if (f == 0)
            first_material = mi;
        else if (mi != first_material)
            return set_error(nullptr, CWF_ERR_UNSUPPORTED, "plane wave faces span more than one material",
                             "face=" + std::to_string(f) + "\nmaterial=" + std::to_string(mi) +
                                 "\nfirst_material=" + std::to_string(first_material));
        c = pwave ? vp : vs;
        if (!(c > 0.0))
            return set_error(nullptr, CWF_ERR_MATERIALS, "absorbing face's material has no wave speeds",
                             "face=" + std::to_string(f) + "\nmaterial=" + std::to_string(mi));
        // the outward normal: away from the owning element's centroid
        const uint32_t *en = connectivity + (uint64_t)nodes_per_element * fr.element[f];
        double away[3];
        for (int q = 0; q < 3; ++q)
        {
            double fc = 0.0, ec = 0.0;
            for (uint32_t a = 0; a < k; ++a)
                fc += coords[3ull * n[a] + q];
            for (uint32_t a = 0; a < nodes_per_element; ++a)
                ec += coords[3ull * en[a] + q];
            away[q] = fc / (double)k - ec / (double)nodes_per_element;
        }
        const double *nw = fr.normal.data() + 3 * f;
        const double sign = ((away[0] * nw[0] + away[1] * nw[1]) + away[2] * nw[2]) < 0.0 ? -1.0 : 1.0;
        const double nu[3] = {sign * nw[0], sign * nw[1], sign * nw[2]};
        const double lam = lame_lambda[mi], mu = lame_mu[mi];
        const double dn = (d[0] * nu[0] + d[1] * nu[1]) + d[2] * nu[2];
        const double kn = (kh[0] * nu[0] + kh[1] * nu[1]) + kh[2] * nu[2];
        const double share = fr.area[f] / (double)k;
        double Af[3];
        for (int q = 0; q < 3; ++q)
        {
            const double dash = r * (vp * (dn * nu[q]) + vs * (d[q] - dn * nu[q]));
            const double trac = -((lam * dk) * nu[q] + mu * (d[q] * kn + kh[q] * dn)) / c;
            Af[q] = share * (dash + trac);
        }
        for (uint32_t a = 0; a < k; ++a)
        {
            auto &dst = acc.try_emplace(n[a], std::array<double, 3>{}).first->second;
            for (int q = 0; q < 3; ++q)
                dst[q] += Af[q];
        }
    }
    uint64_t cnt = 0;
    for (const auto &kv : acc)
    {
        const double *x = coords + 3ull * kv.first;
        node_ids[cnt] = kv.first;
        std::copy(kv.second.begin(), kv.second.end(), A + 3 * cnt);
        tau[cnt] = ((kh[0] * (x[0] - origin[0]) + kh[1] * (x[1] - origin[1])) + kh[2] * (x[2] - origin[2])) / c;
        ++cnt;
    }
    *count = cnt;
    if (wave_speed)
        *wave_speed = c;
    return 0;
}
