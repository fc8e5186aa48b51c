// abi_explicit_plasticity.cpp -- the explicit stepper's plasticity (include/cwf_hip.h "Plasticity" and "Soil
// plasticity", explicit_state.hpp): the J2 set and the Drucker-Prager set with their slot tables (explicit_tables.cpp),
// reset, the state out, and the host-only element update cwf_explicit_j2_update (plasticity.hpp). What the soil model
// has that needs no stepper (cwf_explicit_dp_update among it) is soil.cpp's.
#include <algorithm>
#include <cmath>

#include "explicit_state.hpp"
#include "explicit_tables.hpp"
#include "plasticity.hpp"

using namespace cwf;

namespace
{
// the node pass a soil set launches when its descriptor leaves the choice to the library (DESIGN "Soil plasticity"
// has the measurement behind it)
constexpr int kSoilNodePass = 2;

// the slots' 64-B records on the host
int plastic_state(cwf_hip_explicit *t, std::vector<double> &state)
{
    cwf_hip_system *h = t->sys;
    state.resize(8ull * t->pl.dev.slots);
    if (state.empty())
        return 0;
    HIPTRY(h, hipMemcpyAsync(state.data(), t->pl.dev.state, state.size() * sizeof(double), hipMemcpyDeviceToHost,
                             h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

// What the two setters share once their own arguments passed: the refusals that need the stepper or the handle's
// arrays, then the new set. model 1: params = {sy, H} per material; model 2: {alpha, kappa, beta, H} per material and
// sig0 (nullable) = the caller's [E][6] stress at rest. Nothing changes before the last refusal.
int install_set(cwf_hip_explicit *t, int model, const std::vector<uint8_t> &plastic, const std::vector<double> &params,
                const double *sig0)
{
    cwf_hip_system *h = t->sys;
    const DevSys &ds = h->ds;
    const uint64_t N = ds.N, E = ds.E, M = ds.M;
    const bool any = std::find(plastic.begin(), plastic.end(), 1) != plastic.end();
    if (t->mon.ecum)
        return set_error(h, CWF_ERR_UNSUPPORTED, "the energy ledger and plasticity exclude each other",
                         "energy_every=" + std::to_string(t->mon.eevery));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    std::vector<double> D(36 * M);
    HIPTRY(h, hipMemcpy(D.data(), ds.dmat, D.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (uint64_t m = 0; m < M; ++m)
        if (plastic[m] && !iso_pattern(D.data() + 36 * m))
            return set_error(h, CWF_ERR_UNSUPPORTED, "a plastic material needs an isotropic stiffness",
                             "material=" + std::to_string(m));
    // the slots and the affected nodes' compact CSR, from the handle's own arrays: the node -> incidence CSR is in the
    // handle's node order and ascends in element per node
    std::vector<uint32_t> mat(E), off(N + 1), inc(4 * E);
    PlasticTables T;
    if (any)
    {
        HIPTRY(h, hipMemcpy(mat.data(), ds.mat, E * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPTRY(h, hipMemcpy(off.data(), ds.off, (N + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPTRY(h, hipMemcpy(inc.data(), ds.inc, 4 * E * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (sig0)
            for (uint64_t e = 0; e < E; ++e)
                for (int c = 0; c < 6 && mat[e] < M && plastic[mat[e]]; ++c)
                    if (!std::isfinite(sig0[6 * e + c]))
                        return set_error(h, CWF_ERR_ARGUMENT, "initial stress is not finite",
                                         "element=" + std::to_string(e) + "\ncomponent=" + std::to_string(c));
        if (plastic_tables(mat, off, inc, plastic, &T))
            return set_error(h, CWF_ERR_INDEX, "plastic incidences do not cover the elements' corners",
                             "incidences=" + std::to_string(T.incidences) +
                                 "\ncorners=" + std::to_string(T.cpos.size()));
    }
    if (T.elem.empty())  // every material elastic, or no element of a plastic one: nothing to run
    {
        t->pl.release(t->mem);
        return 0;
    }
    // the new set's buffers; the stepper's once everything went well
    const size_t slots = T.elem.size();
    ArenaStage stage(*t);
    cwf_hip_explicit::Plasticity m;
    ExplicitPlasticity &d = m.dev;
    m.model = model;
    d.slots = (uint32_t)slots;
    d.affected = (uint32_t)T.anode.size();
    d.elem = stage.put(T.elem);
    if (model == 1)
        d.yield_hard = stage.put(params);
    else
        m.soil.params = stage.put(params);
    d.state = stage.zeros<double>(8 * slots);
    d.corner = stage.zeros<float>(12 * slots);
    d.anode = stage.put(T.anode);
    d.aoff = stage.put(T.aoff);
    d.cpos = stage.put(T.cpos);
    d.p = stage.zeros<float>(std::max<size_t>(3 * N, 4));
    std::vector<double> z;  // the stress at rest slot-major; alive until finish() has synchronised
    if (model == 2 && sig0)
    {
        z.resize(6 * slots);
        for (size_t q = 0; q < slots; ++q)
            std::copy(sig0 + 6ull * T.elem[q], sig0 + 6ull * T.elem[q] + 6, &z[6 * q]);
        m.soil.sig0 = stage.put(z);
    }
    if (int st = stage.finish(model == 1 ? "explicit set_plasticity" : "explicit set_soil_plasticity"))
        return st;
    m.bytes = stage.bytes();
    m.elem = std::move(T.elem);
    m.held = stage.adopt();
    t->pl.release(t->mem);
    t->pl = std::move(m);
    return 0;
}
}  // namespace

extern "C" {

int cwf_explicit_j2_update(const double D[36], double yield, double hardening, double volume, const double strain[6],
                           double state[8], double sigma_p[6])
{
    if (!D || !strain || !state || !sigma_p)
        return 0;
    return j2_update(D, yield, hardening, volume, strain, state, state[6], state[7], sigma_p) ? 1 : 0;
}

int cwf_hip_explicit_set_plasticity(cwf_hip_explicit *t, const cwf_explicit_plasticity_desc *desc)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    hipStream_t s = h->stream;
    if (!desc)
    {
        HIPTRY(h, hipStreamSynchronize(s));
        t->pl.release(t->mem);
        return 0;
    }
    // everything that can be refused, on the host, before anything changes
    const DevSys &ds = h->ds;
    const uint64_t M = ds.M;
    if (ds.hex)
        return set_error(h, CWF_ERR_UNSUPPORTED, "plasticity needs tet4 elements", "element=hex8");
    if (desc->material_count != M)
        return set_error(h, CWF_ERR_ARGUMENT, "plasticity material count mismatch",
                         "material_count=" + std::to_string(desc->material_count) +
                             "\nmaterials=" + std::to_string(M));
    if (!desc->yield_stress || !desc->hardening)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    std::vector<uint8_t> plastic(M, 0);
    std::vector<double> yh(2 * M);
    for (uint64_t m = 0; m < M; ++m)
    {
        const double sy = desc->yield_stress[m], H = desc->hardening[m];
        if (!(sy >= 0.0) || !(H >= 0.0))
            return set_error(h, CWF_ERR_ARGUMENT, "yield stress and hardening must be non-negative",
                             "material=" + std::to_string(m) + "\nyield_stress=" + num17(sy) +
                                 "\nhardening=" + num17(H));
        plastic[m] = sy > 0.0 && std::isfinite(sy);
        yh[2 * m] = sy;
        yh[2 * m + 1] = H;
    }
    return install_set(t, 1, plastic, yh, nullptr);
}

int cwf_hip_explicit_set_soil_plasticity(cwf_hip_explicit *t, const cwf_explicit_soil_desc *desc)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    if (!desc)
    {
        HIPTRY(h, hipStreamSynchronize(h->stream));
        t->pl.release(t->mem);
        return 0;
    }
    const DevSys &ds = h->ds;
    const uint64_t M = ds.M;
    if (ds.hex)
        return set_error(h, CWF_ERR_UNSUPPORTED, "plasticity needs tet4 elements", "element=hex8");
    if (desc->material_count != M)
        return set_error(h, CWF_ERR_ARGUMENT, "plasticity material count mismatch",
                         "material_count=" + std::to_string(desc->material_count) +
                             "\nmaterials=" + std::to_string(M));
    if (!desc->alpha || !desc->kappa || !desc->beta || !desc->hardening)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    std::vector<uint8_t> plastic(M, 0);
    std::vector<double> par(4 * M);
    for (uint64_t m = 0; m < M; ++m)
    {
        const double al = desc->alpha[m], ka = desc->kappa[m], be = desc->beta[m], H = desc->hardening[m];
        // a NaN fails every comparison; kappa alone may be +inf (an elastic material)
        const bool ok = al >= 0.0 && std::isfinite(al) && ka >= 0.0 && be >= 0.0 && be <= al && H >= 0.0 &&
                        std::isfinite(H) && !(al == 0.0 && ka == 0.0);
        if (!ok)
            return set_error(h, CWF_ERR_ARGUMENT, "soil plasticity parameters out of range",
                             "material=" + std::to_string(m) + "\nalpha=" + num17(al) + "\nkappa=" + num17(ka) +
                                 "\nbeta=" + num17(be) + "\nhardening=" + num17(H));
        plastic[m] = std::isfinite(ka);
        par[4 * m] = al;
        par[4 * m + 1] = ka;
        par[4 * m + 2] = be;
        par[4 * m + 3] = H;
    }
    if (desc->initial_stress && desc->element_count != ds.E)
        return set_error(h, CWF_ERR_SIZE, "initial stress span size mismatch",
                         "span=" + std::to_string(desc->element_count) + "\nelements=" + std::to_string(ds.E));
    if (desc->node_pass > 3)
        return set_error(h, CWF_ERR_ARGUMENT, "unknown node pass", "node_pass=" + std::to_string(desc->node_pass));
    if (int st = install_set(t, 2, plastic, par, desc->initial_stress))
        return st;
    if (t->pl.dev.slots)
        t->pl.node_pass = desc->node_pass ? (int)desc->node_pass : kSoilNodePass;
    return 0;
}

int cwf_hip_explicit_plasticity_model(cwf_hip_explicit *t, int *model)
{
    if (int st = explicit_ready(t))
        return st;
    if (!model)
        return set_error(t->sys, CWF_ERR_ARGUMENT, "null pointer");
    *model = t->pl.dev.slots ? t->pl.model : 0;
    return 0;
}

int cwf_hip_explicit_reset_plasticity(cwf_hip_explicit *t)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    const ExplicitPlasticity &p = t->pl.dev;
    if (!p.slots)
        return 0;
    HIPTRY(h, hipMemsetAsync(p.state, 0, 8ull * p.slots * sizeof(double), h->stream));
    HIPTRY(h, hipMemsetAsync(p.corner, 0, 12ull * p.slots * sizeof(float), h->stream));
    HIPTRY(h, hipMemsetAsync(p.p, 0, std::max<size_t>(3ull * h->ds.N, 4) * sizeof(float), h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_explicit_plasticity_info(cwf_hip_explicit *t, cwf_explicit_plasticity_info *info)
{
    if (!t || !info)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    if (int st = check_ready(t->sys))
        return st;
    std::vector<double> state;
    if (int st = plastic_state(t, state))
        return st;
    cwf_explicit_plasticity_info I{};
    I.plastic_elements = t->pl.dev.slots;
    I.affected_nodes = t->pl.dev.affected;
    // yielded: abar > 0; the soil model's apex return from a stress without a deviator changes ep and leaves abar at 0,
    // so its elements also count once their plastic strain is not zero
    for (size_t q = 0; q < t->pl.dev.slots; ++q)
    {
        bool yielded = state[8 * q + 6] > 0.0;
        for (int r = 0; r < 6 && t->pl.model == 2 && !yielded; ++r)
            yielded = state[8 * q + r] != 0.0;
        I.yielded_elements += yielded ? 1 : 0;
    }
    I.bytes = t->pl.bytes;
    *info = I;
    return 0;
}

int cwf_hip_explicit_read_plasticity(cwf_hip_explicit *t, double *ep, double *abar, double *wp, uint64_t n)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    if (!t->pl.dev.slots)
        return set_error(h, CWF_ERR_ARGUMENT, "no plasticity is set");
    const uint64_t E = h->ds.E;
    if (n != E)
        return set_error(h, CWF_ERR_SIZE, "plasticity span size mismatch",
                         "span=" + std::to_string(n) + "\nelements=" + std::to_string(E));
    std::vector<double> state;
    if (int st = plastic_state(t, state))
        return st;
    if (ep)
        std::fill(ep, ep + 6 * E, 0.0);
    if (abar)
        std::fill(abar, abar + E, 0.0);
    if (wp)
        std::fill(wp, wp + E, 0.0);
    for (size_t q = 0; q < t->pl.elem.size(); ++q)
    {
        const uint32_t e = t->pl.elem[q];
        if (ep)
            std::copy(&state[8 * q], &state[8 * q] + 6, ep + 6ull * e);
        if (abar)
            abar[e] = state[8 * q + 6];
        if (wp)
            wp[e] = state[8 * q + 7];
    }
    return 0;
}

}  // extern "C"
