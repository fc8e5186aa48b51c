// abi_explicit.cpp -- the core of the explicit central-difference stepper of the C-ABI (include/cwf_hip.h "Explicit
// stepper"): create with the stable-step estimate (power iteration on M^-1 K), advance (per step: the handle's operator
// at scalars (1, 0) on a copy of its DevSys, then the node pass of explicit.hip), state access, the external force, its
// load pattern and curve, and the two host-only helpers. The attachments have a unit each (explicit_state.hpp lists
// them); what they share with the core is defined here.
#include <algorithm>
#include <cmath>

#include "explicit_state.hpp"

using namespace cwf;

namespace
{
// std::lerp as libstdc++ has it (loads.cpp:63-85 calls it)
double lerp_ref(double a, double b, double t)
{
    if ((a <= 0 && b >= 0) || (a >= 0 && b <= 0))
        return t * b + (1 - t) * a;
    if (t == 1)
        return b;
    const double x = a + t * (b - a);
    return ((t > 1) == (b > a)) ? (b < x ? x : b) : (b > x ? x : b);
}

int refuse_unfit(cwf_hip_system *h)
{
    if (h->sharded())
        return set_error(h, CWF_ERR_UNSUPPORTED, "explicit stepping of a sharded handle is not supported",
                         "ranks=" + std::to_string(h->nranks));
    if (!h->ds.E)
        return set_error(h, CWF_ERR_UNSUPPORTED, "explicit stepping needs elements", "elements=0");
    return 0;
}

// lambda_max(M^-1 K) over the free DOFs: x <- M^-1 K x / lambda_k with lambda_k = (y . M^-1 y) / (y . x), y = K x.
// Three vectors of its own, freed on return; the dots go through fast_dot / fast_fold (one fp64 partial per
// 256-DOF block, fixed tree) into the handle's partial and scalar scratch, which every solve rewrites before use
int power_iteration(cwf_hip_system *h, uint32_t iterations, double *lambda_max, double *last_change)
{
    const DevSys s = stiffness_only(h);
    hipStream_t st = h->stream;
    const size_t len = std::max<size_t>((size_t)s.D, 4);
    DevicePtr<float> buf;
    if (buf.alloc(3 * len) != hipSuccess)
        return set_error(h, CWF_ERR_ALLOC, "failed to allocate device buffer",
                         "bytes=" + std::to_string(3 * len * sizeof(float)));
    float *x = buf, *y = x + len, *z = y + len;
    const uint32_t nb = fast_dot_blocks(s.D);
    (void)hipMemsetAsync(h->scal, 0, 4 * sizeof(double), st);
    explicit_power_start(s.N, s.mask, x, st);
    for (uint32_t it = 0; it < iterations; ++it)
    {
        keff_apply_ds(h, s, x, y, true, st);
        explicit_power_z(s.N, s.mass, s.mask, y, z, st);
        fast_dot(y, z, x, s.D, h->part0, h->part1, st);
        fast_fold(h->part0, nb, h->scal + 0, st);
        fast_fold(h->part1, nb, h->scal + 1, st);
        explicit_power_scale(s.D, z, h->scal, x, h->scal + 2 + (it & 1u), st);
    }
    double lam[2] = {0.0, 0.0};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(lam, h->scal + 2, sizeof lam, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e != hipSuccess)
        return hip_fail(h, e, "power iteration");
    const double last = lam[(iterations - 1) & 1u], prev = lam[iterations & 1u];
    if (!(last > 0.0) || !std::isfinite(last))
        return set_error(h, CWF_ERR_DENOM_ZERO, "power iteration found no positive stiffness",
                         "lambda_max=" + num17(last));
    *lambda_max = last;
    if (last_change)
        *last_change = iterations > 1 ? std::fabs(last - prev) / last : 1.0;
    return 0;
}

double curve_at(const cwf_hip_explicit *t, double time)
{
    return cwf_explicit_curve_value(t->ctimes.data(), t->cvalues.data(), t->ctimes.size(), time);
}

void fill(const cwf_hip_explicit *t, cwf_explicit_telemetry *tel, bool finite)
{
    if (!tel)
        return;
    cwf_explicit_telemetry T{};
    T.time = (double)t->steps * t->dt;
    T.dt = t->dt;
    T.lambda_max = t->lambda_max;
    T.critical_dt = t->critical_dt;
    T.steps = t->steps;
    T.finite = finite ? 1 : 0;
    *tel = T;
}
}  // namespace

int cwf::nodes_listed_once(cwf_hip_system *h, const char *stem, const std::string &prefix, const uint32_t *ids,
                           uint64_t count, std::vector<uint32_t> &seen, uint32_t stamp)
{
    const uint64_t N = h->ds.N;
    for (uint64_t i = 0; i < count; ++i)
    {
        const uint32_t node = ids[i];
        if (node >= N || seen[node] == stamp)
            return set_error(h, CWF_ERR_ARGUMENT, std::string(stem) + (node >= N ? " out of range" : " listed twice"),
                             prefix + "index=" + std::to_string(i) + "\nnode=" + std::to_string(node));
        seen[node] = stamp;
    }
    return 0;
}

int cwf::slots_to_internal(TransientState &t, const std::vector<uint32_t> &slot, uint32_t *dev,
                           std::vector<uint32_t> *back)
{
    cwf_hip_system *h = t.sys;
    DevicePtr<uint32_t> own;
    if (!dev)
    {
        if (own.alloc(slot.size()) != hipSuccess)
            return set_error(h, CWF_ERR_ALLOC, t.alloc_error);
        dev = own;
    }
    if (int st = vec_in(h, reinterpret_cast<const float *>(slot.data()), reinterpret_cast<float *>(dev), CWF_PTR_HOST, 1))
        return st;
    if (back)
    {
        back->resize(h->ds.N);
        HIPTRY(h, hipMemcpyAsync(back->data(), dev, h->ds.N * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_explicit::sync_ledger_C(bool ledger, const std::vector<double> &C, const char *what)
{
    ArenaStage stage(*this);
    double *fresh = ledger && !C.empty() ? stage.put(C) : nullptr;
    if (int st = stage.finish(what))
        return st;
    stage.adopt();
    mem.free(dC);
    dC = fresh;
    return 0;
}

extern "C" {

double cwf_explicit_critical_dt(double lambda_max, double rayleigh_beta)
{
    if (!(lambda_max > 0.0))
        return 0.0;
    const double omega = std::sqrt(lambda_max);
    const double xi = rayleigh_beta * omega / 2.0;
    return (2.0 / omega) * (std::sqrt(1.0 + xi * xi) - xi);
}

double cwf_explicit_curve_value(const double *times, const double *values, uint64_t n, double t)
{
    if (n == 0 || !times || !values)
        return 1.0;
    if (t <= times[0])
        return values[0];
    for (uint64_t i = 1; i < n; ++i)
        if (t <= times[i])
        {
            const double span = times[i] - times[i - 1];
            const double w = span > 0.0 ? (t - times[i - 1]) / span : 0.0;
            return lerp_ref(values[i - 1], values[i], w);
        }
    return values[n - 1];
}

int cwf_hip_lambda_max(cwf_hip_system *h, uint32_t iterations, double *lambda_max, double *last_change)
{
    if (int st = check_ready(h))
        return st;
    if (!lambda_max)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    if (int st = refuse_unfit(h))
        return st;
    return power_iteration(h, iterations ? iterations : 60u, lambda_max, last_change);
}

void cwf_hip_explicit_destroy(cwf_hip_explicit *t)
{
    if (!t)
        return;
    transient_quiesce(*t);
    delete t;
}

int cwf_hip_explicit_create(cwf_hip_system *h, const cwf_explicit_desc *desc, cwf_hip_explicit **out)
{
    if (int st = check_ready(h))
        return st;
    if (!desc || !out)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    *out = nullptr;
    if (int st = refuse_unfit(h))
        return st;
    const double safety = desc->safety == 0.0 ? 0.9 : desc->safety;
    if (!(desc->rayleigh_alpha >= 0.0) || !(desc->rayleigh_beta >= 0.0) || !(desc->dt >= 0.0))
        return set_error(h, CWF_ERR_ARGUMENT, "explicit stepper coefficients must be non-negative",
                         "rayleigh_alpha=" + num17(desc->rayleigh_alpha) + "\nrayleigh_beta=" +
                             num17(desc->rayleigh_beta) + "\ndt=" + num17(desc->dt));
    if (!(safety > 0.0 && safety <= 1.0))
        return set_error(h, CWF_ERR_ARGUMENT, "safety must be in (0, 1]", "safety=" + num17(safety));
    double lam = 0.0;
    if (int st = power_iteration(h, desc->power_iterations ? desc->power_iterations : 60u, &lam, nullptr))
        return st;
    const double crit = cwf_explicit_critical_dt(lam, desc->rayleigh_beta);
    const double dt = desc->dt > 0.0 ? desc->dt : safety * crit;
    if (dt > crit)
        return set_error(h, CWF_ERR_ARGUMENT, "time step exceeds the critical step",
                         "dt=" + num17(dt) + "\ncritical_dt=" + num17(crit));
    auto *t = new (std::nothrow) cwf_hip_explicit();
    if (!t)
        return set_error(h, CWF_ERR_ALLOC, "host allocation failed");
    t->sys = h;
    t->alloc_error = "failed to allocate explicit stepper buffers";
    t->alpha = desc->rayleigh_alpha;
    t->beta = desc->rayleigh_beta;
    t->dt = dt;
    t->lambda_max = lam;
    t->critical_dt = crit;
    std::vector<float **> bufs = {&t->u, &t->v, &t->f, &t->bcv};
    if (t->beta != 0.0)
        bufs.push_back(&t->w);
    if (h->mode != CWF_MODE_FAST)
        bufs.push_back(&t->y);
    int st = 0;
    for (float **p : bufs)
        st = st ? st : t->alloc_vector(p);
    st = st ? st : t->alloc(&t->non_finite, 1);
    if (!st)
    {
        if (!t->w)
            t->w = t->u;
        (void)hipMemsetAsync(t->non_finite, 0, sizeof(uint32_t), h->stream);
        st = transient_start(*t, desc->external_force, desc->bc_value, "explicit stepper create");
    }
    if (st)
    {
        cwf_hip_explicit_destroy(t);
        return st;
    }
    *out = t;
    return 0;
}

int cwf_hip_explicit_advance(cwf_hip_explicit *t, uint64_t n_steps, cwf_explicit_telemetry *tel)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    hipStream_t st = h->stream;
    const DevSys s = stiffness_only(h);
    const bool fast = h->mode == CWF_MODE_FAST;
    if (fast != (t->y == nullptr))
        return set_error(h, CWF_ERR_ARGUMENT, "the handle's mode changed after the explicit stepper was created");
    const bool damp = t->w != t->u;
    if (damp && t->input_stale && n_steps)
        explicit_operator_input(s.N, t->u, t->v, t->beta, t->w, st);
    const double half = t->alpha * t->dt / 2.0;
    const bool pattern = t->lbase && !t->ctimes.empty();
    ExplicitPass a{};
    a.u = t->u;
    a.v = t->v;
    a.w = t->w;
    a.y = t->y;
    a.f = t->f;
    a.bcv = t->bcv;
    a.lbase = pattern ? t->lbase : nullptr;
    a.lpat = pattern ? t->lpat : nullptr;
    a.c1 = (1.0 - half) / (1.0 + half);
    a.c2 = t->dt / (1.0 + half);
    a.dt = t->dt;
    a.beta = t->beta;
    a.non_finite = t->non_finite;
    const bool dash = !t->dash_ids.empty();
    const ExplicitTies &tie = t->slots.tie;  // groups == 0: no set, no gather launch, the passes without TIE
    a.dslot = t->slots.dslot;
    a.dpq = t->slots.dpq;
    a.dC = dash ? t->dC : nullptr;
    a.tg = tie.groups ? tie.tg : nullptr;
    a.dgroup = t->slots.dgroup;
    a.dash_slots = t->slots.dash_slots;
    a.alpha = t->alpha;
    const ExplicitPlasticity &pl = t->pl.dev;
    a.p = pl.slots ? pl.p : nullptr;
    const uint32_t blocks = explicit_update_blocks(s.N);
    ExplicitElementPass ep{};
    // the launch order of a step: plasticity, operator, sources, tie gather, update, energy fold, receiver record,
    // element monitors
    for (uint64_t i = 0; i < n_steps; ++i)
    {
        if (pattern)
            a.scale = t->last_scale = curve_at(t, (double)t->steps * t->dt);
        if (pl.slots)  // the return map at u_n and the affected nodes' correction force, before the operator launch
        {
            if (t->pl.model == 2)
                explicit_soil_plasticity(s, t->u, pl, t->pl.soil, t->pl.node_pass, st);
            else
                explicit_plasticity(s, t->u, pl, st);
        }
        if (fast)
            fast_keff_partials_ds(s, t->w, true, st);
        else
            parity_keff_ds(s, t->w, t->y, true, nullptr, st);
        if (t->src.dev.loaded)  // f_n of the loaded nodes into the force buffer the update pass reads
            explicit_sources(t->src.dev, (double)t->steps * t->dt, t->f, st);
        if (tie.groups)  // g_G of every tie group from what the update pass is about to read
            explicit_tie_gather(s, a, tie, st);
        const bool ledger_sampled = t->mon.arm(a, t->steps + 1);
        explicit_update(s, a, st);
        ++t->steps;
        t->mon.sample(t->steps, ledger_sampled, blocks, t->u, t->v, st);
        if (t->emon.arm(ep, t->steps))
        {
            explicit_element_monitors(s, t->u, ep, st);
            t->emon.recorded(ep, t->steps);
        }
    }
    if (n_steps)
        t->input_stale = false;
    uint32_t word = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(&word, t->non_finite, sizeof word, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e != hipSuccess)
        return hip_fail(h, e, "explicit advance");
    fill(t, tel, word == 0);
    if (word)
        return set_error(h, CWF_ERR_HIP, "explicit step produced a non-finite value",
                         "steps=" + std::to_string(t->steps));
    return 0;
}

int cwf_hip_explicit_get_state(cwf_hip_explicit *t, int which, float *out, uint64_t n, int kind)
{
    if (!t || !out)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    const float *src = which == 0   ? t->u
                       : which == 1 ? t->v
                       : which == 4 ? t->f
                       : which == 5 ? (t->pl.dev.slots ? t->pl.dev.p : nullptr)
                                    : nullptr;
    // the update pass formed f_n in registers: the same rounding, on request
    const bool reform = which == 4 && t->lbase && !t->ctimes.empty() && t->steps;
    return transient_get(*t, src, out, n, kind, reform ? &t->last_scale : nullptr);
}

int cwf_hip_explicit_set_state(cwf_hip_explicit *t, int which, const float *in, uint64_t n, int kind)
{
    if (!t || !in)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    cwf_hip_system *h = t->sys;
    float *dst = which == 0 ? t->u : which == 1 ? t->v : nullptr;  // f (4) is set through set_external_force
    if (int st = transient_set(*t, "state", dst, in, n, kind, false))
        return st;
    t->input_stale = true;
    HIPTRY(h, hipMemsetAsync(t->non_finite, 0, sizeof(uint32_t), h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    if (which == 1)  // a tie group keeps one velocity
        return t->project_tied_velocity();
    return 0;
}

int cwf_hip_explicit_set_external_force(cwf_hip_explicit *t, const float *f, uint64_t n, int kind)
{
    if (!t || !f)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    if (int st = transient_set(*t, "external force", t->f, f, n, kind))
        return st;
    if (t->src.dev.loaded)  // the loaded nodes' f_ext follows
    {
        cwf_hip_system *h = t->sys;
        explicit_sources_fext(t->src.dev, t->f, true, h->stream);
        HIPTRY(h, hipGetLastError());
        HIPTRY(h, hipStreamSynchronize(h->stream));
    }
    return 0;
}

int cwf_hip_explicit_set_load_pattern(cwf_hip_explicit *t, const double *base, const double *pattern, uint64_t n)
{
    if (!t || !base || !pattern)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    if (t->src.dev.loaded)
        return set_error(t->sys, CWF_ERR_UNSUPPORTED, "load sources and a load pattern exclude each other",
                         "sources=" + std::to_string(t->src.given.size()));
    return transient_set_load_pattern(*t, base, pattern, n);
}

int cwf_hip_explicit_set_load_curve(cwf_hip_explicit *t, const double *times, const double *values, uint64_t count)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (count == 0)
    {
        t->ctimes.clear();
        t->cvalues.clear();
        return 0;
    }
    if (!times || !values)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    if (count > CWF_EXPLICIT_MAX_CURVE_POINTS)
        return set_error(h, CWF_ERR_SIZE, "load curve has too many points",
                         "count=" + std::to_string(count) + "\nmax=" + std::to_string(CWF_EXPLICIT_MAX_CURVE_POINTS));
    for (uint64_t i = 1; i < count; ++i)
        if (!(times[i] >= times[i - 1]))
            return set_error(h, CWF_ERR_ARGUMENT, "load curve times must ascend", "index=" + std::to_string(i));
    t->ctimes.assign(times, times + count);
    t->cvalues.assign(values, values + count);
    return 0;
}

int cwf_hip_explicit_time(const cwf_hip_explicit *t, double *current_time, double *time_step)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    return transient_time((double)t->steps * t->dt, t->dt, current_time, time_step);
}

}  // extern "C"
