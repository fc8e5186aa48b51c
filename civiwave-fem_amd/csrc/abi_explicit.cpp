// abi_explicit.cpp -- the explicit central-difference stepper of the C-ABI (include/cwf_hip.h "Explicit stepper"):
// create with the stable-step estimate (power iteration on M^-1 K), advance (per step: the handle's operator at
// scalars (1, 0) on a copy of its DevSys, then the node pass of explicit.hip), state access, the external force,
// its load pattern and curve, the load sources, and the two host-only helpers.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "abi_internal.hpp"
#include "plasticity.hpp"

using namespace cwf;

// u, v, f, bcv, the load pattern and the arena: the shared state core (abi_transient.cpp)
struct cwf_hip_explicit : TransientState
{
    double alpha = 0.0, beta = 0.0, dt = 0.0, lambda_max = 0.0, critical_dt = 0.0;
    uint64_t steps = 0;
    bool input_stale = true;  // beta_R != 0: w has to be formed from u and v before the next step
    float *w = nullptr, *y = nullptr;
    uint32_t *non_finite = nullptr;
    std::vector<double> ctimes, cvalues;  // set_load_curve
    double last_scale = 0.0;              // c(t) of the last step taken (get_state 4 with a pattern)
    // set_dashpots: the caller's ids and matrices as given; on the device a u32 slot per node (internal order,
    // allocated at the first set) and the P | Q records of the current set. Empty ids: no dashpots.
    std::vector<uint32_t> dash_ids;
    std::vector<double> dash_C;
    uint32_t *dslot = nullptr;
    DevicePtr<double> dpq;
    // set_monitors: the set in force, its device buffers (the stepper's arena) and the host's sample bookkeeping
    struct Monitors
    {
        uint64_t rcount = 0, revery = 0, rcap = 0, rdropped = 0;
        uint32_t *rnode = nullptr;             // [rcount] internal node of each receiver
        float *ru = nullptr, *rv = nullptr;    // [rcap][rcount][3]
        std::vector<uint64_t> rsteps;          // the step count of each row held
        float *peak = nullptr;                 // [3][peak_stride]
        uint64_t peak_stride = 0;
        uint64_t eevery = 0, ecap = 0, edropped = 0;
        double *ecum = nullptr, *ecur = nullptr, *erows = nullptr;  // [2 blocks], [2 blocks], [ecap][4]
        std::vector<uint64_t> esteps;
        void release(DeviceArena &mem)
        {
            for (void *p : {(void *)rnode, (void *)ru, (void *)rv, (void *)peak, (void *)ecum, (void *)ecur,
                            (void *)erows})
                mem.free(p);
            *this = Monitors();
        }
    } mon;
    double *dC = nullptr;  // the ledger's slot-indexed C array (arena), while a ledger and dashpots are both set
    // set_sources: the set in force as given (get_sources) and its device arrays (the stepper's arena); dev.loaded == 0:
    // no set
    struct Sources
    {
        struct Given
        {
            std::vector<double> times, values, amplitude, delay;
            std::vector<uint32_t> ids;
        };
        std::vector<Given> given;
        uint64_t entries = 0, points = 0, bytes = 0;
        ExplicitSources dev{};
        void release(DeviceArena &mem)
        {
            for (const void *p : {(const void *)dev.node, (const void *)dev.off, (const void *)dev.rec,
                                  (const void *)dev.cur, (const void *)dev.tab, (const void *)dev.fext})
                mem.free(const_cast<void *>(p));
            *this = Sources();
        }
    } src;
    // set_element_monitors: the set in force, its device buffers (the stepper's arena) and the host's sample bookkeeping
    struct ElementMonitors
    {
        uint64_t gcount = 0, gevery = 0, gcap = 0, gdropped = 0;
        uint32_t *gelem = nullptr;     // [gcount] the gauge elements (elements keep the caller's numbering)
        float *grows = nullptr;        // [gcap][gcount][13]
        std::vector<uint64_t> gsteps;  // the step count of each row held
        uint64_t eevery = 0, esamples = 0, stride = 0;
        uint32_t maps = 0;
        float *vm = nullptr, *shear = nullptr;  // [stride]
        float *range = nullptr;                 // [12][stride]: min of component c at plane c, max at 6 + c
        void release(DeviceArena &mem)
        {
            for (void *p : {(void *)gelem, (void *)grows, (void *)vm, (void *)shear, (void *)range})
                mem.free(p);
            *this = ElementMonitors();
        }
    } emon;
    // set_plasticity: the set in force (dev.slots == 0: none), its device arrays (the stepper's arena), the slots'
    // elements on the host (read_plasticity scatters through them) and the values as given
    struct Plasticity
    {
        ExplicitPlasticity dev{};
        std::vector<uint32_t> elem;
        uint64_t bytes = 0;
        void release(DeviceArena &mem)
        {
            for (const void *p : {(const void *)dev.elem, (const void *)dev.yield_hard, (const void *)dev.state,
                                  (const void *)dev.corner, (const void *)dev.anode, (const void *)dev.aoff,
                                  (const void *)dev.cpos, (const void *)dev.p})
                mem.free(const_cast<void *>(p));
            *this = Plasticity();
        }
    } pl;
};

namespace
{
std::string num(double v)
{
    char b[40];
    std::snprintf(b, sizeof b, "%.17g", v);
    return b;
}

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
                         "lambda_max=" + num(last));
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
                         "rayleigh_alpha=" + num(desc->rayleigh_alpha) + "\nrayleigh_beta=" +
                             num(desc->rayleigh_beta) + "\ndt=" + num(desc->dt));
    if (!(safety > 0.0 && safety <= 1.0))
        return set_error(h, CWF_ERR_ARGUMENT, "safety must be in (0, 1]", "safety=" + num(safety));
    double lam = 0.0;
    if (int st = power_iteration(h, desc->power_iterations ? desc->power_iterations : 60u, &lam, nullptr))
        return st;
    const double crit = cwf_explicit_critical_dt(lam, desc->rayleigh_beta);
    const double dt = desc->dt > 0.0 ? desc->dt : safety * crit;
    if (dt > crit)
        return set_error(h, CWF_ERR_ARGUMENT, "time step exceeds the critical step",
                         "dt=" + num(dt) + "\ncritical_dt=" + num(crit));
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
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
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
    a.dslot = dash ? t->dslot : nullptr;
    a.dpq = dash ? t->dpq.get() : nullptr;
    // monitors: the host knows every step count, so which update is sampled and the row it lands in are launch
    // arguments; there are no device counters
    cwf_hip_explicit::Monitors &mon = t->mon;
    a.peak = mon.peak;
    a.peak_stride = mon.peak_stride;
    a.ecum = mon.ecum;
    a.ecur = mon.ecur;
    a.dC = dash ? t->dC : nullptr;
    a.alpha = t->alpha;
    const ExplicitPlasticity &pl = t->pl.dev;
    a.p = pl.slots ? pl.p : nullptr;
    const uint32_t blocks = explicit_update_blocks(s.N);
    cwf_hip_explicit::ElementMonitors &em = t->emon;
    ExplicitElementPass ep{};
    ep.von_mises = em.vm;
    ep.shear_strain = em.shear;
    ep.stress_range = em.range;
    ep.stride = em.stride;
    ep.gauge_count = (uint32_t)em.gcount;
    ep.gauge_elements = em.gelem;
    for (uint64_t i = 0; i < n_steps; ++i)
    {
        if (pattern)
            a.scale = t->last_scale = curve_at(t, (double)t->steps * t->dt);
        if (pl.slots)  // the return map at u_n and the affected nodes' correction force, before the operator launch
            explicit_plasticity(s, t->u, pl, st);
        if (fast)
            fast_keff_partials_ds(s, t->w, true, st);
        else
            parity_keff_ds(s, t->w, t->y, true, nullptr, st);
        if (t->src.dev.loaded)  // f_n of the loaded nodes into the force buffer the update pass reads
            explicit_sources(t->src.dev, (double)t->steps * t->dt, t->f, st);
        const bool edue = mon.eevery && (t->steps + 1) % mon.eevery == 0;
        a.esample = edue && mon.esteps.size() < mon.ecap ? 1u : 0u;
        explicit_update(s, a, st);
        ++t->steps;
        if (a.esample)
        {
            explicit_energy_fold(blocks, mon.ecum, mon.ecur, mon.erows + 4 * mon.esteps.size(), st);
            mon.esteps.push_back(t->steps);
        }
        else if (edue)
            ++mon.edropped;
        if (mon.rcount && t->steps % mon.revery == 0)
        {
            if (mon.rsteps.size() < mon.rcap)
            {
                const size_t row = 3 * mon.rcount * mon.rsteps.size();
                explicit_record((uint32_t)mon.rcount, mon.rnode, t->u, t->v, mon.ru + row, mon.rv + row, st);
                mon.rsteps.push_back(t->steps);
            }
            else
                ++mon.rdropped;
        }
        // element monitors: u_steps through the post stack's element pass, envelopes over all elements, gauges per gauge
        if (em.eevery || em.gcount)
        {
            ep.envelope = em.eevery && t->steps % em.eevery == 0;
            ep.gauge_row = nullptr;
            if (em.gcount && t->steps % em.gevery == 0)
            {
                if (em.gsteps.size() < em.gcap)
                    ep.gauge_row = em.grows + 13 * em.gcount * em.gsteps.size();
                else
                    ++em.gdropped;
            }
            explicit_element_monitors(s, t->u, ep, st);
            if (ep.envelope)
                ++em.esamples;
            if (ep.gauge_row)
                em.gsteps.push_back(t->steps);
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

int cwf_hip_explicit_set_dashpots(cwf_hip_explicit *t, uint64_t count, const uint32_t *node_ids, const double *C)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    if (count && (!node_ids || !C))
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    const uint64_t N = h->ds.N;
    hipStream_t s = h->stream;
    if (count == 0)
    {
        HIPTRY(h, hipStreamSynchronize(s));
        t->dpq.reset();
        t->mem.free(t->dC);
        t->dC = nullptr;
        t->dash_ids.clear();
        t->dash_C.clear();
        return 0;
    }
    // everything that can be refused, on the host, before anything changes
    std::vector<uint32_t> slot(std::max<uint64_t>(N, 4), kNoDashpot);
    for (uint64_t i = 0; i < count; ++i)
    {
        if (node_ids[i] >= N)
            return set_error(h, CWF_ERR_ARGUMENT, "dashpot node out of range",
                             "index=" + std::to_string(i) + "\nnode=" + std::to_string(node_ids[i]));
        if (slot[node_ids[i]] != kNoDashpot)
            return set_error(h, CWF_ERR_ARGUMENT, "dashpot node listed twice",
                             "index=" + std::to_string(i) + "\nnode=" + std::to_string(node_ids[i]));
        slot[node_ids[i]] = (uint32_t)i;
    }
    std::vector<float> mass(std::max<uint64_t>(N, 4));  // the f32 lumped mass in the caller's order
    if (int st = vec_out(h, h->ds.mass, mass.data(), CWF_PTR_HOST, 1))
        return st;
    HIPTRY(h, hipStreamSynchronize(s));
    std::vector<double> pq(18 * count);
    for (uint64_t i = 0; i < count; ++i)
        if (const char *why = dashpot_update(C + 9 * i, (double)mass[node_ids[i]], t->alpha, t->dt, &pq[18 * i],
                                             &pq[18 * i + 9]))
            return set_error(h, CWF_ERR_ARGUMENT, why, "index=" + std::to_string(i));
    DevicePtr<double> rec;  // the new set's records: the stepper's once everything else went well
    if (rec.alloc(pq.size()) != hipSuccess)
        return set_error(h, CWF_ERR_ALLOC, t->alloc_error);
    if (!t->dslot)
        if (int st = t->alloc(&t->dslot, slot.size()))
            return st;
    double *newC = nullptr;  // a ledger reads C as given: its slot-indexed array follows the set
    if (t->mon.ecum)
        if (int st = t->alloc(&newC, 9 * count))
            return st;
    hipError_t e = hipMemcpyAsync(rec, pq.data(), pq.size() * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && newC)
        e = hipMemcpyAsync(newC, C, 9 * count * sizeof(double), hipMemcpyHostToDevice, s);
    int st = 0;
    if (e == hipSuccess)  // the slots move to the internal order as a one-word node vector (bit copies)
        st = vec_in(h, reinterpret_cast<const float *>(slot.data()), reinterpret_cast<float *>(t->dslot),
                    CWF_PTR_HOST, 1);
    if (e == hipSuccess && !st)
        e = hipStreamSynchronize(s);
    if (e != hipSuccess || st)
    {
        (void)hipStreamSynchronize(s);
        t->dash_ids.clear();  // the slot array may be half written: no dashpots until the next set
        t->dash_C.clear();
        t->mem.free(newC);
        return st ? st : hip_fail(h, e, "explicit set_dashpots");
    }
    t->mem.free(t->dC);
    t->dC = newC;
    t->dpq = std::move(rec);
    t->dash_ids.assign(node_ids, node_ids + count);
    t->dash_C.assign(C, C + 9 * count);
    return 0;
}

int cwf_hip_explicit_get_dashpots(cwf_hip_explicit *t, uint64_t *count, uint32_t *node_ids, double *C)
{
    if (!t || !count)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    *count = t->dash_ids.size();
    if (node_ids)
        std::copy(t->dash_ids.begin(), t->dash_ids.end(), node_ids);
    if (C)
        std::copy(t->dash_C.begin(), t->dash_C.end(), C);
    return 0;
}

int cwf_hip_explicit_set_sources(cwf_hip_explicit *t, const cwf_explicit_source_desc *sources, uint32_t count)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    hipStream_t s = h->stream;
    cwf_hip_explicit::Sources &cur = t->src;
    if (count == 0)
    {
        if (cur.dev.loaded)
        {
            explicit_sources_fext(cur.dev, t->f, false, s);  // f_ext back into the force buffer
            HIPTRY(h, hipGetLastError());
            HIPTRY(h, hipStreamSynchronize(s));
        }
        cur.release(t->mem);
        return 0;
    }
    // everything that can be refused, on the host, before anything changes
    if (!sources)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    if (count > CWF_EXPLICIT_MAX_SOURCES)
        return set_error(h, CWF_ERR_SIZE, "too many load sources",
                         "count=" + std::to_string(count) + "\nmax=" + std::to_string(CWF_EXPLICIT_MAX_SOURCES));
    if (t->lbase)
        return set_error(h, CWF_ERR_UNSUPPORTED, "load sources and a load pattern exclude each other");
    const uint64_t N = h->ds.N;
    const uint32_t kNone = 0xFFFFFFFFu;
    std::vector<uint32_t> slot(std::max<uint64_t>(N, 4), kNone);  // caller's node -> its index among the loaded nodes
    std::vector<uint32_t> seen(std::max<uint64_t>(N, 4), kNone);  // caller's node -> the last source that listed it
    uint64_t entries = 0, points = 0, nodes = 0;
    for (uint32_t q = 0; q < count; ++q)
    {
        const cwf_explicit_source_desc &d = sources[q];
        const std::string sq = "source=" + std::to_string(q);
        if (d.curve_points < 1 || d.curve_points > CWF_EXPLICIT_MAX_CURVE_POINTS)
            return set_error(h, CWF_ERR_SIZE, "load source curve must have 1 to 4096 points",
                             sq + "\ncount=" + std::to_string(d.curve_points));
        if (!d.entry_count)
            return set_error(h, CWF_ERR_ARGUMENT, "load source has no entries", sq);
        if (!d.times || !d.values || !d.node_ids || !d.amplitude || !d.delay)
            return set_error(h, CWF_ERR_ARGUMENT, "null pointer", sq);
        for (uint64_t i = 0; i < d.curve_points; ++i)
        {
            if (!std::isfinite(d.times[i]) || !std::isfinite(d.values[i]))
                return set_error(h, CWF_ERR_ARGUMENT, "load source curve is not finite",
                                 sq + "\nindex=" + std::to_string(i));
            if (i && !(d.times[i] >= d.times[i - 1]))
                return set_error(h, CWF_ERR_ARGUMENT, "load source curve times must ascend",
                                 sq + "\nindex=" + std::to_string(i));
        }
        for (uint64_t i = 0; i < d.entry_count; ++i)
        {
            const uint32_t node = d.node_ids[i];
            const std::string at = sq + "\nindex=" + std::to_string(i);
            if (node >= N)
                return set_error(h, CWF_ERR_ARGUMENT, "load source node out of range",
                                 at + "\nnode=" + std::to_string(node));
            if (seen[node] == q)
                return set_error(h, CWF_ERR_ARGUMENT, "load source node listed twice",
                                 at + "\nnode=" + std::to_string(node));
            seen[node] = q;
            if (!std::isfinite(d.delay[i]) || !std::isfinite(d.amplitude[3 * i]) ||
                !std::isfinite(d.amplitude[3 * i + 1]) || !std::isfinite(d.amplitude[3 * i + 2]))
                return set_error(h, CWF_ERR_ARGUMENT, "load source entry is not finite", at);
            if (slot[node] == kNone)
                slot[node] = (uint32_t)nodes++;
        }
        entries += d.entry_count;
        points += d.curve_points;
    }
    // the loaded nodes in the internal order: their indices move as a one-word node vector (bit copies), as
    // set_dashpots moves its slots, and come back as a list
    DevicePtr<uint32_t> order;
    if (order.alloc(slot.size()) != hipSuccess)
        return set_error(h, CWF_ERR_ALLOC, t->alloc_error);
    std::vector<uint32_t> back(slot.size());
    if (int st = vec_in(h, reinterpret_cast<const float *>(slot.data()), reinterpret_cast<float *>(order.get()),
                        CWF_PTR_HOST, 1))
        return st;
    HIPTRY(h, hipMemcpyAsync(back.data(), order.get(), N * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPTRY(h, hipStreamSynchronize(s));
    std::vector<uint32_t> rank(nodes), node(nodes);  // caller-side index -> l; l -> internal node
    uint32_t L = 0;
    for (uint64_t n = 0; n < N; ++n)
        if (back[n] != kNone)
        {
            rank[back[n]] = L;
            node[L++] = (uint32_t)n;
        }
    if (L != nodes)
        return set_error(h, CWF_ERR_INDEX, "load source nodes were lost in the node order");
    // the CSR: counts, offsets, then the entries source by source, so that a node's entries ascend in source index
    std::vector<uint32_t> off(nodes + 1, 0), dir(2 * entries);
    std::vector<double> rec(4 * entries), tab(2 * points);
    for (uint32_t q = 0; q < count; ++q)
        for (uint64_t i = 0; i < sources[q].entry_count; ++i)
            ++off[rank[slot[sources[q].node_ids[i]]] + 1];
    for (uint64_t l = 0; l < nodes; ++l)
        off[l + 1] += off[l];
    std::vector<uint32_t> fill(off.begin(), off.end() - 1);
    uint64_t at = 0;
    for (uint32_t q = 0; q < count; ++q)
    {
        const cwf_explicit_source_desc &d = sources[q];
        std::copy(d.times, d.times + d.curve_points, tab.begin() + at);
        std::copy(d.values, d.values + d.curve_points, tab.begin() + at + d.curve_points);
        for (uint64_t i = 0; i < d.entry_count; ++i)
        {
            const uint32_t e = fill[rank[slot[d.node_ids[i]]]]++;
            rec[4ull * e] = d.amplitude[3 * i];
            rec[4ull * e + 1] = d.amplitude[3 * i + 1];
            rec[4ull * e + 2] = d.amplitude[3 * i + 2];
            rec[4ull * e + 3] = d.delay[i];
            dir[2ull * e] = (uint32_t)at;
            dir[2ull * e + 1] = (uint32_t)d.curve_points;
        }
        at += 2 * d.curve_points;
    }
    // the new set's buffers; the stepper's once everything went well
    cwf_hip_explicit::Sources m;
    uint32_t *dnode = nullptr, *doff = nullptr, *ddir = nullptr;
    double *drec = nullptr, *dtab = nullptr;
    float *dfext = nullptr;
    int st = t->alloc(&dnode, node.size());
    st = st ? st : t->alloc(&doff, off.size());
    st = st ? st : t->alloc(&drec, rec.size());
    st = st ? st : t->alloc(&ddir, dir.size());
    st = st ? st : t->alloc(&dtab, tab.size());
    st = st ? st : t->alloc(&dfext, 3 * (size_t)nodes);
    m.dev = ExplicitSources{(uint32_t)nodes, dnode, doff, drec, ddir, dtab, dfext};
    hipError_t e = hipSuccess;
    const auto up = [&](void *dst, const void *from, size_t bytes) {
        if (!st && e == hipSuccess)
            e = hipMemcpyAsync(dst, from, bytes, hipMemcpyHostToDevice, s);
    };
    up(dnode, node.data(), node.size() * sizeof(uint32_t));
    up(doff, off.data(), off.size() * sizeof(uint32_t));
    up(drec, rec.data(), rec.size() * sizeof(double));
    up(ddir, dir.data(), dir.size() * sizeof(uint32_t));
    up(dtab, tab.data(), tab.size() * sizeof(double));
    if (!st && e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (st || e != hipSuccess)
    {
        (void)hipStreamSynchronize(s);
        m.release(t->mem);
        return st ? st : hip_fail(h, e, "explicit set_sources");
    }
    // the force buffer holds f_n at the previous set's nodes: their f_ext goes back before the new set's is taken out
    if (cur.dev.loaded)
        explicit_sources_fext(cur.dev, t->f, false, s);
    explicit_sources_fext(m.dev, t->f, true, s);
    e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (e != hipSuccess)
    {
        m.release(t->mem);
        return hip_fail(h, e, "explicit set_sources");
    }
    m.entries = entries;
    m.points = points;
    m.bytes = (node.size() + off.size() + dir.size()) * sizeof(uint32_t) + (rec.size() + tab.size()) * sizeof(double) +
              3 * nodes * sizeof(float);
    m.given.resize(count);
    for (uint32_t q = 0; q < count; ++q)
    {
        const cwf_explicit_source_desc &d = sources[q];
        auto &g = m.given[q];
        g.times.assign(d.times, d.times + d.curve_points);
        g.values.assign(d.values, d.values + d.curve_points);
        g.ids.assign(d.node_ids, d.node_ids + d.entry_count);
        g.amplitude.assign(d.amplitude, d.amplitude + 3 * d.entry_count);
        g.delay.assign(d.delay, d.delay + d.entry_count);
    }
    cur.release(t->mem);
    cur = std::move(m);
    return 0;
}

int cwf_hip_explicit_get_sources(cwf_hip_explicit *t, uint32_t *count, cwf_explicit_source_desc *sources)
{
    if (!t || !count)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    *count = (uint32_t)t->src.given.size();
    for (size_t q = 0; sources && q < t->src.given.size(); ++q)
    {
        const auto &g = t->src.given[q];
        sources[q] = cwf_explicit_source_desc{g.times.size(), g.times.data(), g.values.data(), g.ids.size(),
                                              g.ids.data(), g.amplitude.data(), g.delay.data()};
    }
    return 0;
}

int cwf_hip_explicit_source_info(cwf_hip_explicit *t, cwf_explicit_source_info *info)
{
    if (!t || !info)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    cwf_explicit_source_info I{};
    I.source_count = (uint32_t)t->src.given.size();
    I.entry_count = t->src.entries;
    I.loaded_nodes = t->src.dev.loaded;
    I.curve_points = t->src.points;
    I.device_bytes = t->src.bytes;
    *info = I;
    return 0;
}

int cwf_hip_explicit_set_monitors(cwf_hip_explicit *t, const cwf_explicit_monitor_desc *desc)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    hipStream_t s = h->stream;
    const cwf_explicit_monitor_desc none{};
    const cwf_explicit_monitor_desc &d = desc ? *desc : none;
    const uint64_t N = h->ds.N;
    // everything that can be refused, on the host, before anything changes
    if (d.receiver_count && !d.receiver_nodes)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    if (d.receiver_count && d.receiver_every < 1)
        return set_error(h, CWF_ERR_ARGUMENT, "receiver_every must be at least 1");
    if ((d.receiver_count && !d.receiver_capacity) || (d.energy_every && !d.energy_capacity))
        return set_error(h, CWF_ERR_ARGUMENT, "monitor capacity must not be zero",
                         "receiver_capacity=" + std::to_string(d.receiver_capacity) +
                             "\nenergy_capacity=" + std::to_string(d.energy_capacity));
    if (d.energy_every && t->beta != 0.0)
        return set_error(h, CWF_ERR_UNSUPPORTED, "the energy ledger needs rayleigh_beta == 0",
                         "rayleigh_beta=" + num(t->beta));
    if (d.energy_every && t->pl.dev.slots)
        return set_error(h, CWF_ERR_UNSUPPORTED, "the energy ledger and plasticity exclude each other",
                         "plastic_elements=" + std::to_string(t->pl.dev.slots));
    const uint32_t kNone = 0xFFFFFFFFu;
    std::vector<uint32_t> slot(d.receiver_count ? std::max<uint64_t>(N, 4) : 0, kNone);
    for (uint64_t i = 0; i < d.receiver_count; ++i)
    {
        const uint32_t node = d.receiver_nodes[i];
        if (node >= N)
            return set_error(h, CWF_ERR_ARGUMENT, "receiver node out of range",
                             "index=" + std::to_string(i) + "\nnode=" + std::to_string(node));
        if (slot[node] != kNone)
            return set_error(h, CWF_ERR_ARGUMENT, "receiver node listed twice",
                             "index=" + std::to_string(i) + "\nnode=" + std::to_string(node));
        slot[node] = (uint32_t)i;
    }
    const uint64_t kMaxBytes = 1ull << 44;  // no device holds more: a product past it is an allocation failure
    if (d.receiver_count && d.receiver_capacity > kMaxBytes / (12 * d.receiver_count))
        return set_error(h, CWF_ERR_ALLOC, t->alloc_error);
    if (d.energy_every && d.energy_capacity > kMaxBytes / 32)
        return set_error(h, CWF_ERR_ALLOC, t->alloc_error);
    HIPTRY(h, hipStreamSynchronize(s));
    // the new set's buffers; the stepper's once everything went well
    cwf_hip_explicit::Monitors m;
    double *newC = nullptr;
    DevicePtr<uint32_t> order;  // the receivers' slots in the internal node order
    const uint32_t blocks = explicit_update_blocks((uint32_t)N);
    int st = 0;
    hipError_t e = hipSuccess;
    if (d.receiver_count)
    {
        m.rcount = d.receiver_count;
        m.revery = d.receiver_every;
        m.rcap = d.receiver_capacity;
        const size_t cells = (size_t)(3 * m.rcount * m.rcap);
        st = st ? st : t->alloc(&m.rnode, m.rcount);
        st = st ? st : t->alloc(&m.ru, cells);
        st = st ? st : t->alloc(&m.rv, cells);
        if (!st && order.alloc(slot.size()) != hipSuccess)
            st = set_error(h, CWF_ERR_ALLOC, t->alloc_error);
    }
    if (d.peaks)
    {
        m.peak_stride = std::max<uint64_t>(N, 4);
        st = st ? st : t->alloc(&m.peak, 3 * m.peak_stride);
    }
    if (d.energy_every)
    {
        m.eevery = d.energy_every;
        m.ecap = d.energy_capacity;
        st = st ? st : t->alloc(&m.ecum, 2 * (size_t)blocks);
        st = st ? st : t->alloc(&m.ecur, 2 * (size_t)blocks);
        st = st ? st : t->alloc(&m.erows, 4 * (size_t)m.ecap);
        if (!st && !t->dash_ids.empty())
            st = t->alloc(&newC, t->dash_C.size());
    }
    std::vector<uint32_t> rnode(m.rcount);
    if (!st && m.rcount)
    {
        // the receivers' nodes in the internal order: the slots move as a one-word node vector (bit copies), as
        // set_dashpots moves its own, and come back as a list
        std::vector<uint32_t> back(slot.size());
        st = vec_in(h, reinterpret_cast<const float *>(slot.data()), reinterpret_cast<float *>(order.get()),
                    CWF_PTR_HOST, 1);
        if (!st)
            e = hipMemcpyAsync(back.data(), order.get(), N * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (!st && e == hipSuccess)
            e = hipStreamSynchronize(s);
        if (!st && e == hipSuccess)
        {
            for (uint64_t n = 0; n < N; ++n)
                if (back[n] != kNone)
                    rnode[back[n]] = (uint32_t)n;
            e = hipMemcpyAsync(m.rnode, rnode.data(), m.rcount * sizeof(uint32_t), hipMemcpyHostToDevice, s);
        }
    }
    if (!st && e == hipSuccess && m.peak)
        e = hipMemsetAsync(m.peak, 0, 3 * m.peak_stride * sizeof(float), s);
    if (!st && e == hipSuccess && m.ecum)
        e = hipMemsetAsync(m.ecum, 0, 2 * (size_t)blocks * sizeof(double), s);
    if (!st && e == hipSuccess && m.ecur)
        e = hipMemsetAsync(m.ecur, 0, 2 * (size_t)blocks * sizeof(double), s);
    if (!st && e == hipSuccess && newC)
        e = hipMemcpyAsync(newC, t->dash_C.data(), t->dash_C.size() * sizeof(double), hipMemcpyHostToDevice, s);
    if (!st && e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (st || e != hipSuccess)
    {
        (void)hipStreamSynchronize(s);
        m.release(t->mem);
        t->mem.free(newC);
        return st ? st : hip_fail(h, e, "explicit set_monitors");
    }
    m.rsteps.reserve((size_t)std::min<uint64_t>(m.rcap, 1u << 20));
    m.esteps.reserve((size_t)std::min<uint64_t>(m.ecap, 1u << 20));
    t->mon.release(t->mem);
    t->mem.free(t->dC);
    t->mon = std::move(m);
    t->dC = newC;
    return 0;
}

int cwf_hip_explicit_reset_monitors(cwf_hip_explicit *t)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    cwf_hip_explicit::Monitors &m = t->mon;
    const size_t blocks = explicit_update_blocks(h->ds.N);
    if (m.peak)
        HIPTRY(h, hipMemsetAsync(m.peak, 0, 3 * m.peak_stride * sizeof(float), h->stream));
    if (m.ecum)
    {
        HIPTRY(h, hipMemsetAsync(m.ecum, 0, 2 * blocks * sizeof(double), h->stream));
        HIPTRY(h, hipMemsetAsync(m.ecur, 0, 2 * blocks * sizeof(double), h->stream));
    }
    HIPTRY(h, hipStreamSynchronize(h->stream));
    m.rsteps.clear();
    m.esteps.clear();
    m.rdropped = m.edropped = 0;
    return 0;
}

int cwf_hip_explicit_monitor_info(cwf_hip_explicit *t, cwf_explicit_monitor_info *info)
{
    if (!t || !info)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    const cwf_hip_explicit::Monitors &m = t->mon;
    cwf_explicit_monitor_info I{};
    I.receiver_count = m.rcount;
    I.receiver_every = m.revery;
    I.receiver_capacity = m.rcap;
    I.receiver_samples = m.rsteps.size();
    I.receiver_dropped = m.rdropped;
    I.energy_every = m.eevery;
    I.energy_capacity = m.ecap;
    I.energy_samples = m.esteps.size();
    I.energy_dropped = m.edropped;
    I.peaks = m.peak ? 1u : 0u;
    *info = I;
    return 0;
}

namespace
{
int rows_in_range(cwf_hip_system *h, uint64_t first, uint64_t count, uint64_t held)
{
    if (first > held || count > held - first)
        return set_error(h, CWF_ERR_ARGUMENT, "monitor rows out of range",
                         "first=" + std::to_string(first) + "\ncount=" + std::to_string(count) +
                             "\nheld=" + std::to_string(held));
    return 0;
}
}  // namespace

int cwf_hip_explicit_read_receivers(cwf_hip_explicit *t, uint64_t first, uint64_t count, uint64_t *steps, float *u,
                                    float *v)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    const cwf_hip_explicit::Monitors &m = t->mon;
    if (int st = rows_in_range(h, first, count, m.rsteps.size()))
        return st;
    if (!count)
        return 0;
    if (steps)
        std::copy(m.rsteps.begin() + first, m.rsteps.begin() + first + count, steps);
    const size_t off = (size_t)(3 * m.rcount * first), len = (size_t)(3 * m.rcount * count) * sizeof(float);
    if (u)
        HIPTRY(h, hipMemcpyAsync(u, m.ru + off, len, hipMemcpyDeviceToHost, h->stream));
    if (v)
        HIPTRY(h, hipMemcpyAsync(v, m.rv + off, len, hipMemcpyDeviceToHost, h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_explicit_read_peaks(cwf_hip_explicit *t, float *peak_u, float *peak_v, float *peak_a, uint64_t n, int kind)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    const cwf_hip_explicit::Monitors &m = t->mon;
    if (!m.peak)
        return set_error(h, CWF_ERR_ARGUMENT, "no peak maps are set");
    if (n != h->ds.N)
        return set_error(h, CWF_ERR_SIZE, "peak map span size mismatch",
                         "span=" + std::to_string(n) + "\nnodes=" + std::to_string(h->ds.N));
    float *out[3] = {peak_u, peak_v, peak_a};
    for (int j = 0; j < 3; ++j)
        if (out[j])
            if (int st = vec_out(h, m.peak + j * m.peak_stride, out[j], kind, 1))
                return st;
    HIPTRY(h, hipGetLastError());
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_explicit_read_energy(cwf_hip_explicit *t, uint64_t first, uint64_t count, uint64_t *steps, double *rows)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    const cwf_hip_explicit::Monitors &m = t->mon;
    if (int st = rows_in_range(h, first, count, m.esteps.size()))
        return st;
    if (!count)
        return 0;
    if (steps)
        std::copy(m.esteps.begin() + first, m.esteps.begin() + first + count, steps);
    if (rows)
        HIPTRY(h, hipMemcpyAsync(rows, m.erows + 4 * first, 4 * count * sizeof(double), hipMemcpyDeviceToHost,
                                 h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

namespace
{
const uint32_t kBitsPlusInf = 0x7F800000u, kBitsMinusInf = 0xFF800000u;

// the maps at their start values: von Mises and shear strain +0.0, the stress minima +inf, the maxima -inf
hipError_t start_envelopes(const cwf_hip_explicit::ElementMonitors &m, hipStream_t s)
{
    hipError_t e = hipSuccess;
    if (m.vm)
        e = hipMemsetAsync(m.vm, 0, m.stride * sizeof(float), s);
    if (e == hipSuccess && m.shear)
        e = hipMemsetAsync(m.shear, 0, m.stride * sizeof(float), s);
    if (e == hipSuccess && m.range)
        e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m.range), (int)kBitsPlusInf, 6 * m.stride, s);
    if (e == hipSuccess && m.range)
        e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m.range + 6 * m.stride), (int)kBitsMinusInf,
                              6 * m.stride, s);
    return e;
}
}  // namespace

}  // extern "C"

// what cwf_hip_explicit_set_element_monitors refuses of a desc, on the host alone: 0, or the code with *msg and *ctx
int cwf::element_monitor_refusal(const cwf_explicit_element_monitor_desc &d, uint64_t E, std::string *msg,
                                 std::string *ctx)
{
    const auto no = [&](const char *m, std::string c = std::string()) {
        *msg = m;
        *ctx = std::move(c);
        return (int)CWF_ERR_ARGUMENT;
    };
    if (d.gauge_count && !d.gauge_elements)
        return no("null pointer");
    if (d.gauge_count && d.gauge_every < 1)
        return no("gauge_every must be at least 1");
    if (d.gauge_count && !d.gauge_capacity)
        return no("monitor capacity must not be zero", "gauge_capacity=" + std::to_string(d.gauge_capacity));
    const uint32_t known = CWF_ENVELOPE_VON_MISES | CWF_ENVELOPE_SHEAR_STRAIN | CWF_ENVELOPE_STRESS_RANGE;
    if (d.envelope_maps & ~known)
        return no("unknown envelope map", "maps=" + std::to_string(d.envelope_maps));
    if (d.envelope_maps && !d.envelope_every)
        return no("envelope_maps without envelope_every", "maps=" + std::to_string(d.envelope_maps));
    if (d.envelope_every && !d.envelope_maps)
        return no("envelope_every without envelope_maps", "envelope_every=" + std::to_string(d.envelope_every));
    std::vector<bool> seen(d.gauge_count ? E : 0, false);
    for (uint64_t i = 0; i < d.gauge_count; ++i)
    {
        const uint32_t e = d.gauge_elements[i];
        if (e >= E)
            return no("gauge element out of range", "index=" + std::to_string(i) + "\nelement=" + std::to_string(e));
        if (seen[e])
            return no("gauge element listed twice", "index=" + std::to_string(i) + "\nelement=" + std::to_string(e));
        seen[e] = true;
    }
    return 0;
}

extern "C" {

int cwf_hip_explicit_set_element_monitors(cwf_hip_explicit *t, const cwf_explicit_element_monitor_desc *desc)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    hipStream_t s = h->stream;
    const cwf_explicit_element_monitor_desc none{};
    const cwf_explicit_element_monitor_desc &d = desc ? *desc : none;
    const uint64_t E = h->ds.E;
    // everything that can be refused, on the host, before anything changes
    std::string msg, ctx;
    if (int code = element_monitor_refusal(d, E, &msg, &ctx))
        return set_error(h, code, msg, ctx);
    const uint64_t kMaxBytes = 1ull << 44;  // no device holds more: a product past it is an allocation failure
    if (d.gauge_count && d.gauge_capacity > kMaxBytes / (52 * d.gauge_count))
        return set_error(h, CWF_ERR_ALLOC, t->alloc_error);
    HIPTRY(h, hipStreamSynchronize(s));
    // the new set's buffers; the stepper's once everything went well
    cwf_hip_explicit::ElementMonitors m;
    int st = 0;
    if (d.gauge_count)
    {
        m.gcount = d.gauge_count;
        m.gevery = d.gauge_every;
        m.gcap = d.gauge_capacity;
        st = st ? st : t->alloc(&m.gelem, m.gcount);
        st = st ? st : t->alloc(&m.grows, (size_t)(13 * m.gcount * m.gcap));
    }
    if (d.envelope_every)
    {
        m.eevery = d.envelope_every;
        m.maps = d.envelope_maps;
        m.stride = std::max<uint64_t>(E, 4);
        if (m.maps & CWF_ENVELOPE_VON_MISES)
            st = st ? st : t->alloc(&m.vm, m.stride);
        if (m.maps & CWF_ENVELOPE_SHEAR_STRAIN)
            st = st ? st : t->alloc(&m.shear, m.stride);
        if (m.maps & CWF_ENVELOPE_STRESS_RANGE)
            st = st ? st : t->alloc(&m.range, 12 * m.stride);
    }
    hipError_t e = hipSuccess;
    if (!st && m.gcount)  // elements keep the caller's numbering on the device: the ids go up as given
        e = hipMemcpyAsync(m.gelem, d.gauge_elements, m.gcount * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (!st && e == hipSuccess)
        e = start_envelopes(m, s);
    if (!st && e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (st || e != hipSuccess)
    {
        (void)hipStreamSynchronize(s);
        m.release(t->mem);
        return st ? st : hip_fail(h, e, "explicit set_element_monitors");
    }
    m.gsteps.reserve((size_t)std::min<uint64_t>(m.gcap, 1u << 20));
    t->emon.release(t->mem);
    t->emon = std::move(m);
    return 0;
}

int cwf_hip_explicit_reset_element_monitors(cwf_hip_explicit *t)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    cwf_hip_explicit::ElementMonitors &m = t->emon;
    HIPTRY(h, start_envelopes(m, h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    m.gsteps.clear();
    m.gdropped = m.esamples = 0;
    return 0;
}

int cwf_hip_explicit_element_monitor_info(cwf_hip_explicit *t, cwf_explicit_element_monitor_info *info)
{
    if (!t || !info)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    const cwf_hip_explicit::ElementMonitors &m = t->emon;
    cwf_explicit_element_monitor_info I{};
    I.gauge_count = m.gcount;
    I.gauge_every = m.gevery;
    I.gauge_capacity = m.gcap;
    I.gauge_samples = m.gsteps.size();
    I.gauge_dropped = m.gdropped;
    I.envelope_every = m.eevery;
    I.envelope_samples = m.esamples;
    I.envelope_maps = m.maps;
    *info = I;
    return 0;
}

int cwf_hip_explicit_read_gauges(cwf_hip_explicit *t, uint64_t first, uint64_t count, uint64_t *steps, float *rows)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    const cwf_hip_explicit::ElementMonitors &m = t->emon;
    if (int st = rows_in_range(h, first, count, m.gsteps.size()))
        return st;
    if (!count)
        return 0;
    if (steps)
        std::copy(m.gsteps.begin() + first, m.gsteps.begin() + first + count, steps);
    if (rows)
        HIPTRY(h, hipMemcpyAsync(rows, m.grows + 13 * m.gcount * first, (size_t)(13 * m.gcount * count) * sizeof(float),
                                 hipMemcpyDeviceToHost, h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_explicit_read_envelopes(cwf_hip_explicit *t, float *von_mises, float *shear_strain, float *stress_min,
                                    float *stress_max, uint64_t n, int kind)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    const cwf_hip_explicit::ElementMonitors &m = t->emon;
    if ((von_mises && !m.vm) || (shear_strain && !m.shear) || ((stress_min || stress_max) && !m.range))
        return set_error(h, CWF_ERR_ARGUMENT, "envelope map is not set", "maps=" + std::to_string(m.maps));
    const uint64_t E = h->ds.E;
    if (n != E)
        return set_error(h, CWF_ERR_SIZE, "envelope map span size mismatch",
                         "span=" + std::to_string(n) + "\nelements=" + std::to_string(E));
    hipStream_t s = h->stream;
    const hipMemcpyKind back = kind == CWF_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (von_mises)
        HIPTRY(h, hipMemcpyAsync(von_mises, m.vm, E * sizeof(float), back, s));
    if (shear_strain)
        HIPTRY(h, hipMemcpyAsync(shear_strain, m.shear, E * sizeof(float), back, s));
    // the stress range: plane c of the device layout is column c of the caller's [E][6]
    float *const out[2] = {stress_min, stress_max};
    std::vector<float> plane;
    for (int q = 0; q < 2; ++q)
    {
        if (!out[q])
            continue;
        const float *src = m.range + 6 * q * m.stride;
        if (kind == CWF_PTR_DEVICE)
        {
            for (int c = 0; c < 6; ++c)
                HIPTRY(h, hipMemcpy2DAsync(out[q] + c, 6 * sizeof(float), src + c * m.stride, sizeof(float),
                                           sizeof(float), E, hipMemcpyDeviceToDevice, s));
            continue;
        }
        plane.resize(6 * m.stride);
        HIPTRY(h, hipMemcpyAsync(plane.data(), src, plane.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPTRY(h, hipStreamSynchronize(s));
        for (uint64_t e = 0; e < E; ++e)
            for (int c = 0; c < 6; ++c)
                out[q][6 * e + c] = plane[c * m.stride + e];
    }
    HIPTRY(h, hipStreamSynchronize(s));
    return 0;
}

int cwf_explicit_j2_update(const double D[36], double yield, double hardening, double volume, const double strain[6],
                           double state[8], double sigma_p[6])
{
    if (!D || !strain || !state || !sigma_p)
        return 0;
    return j2_update(D, yield, hardening, volume, strain, state, state[6], state[7], sigma_p) ? 1 : 0;
}

int cwf_hip_explicit_set_plasticity(cwf_hip_explicit *t, const cwf_explicit_plasticity_desc *desc)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    hipStream_t s = h->stream;
    if (!desc)
    {
        HIPTRY(h, hipStreamSynchronize(s));
        t->pl.release(t->mem);
        return 0;
    }
    // everything that can be refused, on the host, before anything changes
    const DevSys &ds = h->ds;
    const uint64_t N = ds.N, E = ds.E, M = ds.M;
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
    bool any = false;
    for (uint64_t m = 0; m < M; ++m)
    {
        const double sy = desc->yield_stress[m], H = desc->hardening[m];
        if (!(sy >= 0.0) || !(H >= 0.0))
            return set_error(h, CWF_ERR_ARGUMENT, "yield stress and hardening must be non-negative",
                             "material=" + std::to_string(m) + "\nyield_stress=" + num(sy) + "\nhardening=" + num(H));
        plastic[m] = sy > 0.0 && std::isfinite(sy);
        any = any || plastic[m];
        yh[2 * m] = sy;
        yh[2 * m + 1] = H;
    }
    if (t->mon.ecum)
        return set_error(h, CWF_ERR_UNSUPPORTED, "the energy ledger and plasticity exclude each other",
                         "energy_every=" + std::to_string(t->mon.eevery));
    HIPTRY(h, hipStreamSynchronize(s));
    std::vector<double> D(36 * M);
    HIPTRY(h, hipMemcpy(D.data(), ds.dmat, D.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (uint64_t m = 0; m < M; ++m)
        if (plastic[m] && !iso_pattern(D.data() + 36 * m))
            return set_error(h, CWF_ERR_UNSUPPORTED, "a plastic material needs an isotropic stiffness",
                             "material=" + std::to_string(m));
    if (!any)  // every material elastic: nothing to run
    {
        t->pl.release(t->mem);
        return 0;
    }
    // the slots (plastic elements, ascending) and the affected nodes' compact CSR, from the handle's own arrays: the
    // node -> incidence CSR is in the handle's node order and ascends in element per node
    std::vector<uint32_t> mat(E), off(N + 1), inc(4 * E);
    HIPTRY(h, hipMemcpy(mat.data(), ds.mat, E * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPTRY(h, hipMemcpy(off.data(), ds.off, (N + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPTRY(h, hipMemcpy(inc.data(), ds.inc, 4 * E * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const uint32_t kNone = 0xFFFFFFFFu;
    std::vector<uint32_t> slot_of(E, kNone), elem;
    for (uint64_t e = 0; e < E; ++e)
        if (mat[e] < M && plastic[mat[e]])
        {
            slot_of[e] = (uint32_t)elem.size();
            elem.push_back((uint32_t)e);
        }
    if (elem.empty())
    {
        t->pl.release(t->mem);
        return 0;
    }
    // node-major corner forces: position q of the array is the q-th plastic incidence in node order, so a node's run
    // ascends in element; cpos tells each slot where its four corners go
    std::vector<uint32_t> anode, aoff(1, 0), cpos(4 * elem.size(), 0);
    uint32_t run = 0;
    for (uint64_t n = 0; n < N; ++n)
    {
        for (uint32_t j = off[n]; j < off[n + 1]; ++j)
        {
            const uint32_t e = inc[j] >> 2;
            if (e < E && slot_of[e] != kNone)
                cpos[4ull * slot_of[e] + (inc[j] & 3u)] = run++;
        }
        if (run != aoff.back())
        {
            anode.push_back((uint32_t)n);
            aoff.push_back(run);
        }
    }
    if (run != cpos.size())  // every corner of every plastic element is some node's incidence, once
        return set_error(h, CWF_ERR_INDEX, "plastic incidences do not cover the elements' corners",
                         "incidences=" + std::to_string(run) + "\ncorners=" + std::to_string(cpos.size()));
    // the new set's buffers; the stepper's once everything went well
    const size_t slots = elem.size(), plen = std::max<size_t>(3 * N, 4);
    cwf_hip_explicit::Plasticity m;
    uint32_t *delem = nullptr, *danode = nullptr, *daoff = nullptr, *dcpos = nullptr;
    double *dyh = nullptr, *dstate = nullptr;
    float *dcorner = nullptr, *dp = nullptr;
    int st = t->alloc(&delem, slots);
    st = st ? st : t->alloc(&dyh, yh.size());
    st = st ? st : t->alloc(&dstate, 8 * slots);
    st = st ? st : t->alloc(&dcorner, 12 * slots);
    st = st ? st : t->alloc(&danode, anode.size());
    st = st ? st : t->alloc(&daoff, aoff.size());
    st = st ? st : t->alloc(&dcpos, cpos.size());
    st = st ? st : t->alloc(&dp, plen);
    m.dev = ExplicitPlasticity{(uint32_t)slots, (uint32_t)anode.size(), delem, dyh, dstate, dcorner, danode, daoff,
                               dcpos, dp};
    hipError_t e = hipSuccess;
    const auto up = [&](void *dst, const void *from, size_t bytes) {
        if (!st && e == hipSuccess)
            e = hipMemcpyAsync(dst, from, bytes, hipMemcpyHostToDevice, s);
    };
    const auto zero = [&](void *dst, size_t bytes) {
        if (!st && e == hipSuccess)
            e = hipMemsetAsync(dst, 0, bytes, s);
    };
    up(delem, elem.data(), slots * sizeof(uint32_t));
    up(dyh, yh.data(), yh.size() * sizeof(double));
    up(danode, anode.data(), anode.size() * sizeof(uint32_t));
    up(daoff, aoff.data(), aoff.size() * sizeof(uint32_t));
    up(dcpos, cpos.data(), cpos.size() * sizeof(uint32_t));
    zero(dstate, 8 * slots * sizeof(double));
    zero(dcorner, 12 * slots * sizeof(float));
    zero(dp, plen * sizeof(float));
    if (!st && e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (st || e != hipSuccess)
    {
        (void)hipStreamSynchronize(s);
        m.release(t->mem);
        return st ? st : hip_fail(h, e, "explicit set_plasticity");
    }
    m.bytes = (slots + anode.size() + aoff.size() + cpos.size()) * sizeof(uint32_t) +
              (yh.size() + 8 * slots) * sizeof(double) + (12 * slots + plen) * sizeof(float);
    m.elem = std::move(elem);
    t->pl.release(t->mem);
    t->pl = std::move(m);
    return 0;
}

int cwf_hip_explicit_reset_plasticity(cwf_hip_explicit *t)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
    const ExplicitPlasticity &p = t->pl.dev;
    if (!p.slots)
        return 0;
    HIPTRY(h, hipMemsetAsync(p.state, 0, 8ull * p.slots * sizeof(double), h->stream));
    HIPTRY(h, hipMemsetAsync(p.corner, 0, 12ull * p.slots * sizeof(float), h->stream));
    HIPTRY(h, hipMemsetAsync(p.p, 0, std::max<size_t>(3ull * h->ds.N, 4) * sizeof(float), h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

namespace
{
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
}  // namespace

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
    for (size_t q = 0; q < t->pl.dev.slots; ++q)
        I.yielded_elements += state[8 * q + 6] > 0.0 ? 1 : 0;
    I.bytes = t->pl.bytes;
    *info = I;
    return 0;
}

int cwf_hip_explicit_read_plasticity(cwf_hip_explicit *t, double *ep, double *abar, double *wp, uint64_t n)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_hip_system *h = t->sys;
    if (int st = check_ready(h))
        return st;
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

int cwf_hip_explicit_time(const cwf_hip_explicit *t, double *current_time, double *time_step)
{
    if (!t)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    return transient_time((double)t->steps * t->dt, t->dt, current_time, time_step);
}

}  // extern "C"
