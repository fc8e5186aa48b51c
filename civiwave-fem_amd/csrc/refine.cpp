// refine.cpp -- the refined static solve (include/cwf_hip.h): classical iterative refinement around the handle's own
// PCG. x and b live in fp64 in the handle's internal node order; each outer iteration forms the true residual
// r = b - K_eff x with the fp64 kernels of refine.hip, scales it by a power of two into b's binade (the PCG's guards
// are absolute), solves K_eff d = f32(2^e r) with run_pcg in whatever schedule the handle takes, and adds 2^(-e) d.
#include <cmath>
#include <cstring>

#include "abi_internal.hpp"
#include "refine.hpp"

namespace cwf
{
namespace
{

// fp64 x, b, r, the previous iterate, the node shares and the norm's chunk partials followed by its two results:
// allocated at the first refined call, kept in `owned` (freed with the handle, counted by cwf_hip_system_memory)
int refine_workspace(cwf_hip_system *h)
{
    if (h->rf_part)
        return 0;
    const size_t D = h->ds.D;
    for (double **p : {&h->rf_x, &h->rf_b, &h->rf_r, &h->rf_xp})
        if (int st = dalloc(h, p, D))
            return st;
    if (int st = dalloc(h, &h->rf_share, (size_t)h->ds.N))
        return st;
    return dalloc(h, &h->rf_part, (size_t)refine_norm_chunks(h->ds.N) + 2);
}

double *norm_out(cwf_hip_system *h) { return h->rf_part + refine_norm_chunks(h->ds.N); }

// caller-order fp64 node vector (host or device) -> dst in internal order. The permutation moves a node's three
// doubles as six 4-B payloads (the copy kernel does no arithmetic); stage: D doubles of device scratch
int vec_in64(cwf_hip_system *h, const double *src, double *dst, int kind, double *stage)
{
    const size_t bytes = (size_t)h->ds.D * sizeof(double);
    const hipMemcpyKind in = kind == CWF_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!h->perm)
    {
        HIPTRY(h, hipMemcpyAsync(dst, src, bytes, in, h->stream));
        return 0;
    }
    if (kind != CWF_PTR_DEVICE)
    {
        HIPTRY(h, hipMemcpyAsync(stage, src, bytes, in, h->stream));
        src = stage;
    }
    perm_gather(h->perm, reinterpret_cast<const float *>(src), reinterpret_cast<float *>(dst), h->ds.N, 6, h->stream);
    HIPTRY(h, hipGetLastError());
    return 0;
}

int vec_out64(cwf_hip_system *h, const double *src, double *dst, int kind, double *stage)
{
    const size_t bytes = (size_t)h->ds.D * sizeof(double);
    const hipMemcpyKind out = kind == CWF_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (h->perm)
    {
        perm_scatter(h->perm, reinterpret_cast<const float *>(src), reinterpret_cast<float *>(stage), h->ds.N, 6,
                     h->stream);
        HIPTRY(h, hipGetLastError());
        src = stage;
    }
    HIPTRY(h, hipMemcpyAsync(dst, src, bytes, out, h->stream));
    return 0;
}

int read_norm(cwf_hip_system *h, double *norm)
{
    HIPTRY(h, hipGetLastError());
    HIPTRY(h, hipMemcpyAsync(norm, norm_out(h) + 1, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

// the refusals the two entry points share, then the workspace and the PARITY node tiles (built once per handle)
int refine_ready(cwf_hip_system *h, uint64_t n, const char *what)
{
    if (n != h->ds.D)
        return set_error(h, CWF_ERR_SIZE, "rhs span size mismatch",
                         "rhs=" + std::to_string(n) + "\ndofs=" + std::to_string(h->ds.D));
    if (h->sharded())
        return set_error(h, CWF_ERR_UNSUPPORTED, std::string(what) + " of a sharded handle is not supported",
                         "ranks=" + std::to_string(h->nranks));
    if (h->ds.hex)
        return set_error(h, CWF_ERR_UNSUPPORTED, std::string(what) + " of a hex8 handle is not supported",
                         "there is no fp64 hex8 operator on the device");
    if (!h->ds.E)
        return set_error(h, CWF_ERR_UNSUPPORTED, std::string(what) + " needs elements", "elements=0");
    if (int st = refine_workspace(h))
        return st;
    return parity_force_buffer(h);
}

struct RefinePlan
{
    uint32_t max_outer;
    double tol, ratio;
    bool warm;
    cwf_pcg_settings inner;
};

int refine_iterate(cwf_hip_system *h, const RefinePlan &rp, const double *rhs, double *x_inout, int kind,
                   cwf_refine_telemetry *tel)
{
    const DevSys &s = h->ds;
    hipStream_t st = h->stream;
    Stopwatch sw;
    if (!sw.make())
        return set_error(h, CWF_ERR_HIP, "hipEventCreate failed");
    double *x = h->rf_x, *b = h->rf_b, *r = h->rf_r, *xp = h->rf_xp;
    if (int e = vec_in64(h, rhs, b, kind, r))
        return e;
    double bnorm = 0.0;
    sw.start(st);
    refine_rhs_norm(s, b, h->rf_share, h->rf_part, norm_out(h), st);
    sw.stop(st, &tel->residual_ms);
    if (int e = read_norm(h, &bnorm))
        return e;
    tel->rhs_norm = bnorm;
    const bool warm = rp.warm && bnorm > 0.0;  // |b| = 0: x is the prescribed values
    if (warm)
        if (int e = vec_in64(h, x_inout, x, kind, r))
            return e;
    refine_start(s, x, b, warm, st);
    HIPTRY(h, hipGetLastError());

    const double *result = x;
    double prev = 0.0, norm = 0.0;
    int status = 0;
    uint32_t k = 0;
    for (;;)
    {
        sw.start(st);
        refine_residual(s, x, b, r, h->rf_share, h->rf_part, norm_out(h), st);
        sw.stop(st, &tel->residual_ms);
        if (int e = read_norm(h, &norm))
            return e;
        tel->history[k] = norm;
        tel->residual_norm = norm;
        if (norm <= rp.tol * bnorm)
        {
            tel->converged = 1;
            break;
        }
        if (k > 0 && norm > rp.ratio * prev)
        {
            tel->stagnated = 1;
            if (!(norm < prev))  // the correction did not help: the iterate before it is the best one
            {
                result = xp;
                tel->residual_norm = prev;
            }
            break;
        }
        if (k == rp.max_outer)
            break;
        const int e2 = cwf_refine_scale_exponent(norm, bnorm);
        sw.start(st);
        refine_scale(s, r, e2, h->rhs, st);
        sw.stop(st, &tel->residual_ms);
        HIPTRY(h, hipGetLastError());
        cwf_pcg_telemetry pt{};
        sw.start(st);
        status = run_pcg(h, h->rhs, rp.inner, &pt);
        sw.stop(st, &tel->solve_ms);
        tel->inner_iterations += pt.iterations;
        if (status)
        {
            // a breakdown (or a device error) of the inner solve is the call's status; x stays the iterate before it
            const std::string msg = h->err, ctx = h->ctx;
            set_error(h, status, msg, "outer=" + std::to_string(k) + (ctx.empty() ? "" : "\n" + ctx));
            break;
        }
        // an inner solve that stopped at max_iterations still returned a correction; the stagnation rule judges it
        HIPTRY(h, hipMemcpyAsync(xp, x, (size_t)s.D * sizeof(double), hipMemcpyDeviceToDevice, st));
        sw.start(st);
        refine_update(s, x, h->x, e2, st);
        sw.stop(st, &tel->residual_ms);
        HIPTRY(h, hipGetLastError());
        prev = norm;
        ++k;
    }
    tel->outer_iterations = k;
    if (int e = vec_out64(h, result, x_inout, kind, r))
        return e;
    HIPTRY(h, hipStreamSynchronize(st));
    return status;
}

}  // namespace
}  // namespace cwf

using namespace cwf;

extern "C" {

int cwf_refine_scale_exponent(double residual_norm, double rhs_norm)
{
    // e with 2^e |r| in (|b| / 2, 2 |b|): the difference of the two binades. A zero (or non-finite) residual needs no
    // scale; with |b| = 0 (only prescribed values load the system) the residual goes to the binade of 1.
    if (!(residual_norm > 0.0) || !std::isfinite(residual_norm))
        return 0;
    const double target = rhs_norm > 0.0 && std::isfinite(rhs_norm) ? rhs_norm : 1.0;
    return std::ilogb(target) - std::ilogb(residual_norm);  // ilogb counts a subnormal's leading zeros
}

int cwf_hip_residual_f64(cwf_hip_system *h, const double *rhs, const double *x, double *r_out, uint64_t n, int kind,
                         double *norm)
{
    if (!h)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    if (!rhs || !x)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer", !rhs ? "rhs" : "x");
    if (int st = check_ready(h))
        return st;
    if (int st = refine_ready(h, n, "the fp64 residual"))
        return st;
    if (int st = vec_in64(h, rhs, h->rf_b, kind, h->rf_r))
        return st;
    if (int st = vec_in64(h, x, h->rf_x, kind, h->rf_r))
        return st;
    refine_residual(h->ds, h->rf_x, h->rf_b, h->rf_r, h->rf_share, h->rf_part, norm_out(h), h->stream);
    double v = 0.0;
    if (int st = read_norm(h, &v))
        return st;
    if (norm)
        *norm = v;
    if (r_out)
        if (int st = vec_out64(h, h->rf_r, r_out, kind, h->rf_xp))
            return st;
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_residual_f64_timed(cwf_hip_system *h, int reps, double *avg_ms)
{
    if (!h)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    if (!avg_ms || reps <= 0)
        return set_error(h, CWF_ERR_ARGUMENT, "bad argument");
    if (int st = check_ready(h))
        return st;
    if (int st = refine_ready(h, h->ds.D, "the fp64 residual"))
        return st;
    Stopwatch sw;
    if (!sw.make())
        return set_error(h, CWF_ERR_HIP, "hipEventCreate failed");
    // whatever the workspace holds would do for the timing; zeros keep the arithmetic free of NaN operands
    HIPTRY(h, hipMemsetAsync(h->rf_x, 0, (size_t)h->ds.D * sizeof(double), h->stream));
    HIPTRY(h, hipMemsetAsync(h->rf_b, 0, (size_t)h->ds.D * sizeof(double), h->stream));
    refine_residual_tiles(h->ds, h->rf_x, h->rf_b, h->rf_r, h->rf_share, h->stream);
    double ms = 0.0;
    sw.start(h->stream);
    for (int i = 0; i < reps; ++i)
        refine_residual_tiles(h->ds, h->rf_x, h->rf_b, h->rf_r, h->rf_share, h->stream);
    sw.stop(h->stream, &ms);
    HIPTRY(h, hipGetLastError());
    HIPTRY(h, hipStreamSynchronize(h->stream));
    *avg_ms = ms / reps;
    return 0;
}

int cwf_hip_solve_refined(cwf_hip_system *h, const double *rhs, const cwf_refine_settings *s, double *x_inout,
                          uint64_t n, int kind, cwf_refine_telemetry *tel)
{
    if (!h)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    cwf_refine_telemetry local{};
    if (tel)
        std::memset(tel, 0, sizeof *tel);
    else
        tel = &local;
    if (!rhs || !x_inout)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer", !rhs ? "rhs" : "x_inout");
    if (int st = check_ready(h))
        return st;
    const cwf_refine_settings defaults{};
    if (!s)
        s = &defaults;
    constexpr uint32_t kHistory = sizeof(tel->history) / sizeof(tel->history[0]);
    if (s->max_outer >= kHistory)
        return set_error(h, CWF_ERR_ARGUMENT, "max_outer must be <= 31", "max_outer=" + std::to_string(s->max_outer));
    if (!(s->relative_tolerance >= 0.0))
        return set_error(h, CWF_ERR_ARGUMENT, "relative_tolerance must be >= 0",
                         "relative_tolerance=" + std::to_string(s->relative_tolerance));
    if (!(s->stagnation_ratio >= 0.0))
        return set_error(h, CWF_ERR_ARGUMENT, "stagnation_ratio must be >= 0",
                         "stagnation_ratio=" + std::to_string(s->stagnation_ratio));
    if (int st = refine_ready(h, n, "the refined solve"))
        return st;
    RefinePlan rp{};
    rp.max_outer = s->max_outer ? s->max_outer : 12;
    rp.tol = s->relative_tolerance > 0.0 ? s->relative_tolerance : 1e-10;
    rp.ratio = s->stagnation_ratio > 0.0 ? s->stagnation_ratio : 0.5;
    rp.warm = s->warm_start != 0;
    rp.inner = s->inner;
    rp.inner.warm_start = 0;
    if (!(rp.inner.relative_tolerance > 0.0))
        rp.inner.relative_tolerance = 1e-4;
    if (rp.inner.max_iterations == 0)
        rp.inner.max_iterations = 20000;
    // the inner solves leave the handle's first-batch bookkeeping as the caller's own solves left it
    const uint64_t last = h->last_iters, prev = h->prev_iters;
    const int st = refine_iterate(h, rp, rhs, x_inout, kind, tel);
    h->last_iters = last;
    h->prev_iters = prev;
    return st;
}

}  // extern "C"
