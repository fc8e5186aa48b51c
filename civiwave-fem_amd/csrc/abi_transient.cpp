// abi_transient.cpp -- the state core the Newmark stepper (abi_stepper.cpp) and the explicit stepper
// (explicit_state.hpp, abi_explicit*.cpp) share (TransientState, abi_internal.hpp): the create tail, state and external force in and out
// of the handle's node order, the fp64 load pattern, the time getter. Each C entry point checks its own handle for
// NULL, maps `which` to a pointer of its own and calls in here; a NULL pointer from that table is an unknown field.
#include "abi_internal.hpp"

namespace cwf
{

void transient_quiesce(const TransientState &c)
{
    (void)hipSetDevice(c.sys->device);
    (void)hipStreamSynchronize(c.sys->stream);
}

int transient_start(TransientState &c, const float *external_force, const float *bc_value, const char *what)
{
    cwf_hip_system *h = c.sys;
    for (float *p : {c.u, c.v, c.f, c.bcv})
        (void)hipMemsetAsync(p, 0, h->ds.D * sizeof(float), h->stream);
    int st = 0;
    if (external_force)
        st = vec_in(h, external_force, c.f, CWF_PTR_HOST, 3);
    if (!st && bc_value)
        st = vec_in(h, bc_value, c.bcv, CWF_PTR_HOST, 3);
    const hipError_t e = hipStreamSynchronize(h->stream);
    return st || e == hipSuccess ? st : hip_fail(h, e, what);
}

int transient_form_load(TransientState &c, double scale)
{
    cwf_hip_system *h = c.sys;
    stepper_scaled_load(h->ds.D, c.lbase, c.lpat, scale, c.f, h->stream);
    HIPTRY(h, hipGetLastError());
    return 0;
}

int transient_get(TransientState &c, const float *src, float *out, uint64_t n, int kind, const double *load_scale)
{
    cwf_hip_system *h = c.sys;
    if (int st = check_ready(h))
        return st;
    if (n != h->ds.D)
        return set_error(h, CWF_ERR_SIZE, "state span size mismatch");
    if (!src)
        return set_error(h, CWF_ERR_ARGUMENT, "unknown state field");
    if (load_scale)
        if (int st = transient_form_load(c, *load_scale))
            return st;
    if (int st = vec_out(h, src, out, kind, 3))
        return st;
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int transient_set(TransientState &c, const char *what, float *dst, const float *in, uint64_t n, int kind, bool sync)
{
    cwf_hip_system *h = c.sys;
    if (int st = check_ready(h))
        return st;
    if (n != h->ds.D)
        return set_error(h, CWF_ERR_SIZE, std::string(what) + " span size mismatch");
    if (!dst)
        return set_error(h, CWF_ERR_ARGUMENT, "unknown state field");
    if (int st = vec_in(h, in, dst, kind, 3))
        return st;
    if (sync)
        HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int transient_set_load_pattern(TransientState &c, const double *base, const double *pattern, uint64_t n)
{
    cwf_hip_system *h = c.sys;
    if (int st = check_ready(h))
        return st;
    if (n != h->ds.D)
        return set_error(h, CWF_ERR_SIZE, "load pattern span size mismatch",
                         "input=" + std::to_string(n) + "\ndofs=" + std::to_string(h->ds.D));
    if (!c.lbase)
    {
        if (int st = c.alloc(&c.lbase, 2 * n))
            return st;
        c.lpat = c.lbase + n;
    }
    // a node's 3 f64 = 6 floats: the node-order conversion moves them as 6-float records
    if (int st = vec_in(h, reinterpret_cast<const float *>(base), reinterpret_cast<float *>(c.lbase), CWF_PTR_HOST, 6))
        return st;
    if (int st = vec_in(h, reinterpret_cast<const float *>(pattern), reinterpret_cast<float *>(c.lpat), CWF_PTR_HOST,
                        6))
        return st;
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int transient_time(double now, double dt, double *current_time, double *time_step)
{
    if (current_time)
        *current_time = now;
    if (time_step)
        *time_step = dt;
    return 0;
}

}  // namespace cwf
