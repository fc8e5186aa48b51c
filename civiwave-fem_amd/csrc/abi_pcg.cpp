// abi_pcg.cpp -- the PCG entry points of the C-ABI (include/cwf_hip.h; pcg.hpp:161-227): apply_keff, the block
// Jacobi inverse, dot, solve_pcg (single handle and LOCAL groups) and the residual history, over the device
// PCG driver run_pcg_group (the FAST / PARITY / sharded schedules, enqueued in batches with only
// the control block read back).
#include <cmath>
#include <cstring>

#include "abi_internal.hpp"
#include "blockinv_pack.hpp"

namespace cwf
{

std::string pcg_error_message(int code, int iter, PcgSchedule sch, std::string *ctx)
{
    if (code == CWF_ERR_COMM)  // a PEER exchange step's bounded wait (peer.hip): a peer never arrived
    {
        *ctx = "step=" + std::to_string(iter);
        return "peer exchange timed out";
    }
    if (code == CWF_ERR_HIP && sch == PcgSchedule::Resident)  // resident.hip: a phase's bounded wait ran out
    {
        *ctx = "phase=" + std::to_string(iter);
        return "resident solve: a workgroup missed the phase barrier";
    }
    if (code == CWF_ERR_RHO_ZERO && iter < 0)
    {
        *ctx = "rho~0";
        return "preconditioner produced near-zero rho";  // pcg.cpp:810-813
    }
    *ctx = "iteration=" + std::to_string(iter);
    if (code == CWF_ERR_DENOM_ZERO)
        return "CG denominator approached zero";  // pcg.cpp:846-849
    if (code == CWF_ERR_HIP)  // parity_pcg.hip stream_fail: the chunk partials of a streamed fold never all arrived
        return "PARITY streamed scalar fold timed out";
    return "CG rho approached zero";  // pcg.cpp:889-892
}

namespace
{
// the solve's telemetry and error from the control block read back last (every member's is identical)
int pcg_finish(const std::vector<cwf_hip_system *> &g, PcgSchedule sch, cwf_pcg_telemetry *tel)
{
    cwf_hip_system *h = g[0];
    const Ctl &c = *h->ctl_host;
    for (cwf_hip_system *m : g)
    {
        m->hist_count = c.iterations + 1;
        m->prev_iters = m->last_iters;
        m->last_iters = c.iterations;
    }
    if (tel)
    {
        tel->iterations = c.iterations;
        tel->residual_norm = c.res;
        tel->rhs_norm = c.rhs_norm_raw;
        tel->alpha_last = c.alpha_last;
        tel->beta_last = c.beta_last;
        tel->converged = c.converged;
        tel->reserved = 0;
    }
    if (c.error)
    {
        std::string ctx;
        std::string msg = pcg_error_message(c.error, c.error_iter, sch, &ctx);
        for (size_t i = 1; i < g.size(); ++i)
            set_error(g[i], c.error, msg, ctx);
        return set_error(h, c.error, msg, ctx);
    }
    return 0;
}

// a timed handle's events, two per launch of the largest batch (no L2 write-back per timed launch)
int timing_events(cwf_hip_system *h, size_t n)
{
    const size_t had = h->ev.size();
    if (!h->timing || had >= n)
        return 0;
    h->ev.resize(n);
    for (size_t i = had; i < n; ++i)
        HIPTRY(h, hipEventCreateWithFlags(&h->ev[i], hipEventDisableSystemFence));
    return 0;
}

// ---- the four steps of a solve, by schedule (a shard's group g: every member driven here; else g = {h}) -----------
// r_0, the norms, the tolerance and what the schedule's first launch reads. Resident: the fused init without its
// launch 0 (the one launch runs phase 0 itself)
int pcg_init(PcgSchedule sch, const std::vector<cwf_hip_system *> &g, const std::vector<const float *> &rhs, double tol)
{
    cwf_hip_system *h = g[0];
    const bool sharded = h->sharded();
    switch (sch)
    {
    case PcgSchedule::Resident:
        return sharded ? sharded_resident_init(g, rhs, tol) : (fast_fused_init(h, rhs[0], tol, h->stream, false), 0);
    case PcgSchedule::Fused:
    case PcgSchedule::FusedPeer:
        return sharded ? sharded_fused_init(g, rhs, tol, sch) : (fast_fused_init(h, rhs[0], tol, h->stream), 0);
    case PcgSchedule::TwoKernel:
        return sharded ? sharded_pcg_init(g, rhs, tol) : (fast_pcg_init(h, rhs[0], tol, h->stream), 0);
    case PcgSchedule::Parity:
        return parity_pcg_init_group(g, rhs, tol);
    }
    return 0;
}

// iteration `it` of a launch-per-iteration schedule (member 0's launch carries the timing events)
int pcg_iteration(PcgSchedule sch, const std::vector<cwf_hip_system *> &g, const std::vector<const float *> &rhs,
                  unsigned it, hipEvent_t e0, hipEvent_t e1)
{
    cwf_hip_system *h = g[0];
    const bool sharded = h->sharded();
    switch (sch)
    {
    case PcgSchedule::Fused:
    case PcgSchedule::FusedPeer:
        return sharded ? sharded_fused_iteration(g, it, e0, e1, sch) : (fast_fused_iteration(h, it, h->stream, e0, e1), 0);
    case PcgSchedule::TwoKernel:
        return fast_pcg_iteration_group(g, rhs, it, e0, e1);
    case PcgSchedule::Parity:
        return parity_pcg_iteration_group(g, rhs, e0, e1);
    case PcgSchedule::Resident:  // (no launch per iteration)
        break;
    }
    return 0;
}

// after a batch (`it` iterations enqueued in all): the convergence of its last launch (Fused) or last update
// (TwoKernel), repeated idempotently by the next launch's start. PARITY decides in its own kernels. last: `it` is the
// solve's max_iterations (the fused check then leaves alpha_last and beta_last those of the last update made)
void pcg_batch_check(PcgSchedule sch, const std::vector<cwf_hip_system *> &g, unsigned it, bool last)
{
    switch (sch)
    {
    case PcgSchedule::Fused:
    case PcgSchedule::FusedPeer:
        for (cwf_hip_system *m : g)
            fast_fused_check(m, it, m->stream, last);
        break;
    case PcgSchedule::TwoKernel:
        for (cwf_hip_system *m : g)
            fast_check_pcg(m, it, m->stream);
        break;
    default:
        break;
    }
}

// after the last batch: the solve's x and r where the schedule left them pending
int pcg_flush(PcgSchedule sch, const std::vector<cwf_hip_system *> &g, const std::vector<const float *> &rhs)
{
    switch (sch)
    {
    case PcgSchedule::Fused:  // x is updated in every launch; the solve's r output is the last launch's
    case PcgSchedule::FusedPeer:
        for (cwf_hip_system *m : g)
            fast_fused_finish(m, m->stream);
        return g[0]->sharded() ? sharded_fused_end(g, sch) : 0;
    case PcgSchedule::TwoKernel:  // x += alpha_j p_j of the iterations since the last lazy x update
        for (size_t i = 0; i < g.size(); ++i)
            fast_flush_x(g[i], rhs[i], g[i]->stream);
        return 0;
    default:
        return 0;
    }
}

// the resident solve after its init: ONE launch that runs every iteration on chip (resident.hip) and leaves x, r and
// the control block; hipEvent-timed as a whole when timing is on (the handle's K_eff timing then counts its
// iterations: avg = the time per iteration). A PEER slab shard (one member per process): ghost x from the owners
// after the solve
int run_pcg_resident(cwf_hip_system *h, const cwf_pcg_settings &set, cwf_pcg_telemetry *tel)
{
    hipStream_t st = h->stream;
    if (int e = timing_events(h, 2))
        return e;
    hipEvent_t e0 = h->timing ? h->ev[0] : nullptr, e1 = h->timing ? h->ev[1] : nullptr;
    const uint32_t max_it = (uint32_t)set.max_iterations;  // (<= 2^24: solve_schedule)
    launch_pcg_resident(h, max_it, st, e0, e1);
    // the next solve's tags start past every tag this one can publish (phases 0 .. max_it + 1)
    h->res.tag += max_it + 3u;
    HIPTRY(h, hipGetLastError());
    HIPTRY(h, hipMemcpyAsync(h->ctl_host, h->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st));
    HIPTRY(h, hipStreamSynchronize(st));
    if (h->sharded() && !h->ctl_host->error)  // ghost x <- owners (the stepper's node-wise updates read the ghost rows too)
    {
        if (int e = comm_halo({h}, &cwf_hip_system::x))
            return e;
        HIPTRY(h, hipStreamSynchronize(st));
    }
    if (e0 && h->ctl_host->iterations)
    {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess)
        {
            h->keff_ms += ms;
            h->keff_count += h->ctl_host->iterations;
        }
    }
    return pcg_finish({h}, PcgSchedule::Resident, tel);
}
}  // namespace

// run solve_pcg on device buffers: rhs[i] and g[i]->x (holding the warm start) for every member of a
// group -- one handle, or every rank of a sharded system driven from this process (LOCAL comm).
int run_pcg_group(const std::vector<cwf_hip_system *> &g, const std::vector<const float *> &rhs,
                  const cwf_pcg_settings &set, cwf_pcg_telemetry *tel)
{
    cwf_hip_system *h = g[0];
    if (set.max_iterations == 0)
        return set_error(h, CWF_ERR_MAX_ITERATIONS, "max_iterations must be >= 1", "max_iterations=0");
    const bool sharded = h->sharded();
    if (!sharded && g.size() != 1)
        return set_error(h, CWF_ERR_ARGUMENT, "a group needs attached shards");
    for (cwf_hip_system *m : g)
        if (m->mode != h->mode)
            return set_error(m, CWF_ERR_ARGUMENT, "every rank of a sharded solve runs in the same mode",
                             "rank=" + std::to_string(m->rank));
    for (cwf_hip_system *m : g)
        if (m->hist_cap < set.max_iterations + 1)
        {
            const uint64_t cap = std::max<uint64_t>(set.max_iterations + 1, 1024);
            if (m->hist.alloc(cap) != hipSuccess)
                return set_error(m, CWF_ERR_ALLOC, "failed to grow matrix-free workspace buffers",
                                 "history=" + std::to_string(cap));
            m->hist_cap = cap;
        }
    hipStream_t st = h->stream;
    if (!set.warm_start)
        for (cwf_hip_system *m : g)
            HIPTRY(m, hipMemsetAsync(m->x, 0, m->ds.D * sizeof(float), m->stream));
    // the schedule: planned at the handle's first FAST solve (shards: agreed by every rank), one value per solve
    if (int e = plan_schedule(g))
        return e;
    const PcgSchedule sch =
        h->mode == CWF_MODE_FAST ? solve_schedule(h->sched, set.max_iterations) : PcgSchedule::Parity;
    if (int e = pcg_init(sch, g, rhs, set.relative_tolerance))
        return e;
    if (sch == PcgSchedule::Resident)  // (one member: the plan is resident for a single handle or PEER shard only)
        return run_pcg_resident(h, set, tel);
    HIPTRY(h, hipGetLastError());
    uint64_t enq = 0;
    constexpr uint64_t kMaxBatch = 64;
    uint64_t batch = set.check_interval > 0 ? std::min<uint64_t>((uint64_t)set.check_interval, kMaxBatch) : 4;
    // Batches end in a control-block read-back (a host round trip with the GPU idle) and overshoot the
    // converging iteration by up to a batch of no-op launches. Consecutive solves on one handle (warm-started
    // Newmark steps) take similar iteration counts, so with no check interval set and the handle's last two
    // solves within 25% of each other, the first batch runs up to 24 short of the smaller count and the
    // doubling restarts from 4 there: C2 steps ~17 read-backs and ~50 no-op iterations -> ~4 and <= 8. A
    // handle whose counts moved (its first solves, a static solve before Newmark steps, a changed tolerance)
    // doubles from 4, so a solve that converges early never waits on a long queue of no-op launches. Every
    // rank of a sharded solve has the same history (identical scalars), so their enqueued counts stay equal.
    uint64_t first = batch;
    const uint64_t lo = std::min(h->last_iters, h->prev_iters), hi = std::max(h->last_iters, h->prev_iters);
    if (set.check_interval <= 0 && lo > 40 && 4 * hi <= 5 * lo)
    {
        first = std::min<uint64_t>(lo - 24, kMaxFirstBatch);
        batch = 4;
    }
    if (int e = timing_events(h, 2 * std::max(first, kMaxBatch)))
        return e;
    uint64_t prev_enq = 0, prev_nb = 0;
    for (;;)
    {
        // every member's control block is identical (rank-order folds); member 0's is polled
        HIPTRY(h, hipMemcpyAsync(h->ctl_host, h->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st));
        HIPTRY(h, hipStreamSynchronize(st));
        if (h->timing && prev_nb)
        {
            // only launches that did work: iteration index < completed iterations
            for (uint64_t i = 0; i < prev_nb; ++i)
            {
                if (prev_enq + i >= h->ctl_host->iterations)
                    break;
                if ((prev_enq + i) % (uint64_t)h->timing)
                    continue;
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]) == hipSuccess)
                {
                    h->keff_ms += ms;
                    ++h->keff_count;
                }
            }
            prev_nb = 0;
        }
        if (!h->ctl_host->active || enq >= set.max_iterations)
            break;
        const uint64_t nb = std::min<uint64_t>(enq ? batch : first, set.max_iterations - enq);
        for (uint64_t i = 0; i < nb; ++i)
        {
            const bool timed = h->timing && (enq + i) % (uint64_t)h->timing == 0;
            hipEvent_t e0 = timed ? h->ev[2 * i] : nullptr, e1 = timed ? h->ev[2 * i + 1] : nullptr;
            if (int e = pcg_iteration(sch, g, rhs, (unsigned)(enq + i), e0, e1))
                return e;
        }
        pcg_batch_check(sch, g, (unsigned)(enq + nb), enq + nb >= set.max_iterations);
        HIPTRY(h, hipGetLastError());
        prev_enq = enq;
        prev_nb = nb;
        enq += nb;
        if (set.check_interval <= 0)
            batch = std::min<uint64_t>(batch * 2, kMaxBatch);
    }
    if (int e = pcg_flush(sch, g, rhs))
        return e;
    if (sharded)  // ghost x <- owners, so node-wise stepper updates stay consistent on ghost rows
    {
        if (int e = comm_halo(g, &cwf_hip_system::x))
            return e;
        for (cwf_hip_system *m : g)
            HIPTRY(m, hipStreamSynchronize(m->stream));
    }
    return pcg_finish(g, sch, tel);
}

int run_pcg(cwf_hip_system *h, const float *rhs_dev, const cwf_pcg_settings &set, cwf_pcg_telemetry *tel)
{
    if (h->comm && h->comm->kind == 0 && h->nranks > 1)
        return set_error(h, CWF_ERR_UNSUPPORTED, "a LOCAL-communicator shard solves through cwf_hip_solve_pcg_group");
    return run_pcg_group({h}, {rhs_dev}, set, tel);
}


}  // namespace cwf

using namespace cwf;

extern "C" {

int cwf_hip_apply_keff(cwf_hip_system *h, const float *x, float *y, uint64_t n, int kind)
{
    if (int st = check_ready(h))
        return st;
    if (n != h->ds.D)
        return set_error(h, CWF_ERR_SIZE, "input/output span size mismatch",
                         "input=" + std::to_string(n) + "\ndofs=" + std::to_string(h->ds.D));
    const float *xin = nullptr;
    if (int st = stage_vec(h, x, h->tmp, kind, 3, &xin))
        return st;
    float *yout = kind == CWF_PTR_DEVICE && !h->perm ? y : h->Ap;
    keff_apply(h, xin, yout, h->stream);
    HIPTRY(h, hipGetLastError());
    if (int st = vec_out(h, yout, y, kind, 3))
        return st;
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_build_block_jacobi_inverse(cwf_hip_system *h, float *inv_out, uint64_t n, int kind)
{
    if (int st = check_ready(h))
        return st;
    const uint64_t req = 9ull * h->ds.N;
    if (n < req)
        return set_error(h, CWF_ERR_SIZE, "block inverse span too small",
                         "required=" + std::to_string(req) + "\navailable=" + std::to_string(n));
    float *dst = kind == CWF_PTR_DEVICE && !h->perm ? inv_out : h->inv;
    if (dst == h->inv)
        h->inv_fast = false;  // overwritten with the unsymmetrised reference inverse
    if (h->ds.hex)
        hex_block_jacobi(h, dst, h->stream);
    else
        parity_block_jacobi(h, dst, h->stream);
    HIPTRY(h, hipGetLastError());
    if (int st = vec_out(h, dst, inv_out, kind, 9))
        return st;
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_fast_block_inverse(cwf_hip_system *h, float *inv_out, uint64_t n, int kind, uint32_t *packed_out,
                               uint64_t *fallback_nodes)
{
    if (int st = check_ready(h))
        return st;
    const uint64_t N = h->ds.N, req = 9ull * N;
    if (n < req)
        return set_error(h, CWF_ERR_SIZE, "block inverse span too small",
                         "required=" + std::to_string(req) + "\navailable=" + std::to_string(n));
    if (h->mode != CWF_MODE_FAST)
        return set_error(h, CWF_ERR_ARGUMENT, "FAST-mode operator requested on a PARITY handle");
    fast_block_inverse(h, h->stream);
    HIPTRY(h, hipGetLastError());
    if (int st = vec_out(h, h->inv, inv_out, kind, 9))
        return st;
    if (packed_out || fallback_nodes)
    {
        std::vector<uint32_t> w(4 * N);
        if (N)
            HIPTRY(h, hipMemcpyAsync(w.data(), h->inv6, 16 * N, hipMemcpyDeviceToHost, h->stream));
        HIPTRY(h, hipStreamSynchronize(h->stream));
        std::vector<uint32_t> perm;  // caller's node of internal node i
        if (h->perm)
        {
            perm.resize(N);
            HIPTRY(h, hipMemcpy(perm.data(), h->perm, 4 * N, hipMemcpyDeviceToHost));
        }
        std::vector<uint32_t> out(4 * N);
        uint64_t nf = 0;
        for (uint64_t i = 0; i < N; ++i)
        {
            const uint64_t c = h->perm ? perm[i] : i;
            for (int k = 0; k < 4; ++k)
                out[4 * c + k] = w[4 * i + k];
            nf += (int32_t)w[4 * i] < 0;
        }
        if (packed_out)
            std::memcpy(packed_out, out.data(), out.size() * sizeof(uint32_t));
        if (fallback_nodes)
            *fallback_nodes = nf;
    }
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_pack_block_inverse(const float *v, uint32_t mask, uint32_t *w, float *d)
{
    if (!v || !w || !d)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    return cwf::pack_block_inverse(v, mask, w, d) ? 1 : 0;
}

int cwf_hip_dot(cwf_hip_system *h, const float *a, const float *b, uint64_t n, int kind, double *out,
                double *partials)
{
    if (int st = check_ready(h))
        return st;
    if (!out)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    if (n != h->ds.D)
        return set_error(h, CWF_ERR_SIZE, "dot product span size mismatch",
                         "lhs=" + std::to_string(n) + "\ndofs=" + std::to_string(h->ds.D));
    const float *da = nullptr, *db = nullptr;
    if (int st = stage_in(h, a, h->tmp, n, kind, &da))
        return st;
    if (int st = stage_in(h, b, h->Ap, n, kind, &db))
        return st;
    double *res = h->scal;
    uint32_t count;
    if (h->mode == CWF_MODE_FAST)
    {
        count = fast_dot_blocks(h->ds.D);
        fast_dot(da, db, nullptr, h->ds.D, h->part0, nullptr, h->stream);
        fast_fold(h->part0, count, res, h->stream);
    }
    else
    {
        count = parity_chunk_count(h);
        parity_dot_partials(h->ds.D, (uint32_t)h->reduction_block, da, db, nullptr, h->part0, nullptr, nullptr,
                            h->stream);
        parity_fold(h->part0, count, res, h->stream);
    }
    HIPTRY(h, hipGetLastError());
    HIPTRY(h, hipMemcpyAsync(out, res, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (partials)
    {
        const uint64_t total = h->reduction_partials;
        const uint64_t ncopy = std::min<uint64_t>(count, total);
        if (kind == CWF_PTR_DEVICE)
        {
            HIPTRY(h, hipMemcpyAsync(partials, h->part0, ncopy * sizeof(double), hipMemcpyDeviceToDevice,
                                     h->stream));
            if (total > ncopy)
                HIPTRY(h, hipMemsetAsync(partials + ncopy, 0, (total - ncopy) * sizeof(double), h->stream));
        }
        else
        {
            HIPTRY(h, hipMemcpyAsync(partials, h->part0, ncopy * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            HIPTRY(h, hipStreamSynchronize(h->stream));
            for (uint64_t c = ncopy; c < total; ++c)
                partials[c] = 0.0;
        }
    }
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_solve_pcg(cwf_hip_system *h, const float *rhs, const cwf_pcg_settings *settings, float *x_inout,
                      float *residual_out, uint64_t n, int kind, cwf_pcg_telemetry *telemetry)
{
    if (int st = check_ready(h))
        return st;
    if (!rhs || !settings || !x_inout)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    if (telemetry)
        std::memset(telemetry, 0, sizeof *telemetry);
    if (n != h->ds.D)
        return set_error(h, CWF_ERR_SIZE, "rhs span size mismatch",
                         "rhs=" + std::to_string(n) + "\ndofs=" + std::to_string(h->ds.D));
    if (settings->max_iterations == 0)
        return set_error(h, CWF_ERR_MAX_ITERATIONS, "max_iterations must be >= 1", "max_iterations=0");
    const float *drhs = nullptr;
    if (int st = stage_vec(h, rhs, h->rhs, kind, 3, &drhs))
        return st;
    if (settings->warm_start)
        if (int st = vec_in(h, x_inout, h->x, kind, 3))
            return st;
    int st = run_pcg(h, drhs, *settings, telemetry);
    if (int e = vec_out(h, h->x, x_inout, kind, 3))
        return e;
    if (residual_out)
        if (int e = vec_out(h, h->r, residual_out, kind, 3))
            return e;
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return st;
}

int cwf_hip_solve_pcg_group(cwf_hip_system *const *members, int32_t count, const float *const *rhs,
                            const cwf_pcg_settings *settings, float *const *x_inout, float *const *residual_out,
                            int kind, cwf_pcg_telemetry *telemetry)
{
    if (!members || count < 1 || !rhs || !settings || !x_inout)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    if (telemetry)
        std::memset(telemetry, 0, sizeof *telemetry);
    std::vector<cwf_hip_system *> g(members, members + count);
    cwf_hip_comm *cm = g[0] ? g[0]->comm : nullptr;
    for (int32_t i = 0; i < count; ++i)
    {
        if (int st = check_ready(g[i]))
            return st;
        if (!rhs[i] || !x_inout[i])
            return set_error(g[i], CWF_ERR_ARGUMENT, "null pointer");
        if (count > 1 && (!cm || cm->kind != 0 || g[i]->comm != cm || g[i]->rank != i || cm->nranks != count))
            return set_error(g[i], CWF_ERR_ARGUMENT, "members must be every rank of one LOCAL communicator, in rank order",
                             "member=" + std::to_string(i));
    }
    if (settings->max_iterations == 0)
        return set_error(g[0], CWF_ERR_MAX_ITERATIONS, "max_iterations must be >= 1", "max_iterations=0");
    std::vector<const float *> drhs(count);
    for (int32_t i = 0; i < count; ++i)
    {
        cwf_hip_system *h = g[i];
        if (int st = stage_in(h, rhs[i], h->rhs, h->ds.D, kind, &drhs[i]))
            return st;
        if (settings->warm_start)
            HIPTRY(h, hipMemcpyAsync(h->x, x_inout[i], h->ds.D * sizeof(float),
                                     kind == CWF_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                     h->stream));
    }
    int st = run_pcg_group(g, drhs, *settings, telemetry);
    const hipMemcpyKind back = kind == CWF_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    for (int32_t i = 0; i < count; ++i)
    {
        cwf_hip_system *h = g[i];
        HIPTRY(h, hipMemcpyAsync(x_inout[i], h->x, h->ds.D * sizeof(float), back, h->stream));
        if (residual_out && residual_out[i])
            HIPTRY(h, hipMemcpyAsync(residual_out[i], h->r, h->ds.D * sizeof(float), back, h->stream));
        HIPTRY(h, hipStreamSynchronize(h->stream));
    }
    return st;
}

int cwf_hip_residual_history(cwf_hip_system *h, double *out, uint64_t capacity, uint64_t *count)
{
    if (int st = check_ready(h))
        return st;
    const uint64_t c = std::min(capacity, h->hist_count);
    if (c && out)
        HIPTRY(h, hipMemcpy(out, h->hist, c * sizeof(double), hipMemcpyDeviceToHost));
    if (count)
        *count = c;
    return 0;
}

}  // extern "C"
