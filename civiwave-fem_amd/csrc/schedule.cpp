// schedule.cpp -- which PCG schedule a handle's FAST solves run (PcgSchedule, cwf_internal.hpp; the table is DESIGN.md
// section 3, "Which schedule runs"). Decided once per handle, at its first solve or its first diagnostic query, and
// kept: two pure functions map the facts to the plan and the plan to one solve's schedule; plan_schedule gathers the
// facts (the only place that reads CWF_FUSED, CWF_FUSED_MAXWG and CWF_RESIDENT), makes the resident plan and, for
// shards, takes the ranks' vote. The driver (abi_pcg.cpp) and the diagnostic queries (abi.cpp) read the result.
#include "abi_internal.hpp"

namespace cwf
{

// what this handle could run, were it alone. Fused by default where one round of workgroups covers the work items (C2
// fused 46.6k vs two-kernel 46.9k PCG it/s, same box: one launch and one exchange per iteration for the same time);
// beyond one round the persistent walk (234-248 VGPRs, 2 waves/SIMD) loses to the two kernels: C3 8.3k vs 10.8k it/s
// (profiles/r05b), so only CWF_FUSED=2 takes it. A shard owning a single node plane keeps the two kernels: the fused
// launch's ghost-plane forms assume owned planes on both sides of a brick's first and last plane (slabs one cell
// thick did not converge fused, LOCAL and PEER alike; tests/test_gpu_lattice.py::test_thin_slab_shards_take_two_kernels).
// The in-kernel exchange and the resident solve need one member per process; any explicit CWF_FUSED keeps the
// launch-per-iteration schedules
ScheduleVote own_vote(const ScheduleFacts &f)
{
    const int on = f.fused_knob < 0 ? 1 : f.fused_knob;
    ScheduleVote v;
    v.fuse = f.mode == CWF_MODE_FAST && f.fusable && (on == 2 || (on == 1 && f.grid_covers)) &&
             (!f.sharded || f.thick_slab);
    const bool alone = v.fuse && f.group == 1;
    v.peer = alone && f.sharded && f.peer_eligible;
    v.resident = alone && f.fused_knob < 0 && !f.resident_off && f.resident_plan;
    return v;
}

SchedulePlan choose_schedule(const ScheduleFacts &f)
{
    const ScheduleVote v = f.sharded ? f.all : own_vote(f);  // shards run what every rank can
    SchedulePlan p;
    p.state = SchedulePlan::Decided;
    p.fused_knob = f.fused_knob;
    p.launch = f.mode != CWF_MODE_FAST ? PcgSchedule::Parity
               : !v.fuse               ? PcgSchedule::TwoKernel
               : v.peer                ? PcgSchedule::FusedPeer
                                       : PcgSchedule::Fused;
    p.resident = f.mode == CWF_MODE_FAST && v.fuse && v.resident;
    return p;
}

// the resident kernel counts its phases in 24 bits of the granule tags: a longer solve runs launch by launch
PcgSchedule solve_schedule(const SchedulePlan &p, uint64_t max_iterations)
{
    return p.resident && max_iterations <= (1u << 24) ? PcgSchedule::Resident : p.launch;
}

int exchange_schedule_code(const SchedulePlan &p)
{
    if (p.state != SchedulePlan::Decided || p.launch == PcgSchedule::Parity)
        return -1;  // no vote yet (PARITY shards take none)
    return p.resident ? 3 : p.launch == PcgSchedule::FusedPeer ? 2 : p.launch == PcgSchedule::Fused ? 1 : 0;
}

namespace
{
// what the handle's own data and the knobs say, the cross-rank facts left unset. At the first ask the knobs are read
// and the fused grid sized (CWF_FUSED_MAXWG: the largest grid that fuses: every workgroup folds five shares of each of
// the previous launch's workgroups); until the plan is decided `launch` holds what the handle could run alone (a
// shard's thin slab not counted: its vote does that)
ScheduleFacts local_facts(cwf_hip_system *h)
{
    const DevTiles &t = h->ds.t;
    SchedulePlan &sp = h->sched;
    ScheduleFacts f;
    f.mode = h->mode;
    f.fusable = t.lat && t.lcls && t.lcz && h->r2 && h->fsh && h->g_fsh && t.ntiles;
    if (sp.state == SchedulePlan::Unplanned && f.fusable)
    {
        const char *on = knob("CWF_FUSED"), *cap = knob("CWF_FUSED_MAXWG");
        sp.fused_knob = on ? std::max(atoi(on), 0) : -1;
        sp.grid = pcg_lattice_launch_grid(h->ds, cap && atoi(cap) > 0 ? (unsigned)atoi(cap) : 1024u);
    }
    f.fused_knob = sp.fused_knob;
    f.grid_covers = sp.grid >= t.lnwork;
    if (sp.state == SchedulePlan::Unplanned)
    {
        sp.state = SchedulePlan::Local;
        sp.launch = own_vote(f).fuse ? PcgSchedule::Fused : PcgSchedule::TwoKernel;
    }
    return f;
}

// ... and the facts of a handle driven as one of `group` members
ScheduleFacts own_facts(cwf_hip_system *h, size_t group)
{
    ScheduleFacts f = local_facts(h);
    const char *res = knob("CWF_RESIDENT");
    f.resident_off = res && res[0] == '0';
    f.group = (int)group;
    f.sharded = h->sharded();
    f.thick_slab = h->ds.t.lk1 >= h->ds.t.lk0 + 2;
    // asked only where the answer decides something: the eligibility check reads the halo plan back, a resident plan
    // allocates. A shard's resident kernel stores its surface records into the neighbours' mailboxes itself: PEER only
    f.peer_eligible = f.resident_plan = true;
    const ScheduleVote want = own_vote(f);
    f.peer_eligible = want.peer && peer_fused_eligible(h);
    f.resident_plan = want.resident && (!f.sharded || (h->comm && h->comm->kind == 2 && h->nranks <= kMaxPeers)) &&
                      (h->res.G || plan_resident(h, f.sharded));  // (G: made before a vote that failed)
    return f;
}
}  // namespace

int plan_schedule(const std::vector<cwf_hip_system *> &g)
{
    cwf_hip_system *h0 = g[0];
    if (h0->mode != CWF_MODE_FAST || h0->sched.state == SchedulePlan::Decided)
        return 0;
    std::vector<ScheduleFacts> facts;
    ScheduleVote all{true, true, true};
    for (cwf_hip_system *h : g)
    {
        facts.push_back(own_facts(h, g.size()));
        const ScheduleVote v = own_vote(facts.back());
        all = ScheduleVote{all.fuse && v.fuse, all.peer && v.peer, all.resident && v.resident};
    }
    uint64_t tag = h0->res.tag;
    if (h0->sharded())
    {
        // the decision is collective: every member's vote (and, through one all-gather, every rank's), and the
        // resident tag base every rank then takes from the largest (the ranks' granules must carry the same tags)
        for (cwf_hip_system *h : g)
        {
            const double v[2] = {all.fuse ? 1.0 : 0.0,
                                 (all.peer ? 1.0 : 0.0) + (all.resident ? 2.0 : 0.0) + 4.0 * (double)h->res.tag};
            HIPTRY(h, hipMemcpyAsync(h->g_init + 2 * h->rank, v, sizeof v, hipMemcpyHostToDevice, h->stream));
            HIPTRY(h, hipStreamSynchronize(h->stream));
        }
        // a rank that cannot learn the others' votes must not pick a schedule alone (its peers could agree
        // on the fused one and then wait for exchange steps it never runs): the solve fails instead, decided by nobody
        if (int st = comm_allgather(g, &cwf_hip_system::g_init, 2))
            return st < 0 ? st : set_error(h0, CWF_ERR_COMM, "schedule agreement all-gather failed");
        std::vector<double> got(2 * (size_t)h0->nranks, 0.0);
        HIPTRY(h0, hipStreamSynchronize(h0->stream));
        HIPTRY(h0, hipMemcpy(got.data(), h0->g_init, got.size() * sizeof(double), hipMemcpyDeviceToHost));
        tag = 0;
        for (int r = 0; r < h0->nranks; ++r)
        {
            const uint64_t pv = (uint64_t)got[2 * (size_t)r + 1];
            all = ScheduleVote{all.fuse && got[2 * (size_t)r] == 1.0, all.peer && (pv & 1u), all.resident && (pv & 2u)};
            tag = std::max<uint64_t>(tag, pv >> 2);
        }
    }
    for (size_t i = 0; i < g.size(); ++i)
    {
        facts[i].all = all;
        const unsigned grid = g[i]->sched.grid;
        g[i]->sched = choose_schedule(facts[i]);
        g[i]->sched.grid = grid;
        if (g[i]->sched.resident)
            g[i]->res.tag = (uint32_t)tag;
    }
    return 0;
}

PcgSchedule schedule_of(const cwf_hip_system *h)
{
    if (h->mode != CWF_MODE_FAST)
        return PcgSchedule::Parity;
    if (h->sched.state == SchedulePlan::Unplanned)
    {
        // The one plan made behind a read-only query: a handle asked before its first solve reports the schedule that
        // solve will take (tests/golden/create_layout.json pins the resident traffic and the memory counter read
        // there), so it is planned here as the solve would plan it. A shard plans its own half; its vote waits for
        // the solve, which every rank enters
        cwf_hip_system *m = const_cast<cwf_hip_system *>(h);
        if (h->sharded())
            (void)local_facts(m);
        else
            (void)plan_schedule({m});
    }
    return h->sched.resident ? PcgSchedule::Resident : h->sched.launch;
}

}  // namespace cwf
