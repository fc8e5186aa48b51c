// explicit_state.hpp -- what the explicit stepper's translation units share: the stepper itself (abi_explicit.cpp: the
// core and advance) with its attachments (abi_explicit_loads.cpp: dashpots and load sources,
// abi_explicit_monitors.cpp: node and element monitors, abi_explicit_plasticity.cpp, abi_explicit_ties.cpp: tied
// boundaries and the slot arrays they share with the dashpots), the staging helper every
// set_* builds its device arrays with, and the two node-list helpers.
#pragma once

#include <cstdio>

#include "abi_internal.hpp"
#include "ties_tables.hpp"

namespace cwf
{

// A new set's device arrays, staged in a stepper's arena (what Uploader is to a handle's). Every set_* goes: refuse on
// the host, stage (allocate, upload or zero on the stepper's stream), finish() (one synchronise), then release
// the old set and adopt() the new one. The first failure is kept (set_error's status or a HIP error) and every later
// call does nothing. A stage that ends without adopt() frees what it took: the set in force is untouched.
class ArenaStage
{
  public:
    explicit ArenaStage(TransientState &t) : t_(t), s_(t.sys->stream) {}
    ArenaStage(const ArenaStage &) = delete;
    ~ArenaStage()
    {
        if (!held_.empty())
            (void)hipStreamSynchronize(s_);  // nothing staged still writes what is freed
        for (void *p : held_)
            t_.mem.free(p);
    }
    // an attachment's release(): frees the arrays the set adopted (its `held`) and leaves the empty set
    template <class Set> static void release(DeviceArena &mem, Set &set)
    {
        for (void *p : set.held)
            mem.free(p);
        set = Set();
    }

    bool ok() const { return !st_ && e_ == hipSuccess; }
    size_t bytes() const { return bytes_; }  // sum of count * sizeof(T) asked for, not the arena's rounded sizes
    template <class T> T *alloc(size_t count)
    {
        T *p = nullptr;
        if (ok() && !(st_ = t_.alloc(&p, count)))
        {
            held_.push_back(p);
            bytes_ += count * sizeof(T);
        }
        return p;
    }
    template <class T> T *put(const T *src, size_t count)
    {
        T *p = alloc<T>(count);
        if (ok() && count)
            e_ = hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s_);
        return p;
    }
    template <class T> T *put(const std::vector<T> &v) { return put(v.data(), v.size()); }
    template <class T> T *zeros(size_t count)
    {
        T *p = alloc<T>(count);
        if (ok())
            e_ = hipMemsetAsync(p, 0, count * sizeof(T), s_);
        return p;
    }
    // anything else queued on the stream for the new set (the envelopes' start values, which reset shares; the
    // sources' f_ext kernels) joins the same failure
    void check(hipError_t e)
    {
        if (ok())
            e_ = e;
    }
    // one synchronise; 0, or the first failure's status (a HIP error is reported as `what`)
    int finish(const char *what)
    {
        const hipError_t e = hipStreamSynchronize(s_);
        if (st_)
            return st_;
        check(e);
        return e_ == hipSuccess ? 0 : (st_ = hip_fail(t_.sys, e_, what));
    }
    // hands the arrays over: the set's pointer list, which its release() drops
    std::vector<void *> adopt() { return std::move(held_); }

  private:
    TransientState &t_;
    hipStream_t s_;
    int st_ = 0;
    hipError_t e_ = hipSuccess;
    size_t bytes_ = 0;
    std::vector<void *> held_;
};

inline std::string num17(double v)
{
    char b[40];
    std::snprintf(b, sizeof b, "%.17g", v);
    return b;
}

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;  // == kNoDashpot: a node that a list does not name
// every id below N and listed once: 0, or the refusal "<stem> out of range" / "<stem> listed twice" with the context
// "<prefix>index=i\nnode=n". seen [>= N] is the caller's: seen[n] == stamp says the list named n already, and every
// id leaves its stamp, so lists that may share nodes with each other (the load sources) take a stamp each.
int nodes_listed_once(cwf_hip_system *h, const char *stem, const std::string &prefix, const uint32_t *ids,
                      uint64_t count, std::vector<uint32_t> &seen, uint32_t stamp);
// A caller-order slot vector (one word per node, at least 4) moved to the handle's internal node order as a one-word
// node vector (vec_in: bit copies), on the device in dev [slot.size()] and, with back, as a host list [N] as well.
// dev NULL: a buffer of the call's own.
int slots_to_internal(TransientState &t, const std::vector<uint32_t> &slot, uint32_t *dev, std::vector<uint32_t> *back);

}  // namespace cwf

// u, v, f, bcv, the load pattern and the arena: the shared state core (abi_transient.cpp)
struct cwf_hip_explicit : cwf::TransientState
{
    double alpha = 0.0, beta = 0.0, dt = 0.0, lambda_max = 0.0, critical_dt = 0.0;
    uint64_t steps = 0;
    bool input_stale = true;  // beta_R != 0: w has to be formed from u and v before the next step
    float *w = nullptr, *y = nullptr;
    uint32_t *non_finite = nullptr;
    std::vector<double> ctimes, cvalues;  // set_load_curve
    double last_scale = 0.0;              // c(t) of the last step taken (get_state 4 with a pattern)
    // set_dashpots: the caller's ids and matrices as given. Empty ids: no dashpots.
    std::vector<uint32_t> dash_ids;
    std::vector<double> dash_C;
    // set_ties: the groups as given (offsets [groups + 1], ids). Empty ids: no ties.
    std::vector<uint64_t> tie_offsets;
    std::vector<uint32_t> tie_ids;
    // What the update pass reads of dashpots and ties, one set of arrays for both (ties_tables.hpp has the layout): a
    // u32 slot per node (internal order), the slots' P | Q records, and with ties the slots' group words, the groups'
    // CSR, their masses and g_G. plan_slots / adopt_slots are its only owners: set_dashpots and set_ties each call
    // them with what they are about to put in force (their own new set and the other's current one), so either call
    // order ends in the same arrays. plan_slots refuses on the host and changes nothing; adopt_slots stages the new
    // arrays before the old ones go, and a failure (reported as `what`) leaves the old ones.
    struct Slots
    {
        uint32_t *dslot = nullptr;
        double *dpq = nullptr;
        uint32_t *dgroup = nullptr;
        uint32_t slots = 0, dash_slots = 0;
        cwf::ExplicitTies tie{};
        uint64_t members = 0, dashed_groups = 0, bytes = 0;
        std::vector<void *> held;
        void release(cwf::DeviceArena &mem) { cwf::ArenaStage::release(mem, *this); }
    } slots;
    struct SlotPlan  // the host side of a new set of slot arrays
    {
        cwf::TieSlots tab;
        std::vector<double> pq;     // [18 slots]
        std::vector<double> tmass;  // [groups]
        std::vector<uint64_t> offsets;
        std::vector<uint32_t> ids;
        uint64_t dashed_groups = 0;
    };
    int plan_slots(const std::vector<uint32_t> &dash, const std::vector<double> &C, const std::vector<uint64_t> &offsets,
                   const std::vector<uint32_t> &ids, SlotPlan *plan);
    int adopt_slots(SlotPlan &plan, const char *what);
    // v of every tie group replaced by its mass-weighted mean (set_ties, and set_state(1) while a set is in force)
    int project_tied_velocity();
    // The ledger's slot-indexed copy of the dashpot matrices (arena): present iff a ledger and dashpots are both set.
    // sync_ledger_C is its only owner: set_dashpots and set_monitors call it with what they are about to put in force
    // (a ledger or not, the matrices as given), before they change anything else. The new copy is staged before the
    // old one goes; a failure (reported as `what`) leaves the old one.
    double *dC = nullptr;
    int sync_ledger_C(bool ledger, const std::vector<double> &C, const char *what);

    // Each attachment: the set in force, its device arrays (the stepper's arena; `held` lists them, release() drops
    // them) and the host's bookkeeping. The members that take a step count are advance()'s, in launch order.
    // set_monitors. The host knows every step count, so which update is sampled and the row it lands in are launch
    // arguments; there are no device counters.
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
        std::vector<void *> held;
        void release(cwf::DeviceArena &mem) { cwf::ArenaStage::release(mem, *this); }
        // the pass's monitor fields for the update that reaches step `next`; true: the ledger samples it
        bool arm(cwf::ExplicitPass &a, uint64_t next) const
        {
            a.peak = peak;
            a.peak_stride = peak_stride;
            a.ecum = ecum;
            a.ecur = ecur;
            a.esample = eevery && next % eevery == 0 && esteps.size() < ecap ? 1u : 0u;
            return a.esample != 0;
        }
        // after the update that reached `steps`: the ledger's row, then the receivers' row; a due sample without room
        // is counted as dropped
        void sample(uint64_t steps, bool ledger_sampled, uint32_t blocks, const float *u, const float *v,
                    hipStream_t st);
    } mon;
    // set_sources: the set as given (get_sources); dev.loaded == 0: no set
    struct Sources
    {
        struct Given
        {
            std::vector<double> times, values, amplitude, delay;
            std::vector<uint32_t> ids;
        };
        std::vector<Given> given;
        uint64_t entries = 0, points = 0, bytes = 0;
        cwf::ExplicitSources dev{};
        std::vector<void *> held;
        void release(cwf::DeviceArena &mem) { cwf::ArenaStage::release(mem, *this); }
    } src;
    // set_element_monitors
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
        std::vector<void *> held;
        void release(cwf::DeviceArena &mem) { cwf::ArenaStage::release(mem, *this); }
        // the element pass over u_steps: envelopes over all elements when due, the gauges' row when due and there is
        // room (else counted as dropped). False: nothing is set, no launch
        bool arm(cwf::ExplicitElementPass &ep, uint64_t steps);
        void recorded(const cwf::ExplicitElementPass &ep, uint64_t steps)  // after the launch
        {
            if (ep.envelope)
                ++esamples;
            if (ep.gauge_row)
                gsteps.push_back(steps);
        }
    } emon;
    // set_plasticity and set_soil_plasticity (one set, whichever came last): dev.slots == 0: none; the slots' elements
    // on the host (read_plasticity scatters through them). model: 0 none, 1 J2, 2 soil, whose further arrays are soil's
    struct Plasticity
    {
        cwf::ExplicitPlasticity dev{};
        cwf::ExplicitSoil soil{};
        int model = 0;
        int node_pass = 1;  // the soil set's node pass, cwf_explicit_soil_desc.node_pass resolved (1, 2 or 3)
        std::vector<uint32_t> elem;
        uint64_t bytes = 0;
        std::vector<void *> held;
        void release(cwf::DeviceArena &mem) { cwf::ArenaStage::release(mem, *this); }
    } pl;
};

namespace cwf
{
// an entry point's first check: a stepper, and its handle ready
inline int explicit_ready(const cwf_hip_explicit *t)
{
    return t ? check_ready(t->sys) : set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
}
}  // namespace cwf
