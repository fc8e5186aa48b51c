// abi_explicit_ties.cpp -- the explicit stepper's tied boundaries (include/cwf_hip.h "Tied boundaries"): set / get /
// info, the velocity projection, and the two owner functions of the slot arrays that dashpots and ties share
// (explicit_state.hpp). The index tables themselves are ties_tables.cpp's.
#include <algorithm>

#include "explicit_state.hpp"

using namespace cwf;

namespace
{
// a one-word node vector of the handle (mass, mask) in the caller's order, on the host
template <class T> int node_words(cwf_hip_system *h, const T *dev, std::vector<T> *out)
{
    static_assert(sizeof(T) == 4, "one word per node");
    out->resize(std::max<uint64_t>(h->ds.N, 4));
    if (int st = vec_out(h, reinterpret_cast<const float *>(dev), reinterpret_cast<float *>(out->data()), CWF_PTR_HOST, 1))
        return st;
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}
}  // namespace

int cwf_hip_explicit::plan_slots(const std::vector<uint32_t> &dash, const std::vector<double> &C,
                                 const std::vector<uint64_t> &offsets, const std::vector<uint32_t> &ids, SlotPlan *plan)
{
    cwf_hip_system *h = sys;
    const uint64_t groups = offsets.empty() ? 0 : offsets.size() - 1;
    SlotPlan p;
    p.offsets = offsets;
    p.ids = ids;
    if (p.offsets.empty())
        p.offsets.push_back(0);
    p.tab = tie_slots(h->ds.N, dash.data(), dash.size(), groups, p.offsets.data(), ids.data());
    std::vector<float> mass;  // the f32 lumped mass in the caller's order
    if (!p.tab.node.empty())
        if (int st = node_words(h, h->ds.mass, &mass))
            return st;
    p.pq.assign(18 * p.tab.node.size(), 0.0);
    // every dashpot's own matrix first, tied or not: a refused one is reported by its index, as without ties
    for (uint64_t i = 0; i < dash.size(); ++i)
        if (const char *why = dashpot_update(&C[9 * i], (double)mass[dash[i]], alpha, dt, &p.pq[18 * i], &p.pq[18 * i + 9]))
            return set_error(h, CWF_ERR_ARGUMENT, why, "index=" + std::to_string(i));
    p.tmass.resize(groups);
    for (uint64_t g = 0; g < groups; ++g)
    {
        // M_G and C_G in member order from the first member; a member without a dashpot adds no C
        double M = 0.0, CG[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, rec[18];
        bool dashed = false;
        for (uint64_t i = p.offsets[g]; i < p.offsets[g + 1]; ++i)
        {
            const uint32_t w = p.tab.slot[ids[i]];
            M = i == p.offsets[g] ? (double)mass[ids[i]] : M + (double)mass[ids[i]];
            if (w < p.tab.dash_slots)
            {
                for (int k = 0; k < 9; ++k)
                    CG[k] = dashed ? CG[k] + C[9ull * w + k] : C[9ull * w + k];
                dashed = true;
            }
        }
        if (const char *why = dashpot_update(CG, M, alpha, dt, rec, rec + 9))
            return set_error(h, CWF_ERR_ARGUMENT, why, "group=" + std::to_string(g));
        p.tmass[g] = M;
        p.dashed_groups += dashed ? 1 : 0;
        for (uint64_t i = p.offsets[g]; i < p.offsets[g + 1]; ++i)
            std::copy(rec, rec + 18, &p.pq[18ull * p.tab.slot[ids[i]]]);
    }
    *plan = std::move(p);
    return 0;
}

int cwf_hip_explicit::adopt_slots(SlotPlan &p, const char *what)
{
    cwf_hip_system *h = sys;
    const uint64_t groups = p.offsets.size() - 1;
    if (p.tab.node.empty())
    {
        HIPTRY(h, hipStreamSynchronize(h->stream));
        slots.release(mem);
        return 0;
    }
    ArenaStage stage(*this);
    Slots m;
    m.slots = (uint32_t)p.tab.node.size();
    m.dash_slots = p.tab.dash_slots;
    m.dslot = stage.alloc<uint32_t>(p.tab.slot.size());
    std::vector<uint32_t> back;
    if (stage.ok())
        if (int st = slots_to_internal(*this, p.tab.slot, m.dslot, groups ? &back : nullptr))
            return st;
    m.dpq = stage.put(p.pq);
    if (groups)
    {
        TieCsr csr;
        if (stage.ok() && tie_csr(p.tab, back, groups, p.offsets.data(), p.ids.data(), &csr))
            return set_error(h, CWF_ERR_INDEX, "tied nodes were lost in the node order");
        m.dgroup = stage.put(p.tab.group);
        m.tie.groups = (uint32_t)groups;
        m.tie.toff = stage.put(csr.toff);
        m.tie.tnode = stage.put(csr.tnode);
        m.tie.tmass = stage.put(p.tmass);
        m.tie.tg = stage.zeros<double>(3 * groups);
        m.members = p.ids.size();
        m.dashed_groups = p.dashed_groups;
    }
    if (int st = stage.finish(what))
        return st;
    m.bytes = stage.bytes();
    m.held = stage.adopt();
    slots.release(mem);
    slots = std::move(m);
    return 0;
}

int cwf_hip_explicit::project_tied_velocity()
{
    cwf_hip_system *h = sys;
    if (tie_ids.empty())
        return 0;
    std::vector<float> mass, vel(h->ds.D);
    std::vector<uint32_t> mask;
    if (int st = node_words(h, h->ds.mass, &mass))
        return st;
    if (int st = node_words(h, h->ds.mask, &mask))
        return st;
    if (int st = vec_out(h, v, vel.data(), CWF_PTR_HOST, 3))
        return st;
    HIPTRY(h, hipStreamSynchronize(h->stream));
    tie_project(tie_offsets.size() - 1, tie_offsets.data(), tie_ids.data(), mass.data(), mask.data(), vel.data());
    if (int st = vec_in(h, vel.data(), v, CWF_PTR_HOST, 3))
        return st;
    HIPTRY(h, hipStreamSynchronize(h->stream));
    input_stale = true;
    return 0;
}

extern "C" {

int cwf_hip_explicit_set_ties(cwf_hip_explicit *t, uint64_t group_count, const uint64_t *offsets, const uint32_t *node_ids)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    cwf_hip_explicit::SlotPlan plan;
    if (group_count == 0)
    {
        if (int st = t->plan_slots(t->dash_ids, t->dash_C, {}, {}, &plan))
            return st;
        if (int st = t->adopt_slots(plan, "explicit set_ties"))
            return st;
        t->tie_offsets.clear();
        t->tie_ids.clear();
        return 0;
    }
    // everything that can be refused, on the host, before anything changes
    if (!offsets || !node_ids)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    if (group_count >= 0xFFFFFFFFull)
        return set_error(h, CWF_ERR_SIZE, "too many tie groups", "groups=" + std::to_string(group_count));
    std::vector<uint32_t> mask;
    if (int st = node_words(h, h->ds.mask, &mask))
        return st;
    std::string msg, ctx;
    if (tie_refusal(h->ds.N, mask.data(), group_count, offsets, node_ids, &msg, &ctx))
        return set_error(h, CWF_ERR_ARGUMENT, msg, ctx);
    std::vector<uint64_t> off(offsets, offsets + group_count + 1);
    std::vector<uint32_t> ids(node_ids, node_ids + offsets[group_count]);
    if (int st = t->plan_slots(t->dash_ids, t->dash_C, off, ids, &plan))
        return st;
    if (int st = t->adopt_slots(plan, "explicit set_ties"))
        return st;
    t->tie_offsets = std::move(off);
    t->tie_ids = std::move(ids);
    return t->project_tied_velocity();
}

int cwf_hip_explicit_get_ties(cwf_hip_explicit *t, uint64_t *group_count, uint64_t *member_count, uint64_t *offsets,
                              uint32_t *node_ids)
{
    if (!t || !group_count || !member_count)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    *group_count = t->tie_offsets.empty() ? 0 : t->tie_offsets.size() - 1;
    *member_count = t->tie_ids.size();
    if (offsets)
        std::copy(t->tie_offsets.begin(), t->tie_offsets.end(), offsets);
    if (node_ids)
        std::copy(t->tie_ids.begin(), t->tie_ids.end(), node_ids);
    return 0;
}

int cwf_hip_explicit_tie_info(cwf_hip_explicit *t, cwf_explicit_tie_info *out)
{
    if (!t || !out)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    cwf_explicit_tie_info I{};
    I.group_count = t->slots.tie.groups;
    I.member_count = t->slots.members;
    I.dashed_groups = t->slots.dashed_groups;
    I.device_bytes = t->slots.tie.groups ? t->slots.bytes : 0;
    *out = I;
    return 0;
}

}  // extern "C"
