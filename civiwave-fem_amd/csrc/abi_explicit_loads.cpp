// abi_explicit_loads.cpp -- what loads the explicit stepper besides its external force (explicit_state.hpp): the
// dashpots (include/cwf_hip.h "Absorbing boundaries") and the load sources ("Load sources").
#include <algorithm>
#include <cmath>

#include "explicit_state.hpp"
#include "explicit_tables.hpp"

using namespace cwf;

extern "C" {

int cwf_hip_explicit_set_dashpots(cwf_hip_explicit *t, uint64_t count, const uint32_t *node_ids, const double *C)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    if (count && (!node_ids || !C))
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    const uint64_t N = h->ds.N;
    const bool ledger = t->mon.ecum != nullptr;
    // everything that can be refused, on the host, before anything changes
    if (count)
    {
        std::vector<uint32_t> seen(std::max<uint64_t>(N, 4), kNoDashpot);
        if (int st = nodes_listed_once(h, "dashpot node", "", node_ids, count, seen, 0))
            return st;
    }
    std::vector<uint32_t> ids(node_ids, node_ids + count);
    std::vector<double> given(C, C + 9 * count);
    // the slots and records of the new dashpots and the ties in force (a refused matrix, a node's or a group's)
    cwf_hip_explicit::SlotPlan plan;
    if (int st = t->plan_slots(ids, given, t->tie_offsets, t->tie_ids, &plan))
        return st;
    if (int st = t->sync_ledger_C(ledger, given, "explicit set_dashpots"))  // a ledger reads C as given
        return st;
    if (int st = t->adopt_slots(plan, "explicit set_dashpots"))
    {
        (void)t->sync_ledger_C(ledger, t->dash_C, "explicit set_dashpots");  // the previous set's, with its slots
        return st;
    }
    t->dash_ids = std::move(ids);
    t->dash_C = std::move(given);
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
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
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
    std::vector<uint32_t> slot(std::max<uint64_t>(N, 4), kNoSlot);  // caller's node -> its index among the loaded nodes
    std::vector<uint32_t> seen(std::max<uint64_t>(N, 4), kNoSlot);  // caller's node -> the last source that listed it
    uint32_t nodes = 0;
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
        // a source may share nodes with another source, not with itself
        if (int st = nodes_listed_once(h, "load source node", sq + "\n", d.node_ids, d.entry_count, seen, q))
            return st;
        for (uint64_t i = 0; i < d.entry_count; ++i)
        {
            if (!std::isfinite(d.delay[i]) || !std::isfinite(d.amplitude[3 * i]) ||
                !std::isfinite(d.amplitude[3 * i + 1]) || !std::isfinite(d.amplitude[3 * i + 2]))
                return set_error(h, CWF_ERR_ARGUMENT, "load source entry is not finite",
                                 sq + "\nindex=" + std::to_string(i));
            if (slot[d.node_ids[i]] == kNoSlot)
                slot[d.node_ids[i]] = nodes++;
        }
    }
    // the loaded nodes in the internal order
    std::vector<uint32_t> back;
    if (int st = slots_to_internal(*t, slot, nullptr, &back))
        return st;
    std::vector<uint32_t> rank(nodes), node(nodes);  // caller-side index -> l; l -> internal node
    uint32_t L = 0;
    for (uint64_t n = 0; n < N; ++n)
        if (back[n] != kNoSlot)
        {
            rank[back[n]] = L;
            node[L++] = (uint32_t)n;
        }
    if (L != nodes)
        return set_error(h, CWF_ERR_INDEX, "load source nodes were lost in the node order");
    const SourceTables T = source_tables(sources, count, slot, rank);
    // the new set's buffers; the stepper's once everything went well
    ArenaStage stage(*t);
    cwf_hip_explicit::Sources m;
    m.dev.loaded = nodes;
    m.dev.node = stage.put(node);
    m.dev.off = stage.put(T.off);
    m.dev.rec = stage.put(T.rec);
    m.dev.cur = stage.put(T.dir);
    m.dev.tab = stage.put(T.tab);
    m.dev.fext = stage.alloc<float>(3 * (size_t)nodes);
    if (int st = stage.finish("explicit set_sources"))
        return st;
    // the force buffer holds f_n at the previous set's nodes: their f_ext goes back before the new set's is taken out
    if (cur.dev.loaded)
        explicit_sources_fext(cur.dev, t->f, false, s);
    explicit_sources_fext(m.dev, t->f, true, s);
    stage.check(hipGetLastError());
    if (int st = stage.finish("explicit set_sources"))
        return st;
    m.entries = T.entries;
    m.points = T.points;
    m.bytes = stage.bytes();
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
    m.held = stage.adopt();
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

}  // extern "C"
