// explicit_tables.cpp -- the load sources' CSR and plasticity's slot tables (explicit_tables.hpp): host arrays in, host
// arrays out, no device and no handle.
#include "explicit_tables.hpp"

#include <algorithm>

namespace cwf
{

SourceTables source_tables(const cwf_explicit_source_desc *sources, uint32_t count, const std::vector<uint32_t> &slot,
                           const std::vector<uint32_t> &rank)
{
    SourceTables T;
    for (uint32_t q = 0; q < count; ++q)
    {
        T.entries += sources[q].entry_count;
        T.points += sources[q].curve_points;
    }
    // counts, offsets, then the entries source by source
    const size_t nodes = rank.size();
    T.off.assign(nodes + 1, 0);
    T.dir.resize(2 * T.entries);
    T.rec.resize(4 * T.entries);
    T.tab.resize(2 * T.points);
    for (uint32_t q = 0; q < count; ++q)
        for (uint64_t i = 0; i < sources[q].entry_count; ++i)
            ++T.off[rank[slot[sources[q].node_ids[i]]] + 1];
    for (size_t l = 0; l < nodes; ++l)
        T.off[l + 1] += T.off[l];
    std::vector<uint32_t> fill(T.off.begin(), T.off.end() - 1);
    uint64_t at = 0;
    for (uint32_t q = 0; q < count; ++q)
    {
        const cwf_explicit_source_desc &d = sources[q];
        std::copy(d.times, d.times + d.curve_points, T.tab.begin() + at);
        std::copy(d.values, d.values + d.curve_points, T.tab.begin() + at + d.curve_points);
        for (uint64_t i = 0; i < d.entry_count; ++i)
        {
            const uint32_t e = fill[rank[slot[d.node_ids[i]]]]++;
            T.rec[4ull * e] = d.amplitude[3 * i];
            T.rec[4ull * e + 1] = d.amplitude[3 * i + 1];
            T.rec[4ull * e + 2] = d.amplitude[3 * i + 2];
            T.rec[4ull * e + 3] = d.delay[i];
            T.dir[2ull * e] = (uint32_t)at;
            T.dir[2ull * e + 1] = (uint32_t)d.curve_points;
        }
        at += 2 * d.curve_points;
    }
    return T;
}

int plastic_tables(const std::vector<uint32_t> &mat, const std::vector<uint32_t> &off,
                   const std::vector<uint32_t> &inc, const std::vector<uint8_t> &plastic, PlasticTables *out)
{
    const uint64_t E = mat.size(), M = plastic.size(), N = off.empty() ? 0 : off.size() - 1;
    const uint32_t kNone = 0xFFFFFFFFu;
    PlasticTables T;
    std::vector<uint32_t> slot_of(E, kNone);
    for (uint64_t e = 0; e < E; ++e)
        if (mat[e] < M && plastic[mat[e]])
        {
            slot_of[e] = (uint32_t)T.elem.size();
            T.elem.push_back((uint32_t)e);
        }
    if (T.elem.empty())
    {
        *out = PlasticTables();
        return 0;
    }
    T.aoff.assign(1, 0);
    T.cpos.assign(4 * T.elem.size(), 0);
    uint32_t run = 0;
    for (uint64_t n = 0; n < N; ++n)
    {
        for (uint32_t j = off[n]; j < off[n + 1]; ++j)
        {
            const uint32_t e = inc[j] >> 2;
            if (e < E && slot_of[e] != kNone)
                T.cpos[4ull * slot_of[e] + (inc[j] & 3u)] = run++;
        }
        if (run != T.aoff.back())
        {
            T.anode.push_back((uint32_t)n);
            T.aoff.push_back(run);
        }
    }
    T.incidences = run;
    *out = std::move(T);
    return out->incidences != out->cpos.size();
}

}  // namespace cwf
