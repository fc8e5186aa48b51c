// ties_tables.cpp -- ties_tables.hpp: the tied boundaries' host-side refusals, slot / group words, internal-order CSR
// and the velocity projection. Host arrays in, host arrays out.
#include "ties_tables.hpp"

#include <algorithm>

namespace cwf
{

int tied_ids_once(uint64_t N, const uint32_t *ids, uint64_t count, std::vector<uint8_t> &seen, const std::string &prefix,
                  std::string *msg, std::string *ctx)
{
    for (uint64_t i = 0; i < count; ++i)
    {
        const uint32_t node = ids[i];
        if (node >= N || seen[node])
        {
            *msg = node >= N ? "tied node out of range" : "tied node listed twice";
            *ctx = prefix + "index=" + std::to_string(i) + "\nnode=" + std::to_string(node);
            return 1;
        }
        seen[node] = 1;
    }
    return 0;
}

int tie_refusal(uint64_t N, const uint32_t *mask, uint64_t groups, const uint64_t *offsets, const uint32_t *ids,
                std::string *msg, std::string *ctx)
{
    auto refuse = [&](const char *m, const std::string &c) {
        *msg = m;
        *ctx = c;
        return 1;
    };
    if (offsets[0] != 0)
        return refuse("tie offsets must ascend from 0", "group=0");
    for (uint64_t g = 0; g < groups; ++g)
        if (offsets[g + 1] < offsets[g])
            return refuse("tie offsets must ascend from 0", "group=" + std::to_string(g));
    for (uint64_t g = 0; g < groups; ++g)
        if (offsets[g + 1] - offsets[g] < 2)
            return refuse("tie group needs at least two nodes",
                          "group=" + std::to_string(g) + "\nnodes=" + std::to_string(offsets[g + 1] - offsets[g]));
    const uint64_t members = offsets[groups];
    std::vector<uint8_t> seen(N, 0);
    if (tied_ids_once(N, ids, members, seen, "", msg, ctx))
        return 1;
    for (uint64_t g = 0; mask && g < groups; ++g)
    {
        const uint32_t first = mask[ids[offsets[g]]];
        for (uint64_t i = offsets[g] + 1; i < offsets[g + 1]; ++i)
            if (mask[ids[i]] != first)
                return refuse("tied nodes differ in their constraints",
                              "group=" + std::to_string(g) + "\nnode=" + std::to_string(ids[i]) +
                                  "\nmask=" + std::to_string(mask[ids[i]]) + "\nfirst_mask=" + std::to_string(first));
    }
    return 0;
}

TieSlots tie_slots(uint64_t N, const uint32_t *dash_ids, uint64_t dash_count, uint64_t groups, const uint64_t *offsets,
                   const uint32_t *ids)
{
    TieSlots s;
    s.slot.assign(std::max<uint64_t>(N, 4), kTieNone);
    s.dash_slots = (uint32_t)dash_count;
    s.node.assign(dash_ids, dash_ids + dash_count);
    s.group.assign(dash_count, kTieNone);
    for (uint64_t i = 0; i < dash_count; ++i)
        s.slot[dash_ids[i]] = (uint32_t)i;
    for (uint64_t g = 0; g < groups; ++g)
        for (uint64_t i = offsets[g]; i < offsets[g + 1]; ++i)
        {
            uint32_t &w = s.slot[ids[i]];
            if (w == kTieNone)
            {
                w = (uint32_t)s.node.size();
                s.node.push_back(ids[i]);
                s.group.push_back(kTieNone);
            }
            s.group[w] = (uint32_t)g;
        }
    return s;
}

int tie_csr(const TieSlots &s, const std::vector<uint32_t> &back, uint64_t groups, const uint64_t *offsets,
            const uint32_t *ids, TieCsr *out)
{
    std::vector<uint32_t> internal(s.node.size(), kTieNone);  // slot -> internal node
    for (size_t n = 0; n < back.size(); ++n)
        if (back[n] != kTieNone)
        {
            if (back[n] >= internal.size() || internal[back[n]] != kTieNone)
                return 1;
            internal[back[n]] = (uint32_t)n;
        }
    out->toff.resize(groups + 1);
    out->tnode.resize(offsets[groups]);
    for (uint64_t g = 0; g <= groups; ++g)
        out->toff[g] = (uint32_t)offsets[g];
    for (uint64_t i = 0; i < offsets[groups]; ++i)
    {
        const uint32_t w = s.slot[ids[i]];
        if (w == kTieNone || internal[w] == kTieNone)
            return 1;
        out->tnode[i] = internal[w];
    }
    return 0;
}

void tie_project(uint64_t groups, const uint64_t *offsets, const uint32_t *ids, const float *mass, const uint32_t *mask,
                 float *v)
{
    for (uint64_t g = 0; g < groups; ++g)
    {
        const uint64_t b = offsets[g], e = offsets[g + 1];
        double M = (double)mass[ids[b]];
        for (uint64_t i = b + 1; i < e; ++i)
            M = M + (double)mass[ids[i]];
        const uint32_t mk = mask[ids[b]];
        for (int k = 0; k < 3; ++k)
        {
            double acc = (double)mass[ids[b]] * (double)v[3ull * ids[b] + k];
            for (uint64_t i = b + 1; i < e; ++i)
                acc = acc + (double)mass[ids[i]] * (double)v[3ull * ids[i] + k];
            const float mean = (mk & (1u << k)) ? 0.f : (float)(acc / M);
            for (uint64_t i = b; i < e; ++i)
                v[3ull * ids[i] + k] = mean;
        }
    }
}

}  // namespace cwf
