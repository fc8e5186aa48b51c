// ties.cpp -- host-only helpers that build tie sets for cwf_hip_explicit_set_ties from node coordinates
// (include/cwf_hip.h "Tied boundaries"): the levels of a laminar box, the pairs of two periodic faces, and the merge of
// groups that share nodes. No GPU, no handle: errors go to the thread's record (cwf_hip_last_error(NULL)).
#include <algorithm>
#include <cmath>
#include <map>
#include <numeric>
#include <utility>

#include "abi_internal.hpp"
#include "ties_tables.hpp"

using namespace cwf;

namespace
{
int refuse(const char *msg, const std::string &ctx = "") { return set_error(nullptr, CWF_ERR_ARGUMENT, msg, ctx); }

// the model's extent along axis k times the relative tolerance (0: 1e-9)
double absolute_tolerance(uint64_t N, const double *X, int k, double tolerance)
{
    double lo = X[k], hi = X[k];
    for (uint64_t n = 1; n < N; ++n)
    {
        lo = std::min(lo, X[3 * n + k]);
        hi = std::max(hi, X[3 * n + k]);
    }
    return (tolerance == 0.0 ? 1e-9 : tolerance) * (hi - lo);
}

int check_list(uint64_t N, const uint32_t *ids, uint64_t count, std::vector<uint8_t> &seen, const std::string &prefix)
{
    std::string msg, ctx;
    return tied_ids_once(N, ids, count, seen, prefix, &msg, &ctx) ? refuse(msg.c_str(), ctx) : 0;
}

int check_common(uint64_t N, const double *X, int axis, double tolerance)
{
    if (!N || !X)
        return refuse("null pointer");
    if (axis < 0 || axis > 2)
        return refuse("tie axis must be 0, 1 or 2", "axis=" + std::to_string(axis));
    if (!(tolerance >= 0.0) || !std::isfinite(tolerance))
        return refuse("tie tolerance must be finite and not negative");
    return 0;
}
}  // namespace

extern "C" {

int cwf_tie_levels(uint64_t node_count, const double *coords, uint64_t count, const uint32_t *node_ids, int axis,
                   double tolerance, uint64_t *group_count, uint64_t *offsets, uint32_t *out_ids)
{
    if (int st = check_common(node_count, coords, axis, tolerance))
        return st;
    if (!group_count || !offsets || !out_ids || (count && !node_ids))
        return refuse("null pointer");
    std::vector<uint8_t> seen(node_count, 0);
    if (int st = check_list(node_count, node_ids, count, seen, ""))
        return st;
    const double tol = absolute_tolerance(node_count, coords, axis, tolerance);
    std::vector<uint32_t> order(node_ids, node_ids + count);
    auto z = [&](uint32_t n) { return coords[3ull * n + axis]; };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return z(a) != z(b) ? z(a) < z(b) : a < b; });
    uint64_t G = 0, out = 0;
    offsets[0] = 0;
    for (uint64_t b = 0; b < count;)
    {
        uint64_t e = b + 1;
        while (e < count && z(order[e]) - z(order[b]) <= tol)  // a level: within tol of its lowest node
            ++e;
        if (e - b >= 2)
        {
            std::copy(order.begin() + b, order.begin() + e, out_ids + out);
            std::sort(out_ids + out, out_ids + out + (e - b));
            out += e - b;
            offsets[++G] = out;
        }
        b = e;
    }
    *group_count = G;
    return 0;
}

int cwf_tie_periodic(uint64_t node_count, const double *coords, uint64_t count_a, const uint32_t *ids_a,
                     uint64_t count_b, const uint32_t *ids_b, int axis, double tolerance, uint64_t *group_count,
                     uint64_t *offsets, uint32_t *out_ids)
{
    if (int st = check_common(node_count, coords, axis, tolerance))
        return st;
    if (!group_count || !offsets || !out_ids || (count_a && !ids_a) || (count_b && !ids_b))
        return refuse("null pointer");
    std::vector<uint8_t> seen(node_count, 0);
    if (int st = check_list(node_count, ids_a, count_a, seen, "face=A\n"))
        return st;
    if (int st = check_list(node_count, ids_b, count_b, seen, "face=B\n"))
        return st;
    const int k0 = (axis + 1) % 3, k1 = (axis + 2) % 3;
    const double tol[2] = {absolute_tolerance(node_count, coords, k0, tolerance),
                           absolute_tolerance(node_count, coords, k1, tolerance)};
    const double lo[2] = {coords[k0], coords[k1]};
    // B's nodes in a grid of cells one tolerance wide: a partner lies in the cell of A's node or one next to it
    auto cell = [&](uint32_t n, int q) {
        const double c = coords[3ull * n + (q ? k1 : k0)] - lo[q];
        return tol[q] > 0.0 ? (int64_t)std::floor(c / tol[q]) : (int64_t)0;
    };
    auto near = [&](uint32_t a, uint32_t b) {
        return std::fabs(coords[3ull * a + k0] - coords[3ull * b + k0]) <= tol[0] &&
               std::fabs(coords[3ull * a + k1] - coords[3ull * b + k1]) <= tol[1];
    };
    std::map<std::pair<int64_t, int64_t>, std::vector<uint32_t>> grid;
    for (uint64_t i = 0; i < count_b; ++i)
        grid[{cell(ids_b[i], 0), cell(ids_b[i], 1)}].push_back(ids_b[i]);
    std::vector<uint8_t> taken(node_count, 0);
    for (uint64_t i = 0; i < count_a; ++i)
    {
        const uint32_t a = ids_a[i];
        uint32_t partner = 0;
        int found = 0;
        for (int64_t d0 = -1; d0 <= 1; ++d0)
            for (int64_t d1 = -1; d1 <= 1; ++d1)
            {
                auto it = grid.find({cell(a, 0) + d0, cell(a, 1) + d1});
                if (it == grid.end())
                    continue;
                for (uint32_t b : it->second)
                    if (near(a, b))
                    {
                        partner = b;
                        ++found;
                    }
            }
        if (found != 1 || taken[partner])
            return refuse("periodic faces do not match", "node=" + std::to_string(a) + "\nface=A");
        taken[partner] = 1;
        offsets[i] = 2 * i;
        out_ids[2 * i] = a;
        out_ids[2 * i + 1] = partner;
    }
    for (uint64_t i = 0; i < count_b; ++i)
        if (!taken[ids_b[i]])
            return refuse("periodic faces do not match", "node=" + std::to_string(ids_b[i]) + "\nface=B");
    offsets[count_a] = 2 * count_a;
    *group_count = count_a;
    return 0;
}

int cwf_tie_merge(uint64_t node_count, uint64_t in_groups, const uint64_t *in_offsets, const uint32_t *in_ids,
                  uint64_t *group_count, uint64_t *offsets, uint32_t *out_ids)
{
    if (!group_count || !offsets || !out_ids || (in_groups && (!in_offsets || !in_ids)))
        return refuse("null pointer");
    offsets[0] = 0;
    *group_count = 0;
    if (!in_groups)
        return 0;
    if (in_offsets[0] != 0)
        return refuse("tie offsets must ascend from 0", "group=0");
    for (uint64_t g = 0; g < in_groups; ++g)
        if (in_offsets[g + 1] < in_offsets[g])
            return refuse("tie offsets must ascend from 0", "group=" + std::to_string(g));
    const uint64_t members = in_offsets[in_groups];
    for (uint64_t i = 0; i < members; ++i)
        if (in_ids[i] >= node_count)
            return refuse("tied node out of range", "index=" + std::to_string(i) + "\nnode=" + std::to_string(in_ids[i]));
    // union-find over the listed nodes; a root is the smallest node of its set
    std::vector<uint32_t> parent(node_count);
    std::iota(parent.begin(), parent.end(), 0u);
    auto root = [&](uint32_t n) {
        while (parent[n] != n)
            n = parent[n] = parent[parent[n]];
        return n;
    };
    std::vector<uint8_t> listed(node_count, 0);
    for (uint64_t g = 0; g < in_groups; ++g)
        for (uint64_t i = in_offsets[g]; i < in_offsets[g + 1]; ++i)
        {
            listed[in_ids[i]] = 1;
            const uint32_t a = root(in_ids[in_offsets[g]]), b = root(in_ids[i]);
            if (a != b)
                parent[std::max(a, b)] = std::min(a, b);
        }
    // ascending node order visits every set at its smallest member first: groups by smallest member, members ascending
    std::vector<uint32_t> size(node_count, 0), place(node_count, 0);
    for (uint64_t n = 0; n < node_count; ++n)
        if (listed[n])
            ++size[root((uint32_t)n)];
    uint64_t G = 0, out = 0;
    for (uint64_t n = 0; n < node_count; ++n)
        if (listed[n] && root((uint32_t)n) == n && size[n] >= 2)
        {
            place[n] = (uint32_t)out;
            out += size[n];
            offsets[++G] = out;
        }
    std::vector<uint32_t> fill(node_count, 0);
    for (uint64_t n = 0; n < node_count; ++n)
        if (listed[n])
        {
            const uint32_t r = root((uint32_t)n);
            if (size[r] >= 2)
                out_ids[place[r] + fill[r]++] = (uint32_t)n;
        }
    *group_count = G;
    return 0;
}

}  // extern "C"
