// ties_tables_test.cpp -- csrc/ties_tables.cpp on the host: the refusals, the slot / group words that dashpots and ties
// share, the internal-order CSR and the projection of v. Without arguments it runs its own cases and prints "ok"; with
// a file (N, the dashpot ids, the offsets, the tied ids, the node order perm[internal] = caller's node, one list per
// line, each led by its length) it prints the tables for tests/test_ties_host.py to compare with numpy.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ties_tables.hpp"

using namespace cwf;

#define CHECK(c)                                                        \
    do                                                                  \
    {                                                                   \
        if (!(c))                                                       \
        {                                                               \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c);         \
            return 1;                                                   \
        }                                                               \
    } while (0)

// what slots_to_internal leaves on the host: internal node -> the slot word of the caller's node there
static std::vector<uint32_t> to_internal(const TieSlots &s, const std::vector<uint32_t> &perm)
{
    std::vector<uint32_t> back(perm.size());
    for (size_t i = 0; i < perm.size(); ++i)
        back[i] = s.slot[perm[i]];
    return back;
}

static int refused(uint64_t N, const std::vector<uint32_t> &mask, const std::vector<uint64_t> &off,
                   const std::vector<uint32_t> &ids, const char *msg, const char *ctx)
{
    std::string m, c;
    if (!tie_refusal(N, mask.data(), off.size() - 1, off.data(), ids.data(), &m, &c))
        return 1;
    if (m != msg || c != ctx)
    {
        std::printf("got \"%s\" {%s}, want \"%s\" {%s}\n", m.c_str(), c.c_str(), msg, ctx);
        return 1;
    }
    return 0;
}

static int self_test()
{
    const uint64_t N = 8;
    const std::vector<uint32_t> mask = {0, 0, 2, 2, 0, 0, 7, 0};
    std::string m, c;
    CHECK(!tie_refusal(N, mask.data(), 2, std::vector<uint64_t>{0, 2, 5}.data(), std::vector<uint32_t>{2, 3, 7, 0, 4}.data(), &m, &c));
    CHECK(!refused(N, mask, {1, 3}, {0, 1, 4}, "tie offsets must ascend from 0", "group=0"));
    CHECK(!refused(N, mask, {0, 3, 2}, {0, 1, 4}, "tie offsets must ascend from 0", "group=1"));
    CHECK(!refused(N, mask, {0, 2, 3}, {0, 1, 4}, "tie group needs at least two nodes", "group=1\nnodes=1"));
    CHECK(!refused(N, mask, {0, 2}, {0, 8}, "tied node out of range", "index=1\nnode=8"));
    CHECK(!refused(N, mask, {0, 2, 4}, {0, 1, 4, 1}, "tied node listed twice", "index=3\nnode=1"));
    CHECK(!refused(N, mask, {0, 3}, {2, 3, 6}, "tied nodes differ in their constraints",
                   "group=0\nnode=6\nmask=7\nfirst_mask=2"));
    // dashpots on 5, 3, 1; groups {2, 3} and {7, 0, 4}: slots 0 1 2 the dashpots, then 2, 7, 0, 4
    const std::vector<uint32_t> dash = {5, 3, 1}, ids = {2, 3, 7, 0, 4};
    const std::vector<uint64_t> off = {0, 2, 5};
    const TieSlots s = tie_slots(N, dash.data(), dash.size(), 2, off.data(), ids.data());
    CHECK(s.dash_slots == 3 && s.node == (std::vector<uint32_t>{5, 3, 1, 2, 7, 0, 4}));
    CHECK(s.group == (std::vector<uint32_t>{kTieNone, 0, kTieNone, 0, 1, 1, 1}));
    CHECK(s.slot == (std::vector<uint32_t>{5, 2, 3, 1, 6, 0, kTieNone, 4}));
    // without ties the words are set_dashpots' own; without dashpots the tied nodes take the slots in list order
    const TieSlots d = tie_slots(N, dash.data(), dash.size(), 0, std::vector<uint64_t>{0}.data(), nullptr);
    CHECK(d.node == dash && d.group == (std::vector<uint32_t>{kTieNone, kTieNone, kTieNone}));
    const TieSlots t = tie_slots(N, nullptr, 0, 2, off.data(), ids.data());
    CHECK(t.dash_slots == 0 && t.node == ids && t.group == (std::vector<uint32_t>{0, 0, 1, 1, 1}));
    CHECK(tie_slots(3, nullptr, 0, 0, std::vector<uint64_t>{0}.data(), nullptr).slot.size() == 4);  // at least 4 words
    // the CSR through a permuted node order: members keep their list order
    const std::vector<uint32_t> perm = {6, 4, 2, 0, 7, 5, 3, 1};
    TieCsr csr;
    CHECK(!tie_csr(s, to_internal(s, perm), 2, off.data(), ids.data(), &csr));
    CHECK(csr.toff == (std::vector<uint32_t>{0, 2, 5}) && csr.tnode == (std::vector<uint32_t>{2, 6, 4, 3, 1}));
    std::vector<uint32_t> lost = to_internal(s, perm);
    lost[2] = kTieNone;  // node 2's slot dropped on the way
    CHECK(tie_csr(s, lost, 2, off.data(), ids.data(), &csr));
    lost = to_internal(s, perm);
    lost[0] = lost[2];  // met twice
    CHECK(tie_csr(s, lost, 2, off.data(), ids.data(), &csr));
    // the projection: f32(sum m v / M) in member order, constrained components 0
    const std::vector<float> mass = {1.f, 2.f, 3.f, 5.f, 0.5f, 1.f, 1.f, 0.25f};
    std::vector<float> v(3 * N);
    for (size_t i = 0; i < v.size(); ++i)
        v[i] = 0.1f * (float)(i % 7) - 0.25f;
    const std::vector<float> before = v;
    tie_project(2, off.data(), ids.data(), mass.data(), mask.data(), v.data());
    for (int k = 0; k < 3; ++k)
    {
        const double want0 = ((double)mass[2] * (double)before[6 + k] + (double)mass[3] * (double)before[9 + k]) /
                             ((double)mass[2] + (double)mass[3]);
        CHECK(v[6 + k] == (k == 1 ? 0.f : (float)want0) && v[9 + k] == v[6 + k]);
        const double M = ((double)mass[7] + (double)mass[0]) + (double)mass[4];
        const double want1 = (((double)mass[7] * (double)before[21 + k] + (double)mass[0] * (double)before[k]) +
                              (double)mass[4] * (double)before[12 + k]) / M;
        CHECK(v[21 + k] == (float)want1 && v[k] == v[21 + k] && v[12 + k] == v[21 + k]);
    }
    for (uint32_t n : {1u, 5u, 6u})
        for (int k = 0; k < 3; ++k)
            CHECK(v[3 * n + k] == before[3 * n + k]);
    return 0;
}

template <class T> static std::vector<T> read_list(std::istream &in)
{
    size_t n = 0;
    in >> n;
    std::vector<T> v(n);
    for (T &x : v)
        in >> x;
    return v;
}

template <class T> static void print_list(const char *name, const std::vector<T> &v)
{
    std::cout << name;
    for (const T &x : v)
        std::cout << ' ' << x;
    std::cout << '\n';
}

int main(int argc, char **argv)
{
    if (argc < 2)
    {
        if (self_test())
            return 1;
        std::printf("ok\n");
        return 0;
    }
    std::ifstream in(argv[1]);
    uint64_t N = 0;
    in >> N;
    const auto dash = read_list<uint32_t>(in);
    const auto off = read_list<uint64_t>(in);
    const auto ids = read_list<uint32_t>(in);
    const auto perm = read_list<uint32_t>(in);
    if (!in || off.empty() || perm.size() != N)
        return 2;
    const TieSlots s = tie_slots(N, dash.data(), dash.size(), off.size() - 1, off.data(), ids.data());
    TieCsr csr;
    if (tie_csr(s, to_internal(s, perm), off.size() - 1, off.data(), ids.data(), &csr))
        return 3;
    print_list("slot", s.slot);
    print_list("node", s.node);
    print_list("group", s.group);
    print_list("toff", csr.toff);
    print_list("tnode", csr.tnode);
    return 0;
}
