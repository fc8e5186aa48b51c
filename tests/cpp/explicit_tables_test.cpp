// explicit_tables_test.cpp -- the explicit stepper's two host table builders (csrc/explicit_tables.cpp): the load
// sources' CSR and plasticity's slots with their node-major corner positions, on meshes small enough to state every
// expected entry. No GPU call. Builds against libcwf_hip.so, or stand-alone together with explicit_tables.cpp (then
// also under -fsanitize=address,undefined).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "explicit_tables.hpp"

namespace
{
using U = std::vector<uint32_t>;
using D = std::vector<double>;
int failures = 0;

template <class T> void same(const char *what, const std::vector<T> &got, const std::vector<T> &want)
{
    if (got == want)
        return;
    std::printf("FAIL %s: got", what);
    for (const T &x : got)
        std::printf(" %g", (double)x);
    std::printf(", want");
    for (const T &x : want)
        std::printf(" %g", (double)x);
    std::printf("\n");
    ++failures;
}

void expect(const char *what, bool ok)
{
    if (!ok)
    {
        std::printf("FAIL %s\n", what);
        ++failures;
    }
}

const uint32_t kNone = 0xFFFFFFFFu;

void two_sources_over_five_nodes()
{
    // source 0: one curve point, nodes 4 1 2; source 1: three points, nodes 2 0 3 (node 2 is in both)
    const double t0[] = {0.5}, v0[] = {2.0};
    const double t1[] = {0.0, 1.0, 3.0}, v1[] = {0.0, -1.0, 4.0};
    const uint32_t n0[] = {4, 1, 2}, n1[] = {2, 0, 3};
    const double a0[] = {1, 2, 3, 4, 5, 6, 7, 8, 9}, d0[] = {0.1, 0.2, 0.3};
    const double a1[] = {10, 11, 12, 13, 14, 15, 16, 17, 18}, d1[] = {-0.1, -0.2, -0.3};
    const cwf_explicit_source_desc src[2] = {{1, t0, v0, 3, n0, a0, d0}, {3, t1, v1, 3, n1, a1, d1}};
    // the loaded index in order of first listing: 4 1 2 0 3; the internal order puts them at 2 0 4 1 3
    const U slot = {3, 1, 2, 4, 0}, rank = {2, 0, 4, 1, 3};
    const cwf::SourceTables T = cwf::source_tables(src, 2, slot, rank);
    expect("two sources: totals", T.entries == 6 && T.points == 4);
    same("two sources: off", T.off, U{0, 1, 2, 3, 4, 6});
    // entries by place: l 0 node 1 (s0), l 1 node 0 (s1), l 2 node 4 (s0), l 3 node 3 (s1), l 4 node 2 (s0, then s1)
    same("two sources: dir", T.dir, U{0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3});
    same("two sources: rec", T.rec, D{4, 5, 6, 0.2,  13, 14, 15, -0.2,  1, 2, 3, 0.1,
                                      16, 17, 18, -0.3,  7, 8, 9, 0.3,  10, 11, 12, -0.1});
    same("two sources: tab", T.tab, D{0.5, 2.0, 0.0, 1.0, 3.0, 0.0, -1.0, 4.0});
}

void one_source_of_one_node()
{
    const double t[] = {0.0, 2.0}, v[] = {1.0, 3.0}, a[] = {-1, 0, 1}, d[] = {0.25};
    const uint32_t n[] = {2};
    const cwf_explicit_source_desc src = {2, t, v, 1, n, a, d};
    const cwf::SourceTables T = cwf::source_tables(&src, 1, U{kNone, kNone, 0, kNone}, U{0});
    expect("one source: totals", T.entries == 1 && T.points == 2);
    same("one source: off", T.off, U{0, 1});
    same("one source: dir", T.dir, U{0, 2});
    same("one source: rec", T.rec, D{-1, 0, 1, 0.25});
    same("one source: tab", T.tab, D{0.0, 2.0, 1.0, 3.0});
}

// tet 0 on nodes 0 1 2 3 and tet 1 on nodes 1 2 3 4 (material 0 and 1): the node -> incidence CSR, element << 2 | corner
const U kMat = {0, 1}, kOff = {0, 1, 3, 5, 7, 8}, kInc = {0, 1, 4, 2, 5, 3, 6, 7};

// what must hold of any tables: cpos a permutation of 0 .. 4 slots - 1, each node's run ascending in element, anode
// ascending with no empty run
void well_formed(const char *what, const cwf::PlasticTables &T)
{
    const size_t corners = 4 * T.elem.size();
    U sorted = T.cpos, owner(corners, kNone);
    std::sort(sorted.begin(), sorted.end());
    bool perm = T.cpos.size() == corners;
    for (size_t q = 0; perm && q < corners; ++q)
        perm = sorted[q] == q;
    expect(what, perm);
    if (!perm)
        return;
    for (size_t q = 0; q < corners; ++q)
        owner[T.cpos[q]] = T.elem[q / 4];
    bool ok = T.aoff.size() == T.anode.size() + 1 && T.aoff.front() == 0 && T.aoff.back() == corners &&
              T.incidences == corners;
    for (size_t i = 0; ok && i < T.anode.size(); ++i)
    {
        ok = T.aoff[i] < T.aoff[i + 1] && (i == 0 || T.anode[i - 1] < T.anode[i]);
        for (uint32_t p = T.aoff[i] + 1; ok && p < T.aoff[i + 1]; ++p)
            ok = owner[p - 1] < owner[p];
    }
    expect(what, ok);
}

void two_tets_sharing_a_face()
{
    cwf::PlasticTables T;
    expect("tet 1 plastic: covered", cwf::plastic_tables(kMat, kOff, kInc, {0, 1}, &T) == 0);
    well_formed("tet 1 plastic: well formed", T);
    same("tet 1 plastic: elem", T.elem, U{1});
    same("tet 1 plastic: anode", T.anode, U{1, 2, 3, 4});
    same("tet 1 plastic: aoff", T.aoff, U{0, 1, 2, 3, 4});
    same("tet 1 plastic: cpos", T.cpos, U{0, 1, 2, 3});
    expect("both plastic: covered", cwf::plastic_tables(kMat, kOff, kInc, {1, 1}, &T) == 0);
    well_formed("both plastic: well formed", T);
    same("both plastic: elem", T.elem, U{0, 1});
    same("both plastic: anode", T.anode, U{0, 1, 2, 3, 4});
    same("both plastic: aoff", T.aoff, U{0, 1, 3, 5, 7, 8});
    same("both plastic: cpos", T.cpos, U{0, 1, 3, 5, 2, 4, 6, 7});
}

void a_dropped_corner_is_not_covered()
{
    cwf::PlasticTables T;  // node 4 lost its one incidence (tet 1, corner 3)
    const int st = cwf::plastic_tables(kMat, U{0, 1, 3, 5, 7, 7}, U{0, 1, 4, 2, 5, 3, 6}, {1, 1}, &T);
    expect("dropped corner: refused", st != 0 && T.incidences == 7 && T.cpos.size() == 8);
}

void no_plastic_element_gives_empty_tables()
{
    cwf::PlasticTables T;
    T.elem = {9};
    expect("none plastic: covered", cwf::plastic_tables(kMat, kOff, kInc, {0, 0}, &T) == 0);
    expect("none plastic: empty", T.elem.empty() && T.anode.empty() && T.aoff.empty() && T.cpos.empty());
    // a material index past the flags is elastic too
    expect("unknown material: covered", cwf::plastic_tables(U{7, 7}, kOff, kInc, {1, 1}, &T) == 0 && T.elem.empty());
}
}  // namespace

int main()
{
    two_sources_over_five_nodes();
    one_source_of_one_node();
    two_tets_sharing_a_face();
    a_dropped_corner_is_not_covered();
    no_plastic_element_gives_empty_tables();
    if (failures)
        return 1;
    std::printf("ok\n");
    return 0;
}
