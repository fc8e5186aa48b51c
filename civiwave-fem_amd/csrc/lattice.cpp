// lattice.cpp -- structured-block specialisation of the FAST operator ("structured-block
// specialisation with a single shared K_e").
//
// The reference's operator is the element loop of pcg.cpp:561-662: per tet, f = vol s_K B^T D B u, scattered to
// its 4 corners. On a Kuhn block (every hex cell split into the 6 tets {0,1,3,7} {0,1,5,7} {0,2,3,7} {0,2,6,7}
// {0,4,5,7} {0,4,6,7} of its corner bits (i, j, k)) whose tets of one Kuhn type all carry the same gradients and
// volume, every cell contributes the same 24 x 24 cell stiffness Kc = sum of its 6 K_e (fp64, from the desc's own
// f32 gradients and volumes, the reference's B / D / vol products), and K u = sum over cells of Kc u_cell. Regrouped
// by node pair, an interior node's row is 15 3x3 blocks (the Kuhn edges: +-x, +-y, +-z, +-(1,1,0), +-(1,0,1),
// +-(0,1,1), +-(1,1,1), and the node itself):
//   (K u)_n = sum_d S_d u_(n+d),  S_d = sum over the cell corners c with c + d a corner of Kc[c][c + d].
// The kernel (lattice.hip) forms it in difference form, sum_(d != 0) S_d (u_(n+d) - u_n) (rigid translations
// are in the null space of every row), so each fp32 term is strain-sized as in the element loop. A node on the
// block's surface misses some of its 8 cells: its row is formed in the cell form instead, each existing cell's
// blocks Kc[c][c'] on the same differences. The regrouping changes the fp32 summation order only (FAST's
// tolerance contract, tests/test_lattice.py on the CPU, tests/test_gpu_lattice.py).
//
// detect_lattice() decides it for a desc: integer lattice coordinates of every node (from the first tet's cell
// size), a bijection onto an nx * ny * nz lattice, every tet one Kuhn tet of one cell (each of a cell's 6 types
// exactly once), one material per k-layer of cells, and every tet's gradients / volume within 1e-6 (relative) of the
// first tet of its Kuhn type. With one material in all: the tables above. With several (a layered block, strata): one
// cell stiffness per material, a stencil table per plane class -- the (material below, material above) pair of a node
// plane -- and a cell-pair table per material (layered_tables; at most kLatMaxMaterials materials and
// kLatMaxPlaneClasses classes, else no lattice). Storage order: lexicographic (i fastest) inside each k plane, planes anywhere (a shard's local order:
// owned planes, then its ghost planes; shard.cpp), or, when the handle may renumber, any order (perm).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "abi_internal.hpp"

namespace cwf
{
namespace
{
constexpr int kKuhn[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};

// 6x3 strain-displacement block of one corner (the reference's B rows: xx, yy, zz, xy, yz, zx;
// pcg.cpp:622-630)
void b_block(const double g[3], double B[6][3])
{
    std::memset(B, 0, sizeof(double) * 18);
    B[0][0] = g[0];
    B[1][1] = g[1];
    B[2][2] = g[2];
    B[3][0] = g[1];
    B[3][1] = g[0];
    B[4][1] = g[2];
    B[4][2] = g[1];
    B[5][0] = g[2];
    B[5][2] = g[0];
}
}  // namespace

// kLatPair (cwf_internal.hpp) lists exactly the corner pairs that share a Kuhn tet, in (c, c') order, and
// kLatPairOff names each pair's offset c' - c
bool lattice_tables_ok()
{
    int q = 0;
    for (int c = 0; c < 8; ++c)
        for (int c2 = 0; c2 < 8; ++c2)
        {
            bool edge = c == c2;
            for (int t = 0; t < 6 && !edge; ++t)
            {
                bool a = false, b = false;
                for (int s = 0; s < 4; ++s)
                {
                    a |= kKuhn[t][s] == c;
                    b |= kKuhn[t][s] == c2;
                }
                edge = a && b;
            }
            if (!edge)
                continue;
            if (q >= kLatPairs || kLatPair[q][0] != c || kLatPair[q][1] != c2)
                return false;
            const int o = kLatPairOff[q];
            if (kLatOff[o][0] != (c2 & 1) - (c & 1) || kLatOff[o][1] != ((c2 >> 1) & 1) - ((c >> 1) & 1) ||
                kLatOff[o][2] != ((c2 >> 2) & 1) - ((c >> 2) & 1))
                return false;
            ++q;
        }
    return q == kLatPairs;
}

// storage order: lexicographic inside every k plane (the caller's order: plane[k] = its node (0, 0, k)), or, when
// the handle may renumber, the lexicographic order (perm = at)
bool storage_order(uint64_t N, const uint32_t nn[3], const std::vector<uint32_t> &at, bool allow_perm, Lattice &L)
{
    const uint64_t nx = nn[0], ny = nn[1], nz = nn[2];
    L.nx = (uint32_t)nx;
    L.ny = (uint32_t)ny;
    L.nz = (uint32_t)nz;
    L.plane.assign(nz, 0);
    L.perm.clear();
    bool caller_order = true;
    for (uint64_t k = 0; k < nz && caller_order; ++k)
    {
        const uint32_t base = at[k * nx * ny];
        L.plane[k] = base;
        if ((uint64_t)base + nx * ny > N)
            caller_order = false;
        for (uint64_t j = 0; j < ny && caller_order; ++j)
            for (uint64_t i = 0; i < nx; ++i)
                if (at[(k * ny + j) * nx + i] != base + j * nx + i)
                {
                    caller_order = false;
                    break;
                }
    }
    if (caller_order)
        return true;
    if (!allow_perm)
        return false;
    L.perm = at;
    for (uint64_t k = 0; k < nz; ++k)
        L.plane[k] = (uint32_t)(k * nx * ny);
    return true;
}

// stencil blocks S_d = sum over the corners c with c + d a corner of Kc[c][c + d], then the cell-pair blocks
template <int NOFF, int NPAIR>
void stencil_tables(const double Kc[8][8][3][3], const int (&off)[NOFF][3], const int (&pair)[NPAIR][2], Lattice &L)
{
    double S[NOFF][9] = {};
    double smax = 0.0;
    for (int o = 0; o < NOFF; ++o)
    {
        for (int c = 0; c < 8; ++c)
        {
            const int cx = (c & 1) + off[o][0], cy = ((c >> 1) & 1) + off[o][1], cz = ((c >> 2) & 1) + off[o][2];
            if (cx < 0 || cx > 1 || cy < 0 || cy > 1 || cz < 0 || cz > 1)
                continue;
            const int c2 = cx | cy << 1 | cz << 2;
            for (int r = 0; r < 3; ++r)
                for (int k = 0; k < 3; ++k)
                    S[o][3 * r + k] += Kc[c][c2][r][k];
        }
        for (double v : S[o])
            smax = std::max(smax, std::fabs(v));
    }
    // paired directions: S_(-d) = S_d^T always; S_d symmetric (S_(-d) = S_d) for an isotropic block. The two are
    // summed over the cells in different orders, so they agree to fp64 rounding: within 1e-10 of the largest
    // entry they are taken as equal and both set to their fp64 mean before the f32 rounding
    L.sym = true;
    for (int o = 1; o < NOFF; o += 2)
        for (int j = 0; j < 9; ++j)
            L.sym = L.sym && std::fabs(S[o][j] - S[o + 1][j]) <= 1e-10 * smax;
    if (L.sym)
        for (int o = 1; o < NOFF; o += 2)
            for (int j = 0; j < 9; ++j)
                S[o][j] = S[o + 1][j] = 0.5 * (S[o][j] + S[o + 1][j]);
    for (int o = 0; o < NOFF; ++o)
        for (int j = 0; j < 9; ++j)
            L.coef[9 * o + j] = (float)S[o][j];
    for (int p = 0; p < NPAIR; ++p)
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k)
                L.coef[9 * (NOFF + p) + 3 * r + k] = (float)Kc[pair[p][0]][pair[p][1]][r][k];
}

constexpr int kHexPair[kLatHexPairs][2] = {
#define P8(c) {c, 0}, {c, 1}, {c, 2}, {c, 3}, {c, 4}, {c, 5}, {c, 6}, {c, 7}
    P8(0), P8(1), P8(2), P8(3), P8(4), P8(5), P8(6), P8(7)
#undef P8
};

// Material slots of the cell layers (by first appearance along k) and the plane classes of the node planes: one
// class per (slot below, slot above) pair that occurs; the end planes, which have one layer, take it twice (all
// their nodes are shell nodes: the class only has to exist). lay[kc]: the desc's material of cell layer kc.
bool layer_classes(const std::vector<uint32_t> &lay, Lattice &L, const char **why)
{
    const uint32_t nl = (uint32_t)lay.size();
    L.layer_mat.assign(nl, 0);
    L.mat_id.clear();
    for (uint32_t kc = 0; kc < nl; ++kc)
    {
        uint32_t s = 0;
        while (s < L.mat_id.size() && L.mat_id[s] != lay[kc])
            ++s;
        if (s == L.mat_id.size())
            L.mat_id.push_back(lay[kc]);
        L.layer_mat[kc] = s;
    }
    if (L.mat_id.size() > kLatMaxMaterials)
    {
        *why = "layered block with more than 8 materials";
        return false;
    }
    L.plane_cls.assign(nl + 1, 0);
    L.cls_pair.clear();
    for (uint32_t k = 0; k <= nl; ++k)
    {
        const uint32_t below = L.layer_mat[k ? k - 1 : 0], above = L.layer_mat[k < nl ? k : nl - 1];
        uint32_t c = 0;
        while (2 * c < L.cls_pair.size() && (L.cls_pair[2 * c] != below || L.cls_pair[2 * c + 1] != above))
            ++c;
        if (2 * c == L.cls_pair.size())
        {
            L.cls_pair.push_back(below);
            L.cls_pair.push_back(above);
        }
        L.plane_cls[k] = c;
    }
    if (L.cls_pair.size() / 2 > kLatMaxPlaneClasses)
    {
        *why = "layered block with more than 16 plane classes";
        return false;
    }
    L.layered = L.mat_id.size() > 1;
    return true;
}

// one material: the layered description repeats the block's own tables (one slot, one class)
template <int NOFF, int NPAIR>
void single_material_tables(Lattice &L)
{
    L.cls_coef.assign(L.coef, L.coef + 9 * NOFF);
    L.mat_coef.assign(L.coef + 9 * NOFF, L.coef + 9 * (NOFF + NPAIR));
}

// Layered block: per plane class (below, above) the stencil blocks S_d = sum over the node's corner positions c
// with c + d a corner of Kc^m[c][c + d], m the material of the cell the node sits in at corner c: the cell below
// the node's plane when c's z-bit is 1, the cell above when it is 0. fp64 over both halves, rounded to f32 once.
// S_(-d) = S_d holds only between equal layers (on an interface plane the two differ by 57-88% of the largest
// entry for the strata of tests/test_lattice_layered.py), so no class is paired (sym off).
// Per material slot, the cell-pair blocks for the surface shell.
template <int NOFF, int NPAIR>
void layered_tables(const std::vector<double> &Kc, const int (&off)[NOFF][3], const int (&pair)[NPAIR][2], Lattice &L)
{
    const auto kc = [&](uint32_t m, int a, int b, int r, int k) { return Kc[(((size_t)m * 8 + a) * 8 + b) * 9 + 3 * r + k]; };
    const size_t ncls = L.cls_pair.size() / 2, nmat = L.mat_id.size();
    L.cls_coef.assign(ncls * 9 * NOFF, 0.f);
    for (size_t cl = 0; cl < ncls; ++cl)
        for (int o = 0; o < NOFF; ++o)
        {
            double S[9] = {};
            for (int c = 0; c < 8; ++c)
            {
                const int cx = (c & 1) + off[o][0], cy = ((c >> 1) & 1) + off[o][1], cz = ((c >> 2) & 1) + off[o][2];
                if (cx < 0 || cx > 1 || cy < 0 || cy > 1 || cz < 0 || cz > 1)
                    continue;
                const int c2 = cx | cy << 1 | cz << 2;
                const uint32_t m = L.cls_pair[2 * cl + ((c >> 2) & 1 ? 0 : 1)];
                for (int r = 0; r < 3; ++r)
                    for (int k = 0; k < 3; ++k)
                        S[3 * r + k] += kc(m, c, c2, r, k);
            }
            for (int j = 0; j < 9; ++j)
                L.cls_coef[(cl * NOFF + o) * 9 + j] = (float)S[j];
        }
    L.mat_coef.assign(nmat * 9 * NPAIR, 0.f);
    for (size_t m = 0; m < nmat; ++m)
        for (int p = 0; p < NPAIR; ++p)
            for (int r = 0; r < 3; ++r)
                for (int k = 0; k < 3; ++k)
                    L.mat_coef[(m * NPAIR + p) * 9 + 3 * r + k] = (float)kc((uint32_t)m, pair[p][0], pair[p][1], r, k);
    L.sym = false;
    std::memset(L.coef, 0, sizeof L.coef);
}

// trilinear hex cell stiffness, 2 x 2 x 2 Gauss in fp64, from the cell's corner coordinates by corner bits
bool hex_cell_stiffness(const double Xc[8][3], const double *D, double Kc[8][8][3][3])
{
    std::memset(Kc, 0, sizeof(double) * 8 * 8 * 9);
    const double gq = 1.0 / std::sqrt(3.0);
    for (int gp = 0; gp < 8; ++gp)
    {
        const double qp[3] = {(gp & 1) ? gq : -gq, (gp & 2) ? gq : -gq, (gp & 4) ? gq : -gq};
        double dN[8][3], J[3][3] = {};
        for (int a = 0; a < 8; ++a)
        {
            const double sg[3] = {(a & 1) ? 1.0 : -1.0, (a & 2) ? 1.0 : -1.0, (a & 4) ? 1.0 : -1.0};
            const double f[3] = {1.0 + sg[0] * qp[0], 1.0 + sg[1] * qp[1], 1.0 + sg[2] * qp[2]};
            dN[a][0] = 0.125 * sg[0] * f[1] * f[2];
            dN[a][1] = 0.125 * f[0] * sg[1] * f[2];
            dN[a][2] = 0.125 * f[0] * f[1] * sg[2];
            for (int m = 0; m < 3; ++m)
                for (int l = 0; l < 3; ++l)
                    J[m][l] += Xc[a][m] * dN[a][l];
        }
        double A[3][3];  // adjugate
        A[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
        A[0][1] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
        A[0][2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
        A[1][0] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
        A[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
        A[1][2] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
        A[2][0] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        A[2][1] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
        A[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        const double det = J[0][0] * A[0][0] + J[0][1] * A[1][0] + J[0][2] * A[2][0];
        if (!(std::fabs(det) > 0.0))
            return false;
        double g[8][3];
        for (int a = 0; a < 8; ++a)
            for (int m = 0; m < 3; ++m)
            {
                double sum = 0.0;
                for (int l = 0; l < 3; ++l)
                    sum += dN[a][l] * A[l][m];
                g[a][m] = sum / det;
            }
        for (int a = 0; a < 8; ++a)
            for (int b = 0; b < 8; ++b)
            {
                double Ba[6][3], Bb[6][3];
                b_block(g[a], Ba);
                b_block(g[b], Bb);
                for (int r = 0; r < 3; ++r)
                    for (int k = 0; k < 3; ++k)
                    {
                        double sum = 0.0;
                        for (int i = 0; i < 6; ++i)
                            for (int j = 0; j < 6; ++j)
                                sum += Ba[i][r] * D[6 * i + j] * Bb[j][k];
                        Kc[a][b][r][k] += std::fabs(det) * sum;
                    }
            }
    }
    return true;
}

// Kuhn cell stiffness Kc[c][c'] = sum over the cell's tets of vol B_c^T D B_c' (fp64, pcg.cpp:622-651 products)
void kuhn_cell_stiffness(const double G[6][8][3], const double V[6], const double *D, double Kc[8][8][3][3])
{
    std::memset(Kc, 0, sizeof(double) * 8 * 8 * 9);
    for (int t = 0; t < 6; ++t)
        for (int sa = 0; sa < 4; ++sa)
            for (int sb = 0; sb < 4; ++sb)
            {
                const int a = kKuhn[t][sa], b = kKuhn[t][sb];
                double Ba[6][3], Bb[6][3];
                b_block(G[t][a], Ba);
                b_block(G[t][b], Bb);
                for (int r = 0; r < 3; ++r)
                    for (int k = 0; k < 3; ++k)
                    {
                        double sum = 0.0;
                        for (int i = 0; i < 6; ++i)
                            for (int j = 0; j < 6; ++j)
                                sum += Ba[i][r] * D[6 * i + j] * Bb[j][k];
                        Kc[a][b][r][k] += V[t] * sum;
                    }
            }
}

// the material of each cell layer from the elements' (cell layer, material) pairs; false when a layer holds two
struct LayerMaterials
{
    std::vector<uint32_t> lay;
    explicit LayerMaterials(uint64_t layers) : lay(layers, 0xFFFFFFFFu) {}
    bool add(uint32_t kc, uint32_t m)
    {
        if (lay[kc] == 0xFFFFFFFFu)
            lay[kc] = m;
        return lay[kc] == m;
    }
};

// native hex8 cells (Gmsh / VTK corner order; slot s sits at corner bits kHexSlotBits[s]): one hex per cell, the
// cell stiffness from the first hex's corner coordinates (the lattice's, to 1e-6 of the cell: every cell is a
// translate), 2 x 2 x 2 Gauss in fp64 (the textbook element of oracle/hex8_oracle.c and k_keff_hex_tiles)
bool detect_hex_cells(const cwf_system_desc *d, const std::vector<uint32_t> &q, const uint32_t nn[3],
                      const std::vector<uint32_t> &at, bool allow_perm, Lattice &L, std::string *why)
{
    const auto fail = [&](const char *m) {
        if (why)
            *why = m;
        return false;
    };
    constexpr int kHexSlotBits[8] = {0, 1, 3, 2, 4, 5, 7, 6};
    const uint64_t N = d->node_count, E = d->element_count, nx = nn[0], ny = nn[1], nz = nn[2];
    if (E != (nx - 1) * (ny - 1) * (nz - 1))
        return fail("element count is not one hex per cell");
    const uint32_t *conn = d->element_connectivity;
    std::vector<uint8_t> seen(E, 0);
    LayerMaterials lm(nz - 1);
    for (uint64_t e = 0; e < E; ++e)
    {
        const uint32_t *c = &q[3ull * conn[8 * e]];  // slot 0 is the cell's corner (0, 0, 0)
        if (c[0] >= nx - 1 || c[1] >= ny - 1 || c[2] >= nz - 1)
            return fail("a hex is not a cell");
        if (!lm.add(c[2], d->element_material_index[e]))
            return fail("materials vary inside a cell layer");
        for (int s = 1; s < 8; ++s)
        {
            const uint32_t *qs = &q[3ull * conn[8 * e + s]];
            const uint32_t ox = qs[0] - c[0], oy = qs[1] - c[1], oz = qs[2] - c[2];
            if (ox > 1 || oy > 1 || oz > 1 || (int)(ox | oy << 1 | oz << 2) != kHexSlotBits[s])
                return fail("a hex is not a cell in Gmsh corner order");
        }
        const uint64_t cell = ((uint64_t)c[2] * (ny - 1) + c[1]) * (nx - 1) + c[0];
        if (seen[cell])
            return fail("two hexes on one cell");
        seen[cell] = 1;
    }
    if (!storage_order(N, nn, at, allow_perm, L))
        return fail("node order is not lexicographic within planes");
    double Xc[8][3];  // corner coordinates of the first hex by corner bits
    for (int s = 0; s < 8; ++s)
        for (int k = 0; k < 3; ++k)
            Xc[kHexSlotBits[s]][k] = d->node_coords[3ull * conn[s] + k];
    L.hex = true;
    const char *cwhy = nullptr;
    if (!layer_classes(lm.lay, L, &cwhy))
        return fail(cwhy);
    if (!L.layered)  // one material: today's tables
    {
        const double *D = d->material_stiffness + 36ull * d->element_material_index[0];
        double Kc[8][8][3][3];
        if (!hex_cell_stiffness(Xc, D, Kc))
            return fail("degenerate hex");
        stencil_tables(Kc, kLatHexOff, kHexPair, L);
        single_material_tables<kLatHexOffsets, kLatHexPairs>(L);
        return true;
    }
    std::vector<double> Km(L.mat_id.size() * 576);
    for (size_t m = 0; m < L.mat_id.size(); ++m)
        if (!hex_cell_stiffness(Xc, d->material_stiffness + 36ull * L.mat_id[m],
                                *reinterpret_cast<double(*)[8][8][3][3]>(&Km[576 * m])))
            return fail("degenerate hex");
    layered_tables(Km, kLatHexOff, kHexPair, L);
    return true;
}

bool detect_lattice(const cwf_system_desc *d, bool allow_perm, Lattice &L, std::string *why)
{
    const auto fail = [&](const char *m) {
        if (why)
            *why = m;
        return false;
    };
    const uint64_t N = d->node_count, E = d->element_count;
    static const bool tables_ok = lattice_tables_ok();
    if (!tables_ok)
        return fail("lattice tables inconsistent");
    if (!E || N < 8 || !d->node_coords)
        return fail("no elements or no node coordinates");
    const bool hex = d->element_connectivity[4] != 0xFFFFFFFFu;
    const int K = hex ? 8 : 4;
    const uint32_t *conn = d->element_connectivity;
    const double *X = d->node_coords;
    // cell size from the first element (a Kuhn tet spans its whole cell: it holds corners 0 and 7)
    double h[3], lo[3];
    for (int k = 0; k < 3; ++k)
    {
        double a = X[3ull * conn[0] + k], b = a;
        for (int s = 1; s < K; ++s)
        {
            a = std::min(a, X[3ull * conn[s] + k]);
            b = std::max(b, X[3ull * conn[s] + k]);
        }
        h[k] = b - a;
        if (!(h[k] > 0.0))
            return fail("degenerate first element");
        lo[k] = X[k];
    }
    for (uint64_t n = 1; n < N; ++n)
        for (int k = 0; k < 3; ++k)
            lo[k] = std::min(lo[k], X[3 * n + k]);
    std::vector<uint32_t> q(3 * N);
    uint32_t nn[3] = {0, 0, 0};
    for (uint64_t n = 0; n < N; ++n)
        for (int k = 0; k < 3; ++k)
        {
            // tets: the element records define the operator (checked below), so coordinates only place the nodes;
            // hex8: the operator is formed from the coordinates, so they must be the lattice's
            const double f = (X[3 * n + k] - lo[k]) / h[k];
            const double r = std::nearbyint(f);
            if (!(std::fabs(f - r) <= (hex ? 1e-6 : 1e-3)) || r >= 1048576.0)
                return fail("nodes off the lattice");
            q[3 * n + k] = (uint32_t)r;
            nn[k] = std::max(nn[k], (uint32_t)r + 1u);
        }
    if (nn[0] < 2 || nn[1] < 2 || nn[2] < 2 || (uint64_t)nn[0] * nn[1] * nn[2] != N)
        return fail("nodes do not fill a box lattice");
    const uint64_t nx = nn[0], ny = nn[1], nz = nn[2];
    std::vector<uint32_t> at(N, 0xFFFFFFFFu);  // lexicographic lattice index -> node
    for (uint64_t n = 0; n < N; ++n)
    {
        const uint64_t li = ((uint64_t)q[3 * n + 2] * ny + q[3 * n + 1]) * nx + q[3 * n];
        if (at[li] != 0xFFFFFFFFu)
            return fail("two nodes on one lattice point");
        at[li] = (uint32_t)n;
    }
    const uint64_t C = (nx - 1) * (ny - 1) * (nz - 1);
    if (hex)
        return detect_hex_cells(d, q, nn, at, allow_perm, L, why);
    if (E != 6 * C)
        return fail("element count is not 6 per cell");
    // every tet a Kuhn tet of one cell, each of a cell's 6 types once; gradients / volume per type
    int type_of[256];
    std::fill(type_of, type_of + 256, -1);
    for (int t = 0; t < 6; ++t)
    {
        int m = 0;
        for (int s = 0; s < 4; ++s)
            m |= 1 << kKuhn[t][s];
        type_of[m] = t;
    }
    std::vector<uint8_t> seen(C, 0);
    LayerMaterials lm(nz - 1);
    double G[6][8][3];
    double V[6], gmax[6];
    bool have[6] = {false, false, false, false, false, false};
    const float *grad = d->element_gradients;
    for (uint64_t e = 0; e < E; ++e)
    {
        uint32_t c[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        for (int s = 0; s < 4; ++s)
            for (int k = 0; k < 3; ++k)
                c[k] = std::min(c[k], q[3ull * conn[8 * e + s] + k]);
        int bits[4], m = 0;
        for (int s = 0; s < 4; ++s)
        {
            const uint32_t *qs = &q[3ull * conn[8 * e + s]];
            const uint32_t ox = qs[0] - c[0], oy = qs[1] - c[1], oz = qs[2] - c[2];
            if (ox > 1 || oy > 1 || oz > 1)
                return fail("an element spans more than one cell");
            bits[s] = (int)(ox | oy << 1 | oz << 2);
            m |= 1 << bits[s];
        }
        const int t = type_of[m];
        if (t < 0 || c[0] >= nx - 1 || c[1] >= ny - 1 || c[2] >= nz - 1)
            return fail("an element is not a Kuhn tet of a cell");
        if (!lm.add(c[2], d->element_material_index[e]))
            return fail("materials vary inside a cell layer");
        const uint64_t cell = ((uint64_t)c[2] * (ny - 1) + c[1]) * (nx - 1) + c[0];
        if (seen[cell] & (1u << t))
            return fail("a cell holds one Kuhn type twice");
        seen[cell] |= (uint8_t)(1u << t);
        const float *g = grad + 24 * e;
        const double vol = d->element_volume[e];
        if (!have[t])
        {
            have[t] = true;
            V[t] = vol;
            gmax[t] = 0.0;
            for (int s = 0; s < 4; ++s)
                for (int k = 0; k < 3; ++k)
                {
                    G[t][bits[s]][k] = g[3 * s + k];
                    gmax[t] = std::max(gmax[t], std::fabs((double)g[3 * s + k]));
                }
            if (!(V[t] > 0.0) || !(gmax[t] > 0.0))
                return fail("degenerate element");
            continue;
        }
        if (!(std::fabs(vol - V[t]) <= 1e-6 * V[t]))
            return fail("element volumes differ within a Kuhn type");
        for (int s = 0; s < 4; ++s)
            for (int k = 0; k < 3; ++k)
                if (!(std::fabs((double)g[3 * s + k] - G[t][bits[s]][k]) <= 1e-6 * gmax[t]))
                    return fail("element gradients differ within a Kuhn type");
    }
    if (!storage_order(N, nn, at, allow_perm, L))
        return fail("node order is not lexicographic within planes");
    L.hex = false;
    const char *cwhy = nullptr;
    if (!layer_classes(lm.lay, L, &cwhy))
        return fail(cwhy);
    // every block outside the Kuhn pattern is structurally zero (never accumulated): nothing to check
    if (!L.layered)  // one material: today's tables
    {
        double Kc[8][8][3][3];
        kuhn_cell_stiffness(G, V, d->material_stiffness + 36ull * d->element_material_index[0], Kc);
        stencil_tables(Kc, kLatOff, kLatPair, L);
        single_material_tables<kLatOffsets, kLatPairs>(L);
        return true;
    }
    std::vector<double> Km(L.mat_id.size() * 576);
    for (size_t m = 0; m < L.mat_id.size(); ++m)
        kuhn_cell_stiffness(G, V, d->material_stiffness + 36ull * L.mat_id[m],
                            *reinterpret_cast<double(*)[8][8][3][3]>(&Km[576 * m]));
    layered_tables(Km, kLatOff, kLatPair, L);
    return true;
}

// Work items: the surface shell of the computed planes [lk0, lk1), one node per thread (256-thread workgroups,
// rounded up to whole XCD groups so the bricks after them keep the XCD mapping), then 32 x 8 column bricks of the
// strict interior times L planes. L = 6 while the brick columns are fewer than one round of resident workgroups
// (1024: four per CU), else one column's planes per brick (about kLatTargetItems bricks). Measured (PCG it/s, same
// box, two passes, k_keff_lattice with the uniform mass): C2 (27 columns) L = 3 / 4 / 5 / 6 / 7 / 8: 40.2k / 40.1k
// / 41.6k / 41.6k / 39.3k / 39.5k; C3 (95 columns) L = 5 / 6 / 7 / 8 / 9 / 11 / 14 / 20 / 28: 58.8-60.9 / 54.3-57.9
// / 56.4-61.0 / 54.0-58.0 / 55.1-55.9 / 56.0-59.8 / 55.4-59.9 / 60.1-62.4 / 67.0-69.0 us; C3 hex8 L = 6 / 12 /
// 14 / 24: 65.4 / 66.6 / 68.0 / 75.4 us; C5 (1250 columns) L = 6 / 12 / 24 / 48 (all): 252 / 242 / 267 / 224 us
void lattice_plan(DevTiles &t)
{
    constexpr uint64_t kLatTargetItems = 262144 / kLatThreads;  // 1024 bricks of 256 threads
    const uint64_t nx = t.lnx, ny = t.lny, nz = t.lnz;
    const uint64_t k0 = t.lk0, k1 = std::max(t.lk1, t.lk0);
    t.lkI0 = (uint32_t)std::max<uint64_t>(k0, 1);
    t.lkI1 = (uint32_t)std::max<uint64_t>(std::min<uint64_t>(k1, nz - 1), t.lkI0);
    uint64_t shell = 0;
    if (k0 == 0 && k1 > 0)
        shell += nx * ny;
    if (k1 == nz && nz > 1 && k1 > k0)
        shell += nx * ny;
    shell += (uint64_t)(t.lkI1 - t.lkI0) * (2 * nx + 2 * (ny - 2));
    t.lnshell = (uint32_t)shell;
    t.lnsb = (uint32_t)(((shell + kLatThreads - 1) / kLatThreads + 7) / 8 * 8);
    t.lnbx = (uint32_t)((nx - 2 + kLatBrickX - 1) / kLatBrickX);
    t.lnby = (uint32_t)((ny - 2 + kLatBrickY - 1) / kLatBrickY);
    const uint64_t planes = t.lkI1 - t.lkI0, cols = (uint64_t)t.lnbx * t.lnby;
    uint64_t L = cols < kLatTargetItems ? 6 : (planes * cols + kLatTargetItems - 1) / kLatTargetItems;
    const char *lk = knob("CWF_LAT_L");
    if (lk && atoi(lk) > 0)
        L = (uint64_t)atoi(lk);
    L = std::max<uint64_t>(lk && atoi(lk) > 0 ? 2 : 4, std::min<uint64_t>(L, 64));
    t.lL = (uint32_t)L;
    t.lnwm = (uint32_t)(cols * ((planes + L - 1) / L));
    t.lnwork = t.lnsb + t.lnwm;
    // the shell workgroups lead the bricks when the grid takes several rounds of resident workgroups (C3: 2.8
    // rounds, shell last -2.6%) and follow them when it fits in one (C2: 436 workgroups, shell last +6.2%, keff 14.2
    // -> 12.9 us; same box, two passes)
    // several rounds of many k-chunks: each chunk's perimeter workgroups right after its bricks (C3 +0.5-1.4%, C3
    // hex8 +1.5% over the shell first, same box: the perimeter gathers find the chunk's lines in the XCD's L2;
    // profiles/r04w_*). Not with few chunks: each XCD takes a contiguous share of the items, so C5's one chunk put
    // its 1,250 whole-column bricks on three XCDs and the end planes on the rest (K_eff 241 -> 476 us, r04z)
    const uint64_t nchunks = (planes + L - 1) / L;
    t.lshl = t.lnwork <= kLatTargetItems ? 1 : nchunks >= 16 ? 2 : 0;
    t.lnsc = 0;
    if (t.lshl == 2)  // interleaved: per k-chunk its bricks, then the perimeters of its planes; the end planes last
    {
        const uint64_t per = 2 * nx + 2 * (ny - 2), nchunk = (planes + L - 1) / L;
        const uint64_t nlo = (k0 == 0 && k1 > 0) ? nx * ny : 0, nhi = (k1 == nz && nz > 1 && k1 > k0) ? nx * ny : 0;
        t.lnsc = (uint32_t)((L * per + kLatThreads - 1) / kLatThreads);
        t.lnwork = (uint32_t)(nchunk * (cols + t.lnsc) + (nlo + kLatThreads - 1) / kLatThreads +
                              (nhi + kLatThreads - 1) / kLatThreads);
    }
    t.ntiles = t.lnwork;
}

// The device copy's stencil blocks are stored row-pair interleaved for the packed rows of k_keff_lattice: per
// offset {S00 S10 S01 S11 S02 S12 S20 S21 S22}; the cell-pair blocks after them keep row-major order
// A layered block's copy: one such slice of stencil blocks per plane class, then the cell-pair blocks of every
// material slot, then one word per node plane (its bits in a float): the plane's class | the material slot of the
// cell layer above it << 16 (k_keff_lattice_layered; DevTiles::llayers)
std::vector<float> lattice_device_coef(const Lattice &lat)
{
    const int noff = lat.hex ? kLatHexOffsets : kLatOffsets;
    std::vector<float> cdev;
    if (lat.layered)
    {
        cdev = lat.cls_coef;
        cdev.insert(cdev.end(), lat.mat_coef.begin(), lat.mat_coef.end());
    }
    else
        cdev.assign(lat.coef, lat.coef + (lat.hex ? kLatHexCoef : kLatCoef));
    const std::vector<float> src = cdev;
    for (size_t o = 0; o < (lat.layered ? lat.cls_pair.size() / 2 : 1) * noff; ++o)
        for (int c = 0; c < 3; ++c)
        {
            cdev[9 * o + 2 * c] = src[9 * o + c];
            cdev[9 * o + 2 * c + 1] = src[9 * o + 3 + c];
            cdev[9 * o + 6 + c] = src[9 * o + 6 + c];
        }
    for (uint32_t k = 0; lat.layered && k < lat.nz; ++k)
    {
        const uint32_t w = lat.plane_cls[k] | lat.layer_mat[std::min(k, lat.nz - 2)] << 16;
        float f;
        std::memcpy(&f, &w, sizeof f);
        cdev.push_back(f);
    }
    return cdev;
}

// Per-class preconditioner (the update pass reads one byte per node instead of the 16-B record and the
// partial-run bounds) when the lumped mass is a function of the boundary type
LatticeClasses lattice_classes(const Lattice &lat, const uint32_t *bc_mask, const float *lumped_mass)
{
    LatticeClasses lc;
    lc.cls.resize((size_t)lat.nx * lat.ny * lat.nz);
    lc.rep.assign(kLatClasses, 0xFFFFFFFFu);
    float tmass[27] = {};
    bool tseen[27] = {};
    for (uint32_t k = 0; k < lat.nz && lc.uniform; ++k)
        for (uint32_t j = 0; j < lat.ny; ++j)
            for (uint32_t i = 0; i < lat.nx; ++i)
            {
                const uint32_t n = lat.plane[k] + j * lat.nx + i;
                const auto side = [](uint32_t a, uint32_t na) { return a == 0 ? 0u : a + 1 == na ? 2u : 1u; };
                const uint32_t ty = side(i, lat.nx) + 3 * side(j, lat.ny) + 9 * side(k, lat.nz);
                const uint32_t c = ty << 3 | (bc_mask[n] & 7u);
                lc.cls[n] = (uint8_t)c;
                if (lc.rep[c] == 0xFFFFFFFFu || n < lc.rep[c])
                    lc.rep[c] = n;
                if (!tseen[ty])
                {
                    tseen[ty] = true;
                    tmass[ty] = lumped_mass[n];
                }
                else if (std::memcmp(&tmass[ty], &lumped_mass[n], sizeof(float)) != 0)
                    lc.uniform = false;
            }
    lc.interior = tseen[13];  // type 13: inside along x, y and z (the bricks' nodes)
    lc.interior_mass = tmass[13];
    return lc;
}

}  // namespace cwf

extern "C" int cwf_lattice_describe(const cwf_system_desc *desc, int renumber, uint32_t dims[3], float *coef,
                                    uint32_t *plane)
{
    static_assert(cwf::kLatCoef == CWF_LATTICE_COEFS, "cwf_hip.h CWF_LATTICE_COEFS");
    if (!desc || !dims || !coef || !desc->element_connectivity || !desc->element_gradients || !desc->element_volume ||
        !desc->element_material_index || !desc->material_stiffness)
        return CWF_ERR_ARGUMENT;
    // tet4 blocks (the reference's element; native hex8 blocks run the 27-point instantiation and are not described)
    if (desc->mode != CWF_MODE_FAST || desc->node_count >= 0x15555555ull || !desc->element_count ||
        desc->element_connectivity[4] != 0xFFFFFFFFu)
        return 0;
    for (uint64_t e = 0; e < desc->element_count; ++e)
    {
        if (desc->element_material_index[e] >= desc->material_count)
            return CWF_ERR_MATERIAL_RANGE;
        for (int a = 0; a < 4; ++a)
            if (desc->element_connectivity[8 * e + a] >= desc->node_count)
                return CWF_ERR_NODE_RANGE;
    }
    cwf::Lattice L;
    if (!cwf::detect_lattice(desc, renumber != 0, L) || L.layered)  // layered: cwf_lattice_describe_layers
        return 0;
    dims[0] = L.nx;
    dims[1] = L.ny;
    dims[2] = L.nz;
    std::memcpy(coef, L.coef, sizeof(float) * cwf::kLatCoef);
    dims[0] |= L.sym ? 0x80000000u : 0u;
    if (plane)
        std::memcpy(plane, L.plane.data(), L.plane.size() * sizeof(uint32_t));
    return 1;
}

extern "C" int cwf_lattice_describe_layers(const cwf_system_desc *desc, int renumber, uint32_t dims[3], uint32_t info[4],
                                           uint32_t plane_capacity, uint32_t *plane, uint32_t *plane_class,
                                           uint32_t *layer_material, uint32_t class_capacity, uint32_t *class_pair,
                                           float *class_coef, uint32_t material_capacity, uint32_t *material_ids,
                                           float *pair_coef)
{
    static_assert(cwf::kLatMaxMaterials == CWF_LATTICE_MAX_MATERIALS, "cwf_hip.h CWF_LATTICE_MAX_MATERIALS");
    static_assert(cwf::kLatMaxPlaneClasses == CWF_LATTICE_MAX_PLANE_CLASSES, "cwf_hip.h CWF_LATTICE_MAX_PLANE_CLASSES");
    if (!desc || !dims || !info || !desc->element_connectivity || !desc->element_gradients || !desc->element_volume ||
        !desc->element_material_index || !desc->material_stiffness)
        return CWF_ERR_ARGUMENT;
    if (desc->mode != CWF_MODE_FAST || desc->node_count >= 0x15555555ull || !desc->element_count)
        return 0;
    const bool hex = desc->element_connectivity[4] != 0xFFFFFFFFu;
    for (uint64_t e = 0; e < desc->element_count; ++e)
    {
        if (desc->element_material_index[e] >= desc->material_count)
            return CWF_ERR_MATERIAL_RANGE;
        if ((desc->element_connectivity[8 * e + 4] != 0xFFFFFFFFu) != hex)
            return 0;
        for (int a = 0; a < (hex ? 8 : 4); ++a)
            if (desc->element_connectivity[8 * e + a] >= desc->node_count)
                return CWF_ERR_NODE_RANGE;
    }
    cwf::Lattice L;
    if (!cwf::detect_lattice(desc, renumber != 0, L))
        return 0;
    const uint32_t nmat = (uint32_t)L.mat_id.size(), ncls = (uint32_t)(L.cls_pair.size() / 2);
    const size_t noff = L.hex ? cwf::kLatHexOffsets : cwf::kLatOffsets, npair = L.hex ? cwf::kLatHexPairs : cwf::kLatPairs;
    dims[0] = L.nx;
    dims[1] = L.ny;
    dims[2] = L.nz;
    info[0] = nmat;
    info[1] = ncls;
    info[2] = L.hex ? 1u : 0u;
    info[3] = L.sym ? 1u : 0u;
    if (((plane || plane_class || layer_material) && plane_capacity < L.nz) ||
        ((class_pair || class_coef) && class_capacity < ncls) || ((material_ids || pair_coef) && material_capacity < nmat))
        return CWF_ERR_SIZE;
    if (plane)
        std::memcpy(plane, L.plane.data(), L.nz * sizeof(uint32_t));
    if (plane_class)
        std::memcpy(plane_class, L.plane_cls.data(), L.nz * sizeof(uint32_t));
    if (layer_material)
        for (uint32_t kc = 0; kc + 1 < L.nz; ++kc)
            layer_material[kc] = L.mat_id[L.layer_mat[kc]];
    if (class_pair)
        for (uint32_t i = 0; i < 2 * ncls; ++i)
            class_pair[i] = L.mat_id[L.cls_pair[i]];
    if (class_coef)
        std::memcpy(class_coef, L.cls_coef.data(), ncls * 9 * noff * sizeof(float));
    if (material_ids)
        std::memcpy(material_ids, L.mat_id.data(), nmat * sizeof(uint32_t));
    if (pair_coef)
        std::memcpy(pair_coef, L.mat_coef.data(), nmat * 9 * npair * sizeof(float));
    return 1;
}
