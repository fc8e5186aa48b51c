// abi.cpp -- C-ABI (include/cwf_hip.h) over the gfx950 kernels: handle lifetime, mode / scalar / timing switches
// and the measurement entry points. One HIP stream per handle. The PCG entry points are in abi_pcg.cpp, the
// Stepper in abi_stepper.cpp, the communicators in comm.cpp and peer.hip.
// cwf_hip_system_create is a sequence of stages: validate_desc, find_lattice, choose_fast_path (the one place
// that decides the FAST layout), renumber_desc, open_handle, upload_mesh_arrays, upload_incidence, one of
// layout_lattice / layout_groups / layout_tiles, upload_hex_jacobi, alloc_scratch. A guard (HandlePtr) holds the
// handle and one catch takes host allocation failures, so every failing exit frees what was allocated.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "blockinv_pack.hpp"
#include "cwf_internal.hpp"

namespace cwf
{

static thread_local std::string g_err, g_ctx;

int set_error(cwf_hip_system *h, int code, const std::string &msg, const std::string &ctx)
{
    if (h)
    {
        h->err = msg;
        h->ctx = ctx;
    }
    g_err = msg;
    g_ctx = ctx;
    return code;
}

int hip_fail(cwf_hip_system *h, hipError_t e, const char *what)
{
    return set_error(h, CWF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e), hipGetErrorName(e));
}

}  // namespace cwf

cwf_hip_system::~cwf_hip_system() = default;  // here, not in the header: cwf_internal.hpp

using namespace cwf;

#include "abi_internal.hpp"

namespace cwf
{

bool iso_pattern(const double *D)
{
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c)
        {
            const bool nz = (r < 3 && c < 3) || (r == c);
            if (!nz && D[6 * r + c] != 0.0)
                return false;
        }
    return true;
}

// Built on first use (a PARITY create or set_mode(PARITY)), from the node -> incidence CSR already on the device:
// the node tiles of k_keff_parity_tile. Tile b holds nodes [256 b, 256 b + 256) (three whole 256-DOF reduction
// chunks, so the p.Ap chunk partials stay fused), its incident tets in ascending element order, and for each of its
// nodes' incidences the tet's index in that list. FAST handles never build it.
// above this many tets the host-side breadth-first pass (random reads of 16 B of connectivity per incidence) takes
// tens of seconds: strips there (C5's 96M tets)
constexpr uint64_t kParityCompactMaxTets = 1ull << 25;

// Compact PARITY tiles: greedy breadth-first blobs of <= 256 nodes over the node graph (two nodes adjacent when
// they share a tet), seeded in node order. On C2 the strip tiles (256 consecutive nodes of the caller's
// lexicographic order, one plane thick) evaluate each tet ~2.4 times; blobs fewer.
std::vector<uint32_t> parity_compact_tiles(const std::vector<uint32_t> &off, const std::vector<uint32_t> &inc,
                                           const std::vector<uint32_t> &conn, uint64_t N)
{
    std::vector<uint32_t> nodes;
    nodes.reserve(N + N / 4);
    std::vector<uint8_t> state(N, 0);  // 0 free, 1 queued for the current tile, 2 placed
    std::vector<uint32_t> queue;
    queue.reserve(4096);
    for (uint64_t seed = 0; seed < N; ++seed)
    {
        if (state[seed])
            continue;
        queue.clear();
        queue.push_back((uint32_t)seed);
        state[seed] = 1;
        size_t head = 0, placed = 0;
        while (head < queue.size() && placed < 256)
        {
            const uint32_t u = queue[head++];
            state[u] = 2;
            nodes.push_back(u);
            ++placed;
            for (uint32_t j = off[u]; j < off[u + 1]; ++j)
                for (int c = 0; c < 4; ++c)
                {
                    const uint32_t v = conn[4ull * (inc[j] >> 2) + c];
                    if (!state[v])
                    {
                        state[v] = 1;
                        queue.push_back(v);
                    }
                }
        }
        for (size_t q = head; q < queue.size(); ++q)  // queued but not placed: free again
            state[queue[q]] = 0;
        nodes.resize((nodes.size() + 255) / 256 * 256, 0xFFFFFFFFu);
    }
    return nodes;
}

// compact tiles for single handles (a shard's PCG loop folds p.Ap into rank-ordered chunk partials in the tile
// kernel, which needs tiles of consecutive nodes); CWF_PARITY_TILES=strip keeps the strips
bool parity_compact_tiles_wanted(const cwf_hip_system *h)
{
    const char *pt = knob("CWF_PARITY_TILES");
    return !h->sharded() && h->ds.E <= kParityCompactMaxTets && !(pt && std::strcmp(pt, "strip") == 0);
}

int parity_incidence_slots(cwf_hip_system *h)
{
    DevSys &s = h->ds;
    const uint64_t N = s.N, E = s.E;
    const bool compact = parity_compact_tiles_wanted(h);
    std::vector<uint32_t> off, inc, toff, tets, pinc, conn, tnodes;
    try
    {
        off.resize(N + 1);
        inc.resize(4 * E);
        pinc.resize(4 * E);
        tets.reserve(3 * E);
        if (compact)
            conn.resize(4 * E);
    }
    catch (const std::bad_alloc &)
    {
        return set_error(h, CWF_ERR_ALLOC, "host allocation failed");
    }
    HIPTRY(h, hipMemcpy(off.data(), s.off, (N + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPTRY(h, hipMemcpy(inc.data(), s.inc, 4 * E * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (compact)
    {
        // the corner ids: the first 16 B of every 64-B element record
        HIPTRY(h, hipMemcpy2D(conn.data(), 16, s.erec, 64, 16, E, hipMemcpyDeviceToHost));
        try
        {
            tnodes = parity_compact_tiles(off, inc, conn, N);
        }
        catch (const std::bad_alloc &)
        {
            return set_error(h, CWF_ERR_ALLOC, "host allocation failed");
        }
    }
    const uint64_t nt = compact ? tnodes.size() / 256 : (N + 255) / 256;
    toff.resize(nt + 1);
    std::vector<uint32_t> loc;
    for (uint64_t b = 0; b < nt; ++b)
    {
        toff[b] = (uint32_t)tets.size();
        loc.clear();
        const auto tile_node = [&](uint64_t t) -> uint64_t {
            return compact ? (uint64_t)tnodes[256 * b + t] : 256 * b + t;
        };
        for (uint64_t t = 0; t < 256; ++t)
        {
            const uint64_t n = tile_node(t);
            if (n < N)
                for (uint32_t j = off[n]; j < off[n + 1]; ++j)
                    loc.push_back(inc[j] >> 2);
        }
        std::sort(loc.begin(), loc.end());
        loc.erase(std::unique(loc.begin(), loc.end()), loc.end());
        for (uint64_t t = 0; t < 256; ++t)
        {
            const uint64_t n = tile_node(t);
            if (n < N)
                for (uint32_t j = off[n]; j < off[n + 1]; ++j)
                    pinc[j] = (uint32_t)(std::lower_bound(loc.begin(), loc.end(), inc[j] >> 2) - loc.begin()) << 2 |
                              (inc[j] & 3u);
        }
        try
        {
            tets.insert(tets.end(), loc.begin(), loc.end());
        }
        catch (const std::bad_alloc &)
        {
            return set_error(h, CWF_ERR_ALLOC, "host allocation failed");
        }
        if (tets.size() >= (1ull << 32))
            return set_error(h, CWF_ERR_UNSUPPORTED, "mesh too large for one PARITY handle (shard it)",
                             "tile_tets=" + std::to_string(tets.size()));
    }
    toff[nt] = (uint32_t)tets.size();
    uint32_t *dto, *dte, *dpi, *dtn = nullptr;
    if (int st = upload(h, &dto, toff.data(), nt + 1))
        return st;
    if (int st = upload(h, &dte, tets.data(), tets.size()))
        return st;
    if (int st = upload(h, &dpi, pinc.data(), 4 * E))
        return st;
    if (compact)
        if (int st = upload(h, &dtn, tnodes.data(), tnodes.size()))
            return st;
    s.ptile_off = dto;
    s.ptile_tets = dte;
    s.pinc = dpi;
    s.ptile_nodes = dtn;
    s.pntile = (uint32_t)nt;
    return 0;
}

int parity_force_buffer(cwf_hip_system *h)
{
    if (h->ds.ptile_off || h->ds.hex || !h->ds.E)
        return 0;
    return parity_incidence_slots(h);
}

int check_ready(cwf_hip_system *h)
{
    if (!h)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null handle");
    if (h->unusable)
        return set_error(h, CWF_ERR_ARGUMENT, "handle unusable after a failed attach",
                         "its operator plan was cut to a shard's owned rows; destroy it");
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess)
        return hip_fail(h, e, "hipSetDevice");
    return 0;
}

// stage a DOF vector: host -> device scratch, or use the device pointer directly
int stage_in(cwf_hip_system *h, const float *src, float *scratch, uint64_t n, int kind, const float **out)
{
    if (kind == CWF_PTR_DEVICE)
    {
        *out = src;
        return 0;
    }
    HIPTRY(h, hipMemcpyAsync(scratch, src, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    *out = scratch;
    return 0;
}

// caller-order node vector (w floats per node, host or device) -> internal order. Without renumbering a
// device input is used in place (*out = src); otherwise it lands in `scratch` (internal order).
int stage_vec(cwf_hip_system *h, const float *src, float *scratch, int kind, int w, const float **out)
{
    const uint64_t n = (uint64_t)w * h->ds.N;
    if (!h->perm)
        return stage_in(h, src, scratch, n, kind, out);
    const float *s = src;
    if (kind != CWF_PTR_DEVICE)
    {
        HIPTRY(h, hipMemcpyAsync(h->pbuf, src, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
        s = h->pbuf;
    }
    perm_gather(h->perm, s, scratch, h->ds.N, w, h->stream);
    *out = scratch;
    return 0;
}

// caller-order input into a fixed internal buffer (always copies)
int vec_in(cwf_hip_system *h, const float *src, float *dst, int kind, int w)
{
    const float *p = nullptr;
    if (int st = stage_vec(h, src, dst, kind, w, &p))
        return st;
    if (p != dst)
        HIPTRY(h, hipMemcpyAsync(dst, p, (uint64_t)w * h->ds.N * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// internal-order device vector -> caller order (host or device)
int vec_out(cwf_hip_system *h, const float *src, float *dst, int kind, int w)
{
    const uint64_t n = (uint64_t)w * h->ds.N;
    if (!h->perm)
    {
        if (src != dst)
            HIPTRY(h, hipMemcpyAsync(dst, src, n * sizeof(float),
                                     kind == CWF_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                                     h->stream));
        return 0;
    }
    if (kind == CWF_PTR_DEVICE)
    {
        perm_scatter(h->perm, src, dst, h->ds.N, w, h->stream);
        return 0;
    }
    perm_scatter(h->perm, src, h->pbuf, h->ds.N, w, h->stream);
    HIPTRY(h, hipMemcpyAsync(dst, h->pbuf, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return 0;
}

// Morton order of the node coordinates: perm[i] = caller node of internal node i
std::vector<uint32_t> morton_node_order(const double *X, uint64_t N)
{
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint64_t n = 0; n < N; ++n)
        for (int k = 0; k < 3; ++k)
        {
            lo[k] = std::min(lo[k], X[3 * n + k]);
            hi[k] = std::max(hi[k], X[3 * n + k]);
        }
    double ext = 0.0;
    for (int k = 0; k < 3; ++k)
        ext = std::max(ext, hi[k] - lo[k]);
    const double scale = ext > 0 ? (double)((1u << 21) - 1) / ext : 0.0;
    std::vector<uint64_t> key(N);
    for (uint64_t n = 0; n < N; ++n)
    {
        uint64_t q[3];
        for (int k = 0; k < 3; ++k)
            q[k] = (uint64_t)std::llround((X[3 * n + k] - lo[k]) * scale);
        key[n] = spread21(q[0]) | spread21(q[1]) << 1 | spread21(q[2]) << 2;
    }
    std::vector<uint32_t> perm(N);
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    return perm;
}

// ---- cwf_hip_system_create: the path choice, then one function per stage. A stage returns a status; the
// handle's guard in create (HandlePtr) frees whatever a failing stage had allocated, so HIPTRY is safe in them.

// CWF_GROUPS=0 (diagnostic): the per-tet tiles instead of the fan groups
bool groups_enabled()
{
    const char *gv = knob("CWF_GROUPS");
    return !(gv && gv[0] == '0');
}

// fan-group tile lanes: 256 (<= 256 groups, <= 512 nodes: T/N 1.59 against 1.77 on C3, 1.60 against 1.76 on
// C2). 128-lane tiles give C2's resident workgroups two tiles each instead of 1.7, but twice the workgroups
// whose per-workgroup p.Ap shares every update workgroup refolds: with write-through partials C2 runs +2.3%
// on 256 lanes (same-box A/B, two passes; 128 had been +6% before the partials were written through).
// CWF_GROUP_NT=128|256 overrides
uint32_t group_lanes()
{
    const char *gn = knob("CWF_GROUP_NT");
    return gn && atoi(gn) == 128 ? 128u : 256u;
}

// hex8 tile lanes: 256 (<= 256 hexes, <= 512 nodes) from 1M hexes up, else 128. The per-workgroup p.Ap shares
// every update workgroup refolds (and the r.r / r.z shares every hex workgroup refolds) halve with the
// workgroup count: C3 hex8 +2.5-3.9% on 256 lanes, C2 hex8 -2.0-2.5% (same-box A/B, two passes).
// CWF_HEX_NT=128|256 overrides
uint32_t hex_tile_lanes(uint64_t hexes)
{
    const char *e = knob("CWF_HEX_NT");
    if (e)
        return atoi(e) == 256 ? 256u : 128u;
    return hexes >= 1000000ull ? 256u : 128u;
}

// hex8: all 8 connectivity slots used; tet4 pads slots 4..7 with UINT32_MAX
static bool desc_hex(const cwf_system_desc *d)
{
    return d->element_count && d->element_connectivity[4] != 0xFFFFFFFFu;
}

// Which FAST layout create builds for the caller's desc (is_lat: detect_lattice's verdict; geo_ok: the
// coordinates reproduce the gradients). Structured blocks take the lattice stencil, hex8 meshes the hex tiles.
// Tets take the fan groups when the geometry can be recomputed (the groups kernel has no gradient stream) and
// there are <= 16 materials (D from kernel arguments or an LDS table), else the pipelined per-tet tiles, else
// (no usable coordinates) the 48-B records; CWF_GROUPS=0 and CWF_TILE_PIPE=0 each step one kernel down.
// owner_renumber ignores CWF_TILE_PIPE: under CWF_TILE_PIPE=0 a mesh that would take the fan groups is still
// renumbered by their owner tiles although it runs k_keff_tiles. The knob has always behaved so; kept as it is.
PathChoice choose_fast_path(const cwf_system_desc *d, bool is_lat, bool geo_ok)
{
    if (!d->element_count)
        return {FastPath::None, false};
    if (is_lat)
        return {FastPath::Lattice, false};
    if (desc_hex(d))
        return {FastPath::HexTiles, true};
    const bool fans = geo_ok && groups_enabled() && d->material_count <= 16;
    const char *pp = knob("CWF_TILE_PIPE");  // diagnostic: 0 = the one-tile-per-workgroup kernel
    const bool pipe = geo_ok && !(pp && pp[0] == '0');
    return {!pipe ? FastPath::Tiles : fans ? FastPath::Groups : FastPath::TilesPipe, fans};
}

// validate_system (pcg.cpp:82-139)
static int validate_desc(const cwf_system_desc *d)
{
    const uint64_t N = d->node_count, E = d->element_count;
    if (d->dof_count != N * 3)
        return set_error(nullptr, CWF_ERR_SIZE, "dof count mismatch (expected node_count * 3)",
                         "node_count=" + std::to_string(N) + "\ndof_count=" + std::to_string(d->dof_count));
    if (d->material_count == 0 || !d->material_stiffness)
        return set_error(nullptr, CWF_ERR_MATERIALS, "materials table is empty");
    if (d->reduction_block == 0)
        return set_error(nullptr, CWF_ERR_REDUCTION, "reduction block must be >= 1", "reduction_block=0");
    if (d->reduction_partials == 0)
        return set_error(nullptr, CWF_ERR_REDUCTION, "reduction partial count must be >= 1", "reduction_partials=0");
    if ((E && (!d->element_connectivity || !d->element_gradients || !d->element_volume ||
               !d->element_material_index)) ||
        (N && (!d->lumped_mass || !d->bc_mask)))
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null system array");
    if (N * 3 >= (1ull << 32) || E >= (1ull << 30))
        return set_error(nullptr, CWF_ERR_UNSUPPORTED, "mesh too large for one handle (shard it)",
                         "nodes=" + std::to_string(N) + "\nelements=" + std::to_string(E));
    const bool hex = desc_hex(d);
    const int K = hex ? 8 : 4;
    if (hex && d->mode != CWF_MODE_FAST)
        return set_error(nullptr, CWF_ERR_UNSUPPORTED, "hex8 elements run in CWF_MODE_FAST only",
                         "the reference has no hex8 arithmetic to reproduce (preprocess.cpp:326-330)");
    if (hex && !d->node_coords)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "hex8 systems need node_coords");
    for (uint64_t e = 0; e < E; ++e)
    {
        if (d->element_material_index[e] >= d->material_count)
            return set_error(nullptr, CWF_ERR_MATERIAL_RANGE, "element references material out of range",
                             "element=" + std::to_string(e) +
                                 "\nmaterial_index=" + std::to_string(d->element_material_index[e]));
        if ((d->element_connectivity[e * 8 + 4] != 0xFFFFFFFFu) != hex)
            return set_error(nullptr, CWF_ERR_UNSUPPORTED, "mixed tet4/hex8 meshes are not supported",
                             "element=" + std::to_string(e));
        for (int a = 0; a < K; ++a)
            if (d->element_connectivity[e * 8 + a] >= N)
                return set_error(nullptr, CWF_ERR_NODE_RANGE, "element connectivity references node out of range",
                                 "element=" + std::to_string(e) +
                                     "\nnode=" + std::to_string(d->element_connectivity[e * 8 + a]));
    }
    return 0;
}

// Structured Kuhn block (lattice.cpp): the FAST operator is the node-pair stencil of the one shared cell
// stiffness (k_keff_lattice). Its nodes stay in the caller's order when that is lexicographic within planes
// (a shard's local order too); otherwise a handle that may renumber takes the lexicographic order (lat.perm).
static bool find_lattice(const cwf_system_desc *d, bool may_renumber, Lattice &lat)
{
    const char *lv = knob("CWF_LATTICE");
    if (d->mode != CWF_MODE_FAST || !d->element_count || !d->node_count || d->node_count >= 0x15555555ull ||
        !d->node_coords || (lv && lv[0] == '0'))
        return false;
    std::string why;
    const bool is_lat = detect_lattice(d, may_renumber, lat, &why);
    if (knob("CWF_VERBOSE"))
        fprintf(stderr, "[cwf] lattice: %s (%u x %u x %u nodes%s)\n", is_lat ? "yes" : why.c_str(), lat.nx, lat.ny,
                lat.nz, is_lat && !lat.perm.empty() ? ", renumbered" : "");
    return is_lat;
}

// The caller's desc in the handle's internal node order: perm[i] = caller node of internal node i, the node
// arrays permuted by it, and `desc`, the caller's desc over them (perm converts at the ABI boundary)
struct RenumberedDesc
{
    std::vector<uint32_t> perm, conn, mask;
    std::vector<float> mass;
    std::vector<double> coords;
    cwf_system_desc desc{};

    void apply(const cwf_system_desc *d)
    {
        const uint64_t N = d->node_count, E = d->element_count;
        std::vector<uint32_t> inv(N);
        for (uint64_t i = 0; i < N; ++i)
            inv[perm[i]] = (uint32_t)i;
        conn.assign(d->element_connectivity, d->element_connectivity + 8 * E);
        for (auto &c : conn)
            if (c != 0xFFFFFFFFu)
                c = inv[c];
        mass.resize(N);
        mask.resize(N);
        coords.resize(3 * N);
        for (uint64_t i = 0; i < N; ++i)
        {
            const uint64_t n = perm[i];
            mass[i] = d->lumped_mass[n];
            mask[i] = d->bc_mask[n];
            for (int k = 0; k < 3; ++k)
                coords[3 * i + k] = d->node_coords[3 * n + k];
        }
        desc = *d;
        desc.element_connectivity = conn.data();
        desc.lumped_mass = mass.data();
        desc.bc_mask = mask.data();
        desc.node_coords = coords.data();
        desc.adjacency_offsets = desc.adjacency_elements = nullptr;  // rebuilt in internal order (ascending
        desc.adjacency_local = nullptr;                               // element per node)
    }
};

// owner tile of every node (its record there carries the owner bit); range(tl): the tile's span of tile_nodes
template <class Range>
static std::vector<uint32_t> node_owner_tiles(uint64_t N, const std::vector<uint32_t> &tile_nodes, uint32_t ntiles,
                                              Range range)
{
    std::vector<uint32_t> own(N, 0xFFFFFFFFu);
    for (uint32_t tl = 0; tl < ntiles; ++tl)
    {
        const std::pair<uint32_t, uint32_t> r = range(tl);
        for (uint32_t q = r.first; q < r.second; ++q)
            if (tile_nodes[q] & 0x80000000u)
                own[tile_nodes[q] & 0x7fffffffu] = tl;
    }
    return own;
}

// FAST handles renumber their nodes (cwf_hip.h CWF_DESC_KEEP_NODE_ORDER): a lattice into its lexicographic
// order (lat.perm, taken), everything else along a Morton curve. Fan-group and hex8 meshes (pc.owner_renumber)
// renumber again by (owner tile, Morton) so every tile's owned nodes are one contiguous id range (whole-line
// owner p / partial stores, coalesced owned gathers). The groups and tiles are built from coordinates and tet
// order only, so the rebuild after this renumbering gives the same partition.
static void renumber_desc(const cwf_system_desc *d, Lattice &lat, PathChoice pc, RenumberedDesc &r)
{
    const uint64_t N = d->node_count, E = d->element_count;
    if (pc.path == FastPath::Lattice)
        r.perm.swap(lat.perm);
    else
        r.perm = morton_node_order(d->node_coords, N);
    r.apply(d);
    if (!pc.owner_renumber)
        return;
    std::vector<uint32_t> own;
    if (pc.path == FastPath::HexTiles)  // the hex tiles (tiles.cpp, 8 corners): the same owner = first tile of the node
    {
        HostTiles ht;
        build_tiles(&r.desc, ht, 2u * hex_tile_lanes(E), hex_tile_lanes(E), 8);
        own = node_owner_tiles(N, ht.tile_nodes, ht.ntiles, [&](uint32_t tl) {
            return std::make_pair(ht.tile_node_off[tl], ht.tile_node_off[tl + 1]);
        });
    }
    else
    {
        GroupTiles gt;
        const uint32_t gnt = group_lanes();
        if (!fan_groups_usable(build_group_tiles(&r.desc, gt, gnt, 2 * gnt, kGroupSlotsPerLane * gnt, false), gt))
            return;
        own = node_owner_tiles(N, gt.tile_nodes, gt.ntiles,
                               [&](uint32_t tl) { return std::make_pair(gt.hdr[tl].z, gt.hdr[tl].z + gt.hdr[tl].w); });
    }
    std::vector<uint32_t> order(N);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return own[a] < own[b]; });
    std::vector<uint32_t> p2(N);
    for (uint64_t i = 0; i < N; ++i)
        p2[i] = r.perm[order[i]];
    r.perm.swap(p2);
    r.apply(d);
}

// the handle, its stream and pinned control block, and the scalars of DevSys
static int open_handle(const cwf_system_desc *d, int device, HandlePtr &hp)
{
    hipError_t he = hipSetDevice(device);
    if (he != hipSuccess)
        return hip_fail(nullptr, he, "hipSetDevice");
    hp.reset(new (std::nothrow) cwf_hip_system());
    cwf_hip_system *h = hp.get();
    if (!h)
        return set_error(nullptr, CWF_ERR_ALLOC, "host allocation failed");
    h->device = device;
    h->mode = d->mode == CWF_MODE_FAST ? CWF_MODE_FAST : CWF_MODE_PARITY;
    h->reduction_block = d->reduction_block;
    h->reduction_partials = d->reduction_partials;
    if ((he = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess)
        return hip_fail(h, he, "hipStreamCreate");
    if ((he = hipHostMalloc(reinterpret_cast<void **>(&h->ctl_host), sizeof(Ctl), hipHostMallocDefault)) !=
        hipSuccess)
        return hip_fail(h, he, "hipHostMalloc");
    DevSys &s = h->ds;
    s.N = (uint32_t)d->node_count;
    s.Nown = s.N;
    s.E = (uint32_t)d->element_count;
    s.D = 3 * s.N;
    s.M = (uint32_t)d->material_count;
    s.sK = d->stiffness_scale;
    s.sM = d->mass_factor;
    s.iso = 1;
    for (uint64_t m = 0; m < d->material_count; ++m)
        s.iso &= iso_pattern(d->material_stiffness + 36 * m) ? 1 : 0;
    if (s.M == 1)  // table order of the FAST kernels (dsrc): iso = 3x3 normal block + 3 shear diagonals
        for (int t = 0; t < (s.iso ? 12 : 36); ++t)
            s.d1[t] = (float)d->material_stiffness[s.iso ? (t < 9 ? (t / 3) * 6 + (t % 3) : (t - 6) * 7) : t];
    s.hex = desc_hex(d) ? 1 : 0;
    return 0;
}

// element records (64 B/tet; the PARITY kernels only, so none for hex8) and the per-element / per-node arrays
static int upload_mesh_arrays(cwf_hip_system *h, const cwf_system_desc *d)
{
    DevSys &s = h->ds;
    const uint64_t N = s.N, E = s.E;
    Uploader up{h};
    if (!s.hex)
    {
        std::vector<uint32_t> rec(E * 16);
        for (uint64_t e = 0; e < E; ++e)
        {
            uint32_t *r = rec.data() + e * 16;
            for (int a = 0; a < 4; ++a)
                r[a] = d->element_connectivity[e * 8 + a];
            std::memcpy(r + 4, d->element_gradients + e * 24, 12 * sizeof(float));
        }
        s.erec = up.put(reinterpret_cast<const uint4 *>(rec.data()), E * 4);
    }
    s.vol = up.put(d->element_volume, E);
    s.mat = up.put(d->element_material_index, E);
    s.dmat = up.put(d->material_stiffness, 36 * d->material_count);
    s.mass = up.put(d->lumped_mass, N);
    s.mask = up.put(d->bc_mask, N);
    return up.st;
}

// node -> element CSR, ascending element per node (preprocess.cpp:380-403): the caller's, checked, or built
static int upload_incidence(cwf_hip_system *h, const cwf_system_desc *d)
{
    DevSys &s = h->ds;
    const uint64_t N = s.N, E = s.E;
    const int K = s.hex ? 8 : 4;
    const uint32_t sh = s.hex ? 3u : 2u;  // inc = element << sh | corner
    std::vector<uint32_t> off(N + 1, 0), inc(E * K);
    if (d->adjacency_offsets && d->adjacency_elements && d->adjacency_local)
    {
        std::memcpy(off.data(), d->adjacency_offsets, (N + 1) * sizeof(uint32_t));
        if (off[N] != E * K || off[0] != 0)
            return set_error(h, CWF_ERR_SIZE, "adjacency size mismatch",
                             "expected=" + std::to_string(E * K) + "\nactual=" + std::to_string(off[N]));
        // the caller's CSR must be exactly the node -> (element, corner) incidences in ascending element order
        // (preprocess.cpp:389-400): every later pass indexes through it without bounds checks
        for (uint64_t n = 0; n < N; ++n)
        {
            if (off[n] > off[n + 1])
                return set_error(h, CWF_ERR_ARGUMENT, "adjacency offsets must be non-decreasing",
                                 "node=" + std::to_string(n));
            for (uint32_t j = off[n]; j < off[n + 1]; ++j)
            {
                const uint32_t e = d->adjacency_elements[j], a = d->adjacency_local[j];
                if (e >= E || a >= (uint32_t)K || d->element_connectivity[8ull * e + a] != n ||
                    (j > off[n] && d->adjacency_elements[j - 1] >= e))
                    return set_error(h, CWF_ERR_ARGUMENT, "adjacency does not match the connectivity",
                                     "node=" + std::to_string(n) + "\nentry=" + std::to_string(j));
                inc[j] = (e << sh) | a;
            }
        }
    }
    else
    {
        std::vector<uint32_t> cnt(N, 0);
        for (uint64_t e = 0; e < E; ++e)
            for (int a = 0; a < K; ++a)
                ++cnt[d->element_connectivity[e * 8 + a]];
        uint32_t acc = 0;
        for (uint64_t n = 0; n < N; ++n)
        {
            off[n] = acc;
            acc += cnt[n];
            cnt[n] = 0;
        }
        off[N] = acc;
        for (uint64_t e = 0; e < E; ++e)
            for (int a = 0; a < K; ++a)
            {
                const uint32_t n = d->element_connectivity[e * 8 + a];
                inc[off[n] + cnt[n]++] = ((uint32_t)e << sh) | (uint32_t)a;
            }
    }
    Uploader up{h};
    s.off = up.put(off);
    s.inc = up.put(inc);
    return up.st;
}

// structured Kuhn block: the stencil blocks, the plane table and one row value per node (lattice.hip); the
// per-class preconditioner tables when the lumped mass is a function of the boundary type
static int layout_lattice(cwf_hip_system *h, const cwf_system_desc *d, Lattice &lat)
{
    DevTiles &t = h->ds.t;
    const uint64_t N = h->ds.N;
    std::vector<uint32_t> npo(N + 1);
    std::iota(npo.begin(), npo.end(), 0u);
    t.off_mask = pack_off_mask(npo, d->bc_mask, N);  // N < 2^29 (find_lattice): always packs
    Uploader up{h};
    t.lplane = up.put(lat.plane);
    t.lcoef = up.put(lattice_device_coef(lat));
    t.node_part_off = up.put(npo);
    t.part = up.alloc<float>(3 * (N + 2));  // + 2 padding slots (update pass)
    t.lat = 1;
    t.lnx = lat.nx;
    t.lny = lat.ny;
    t.lnz = lat.nz;
    t.lk1 = lat.nz;
    t.lpstride = lat.nx * lat.ny;
    for (uint32_t k = 0; k < lat.nz; ++k)
        if (lat.plane[k] != k * t.lpstride)
            t.lpstride = 0;
    t.lsym = lat.sym ? 1 : 0;
    t.lhex = lat.hex ? 1 : 0;
    t.node_major = 1;
    t.E = h->ds.E;
    t.geo = 1;
    t.total_tile_nodes = (uint32_t)N;
    if (lat.layered)  // k_keff_lattice_layered: a stencil table per plane class, a cell-pair table per material
        t.llayers = (uint32_t)(lat.cls_pair.size() / 2) | (uint32_t)lat.mat_id.size() << 16;
    // A layered block carries no class preconditioner, even where every density is equal: a node's block inverse
    // depends on the material pair of its plane, which the 27 boundary types x mask classes do not tell apart. So
    // lcls, lcz, lmu and lzr stay off, and with lcls off the resident solve (resident.cpp), the fused one-launch
    // iteration (schedule.cpp) and z-from-r all decline the handle: it runs the two-kernel loop on the per-node inverse.
    LatticeClasses lc;
    if (lat.layered)
        lc.uniform = false;
    else
        lc = lattice_classes(lat, d->bc_mask, d->lumped_mass);
    if (lc.uniform && lc.interior)
    {
        t.lmu = 1;
        t.lmass = lc.interior_mass;
        // z from r in the K_eff pass, no z store in the update pass (attach turns it off, comm.cpp): from
        // 2M nodes, where the iteration's vectors leave the 256 MB MALL and the 12 B per node the update
        // pass no longer writes are HBM bytes (C3 +4-5% PCG it/s); on C2 the K_eff pass's class-table fill
        // and the 3 x 3 products per halo entry sit on its latency-bound critical path (-8%), same box
        const char *zr = knob("CWF_LAT_ZR");
        t.lzr = zr ? (zr[0] == '1' ? 1 : 0) : (N >= (1ull << 21) ? 1 : 0);
    }
    if (lc.uniform)
    {
        t.lcls = up.put(lc.cls.data(), N);
        t.lrep = up.put(lc.rep);
        // classes without a node keep zero inverses (k_lat_class_inverse fills only represented ones; halo
        // lanes of the z-from-r and single-launch passes may read any class)
        t.lcinv6 = up.zeros<uint4>(kLatClasses);
        t.lcinv9 = up.zeros<float>(9 * kLatClasses);
        t.lcz = up.zeros<float4>(2 * kLatClasses);
    }
    h->lat_plane.swap(lat.plane);
    lattice_plan(t);
    return up.st;
}

// Fan groups (groups.cpp, k_keff_groups_pipe): the default FAST tet path when the mesh groups into fans
// (fan_groups_usable). Sets t.grp when it does; otherwise leaves the handle for layout_tiles.
static int layout_groups(cwf_hip_system *h, const cwf_system_desc *d)
{
    DevSys &s = h->ds;
    DevTiles &t = s.t;
    const uint64_t N = s.N, E = s.E;
    GroupTiles gt;
    const uint32_t gnt = group_lanes();
    const int gst = build_group_tiles(d, gt, gnt, 2 * gnt, kGroupSlotsPerLane * gnt);
    if (knob("CWF_VERBOSE"))
        fprintf(stderr, "[cwf] fan groups: status %d, %u groups (%.2f tets each), %u tiles, %zu tile nodes "
                        "(%.3f per node), max %u nodes / %u slots per tile\n",
                gst, gt.ngroups, gt.tets_per_group, gt.ntiles, gt.tile_nodes.size(),
                N ? (double)gt.tile_nodes.size() / (double)N : 0.0, gt.max_tile_nodes, gt.max_tile_slots);
    if (!fan_groups_usable(gst, gt))
        return 0;
    const size_t T = gt.tile_nodes.size();
    std::vector<uint2> tnode(T);
    for (size_t q = 0; q < T; ++q)
        tnode[q] = uint2{gt.tile_nodes[q], gt.run[q]};
    t.off_mask = pack_off_mask(gt.node_part_off, d->bc_mask, N);
    Uploader up{h};
    t.grec = up.put(gt.grec);
    t.hdr = up.put(gt.hdr);
    t.tnode = up.put(tnode);
    t.node_part_off = up.put(gt.node_part_off);
    t.tslot = up.put(gt.tile_slot.data(), T);
    t.tcoord = up.put3(gt.tcoord, T);
    t.part = up.alloc<float>(3 * (T + 2));  // + 2 padding slots (update pass)
    t.grp = 1;
    t.geo = 1;
    t.node_major = 1;
    t.push = 1;
    t.pipe = 1;
    t.pipe_nt = (int)gnt;
    t.wt_part = E < 4000000ull ? 1 : 0;  // write-through tile partials below 4M tets
    t.ntiles = gt.ntiles;
    t.ngroups = gt.ngroups;
    t.max_tile_nodes = gt.max_tile_nodes;
    t.total_tile_nodes = (uint32_t)T;
    t.E = (uint32_t)E;
    t.pipe_grid = fast_pipe_grid(s);
    return up.st;
}

// FAST-mode element tiles (tiles.cpp): the hex tiles (k_keff_hex_tiles: hex_nt lanes, one hex and two tile
// nodes per lane, push fold), the pipelined per-tet tiles or one tile per workgroup.
// GEO (geo_ok): stream 8-B corner ids + tile-node coordinates and recompute gradients/volume on the fly, when
// the desc carries coordinates that reproduce its gradients (CWF_GEO=0 forces the 48-B records)
static int layout_tiles(cwf_hip_system *h, const cwf_system_desc *d, FastPath path, bool geo_ok)
{
    DevSys &s = h->ds;
    DevTiles &t = s.t;
    const uint64_t N = s.N, E = s.E;
    const bool hex = path == FastPath::HexTiles, pipe = path == FastPath::TilesPipe;
    t.geo = hex || geo_ok ? 1 : 0;
    t.pipe = pipe ? 1 : 0;
    t.push = hex || pipe ? 1 : 0;  // the pipelined kernel folds pushed forces (epos), not local-CSR entries
    HostTiles ht;
    if (hex)
    {
        t.hex = 1;
        t.hex_nt = (int)hex_tile_lanes(E);
        build_tiles(d, ht, 2u * (uint32_t)t.hex_nt, (uint32_t)t.hex_nt, 8);
    }
    else if (pipe)
    {
        // 256-thread workgroups over 512-element tiles, or 128 over 256 (128 below 4M tets: the meshes whose
        // 512-element tiles would give each resident workgroup < 8 tiles)
        t.pipe_nt = E < 4000000ull ? 128 : 256;
        build_tiles(d, ht, (uint32_t)t.pipe_nt, 2u * (uint32_t)t.pipe_nt);
    }
    else
        build_tiles(d, ht, (uint32_t)kMaxTileNodes, (uint32_t)kTileElems);
    const size_t T = ht.tile_nodes.size();
    if (knob("CWF_VERBOSE"))
        fprintf(stderr, "[cwf] tiles: %u tiles, %zu tile nodes (%.3f per node), max %u nodes/tile, %s records\n",
                ht.ntiles, T, N ? (double)T / (double)N : 0.0, ht.max_tile_nodes,
                t.geo ? "8-B geometric" : "48-B gradient");
    Uploader up{h};
    if (t.geo)
    {
        if (hex)
            t.eid8 = up.put(ht.eid8.data(), E);
        else
            t.eid = up.put(ht.eid.data(), E);
        t.tcoord = up.put3(ht.tcoord, T);
    }
    else
        t.planes = up.put3(ht.planes, E);
    if (!ht.mat.empty())
        t.mat = up.put(ht.mat.data(), E);
    // only the tet push fold pads its runs, within the pipelined kernel's slot budget (4 te + 2 nt)
    const TileRecords rec = pack_tile_records(ht, hex ? 8 : 4, pipe, 8u * (uint32_t)t.pipe_nt + 2u * (uint32_t)t.pipe_nt);
    t.hdr = up.put(rec.hdr);
    t.tnode = up.put(rec.tnode);
    if (!t.push)  // PUSH streams the per-element positions (epos) instead
    {
        ht.csr_ent.resize(ht.csr_ent.size() + 8, 0);  // the kernel reads a tile's entries as 16-B words
        t.csr_ent = up.put(ht.csr_ent);
    }
    t.off_mask = pack_off_mask(ht.node_part_off, d->bc_mask, N);
    t.node_part_off = up.put(ht.node_part_off);
    t.part_slot = up.put(ht.node_part_slot);
    if (hex)
        t.epos8 = up.put(ht.epos8);
    else if (pipe)
        t.epos = up.put(ht.epos);
    if (pipe || hex)
    {
        t.tslot = up.put(ht.tile_slot);
        t.node_major = 1;
    }
    t.part = up.alloc<float>(3 * (T + 2));  // + 2 padding slots (update pass)
    t.ntiles = ht.ntiles;
    t.hex_all_affine = hex && !ht.tile_affine.empty() &&
                       std::all_of(ht.tile_affine.begin(), ht.tile_affine.end(), [](uint8_t a) { return a != 0; });
    t.max_tile_nodes = ht.max_tile_nodes;
    t.total_tile_nodes = (uint32_t)T;
    t.E = (uint32_t)E;
    if (pipe || hex)
        t.pipe_grid = fast_pipe_grid(s);
    return up.st;
}

// the hex block-Jacobi setup integrates from the global corners (fp64)
static int upload_hex_jacobi(cwf_hip_system *h, const cwf_system_desc *d)
{
    DevSys &s = h->ds;
    Uploader up{h};
    s.hconn = up.put(d->element_connectivity, 8ull * s.E);
    s.hcoord = up.put(d->node_coords, 3ull * s.N);
    s.hgrad = up.put(d->element_gradients, 24ull * s.E);
    return up.st;
}

// solver vectors, reduction partials and scalars; perm (a renumbered handle's node order) or NULL
static int alloc_scratch(cwf_hip_system *h, const cwf_system_desc *d, const std::vector<uint32_t> *perm)
{
    const DevSys &s = h->ds;
    const uint64_t N = s.N, D = 3 * N;
    Uploader up{h};
    for (float **v : {&h->x, &h->r, &h->p, &h->p2, &h->p3, &h->p4, &h->z, &h->Ap, &h->rhs, &h->tmp})
        *v = up.alloc<float>(D);
    if (s.t.lat && s.t.lcls)  // the fused lattice iteration's second r / Ap and its shares (lattice_fused.hip)
    {
        h->r2 = up.alloc<float>(D);
        h->ap2 = up.alloc<float>(D);
        h->fsh = up.alloc<double>(2ull * 5 * std::max<uint32_t>(s.t.lnwork, 1u));
        h->g_fsh = up.alloc<double>(8);  // one rank until attach (comm.cpp grows it to [nranks][8])
    }
    h->inv = up.alloc<float>(9 * N);
    h->inv6 = up.alloc<float>(4 * N);
    const uint64_t chunks = (D + d->reduction_block - 1) / d->reduction_block;
    h->part_cap = std::max<uint64_t>(
        {chunks, (uint64_t)fast_block_count(h), (uint64_t)fast_dot_blocks(s.D), (uint64_t)s.t.ntiles,
         (uint64_t)s.t.pipe_grid, 1});
    for (double **v : {&h->part0, &h->part1, &h->part2})
        *v = up.alloc<double>(h->part_cap);
    h->ctl = up.alloc<Ctl>(1);
    h->scal = up.alloc<double>(8);
    // folded per-rank scalars (one rank until cwf_hip_system_attach): p.Ap, {r.r, r.z}, {rhs.rhs, r0.r0}, r0.z0
    h->g_pap = up.alloc<double>(6);
    h->g_rrz = h->g_pap + 1;
    h->g_init = h->g_rrz + 2;
    h->g_rz0 = h->g_init + 2;
    if (perm)
    {
        h->perm = up.put(*perm);
        h->pbuf = up.alloc<float>(13 * N);
    }
    if (!up.st && h->mode == CWF_MODE_PARITY)
        up.st = parity_force_buffer(h);
    if (up.st)
        return up.st;
    HIPTRY(h, hipMemset(h->x, 0, D * sizeof(float)));
    HIPTRY(h, hipMemset(h->ctl, 0, sizeof(Ctl)));
    HIPTRY(h, hipMemset(h->g_pap, 0, 6 * sizeof(double)));
    HIPTRY(h, hipDeviceSynchronize());
    return 0;
}

}  // namespace cwf

extern "C" {

int cwf_hip_abi_version(void) { return CWF_HIP_ABI_VERSION; }

int cwf_hip_device_count(int *count)
{
    if (!count)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess)
    {
        *count = 0;
        return hip_fail(nullptr, e, "hipGetDeviceCount");
    }
    return 0;
}

const char *cwf_hip_last_error(const cwf_hip_system *h) { return h ? h->err.c_str() : g_err.c_str(); }
const char *cwf_hip_last_context(const cwf_hip_system *h) { return h ? h->ctx.c_str() : g_ctx.c_str(); }

void cwf_hip_system_destroy(cwf_hip_system *h)
{
    if (!h)
        return;
    (void)hipSetDevice(h->device);
    if (h->stream)
        (void)hipStreamSynchronize(h->stream);
    if (h->comm && h->comm->kind == 0)  // give the LOCAL communicator's stream back
    {
        h->comm->members[h->rank] = nullptr;
        h->stream = h->own_stream;
    }
    h->mem.clear();
    h->hist.reset();
    if (h->ctl_host)
        (void)hipHostFree(h->ctl_host);
    for (hipEvent_t e : h->ev)
        (void)hipEventDestroy(e);
    if (h->stream)
        (void)hipStreamDestroy(h->stream);
    delete h;
}

// validate, choose the FAST path, renumber, open the handle, then one stage per group of device arrays (above).
// Host arrays live and die inside their stage. Every exit after the handle exists goes through hp.
int cwf_hip_system_create(const cwf_system_desc *d, int device, cwf_hip_system **out)
{
    if (!d || !out)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    *out = nullptr;
    HandlePtr hp(nullptr, cwf_hip_system_destroy);
    // the handle's message and context outlive it in the thread-local error
    const auto bail = [&hp](int st) {
        if (hp)
        {
            const std::string m = hp->err, c = hp->ctx;
            hp.reset();
            set_error(nullptr, st, m, c);
        }
        return st;
    };
    try
    {
        if (int st = validate_desc(d))
            return st;
        const bool hex = desc_hex(d);
        const char *rn = knob("CWF_RENUMBER");
        const bool may_renumber = d->mode == CWF_MODE_FAST && d->element_count && d->node_count && d->node_coords &&
                                  !(d->reserved & CWF_DESC_KEEP_NODE_ORDER) && !(rn && rn[0] == '0');
        Lattice lat;
        const bool is_lat = find_lattice(d, may_renumber, lat);
        // FAST recomputes tet geometry from node coordinates when they reproduce the desc's gradients (GEO).
        // Node renumbering does not change it, so it is decided once, on the caller's desc.
        const char *ge = knob("CWF_GEO");
        const bool geo_ok = d->element_count && d->node_count && d->node_coords && !(ge && ge[0] == '0') &&
                            (hex || geometry_matches(d));
        const PathChoice pc = choose_fast_path(d, is_lat, geo_ok);
        RenumberedDesc rd;  // the rest of create sees the desc in internal order
        const bool renumber = may_renumber && (!is_lat || !lat.perm.empty());
        if (renumber)
        {
            renumber_desc(d, lat, pc, rd);
            d = &rd.desc;
        }
        int st = open_handle(d, device, hp);
        cwf_hip_system *h = hp.get();
        st = st ? st : upload_mesh_arrays(h, d);
        st = st ? st : upload_incidence(h, d);
        if (!st && pc.path == FastPath::Lattice)
            st = layout_lattice(h, d, lat);
        if (!st && pc.path == FastPath::Groups)
            st = layout_groups(h, d);
        // a mesh that was to group into fans and does not takes the pipelined per-tet tiles
        if (!st && pc.path != FastPath::None && pc.path != FastPath::Lattice && !h->ds.t.grp)
            st = layout_tiles(h, d, pc.path == FastPath::Groups ? FastPath::TilesPipe : pc.path, geo_ok);
        if (!st && hex)
            st = upload_hex_jacobi(h, d);
        st = st ? st : alloc_scratch(h, d, renumber ? &rd.perm : nullptr);
        if (st)
            return bail(st);
    }
    catch (const std::bad_alloc &)
    {
        return bail(set_error(hp.get(), CWF_ERR_ALLOC, "host allocation failed"));
    }
    *out = hp.release();
    return 0;
}

int cwf_hip_system_set_scalars(cwf_hip_system *h, double stiffness_scale, double mass_factor)
{
    if (int st = check_ready(h))
        return st;
    h->ds.sK = stiffness_scale;
    h->ds.sM = mass_factor;
    return 0;
}

int cwf_hip_system_set_mode(cwf_hip_system *h, int mode)
{
    if (int st = check_ready(h))
        return st;
    if (h->ds.hex && mode != CWF_MODE_FAST)
        return set_error(h, CWF_ERR_UNSUPPORTED, "hex8 elements run in CWF_MODE_FAST only",
                         "the reference has no hex8 arithmetic to reproduce (preprocess.cpp:326-330)");
    if (h->perm && mode != CWF_MODE_FAST)
        return set_error(h, CWF_ERR_UNSUPPORTED, "a renumbered FAST handle cannot switch to CWF_MODE_PARITY",
                         "create the PARITY handle separately (or with CWF_DESC_KEEP_NODE_ORDER)");
    h->mode = mode == CWF_MODE_FAST ? CWF_MODE_FAST : CWF_MODE_PARITY;
    if (h->mode == CWF_MODE_PARITY)
        return parity_force_buffer(h);
    return 0;
}

int cwf_hip_system_set_timing(cwf_hip_system *h, int enabled)
{
    if (int st = check_ready(h))
        return st;
    h->timing = enabled > 0 ? enabled : 0;  // time every `enabled`-th PCG-loop K_eff launch
    h->keff_ms = 0.0;
    h->keff_count = 0;
    return 0;
}

int cwf_hip_system_timing(cwf_hip_system *h, double *keff_ms, uint64_t *keff_launches)
{
    if (int st = check_ready(h))
        return st;
    if (keff_ms)
        *keff_ms = h->keff_ms;
    if (keff_launches)
        *keff_launches = h->keff_count;
    h->keff_ms = 0.0;
    h->keff_count = 0;
    return 0;
}

int cwf_hip_keff_timed(cwf_hip_system *h, const float *x, float *y, int reps, double *avg_ms)
{
    if (int st = check_ready(h))
        return st;
    if (!x || !y || !avg_ms || reps <= 0)
        return set_error(h, CWF_ERR_ARGUMENT, "bad argument");
    hipEvent_t a, b;
    HIPTRY(h, hipEventCreate(&a));
    HIPTRY(h, hipEventCreate(&b));
    const char *dry = knob("CWF_TIMED_PCG");  // diagnostic: time the PCG-mode tiles kernel instead
    if (dry && h->mode == CWF_MODE_FAST && h->ds.iso)
    {
        Ctl c{};
        c.active = 1;
        c.beta = 0.5;
        c.rho2[0] = c.rho2[1] = 1.0;
        c.tol = 0.0;
        HIPTRY(h, hipMemcpyAsync(h->ctl, &c, sizeof c, hipMemcpyHostToDevice, h->stream));
        HIPTRY(h, hipMemsetAsync(h->part1, 0, h->part_cap * sizeof(double), h->stream));
        HIPTRY(h, hipMemsetAsync(h->part2, 0, h->part_cap * sizeof(double), h->stream));
        fast_tiles_pcg_dry(h, (unsigned)atoi(dry), 5, h->stream);
    }
    HIPTRY(h, hipEventRecord(a, h->stream));
    for (int i = 0; i < reps; ++i)
    {
        if (dry && h->mode == CWF_MODE_FAST && h->ds.iso)
            fast_tiles_pcg_dry(h, (unsigned)atoi(dry), 1, h->stream);
        else
            keff_apply_ds(h, h->ds, x, y, false, h->stream);
    }
    HIPTRY(h, hipEventRecord(b, h->stream));
    HIPTRY(h, hipEventSynchronize(b));
    float ms = 0.f;
    HIPTRY(h, hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *avg_ms = (double)ms / reps;
    return 0;
}

int cwf_hip_bandwidth_probe(int device, uint64_t bytes, int reps, double *gbs)
{
    if (!gbs || bytes < 16 || reps < 1)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "bandwidth probe: bad arguments");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess)
        return hip_fail(nullptr, e, "hipSetDevice");
    bytes &= ~(uint64_t)15;
    DevicePtr<char> a, b;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.f;
    if ((e = a.alloc(bytes)) == hipSuccess && (e = b.alloc(bytes)) == hipSuccess &&
        (e = hipMemset(a, 0, bytes)) == hipSuccess && (e = hipEventCreate(&e0)) == hipSuccess &&
        (e = hipEventCreate(&e1)) == hipSuccess)
    {
        copy16(a, b, bytes, nullptr);  // warm
        (void)hipEventRecord(e0, nullptr);
        for (int r = 0; r < reps; ++r)
            copy16(a, b, bytes, nullptr);
        (void)hipEventRecord(e1, nullptr);
        e = hipEventSynchronize(e1);
        if (e == hipSuccess)
            e = hipEventElapsedTime(&ms, e0, e1);
    }
    if (e0)
        (void)hipEventDestroy(e0);
    if (e1)
        (void)hipEventDestroy(e1);
    if (e != hipSuccess)
        return hip_fail(nullptr, e, "bandwidth probe");
    *gbs = 2.0 * (double)bytes * reps / ((double)ms * 1e-3) / 1e9;  // read + write
    return 0;
}

int cwf_hip_system_memory(const cwf_hip_system *h, uint64_t *bytes)
{
    if (!h || !bytes)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    *bytes = h->mem.total();
    return 0;
}

int cwf_hip_system_keff_traffic(const cwf_hip_system *h, uint64_t *layout_bytes, uint64_t *reference_layout_bytes)
{
    if (!h || !layout_bytes || !reference_layout_bytes)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    const DevSys &s = h->ds;
    const uint64_t N = s.N, E = s.E, T = s.t.total_tile_nodes;
    *reference_layout_bytes = 32 * N + 72 * E;
    if (h->mode == CWF_MODE_FAST && s.t.ntiles)
    {
        // per tile: 16-B header; per tet: corner ids (8 B GEO, 48-B records otherwise) + 4 u16 local-CSR
        // entries or (PUSH) positions (+ material id when M > 1); per tile node: {node, csr range} 8 B, coordinates 12 B (GEO), the node-major slot 4 B
        // (pipelined / hex), partial written 12 B; per node: p_old and z read once (24 B) + mass 4 B + the new
        // p written by its owner slot (12 B, PCG mode: the launches bench.py times)
        // hex8: 16-B corner ids + 16-B positions per hex (no material stream for one material)
        // fan groups: 16-B group record (ids, push ranks, tet count, material) instead of the per-tet records
        const uint64_t rec = s.t.hex ? 32 : s.t.geo ? 16 : 56;
        const PcgSchedule sch = schedule_of(h);
        if (sch == PcgSchedule::Resident)
        {  // the resident solve (resident.hip), per iteration: only what crosses a CU -- the halo records read, the
           // box-surface records and the shares written, the G x 5 shares read -- the vectors stay on chip
            *layout_bytes = resident_offchip_bytes(h);
            return 0;
        }
        if (sch == PcgSchedule::Fused || sch == PcgSchedule::FusedPeer)
        {  // the fused iteration (lattice_fused.hip): per owned node r_(j-1), Ap_(j-1), p_(j-1), the class byte and x
           // read, r_j, p_j, Ap_j and x written; the mass of the shell's nodes (the strict interior's is one value when lmu)
            *layout_bytes = (uint64_t)s.Nown * (4 * 12 + 1 + 4 * 12) + 4ull * (s.t.lmu ? s.t.lnshell : s.Nown);
            return 0;
        }
        if (s.t.lat && s.t.llayers)  // layered: the same streams with the per-node mass, plus the plane-class and
        {                            // material tables and the per-plane word
            *layout_bytes = (uint64_t)s.Nown * (12 + 12 + 12 + 12 + 4) + 4ull * lattice_table_floats(s.t) + 4ull * s.t.lnz;
            return 0;
        }
        if (s.t.lat)  // per owned node: z and p_old read, the new p and the row value written; the mass read
        {             // (only the shell's when the strict interior's is one value, lmu)
            *layout_bytes = (uint64_t)s.Nown * (12 + 12 + 12 + 12 + (s.t.lmu && s.t.lzr ? 1 : 0)) +
                            4ull * (s.t.lmu ? s.t.lnshell : s.Nown);
            return 0;
        }
        if (s.t.grp)
        {
            *layout_bytes = 16ull * s.t.ntiles + (uint64_t)s.t.ngroups * 16 +
                            T * (8 + 12 + 4 + 12) + N * (24 + 4 + 12);
            return 0;
        }
        *layout_bytes = 16ull * s.t.ntiles + E * (rec + (s.t.mat ? 4 : 0)) +
                        T * (8 + (s.t.geo ? 12 : 0) + (s.t.node_major ? 4 : 0) + 12) + N * (24 + 4 + 12);
    }
    else  // PARITY node tiles (k_keff_parity_tile), compulsory: per tet the 64-B record, vol, its 4 incidence
          // entries (pinc) and its tile-list entry (+ material); per node CSR offset, x in, y out, mass, mask
        *layout_bytes = E * (64 + 4 + 16 + 4 + (s.M > 1 ? 4 : 0)) + N * (4 + 12 + 12 + 4 + 4);
    return 0;
}

#ifndef CWF_FAST_SRC_HASH
#define CWF_FAST_SRC_HASH "unknown"
#endif
#ifndef CWF_PARITY_SRC_HASH
#define CWF_PARITY_SRC_HASH "unknown"
#endif
const char *cwf_hip_system_keff_source_hash(const cwf_hip_system *h)
{
    if (!h)
        return nullptr;
    return h->mode != CWF_MODE_FAST || !h->ds.t.ntiles ? CWF_PARITY_SRC_HASH : CWF_FAST_SRC_HASH;
}

int cwf_hip_system_exchange_schedule(const cwf_hip_system *h)
{
    return h && h->sharded() ? exchange_schedule_code(h->sched) : -1;
}

// the PCG loop's instantiation (no sanitize) of the element pass, from the picker that launches it
const char *cwf_hip_system_keff_kernel(const cwf_hip_system *h)
{
    if (!h)
        return nullptr;
    if (h->mode != CWF_MODE_FAST || !h->ds.t.ntiles)  // the tiles as built, else as parity_incidence_slots will build them
        return parity_keff_kernel_name(h, h->ds.ptile_nodes || (!h->ds.ptile_off && parity_compact_tiles_wanted(h)));
    const PcgSchedule sch = schedule_of(h);
    if (sch == PcgSchedule::Resident)
        return resident_kernel_name(h->ds, h->res);
    if (sch == PcgSchedule::Fused || sch == PcgSchedule::FusedPeer)
        return pcg_lattice_kernel_name(h->ds, h->sched.grid);
    return fast_tiles_kernel_name(h->ds);
}

int cwf_hip_derived_fields(cwf_hip_system *h, const float *u, uint64_t n, int u_kind, float *elements,
                           float *nodes, int out_kind)
{
    if (int st = check_ready(h))
        return st;
    if (!u || (!elements && !nodes))
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    if (n != h->ds.D)
        return set_error(h, CWF_ERR_SIZE, "displacement span size mismatch",
                         "input=" + std::to_string(n) + "\ndofs=" + std::to_string(h->ds.D));
    const float *uin = nullptr;
    if (int st = stage_vec(h, u, h->tmp, u_kind, 3, &uin))
        return st;
    const uint64_t ne = 13ull * h->ds.E, nn = 13ull * h->ds.N;
    float *de = elements, *dn = nodes;
    if (out_kind != CWF_PTR_DEVICE || h->perm)  // stage through one scratch allocation
    {
        DevicePtr<float> scratch;
        if (hipError_t e = scratch.alloc(ne + nn + 1); e != hipSuccess)
            return hip_fail(h, e, "derived fields");
        de = elements ? scratch.get() : nullptr;
        dn = nodes ? scratch + ne : nullptr;
        derived_fields(h, uin, de, dn, h->stream);
        hipError_t e1 = hipGetLastError();
        const hipMemcpyKind back = out_kind == CWF_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (e1 == hipSuccess && elements)
            e1 = hipMemcpyAsync(elements, de, ne * sizeof(float), back, h->stream);
        if (e1 == hipSuccess && nodes)
        {
            if (h->perm)  // node fields back to the caller's node order
                e1 = vec_out(h, dn, nodes, out_kind, 13) ? hipErrorUnknown : hipSuccess;
            else
                e1 = hipMemcpyAsync(nodes, dn, nn * sizeof(float), back, h->stream);
        }
        if (e1 == hipSuccess)
            e1 = hipStreamSynchronize(h->stream);
        if (e1 != hipSuccess)
            return hip_fail(h, e1, "derived fields");
        return 0;
    }
    derived_fields(h, uin, de, dn, h->stream);
    HIPTRY(h, hipGetLastError());
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
