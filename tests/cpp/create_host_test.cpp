// create_host_test.cpp -- the host-only pieces of cwf_hip_system_create (abi_internal.hpp), on descs built here:
// the FAST path choice, the push-run padding of the per-tet tiles and the lattice class table; and the PCG schedule's
// decision table (schedule.cpp's pure functions) with pcg_error_message. No GPU call.
// Built and run by tests/test_host.py (g++, -D__HIP_PLATFORM_AMD__, -lcwf_hip). Prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "abi_internal.hpp"

using namespace cwf;

#define CHECK(cond)                                                                                            \
    do                                                                                                         \
    {                                                                                                          \
        if (!(cond))                                                                                           \
        {                                                                                                      \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);                      \
            std::exit(1);                                                                                      \
        }                                                                                                      \
    } while (0)

namespace
{

// a structured block of nx * ny * nz cells (Kuhn tets or hex8), preprocessed by the library; the desc views it
struct Block
{
    uint64_t N = 0, E = 0;
    uint32_t nn[3] = {0, 0, 0};  // nodes per axis
    std::vector<double> coords, stiffness, mass64;
    std::vector<uint32_t> conn8, mat, mask, off, adj_elem;
    std::vector<uint8_t> adj_local;
    std::vector<float> grads, vol, mass;
    cwf_system_desc desc{};

    uint32_t node(uint32_t i, uint32_t j, uint32_t k) const { return (k * nn[1] + j) * nn[0] + i; }
    bool interior(uint32_t n) const
    {
        const uint32_t i = n % nn[0], j = n / nn[0] % nn[1], k = n / (nn[0] * nn[1]);
        return i && j && k && i + 1 < nn[0] && j + 1 < nn[1] && k + 1 < nn[2];
    }
};

// isotropic Voigt stiffness (E = 30 GPa, nu = 0.2)
void steel(double *D)
{
    const double Em = 30.0e9, nu = 0.2, lam = Em * nu / ((1 + nu) * (1 - 2 * nu)), mu = Em / (2 * (1 + nu));
    for (int i = 0; i < 36; ++i)
        D[i] = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            D[6 * r + c] = lam + (r == c ? 2 * mu : 0.0);
    for (int r = 3; r < 6; ++r)
        D[7 * r] = mu;
}

void make_block(Block &b, uint32_t nx, uint32_t ny, uint32_t nz, bool hex, bool jitter, uint32_t materials)
{
    const double h = 0.1;
    b.nn[0] = nx + 1, b.nn[1] = ny + 1, b.nn[2] = nz + 1;
    b.N = (uint64_t)b.nn[0] * b.nn[1] * b.nn[2];
    b.coords.resize(3 * b.N);
    uint32_t lcg = 12345u;
    for (uint32_t n = 0; n < b.N; ++n)
    {
        const uint32_t ijk[3] = {n % b.nn[0], n / b.nn[0] % b.nn[1], n / (b.nn[0] * b.nn[1])};
        for (int k = 0; k < 3; ++k)
        {
            b.coords[3 * n + k] = h * ijk[k];
            if (jitter && b.interior(n))  // +-0.15 h, interior nodes only
            {
                lcg = lcg * 1664525u + 1013904223u;
                b.coords[3 * n + k] += 0.15 * h * ((double)(lcg >> 8) / (double)(1u << 23) - 1.0);
            }
        }
    }
    static const int kuhn[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
    static const int gmsh[8] = {0, 1, 3, 2, 4, 5, 7, 6};
    std::vector<uint32_t> elems;  // [E][4] or [E][8]
    for (uint32_t k = 0; k < nz; ++k)
        for (uint32_t j = 0; j < ny; ++j)
            for (uint32_t i = 0; i < nx; ++i)
            {
                uint32_t c[8];
                for (int q = 0; q < 8; ++q)
                    c[q] = b.node(i + (q & 1), j + ((q >> 1) & 1), k + ((q >> 2) & 1));
                if (hex)
                    for (int q = 0; q < 8; ++q)
                        elems.push_back(c[gmsh[q]]);
                else
                    for (const auto &t : kuhn)
                        for (int a = 0; a < 4; ++a)
                            elems.push_back(c[t[a]]);
            }
    const int K = hex ? 8 : 4;
    b.E = elems.size() / K;
    b.mat.resize(b.E);
    for (uint64_t e = 0; e < b.E; ++e)
        b.mat[e] = (uint32_t)(e % materials);
    b.stiffness.resize(36 * materials);
    for (uint32_t m = 0; m < materials; ++m)
        steel(&b.stiffness[36 * m]);
    const std::vector<double> density(materials, 2500.0);
    b.grads.resize(24 * b.E);
    b.vol.resize(b.E);
    b.mass64.resize(b.N);
    b.mass.resize(b.N);
    b.off.resize(b.N + 1);
    b.adj_elem.resize(b.E * K);
    b.adj_local.resize(b.E * K);
    b.conn8.resize(8 * b.E);
    const int st = (hex ? cwf_preprocess_hex8 : cwf_preprocess_tets)(
        b.N, b.E, b.coords.data(), elems.data(), b.mat.data(), density.data(), materials, b.grads.data(), b.vol.data(),
        b.mass64.data(), b.mass.data(), b.off.data(), b.adj_elem.data(), b.adj_local.data(), b.conn8.data());
    CHECK(st == 0);
    b.mask.assign(b.N, 0u);
    for (uint32_t n = 0; n < b.N; ++n)
        if (n % b.nn[0] == 0)  // the x = 0 face fixed
            b.mask[n] = 7u;
    cwf_system_desc &d = b.desc;
    d.node_count = b.N;
    d.element_count = b.E;
    d.dof_count = 3 * b.N;
    d.element_connectivity = b.conn8.data();
    d.element_gradients = b.grads.data();
    d.element_volume = b.vol.data();
    d.element_material_index = b.mat.data();
    d.material_stiffness = b.stiffness.data();
    d.material_count = materials;
    d.lumped_mass = b.mass.data();
    d.bc_mask = b.mask.data();
    d.stiffness_scale = 1.0;
    d.mass_factor = 0.0;
    d.reduction_block = 256;
    d.reduction_partials = (d.dof_count + 255) / 256;
    d.mode = CWF_MODE_FAST;
    d.node_coords = b.coords.data();
}

// the two inputs of choose_fast_path as cwf_hip_system_create forms them (every knob unset)
PathChoice choice(const cwf_system_desc &d, bool allow_lattice = true)
{
    const bool hex = d.element_connectivity[4] != 0xFFFFFFFFu;
    Lattice lat;
    const bool is_lat = allow_lattice && d.node_coords && detect_lattice(&d, true, lat);
    const bool geo_ok = d.node_coords && (hex || geometry_matches(&d));
    return choose_fast_path(&d, is_lat, geo_ok);
}

void test_path_choice()
{
    Block kuhn, jit, jit17, hexb;
    make_block(kuhn, 4, 3, 2, false, false, 1);
    make_block(jit, 4, 3, 2, false, true, 1);
    make_block(jit17, 4, 3, 2, false, true, 17);
    make_block(hexb, 3, 2, 2, true, false, 1);
    PathChoice pc = choice(kuhn.desc);
    CHECK(pc.path == FastPath::Lattice && !pc.owner_renumber);
    pc = choice(jit.desc);
    CHECK(pc.path == FastPath::Groups && pc.owner_renumber);
    pc = choice(jit17.desc);
    CHECK(pc.path == FastPath::TilesPipe && !pc.owner_renumber);
    cwf_system_desc nocoords = jit.desc;
    nocoords.node_coords = nullptr;
    pc = choice(nocoords);
    CHECK(pc.path == FastPath::Tiles && !pc.owner_renumber);
    pc = choice(hexb.desc);  // a structured hex block is a lattice first ...
    CHECK(pc.path == FastPath::Lattice && !pc.owner_renumber);
    pc = choice(hexb.desc, false);  // ... and hex tiles otherwise
    CHECK(pc.path == FastPath::HexTiles && pc.owner_renumber);
    cwf_system_desc empty = kuhn.desc;
    empty.element_count = 0;
    CHECK(choose_fast_path(&empty, false, false).path == FastPath::None);
}

void test_push_run_padding()
{
    Block jit;
    make_block(jit, 4, 3, 2, false, true, 1);
    const uint32_t nt = 128, budget = 8u * nt + 2u * nt;
    HostTiles ht;
    CHECK(build_tiles(&jit.desc, ht, nt, 2 * nt) == 0);
    CHECK(ht.ntiles >= 1 && ht.epos.size() == jit.E);
    const TileRecords rec = pack_tile_records(ht, 4, true, budget);
    CHECK(rec.hdr.size() == ht.ntiles && rec.tnode.size() == ht.tile_nodes.size());
    for (uint32_t k = 0; k < ht.ntiles; ++k)
    {
        const uint4 hd = rec.hdr[k];
        CHECK(hd.x == ht.tile_elem_off[k] && hd.x + hd.y == ht.tile_elem_off[k + 1]);
        CHECK(hd.z == ht.tile_node_off[k] && hd.z + hd.w == ht.tile_node_off[k + 1]);
        uint32_t prev_end = 0;
        for (uint32_t q = hd.z; q < hd.z + hd.w; ++q)
        {
            const uint32_t begin = rec.tnode[q].y & 0xffffu, end = rec.tnode[q].y >> 16;
            CHECK(rec.tnode[q].x == ht.tile_nodes[q]);
            CHECK(begin % 2 == 0);                                  // every run starts on an even slot
            CHECK(begin >= prev_end);                               // runs do not overlap
            CHECK(end - begin == ht.csr_off[q + 1] - ht.csr_off[q]);  // one slot per incident (tet, corner)
            prev_end = end;
        }
        CHECK(prev_end <= budget);  // the total stays within the kernel's slot budget
        std::set<uint32_t> used;
        for (uint32_t j = hd.x; j < hd.x + hd.y; ++j)
        {
            const uint2 id = ht.eid[j], ep = ht.epos[j];
            const uint32_t li[4] = {id.x & 0xffffu, id.x >> 16, id.y & 0xffffu, id.y >> 16};
            const uint32_t p[4] = {ep.x & 0xffffu, ep.x >> 16, ep.y & 0xffffu, ep.y >> 16};
            for (int a = 0; a < 4; ++a)
            {
                CHECK(li[a] < hd.w);
                const uint32_t run = rec.tnode[hd.z + li[a]].y;
                CHECK(p[a] >= (run & 0xffffu) && p[a] < (run >> 16));  // inside its node's run
                CHECK(used.insert(p[a]).second);                        // and nobody else's slot
            }
        }
    }
}

void test_lattice_classes()
{
    Block kuhn;
    make_block(kuhn, 4, 3, 2, false, false, 1);
    Lattice lat;
    CHECK(detect_lattice(&kuhn.desc, true, lat));
    CHECK(lat.perm.empty() && lat.nx == 5 && lat.ny == 4 && lat.nz == 3);
    const LatticeClasses lc = lattice_classes(lat, kuhn.mask.data(), kuhn.mass.data());
    CHECK(lc.uniform && lc.cls.size() == kuhn.N && lc.rep.size() == kLatClasses);
    std::vector<uint32_t> lowest(kLatClasses, 0xFFFFFFFFu);
    const auto side = [](uint32_t a, uint32_t na) { return a == 0 ? 0u : a + 1 == na ? 2u : 1u; };
    for (uint32_t n = 0; n < kuhn.N; ++n)
    {
        const uint32_t i = n % lat.nx, j = n / lat.nx % lat.ny, k = n / (lat.nx * lat.ny);
        const uint32_t type = side(i, lat.nx) + 3 * side(j, lat.ny) + 9 * side(k, lat.nz);
        CHECK(lc.cls[n] == (type << 3 | kuhn.mask[n]));
        if (lowest[lc.cls[n]] == 0xFFFFFFFFu)
            lowest[lc.cls[n]] = n;
    }
    for (uint32_t c = 0; c < kLatClasses; ++c)
        CHECK(lc.rep[c] == lowest[c]);  // the lowest node of a represented class, none otherwise
    CHECK(lc.interior && lc.interior_mass == kuhn.mass[kuhn.node(1, 1, 1)]);
}

// ---- the PCG schedule (schedule.cpp): facts -> plan -> one solve's schedule -----------------------------------
using S = PcgSchedule;

// an unsharded structured block whose fused grid covers its work items and whose resident plan fits, no knob set
ScheduleFacts block_facts()
{
    ScheduleFacts f;
    f.mode = CWF_MODE_FAST;
    f.fusable = f.grid_covers = f.resident_plan = true;
    return f;
}
// a PEER slab shard of the same (one member per process), every rank voting for everything
ScheduleFacts shard_facts()
{
    ScheduleFacts f = block_facts();
    f.sharded = f.thick_slab = f.peer_eligible = true;
    f.all = ScheduleVote{true, true, true};
    return f;
}
// the plan's launch-per-iteration schedule and whether the resident solve replaces it
void check_plan(const ScheduleFacts &f, S launch, bool resident)
{
    const SchedulePlan p = choose_schedule(f);
    CHECK(p.state == SchedulePlan::Decided && p.launch == launch && p.resident == resident);
    CHECK(solve_schedule(p, 1) == (resident ? S::Resident : launch));
}

void test_schedule_choice()
{
    const uint64_t lim = 1u << 24;
    ScheduleFacts f;  // a PARITY handle, whatever else holds
    check_plan(f, S::Parity, false);
    f = block_facts();
    f.mode = CWF_MODE_PARITY;
    check_plan(f, S::Parity, false);
    f = shard_facts();
    f.mode = CWF_MODE_PARITY;
    check_plan(f, S::Parity, false);
    CHECK(exchange_schedule_code(choose_schedule(f)) == -1);  // PARITY shards take no vote
    f = block_facts();  // a non-lattice FAST handle
    f.fusable = f.grid_covers = f.resident_plan = false;
    check_plan(f, S::TwoKernel, false);
    check_plan(block_facts(), S::Fused, true);  // the grid covers the items
    f = block_facts();                          // it does not: never resident, even where a plan would fit
    f.grid_covers = false;
    check_plan(f, S::TwoKernel, false);
    // CWF_FUSED unset / 0 / 1 / 2 x CWF_RESIDENT=0 x the grid covering the items: any CWF_FUSED turns resident off
    for (int knob = -1; knob <= 2; ++knob)
        for (int off = 0; off < 2; ++off)
            for (int covers = 0; covers < 2; ++covers)
            {
                f = block_facts();
                f.fused_knob = knob;
                f.resident_off = off != 0;
                f.grid_covers = covers != 0;
                const bool fuse = knob == 2 || (knob != 0 && covers);
                check_plan(f, fuse ? S::Fused : S::TwoKernel, fuse && knob < 0 && !off);
                CHECK(choose_schedule(f).fused_knob == knob);
            }
    f = block_facts();  // no resident plan could be made
    f.resident_plan = false;
    check_plan(f, S::Fused, false);

    // shards: this rank's vote, then the plan from every rank's
    f = shard_facts();
    ScheduleVote v = own_vote(f);
    CHECK(v.fuse && v.peer && v.resident);
    check_plan(f, S::FusedPeer, true);
    f.thick_slab = false;  // a thin slab votes against fusing, and so against everything
    v = own_vote(f);
    CHECK(!v.fuse && !v.peer && !v.resident);
    f.all = v;
    check_plan(f, S::TwoKernel, false);
    f = shard_facts();  // a LOCAL group of 2: fused with an exchange step, never in-kernel or resident
    f.group = 2;
    v = own_vote(f);
    CHECK(v.fuse && !v.peer && !v.resident);
    f.all = v;
    check_plan(f, S::Fused, false);
    f = shard_facts();  // one rank lacks PEER eligibility
    f.all.peer = false;
    check_plan(f, S::Fused, true);
    f.peer_eligible = false;  // (this one)
    CHECK(own_vote(f).fuse && !own_vote(f).peer && own_vote(f).resident);
    f = shard_facts();  // one rank lacks a resident plan
    f.all.resident = false;
    check_plan(f, S::FusedPeer, false);
    f.resident_plan = false;  // (this one)
    CHECK(own_vote(f).fuse && own_vote(f).peer && !own_vote(f).resident);
    f = shard_facts();  // one rank cannot fuse: nobody does, whatever this rank could
    f.all = ScheduleVote{false, false, false};
    check_plan(f, S::TwoKernel, false);
    f.all = ScheduleVote{false, true, true};  // (votes that cannot be cast: still nothing without the fused iteration)
    check_plan(f, S::TwoKernel, false);
    f = shard_facts();  // an explicit CWF_FUSED, or CWF_RESIDENT=0, on a shard: no resident vote
    f.fused_knob = 1;
    CHECK(own_vote(f).peer && !own_vote(f).resident);
    f = shard_facts();
    f.resident_off = true;
    CHECK(own_vote(f).peer && !own_vote(f).resident);

    // the resident solve counts at most 2^24 iterations: a longer solve takes the launch-per-iteration schedule
    SchedulePlan p = choose_schedule(shard_facts());  // PEER in-kernel exchange underneath
    CHECK(solve_schedule(p, lim) == S::Resident && solve_schedule(p, lim + 1) == S::FusedPeer);
    p = choose_schedule(block_facts());  // ... and without
    CHECK(solve_schedule(p, lim) == S::Resident && solve_schedule(p, lim + 1) == S::Fused);
    f = block_facts();
    f.resident_plan = false;
    p = choose_schedule(f);
    CHECK(solve_schedule(p, lim) == S::Fused && solve_schedule(p, lim + 1) == S::Fused);

    // cwf_hip_system_exchange_schedule of a shard: -1 until the vote, then 0 two kernels / 1 fused / 2 in-kernel / 3 resident
    p = SchedulePlan{};
    CHECK(exchange_schedule_code(p) == -1);
    p.state = SchedulePlan::Local;  // its own half planned (a query before the first solve)
    p.launch = S::Fused;
    CHECK(exchange_schedule_code(p) == -1);
    f = shard_facts();
    CHECK(exchange_schedule_code(choose_schedule(f)) == 3);
    f.all.resident = false;
    CHECK(exchange_schedule_code(choose_schedule(f)) == 2);
    f.all.peer = false;
    CHECK(exchange_schedule_code(choose_schedule(f)) == 1);
    f.all.resident = true;  // resident over the exchange-step fused iteration
    CHECK(exchange_schedule_code(choose_schedule(f)) == 3);
    f.all = ScheduleVote{};
    CHECK(exchange_schedule_code(choose_schedule(f)) == 0);
}

void test_pcg_error_message()
{
    std::string ctx;
    // CWF_ERR_HIP: the resident solve's phase barrier after a Resident solve, the PARITY streamed fold otherwise
    CHECK(pcg_error_message(CWF_ERR_HIP, 7, S::Resident, &ctx) == "resident solve: a workgroup missed the phase barrier");
    CHECK(ctx == "phase=7");
    CHECK(pcg_error_message(CWF_ERR_HIP, 7, S::Parity, &ctx) == "PARITY streamed scalar fold timed out");
    CHECK(ctx == "iteration=7");
    for (S sch : {S::Parity, S::TwoKernel, S::Fused, S::FusedPeer, S::Resident})  // the other codes: as they were
    {
        CHECK(pcg_error_message(CWF_ERR_DENOM_ZERO, 3, sch, &ctx) == "CG denominator approached zero" && ctx == "iteration=3");
        CHECK(pcg_error_message(CWF_ERR_COMM, 4, sch, &ctx) == "peer exchange timed out" && ctx == "step=4");
        CHECK(pcg_error_message(CWF_ERR_RHO_ZERO, -1, sch, &ctx) == "preconditioner produced near-zero rho" && ctx == "rho~0");
        CHECK(pcg_error_message(CWF_ERR_RHO_ZERO, 5, sch, &ctx) == "CG rho approached zero" && ctx == "iteration=5");
    }
}

}  // namespace

int main()
{
    test_path_choice();
    test_push_run_padding();
    test_lattice_classes();
    test_schedule_choice();
    test_pcg_error_message();
    std::puts("ok");
    return 0;
}
