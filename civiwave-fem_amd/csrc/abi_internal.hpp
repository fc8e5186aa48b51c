// abi_internal.hpp -- what the C-ABI translation units (abi.cpp: handles, abi_pcg.cpp: apply_keff / block
// Jacobi / dot / solve_pcg, abi_stepper.cpp: the Stepper, abi_explicit.cpp and abi_explicit_{loads,monitors,
// plasticity}.cpp: the explicit stepper (explicit_state.hpp is what those four share), comm.cpp, modal.cpp,
// refine.cpp) share: the HIP error macro, device allocation and upload from the handle's arena (devmem.hpp: dalloc,
// upload, Uploader), the operator apply by the handle's mode (keff_apply, keff_apply_ds, stiffness_only), the scope
// guard of the operator scalars (ScalarScope), vector staging between the caller's layout and the handle's, the PCG
// driver, the steppers' state core (TransientState, abi_transient.cpp), and the host-only pieces of
// cwf_hip_system_create (abi.cpp, tiles.cpp, lattice.cpp; tests/cpp/create_host_test.cpp calls them).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "cwf_internal.hpp"

#define HIPTRY(h, expr)                                                                                        \
    do                                                                                                         \
    {                                                                                                          \
        hipError_t e__ = (expr);                                                                               \
        if (e__ != hipSuccess)                                                                                 \
            return hip_fail((h), e__, #expr);                                                                  \
    } while (0)


namespace cwf
{

template <class T> inline int dalloc(cwf_hip_system *h, T **p, size_t count)
{
    *p = h->mem.alloc<T>(count);
    if (!*p)
        return set_error(h, CWF_ERR_ALLOC, "failed to allocate device buffer",
                         "bytes=" + std::to_string(device_bytes<T>(count)));
    return 0;
}

// The handle's operator on device vectors, FAST or PARITY by its mode: with the scalars of s (the handle's DevSys or
// a copy of it), and with the handle's own
inline void keff_apply_ds(const cwf_hip_system *h, const DevSys &s, const float *x, float *y, bool sanitize,
                          hipStream_t st)
{
    h->mode == CWF_MODE_FAST ? fast_keff_ds(s, x, y, sanitize, st) : parity_keff_ds(s, x, y, sanitize, nullptr, st);
}
inline void keff_apply(const cwf_hip_system *h, const float *x, float *y, hipStream_t st)
{
    keff_apply_ds(h, h->ds, x, y, true, st);
}

// the handle's operator at scalars (1, 0), the handle itself untouched (newmark_stepper.cpp:1051-1053)
inline DevSys stiffness_only(const cwf_hip_system *h)
{
    DevSys s = h->ds;
    s.sK = 1.0;
    s.sM = 0.0;
    return s;
}

// the handle's operator scalars for one scope: the caller's come back on every path out of it
struct ScalarScope
{
    cwf_hip_system *const h;
    const double sK, sM;  // the caller's
    ScalarScope(cwf_hip_system *h, double k, double m) : h(h), sK(h->ds.sK), sM(h->ds.sM)
    {
        h->ds.sK = k;
        h->ds.sM = m;
    }
    ~ScalarScope()
    {
        h->ds.sK = sK;
        h->ds.sM = sM;
    }
    ScalarScope(const ScalarScope &) = delete;
};

// a hipEvent pair on the handle's stream whose elapsed times add up into *ms
struct Stopwatch
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Stopwatch()
    {
        if (e0)
            (void)hipEventDestroy(e0);
        if (e1)
            (void)hipEventDestroy(e1);
    }
    bool make() { return hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess; }
    void start(hipStream_t st) { (void)hipEventRecord(e0, st); }
    void stop(hipStream_t st, double *ms)
    {
        float t = 0.f;
        if (hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
            hipEventElapsedTime(&t, e0, e1) == hipSuccess)
            *ms += t;
    }
};

// the Dirichlet mask can ride in node_part_off's top bits when the offsets leave them free
inline bool ht_off_mask_ok(const std::vector<uint32_t> &npo) { return npo.back() <= cwf::kPartOffBits; }
// ... and then does (the update pass reads the offsets anyway: one 4-B stream less). Returns DevTiles::off_mask
inline int pack_off_mask(std::vector<uint32_t> &npo, const uint32_t *bc_mask, uint64_t N)
{
    if (!ht_off_mask_ok(npo))
        return 0;
    for (uint64_t n = 0; n < N; ++n)
        npo[n] |= (bc_mask[n] & 7u) << 29;
    return 1;
}

template <class T> inline int upload(cwf_hip_system *h, T **dst, const T *src, size_t count)
{
    if (int st = dalloc(h, dst, count))
        return st;
    if (count)
        HIPTRY(h, hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// A create stage's device allocations and uploads: the first failure is kept in st (the message is on the
// handle) and every later call does nothing, so a stage checks st once, before it uses the pointers.
struct Uploader
{
    cwf_hip_system *h;
    int st = 0;
    int check(hipError_t e, const char *what) { return !st && e != hipSuccess ? st = hip_fail(h, e, what) : st; }
    template <class T> T *alloc(size_t count)
    {
        T *p = nullptr;
        st = st ? st : dalloc(h, &p, count);
        return p;
    }
    template <class T> T *zeros(size_t count)
    {
        T *p = alloc<T>(count);
        check(st ? hipSuccess : hipMemset(p, 0, count * sizeof(T)), "hipMemset");
        return p;
    }
    template <class T> T *put(const T *src, size_t count)
    {
        T *p = nullptr;
        st = st ? st : upload(h, &p, src, count);
        return p;
    }
    template <class T> T *put(const std::vector<T> &v) { return put(v.data(), v.size()); }
    // three host planes of n entries each into one device array [3][n]
    template <class T> T *put3(const std::vector<T> (&v)[3], size_t n)
    {
        T *p = alloc<T>(3 * n);
        for (int q = 0; q < 3 && !st; ++q)
            check(hipMemcpy(p + q * n, v[q].data(), n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy");
        return p;
    }
};

// cwf_hip_system_create holds the handle in one of these from allocation to *out = h: every failing exit
// destroys the stream, the pinned block and the device buffers uploaded so far
using HandlePtr = std::unique_ptr<cwf_hip_system, decltype(&cwf_hip_system_destroy)>;

// The FAST K_eff path of a desc with elements (choose_fast_path, abi.cpp). Groups is a wish: a mesh that does not
// group into fans (fan_groups_usable) takes TilesPipe instead.
enum class FastPath
{
    None,       // no elements
    Lattice,    // k_keff_lattice / k_pcg_lattice / k_pcg_resident: structured blocks (lattice.cpp)
    Groups,     // k_keff_groups_pipe: tet fan groups (groups.cpp)
    TilesPipe,  // k_keff_tiles_pipe: per-tet 8-B geometric records, pipelined
    Tiles,      // k_keff_tiles: one tile per workgroup (48-B records, or 8-B ones under CWF_TILE_PIPE=0)
    HexTiles,   // k_keff_hex_tiles
};
struct PathChoice
{
    FastPath path;
    bool owner_renumber;  // a handle that renumbers orders its nodes by (owner tile, Morton), not Morton alone
};
PathChoice choose_fast_path(const cwf_system_desc *d, bool is_lat, bool geo_ok);
bool groups_enabled();
uint32_t group_lanes();
inline bool fan_groups_usable(int status, const GroupTiles &gt) { return status == 0 && gt.tets_per_group >= 3.0; }

// tiles.cpp: the device records of the per-tet / hex tiles. pad_runs (the tet push fold) moves ht.epos with the runs
struct TileRecords
{
    std::vector<uint4> hdr;    // [ntiles] {first element | affine bit 31, #elements, first tile node, #nodes}
    std::vector<uint2> tnode;  // [total] {node | owner bit 31, run begin | run end << 16}
};
TileRecords pack_tile_records(HostTiles &ht, int corners, bool pad_runs, uint32_t slot_budget);

// lattice.cpp: what the lattice layout uploads besides the Lattice itself
std::vector<float> lattice_device_coef(const Lattice &lat);
struct LatticeClasses
{
    std::vector<uint8_t> cls;   // [N] boundary type << 3 | Dirichlet mask
    std::vector<uint32_t> rep;  // [kLatClasses] lowest node of the class, 0xFFFFFFFF: none
    bool uniform = true;        // the lumped mass is a function of the boundary type (else cls / rep are partial)
    bool interior = false;      // a node inside along x, y and z exists; interior_mass is its lumped mass
    float interior_mass = 0.f;
};
LatticeClasses lattice_classes(const Lattice &lat, const uint32_t *bc_mask, const float *lumped_mass);

bool iso_pattern(const double *D);
bool parity_compact_tiles_wanted(const cwf_hip_system *h);
int parity_incidence_slots(cwf_hip_system *h);
int parity_force_buffer(cwf_hip_system *h);
int check_ready(cwf_hip_system *h);
int stage_in(cwf_hip_system *h, const float *src, float *scratch, uint64_t n, int kind, const float **out);
int stage_vec(cwf_hip_system *h, const float *src, float *scratch, int kind, int w, const float **out);
int vec_in(cwf_hip_system *h, const float *src, float *dst, int kind, int w);
int vec_out(cwf_hip_system *h, const float *src, float *dst, int kind, int w);
std::vector<uint32_t> morton_node_order(const double *X, uint64_t N);
// schedule.cpp: the facts a handle's PCG schedule is chosen from (a shard's: with every rank's vote gathered in `all`)
struct ScheduleVote
{
    bool fuse = false, peer = false, resident = false;  // the fused iteration; its in-kernel PEER exchange; the resident solve
};
struct ScheduleFacts
{
    int mode = CWF_MODE_PARITY;
    bool fusable = false;        // a structured block with the fused launch's tables and buffers
    bool grid_covers = false;    // the fused grid runs every work item in one round
    int fused_knob = -1;         // CWF_FUSED: -1 unset, else 0 / 1 / 2
    bool resident_off = false;   // CWF_RESIDENT=0
    bool resident_plan = false;  // a resident plan could be made
    bool sharded = false;
    bool thick_slab = false;     // a shard: it owns at least two node planes
    int group = 1;               // members driven from this process (a LOCAL communicator: every rank)
    bool peer_eligible = false;  // a shard: peer_fused_eligible
    ScheduleVote all;            // a shard: what every rank voted for
};
ScheduleVote own_vote(const ScheduleFacts &f);        // pure: what the handle could run were it alone
SchedulePlan choose_schedule(const ScheduleFacts &f);  // pure: the handle's plan (state, launch, resident)
PcgSchedule solve_schedule(const SchedulePlan &p, uint64_t max_iterations);  // pure: one solve's schedule
int exchange_schedule_code(const SchedulePlan &p);  // cwf_hip_system_exchange_schedule's value for a shard's plan
// plans every member of a group at its first FAST solve (the knobs, the fused grid, the resident plan; shards: the
// collective vote, whose failure is an error); later calls return at once
int plan_schedule(const std::vector<cwf_hip_system *> &g);
// what the handle's solves run (Resident where the plan has it); plans an unplanned handle as its first solve would
PcgSchedule schedule_of(const cwf_hip_system *h);
// sch: the schedule that ran
std::string pcg_error_message(int code, int iter, PcgSchedule sch, std::string *ctx);
// solve_pcg on device buffers for a group (one handle, or every rank of a LOCAL sharded system)
int run_pcg_group(const std::vector<cwf_hip_system *> &g, const std::vector<const float *> &rhs,
                  const cwf_pcg_settings &set, cwf_pcg_telemetry *tel);
int run_pcg(cwf_hip_system *h, const float *rhs_dev, const cwf_pcg_settings &set, cwf_pcg_telemetry *tel);

// abi_transient.cpp: the state core of the two time steppers (cwf_hip_stepper and cwf_hip_explicit derive from it).
// Its buffers live in its own arena: freed with the stepper, not counted by cwf_hip_system_memory.
struct TransientState
{
    cwf_hip_system *sys = nullptr;
    const char *alloc_error = "";  // the stepper's message of a failed allocation
    DeviceArena mem;
    float *u = nullptr, *v = nullptr, *f = nullptr, *bcv = nullptr;  // f32 [D], the handle's node order
    double *lbase = nullptr, *lpat = nullptr;  // set_load_pattern: f64 [D] each, allocated at the first set
    template <class T> int alloc(T **p, size_t count)
    {
        *p = mem.alloc<T>(count);
        return *p ? 0 : set_error(sys, CWF_ERR_ALLOC, alloc_error);
    }
    int alloc_vector(float **p) { return alloc(p, sys->ds.D); }
};
void transient_quiesce(const TransientState &c);  // before the stepper is deleted: its device, its stream drained
// the create tail: u, v, f, bcv zeroed, the desc's external_force and bc_value (either may be NULL) in, one sync
int transient_start(TransientState &c, const float *external_force, const float *bc_value, const char *what);
int transient_form_load(TransientState &c, double scale);  // f = base + scale pattern (stepper_scaled_load)
// an internal vector out / a caller's vector in, after the span check; src / dst NULL: "unknown state field".
// load_scale: f is formed from the pattern at *load_scale first; what: the span's name in the size message
int transient_get(TransientState &c, const float *src, float *out, uint64_t n, int kind,
                  const double *load_scale = nullptr);
int transient_set(TransientState &c, const char *what, float *dst, const float *in, uint64_t n, int kind,
                  bool sync = true);
int transient_set_load_pattern(TransientState &c, const double *base, const double *pattern, uint64_t n);
int transient_time(double now, double dt, double *current_time, double *time_step);

// abi_explicit_monitors.cpp: what cwf_hip_explicit_set_element_monitors refuses of a desc for a handle of E elements, on the
// host alone (no device, no handle): 0, or the error code with the message in *msg and its context lines in *ctx
int element_monitor_refusal(const cwf_explicit_element_monitor_desc &d, uint64_t E, std::string *msg,
                            std::string *ctx);

}  // namespace cwf
