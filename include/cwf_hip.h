/*
 * cwf_hip.h -- C-ABI of the MI355X (gfx950) matrix-free Newmark/PCG hot path.
 *
 * Drop-in boundary for CiviWave-FEM's L4 solver core. Every entry point below replaces a
 * reference C++ interface (cited as /root/reference file:line); plain pointers and sizes
 * only, no torch or C++ types, no exceptions. Return value: 0 on success, a negative
 * cwf_status on failure; cwf_hip_last_error()/cwf_hip_last_context() then hold the
 * reference's message text and breadcrumb (e.g. "CG denominator approached zero",
 * "iteration=12").
 *
 * Threading: one handle = one device + one HIP stream, externally synchronised
 * (the reference Stepper is single-threaded, newmark_stepper.hpp:92). Distinct handles may
 * run concurrently on distinct threads.
 *
 * Pointer kinds: every vector argument is host memory when `ptr_kind == CWF_PTR_HOST`
 * (copied in/out, call is synchronous) or device memory (HBM) when CWF_PTR_DEVICE
 * (used in place, the call still returns after the work completes on the handle's stream).
 */
#ifndef CWF_HIP_H
#define CWF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CWF_HIP_ABI_VERSION 1

typedef enum cwf_status
{
    CWF_OK = 0,
    CWF_ERR_SIZE = -1,           /* pcg.cpp:82-125 "... size mismatch" */
    CWF_ERR_NODE_RANGE = -2,     /* pcg.cpp:609-613 "element connectivity references node out of range" */
    CWF_ERR_MATERIAL_RANGE = -3, /* pcg.cpp:566-570 "element references material out of range" */
    CWF_ERR_MATERIALS = -4,      /* pcg.cpp:126-129 "materials table is empty" */
    CWF_ERR_REDUCTION = -5,      /* pcg.cpp:130-137 reduction_block / reduction_partials == 0 */
    CWF_ERR_MAX_ITERATIONS = -6, /* pcg.cpp:739-742 "max_iterations must be >= 1" */
    CWF_ERR_RHO_ZERO = -7,       /* pcg.cpp:810-813, 889-892 */
    CWF_ERR_DENOM_ZERO = -8,     /* pcg.cpp:846-849 "CG denominator approached zero" */
    CWF_ERR_ALLOC = -9,          /* pcg.cpp:65-68 workspace allocation failure */
    CWF_ERR_HIP = -10,           /* HIP runtime error (message holds hipGetErrorString) */
    CWF_ERR_ARGUMENT = -11,      /* NULL handle / pointer */
    CWF_ERR_COMM = -12,          /* RCCL / communicator failure */
    CWF_ERR_UNSUPPORTED = -13,
    CWF_ERR_IO = -14,            /* vtu_writer.cpp / probe_logger.cpp / config / mesh file errors */
    CWF_ERR_INDEX = -15,         /* probe_logger.cpp:116-119 "probe index out of range" */
    CWF_ERR_PARSE = -16          /* config.cpp / mesh.cpp parse and validation errors */
} cwf_status;

typedef enum cwf_ptr_kind
{
    CWF_PTR_HOST = 0,
    CWF_PTR_DEVICE = 1
} cwf_ptr_kind;

/* Arithmetic mode. PARITY reproduces the reference fold order bit for bit (fp64 element math,
 * 256-DOF chunked sequential fp64 dots). FAST: fp32 element math, fp64 tree reductions,
 * tolerance-checked against the oracle. Both consume the same inputs. */
typedef enum cwf_mode
{
    CWF_MODE_PARITY = 0,
    CWF_MODE_FAST = 1
} cwf_mode;

/* Mirrors cwf::gpu::pcg::MatrixFreeSystem (include/cwf/gpu/pcg.hpp:67-86) plus the packed
 * adjacency of cwf::mesh::pack::AdjacencyBuffers (include/cwf/mesh/pack.hpp:120-125).
 * All pointers are host memory; the handle copies them to HBM at create time. */
/* cwf_system_desc.reserved flags. A CWF_MODE_FAST handle renumbers its nodes internally along a Morton
 * curve of node_coords (locality of the tile gathers and partial stores; 1.8x on a permuted mesh), and
 * converts every vector at the boundary, so callers always see their own node order. KEEP_NODE_ORDER
 * disables that: required for handles that are attached as shards (local numbering = the halo plan). */
#define CWF_DESC_KEEP_NODE_ORDER 1

typedef struct cwf_system_desc
{
    uint64_t node_count;
    uint64_t element_count;
    uint64_t dof_count;                 /* must equal 3 * node_count */
    const uint32_t *element_connectivity; /* [element_count * 8], tets use slots 0..3 */
    const float *element_gradients;     /* [element_count * 24], grad N_a xyz, a = 0..7 */
    const float *element_volume;        /* [element_count] */
    const uint32_t *element_material_index; /* [element_count] */
    const double *material_stiffness;   /* [material_count * 36], ElasticProperties::stiffness */
    uint64_t material_count;
    const float *lumped_mass;           /* [node_count] */
    const uint32_t *bc_mask;            /* [node_count], bit0/1/2 = x/y/z constrained */
    const uint32_t *adjacency_offsets;  /* [node_count + 1] or NULL (built from connectivity) */
    const uint32_t *adjacency_elements; /* [offsets[N]] ascending element index per node, or NULL */
    const uint8_t *adjacency_local;     /* [offsets[N]] local slot 0..3, or NULL */
    double stiffness_scale;             /* 1 + a1 * beta_R */
    double mass_factor;                 /* a0 + a1 * alpha_R */
    uint64_t reduction_block;           /* 256 in the reference (pack.hpp:183) */
    uint64_t reduction_partials;        /* >= ceil(dof_count / reduction_block) */
    int32_t mode;                       /* cwf_mode */
    int32_t reserved;                   /* flags: CWF_DESC_KEEP_NODE_ORDER */
    const double *node_coords;          /* [node_count * 3] or NULL: only used to order FAST-mode tiles */
} cwf_system_desc;

/* PcgSettings (pcg.hpp:115-120) */
typedef struct cwf_pcg_settings
{
    uint64_t max_iterations;
    double relative_tolerance;
    int32_t warm_start;
    int32_t check_interval; /* iterations enqueued between host convergence checks; 0 = auto */
} cwf_pcg_settings;

/* PcgTelemetry (pcg.hpp:125-133) */
typedef struct cwf_pcg_telemetry
{
    uint64_t iterations;
    double residual_norm;
    double rhs_norm;
    double alpha_last;
    double beta_last;
    int32_t converged;
    int32_t reserved;
} cwf_pcg_telemetry;

typedef struct cwf_hip_system cwf_hip_system;

/* Library / device info. */
int cwf_hip_abi_version(void);
int cwf_hip_device_count(int *count);
const char *cwf_hip_last_error(const cwf_hip_system *h);   /* h may be NULL: last create error */
const char *cwf_hip_last_context(const cwf_hip_system *h);

/* Create / destroy: replaces building a MatrixFreeSystem over packed buffers
 * (newmark_stepper.cpp:1034-1049) and DeviceBufferArena::create (device_buffers.cpp:132). */
int cwf_hip_system_create(const cwf_system_desc *desc, int device, cwf_hip_system **out);
void cwf_hip_system_destroy(cwf_hip_system *h);
/* update stiffness_scale / mass_factor (newmark_stepper.cpp:1322-1326) */
int cwf_hip_system_set_scalars(cwf_hip_system *h, double stiffness_scale, double mass_factor);
int cwf_hip_system_set_mode(cwf_hip_system *h, int mode);
/* bytes of HBM held by the handle */
int cwf_hip_system_memory(const cwf_hip_system *h, uint64_t *bytes);
/* STREAM-like device copy (16-B lanes, grid-stride) on `device`: *gbs = (read + write bytes) / time. The
 * measured HBM ceiling bench.py reports beside the 8 TB/s spec. No reference counterpart. */
int cwf_hip_bandwidth_probe(int device, uint64_t bytes, int reps, double *gbs);
/* Algorithmic (compulsory) HBM bytes of one PCG-loop K_eff launch (measurement support, not a
 * reference interface): `layout_bytes` = every array the handle's own K_eff kernel touches, counted
 * once (the headline roofline uses the build's own layout when it reads less);
 * `reference_layout_bytes` = 32 N + 72 E, the same SpMV over the reference's packed layout. */
int cwf_hip_system_keff_traffic(const cwf_hip_system *h, uint64_t *layout_bytes, uint64_t *reference_layout_bytes);
/* Name of the kernel the handle's K_eff launches in its current mode ("k_keff_lattice", "k_keff_groups_pipe",
 * "k_keff_tiles_pipe", "k_keff_tiles", "k_keff_hex_tiles" or "k_keff_parity"); NULL for a NULL handle. */
const char *cwf_hip_system_keff_kernel(const cwf_hip_system *h);
/* Diagnostic: the PCG schedule a sharded handle's FAST solves run, decided collectively at its first solve:
 * -1 not decided yet (or not sharded), 0 the two-kernel iteration (two exchange steps per iteration), 1 the fused
 * lattice iteration with one exchange step per iteration, 2 the fused iteration exchanging inside its launches
 * (PEER: the Ap send rows, rank totals and epoch flags pushed by the launch itself, no exchange launch), 3 the
 * resident solve (PEER slab shards: every iteration in one launch per solve, its surface records and rank totals
 * stored into the peers' mailboxes by the kernel). */
int cwf_hip_system_exchange_schedule(const cwf_hip_system *h);
/* 16 hex digits: a hash of the source files and build flags of the translation unit that holds that kernel
 * (csrc/Makefile FAST_SRC / PARITY_SRC), so a committed PMC profile can be matched to the code that ran */
const char *cwf_hip_system_keff_source_hash(const cwf_hip_system *h);
/* Structured-block introspection (host only, no device; not a reference interface): whether a FAST handle
 * created from the tet4 `desc` runs the structured Kuhn-block stencil (lattice.cpp; native hex8 blocks run their
 * own 27-point stencil and are not described here). Returns 1 and fills dims (nodes per
 * axis; bit 31 of dims[0]: the stencil pairs S_(-d) = S_d), coef (CWF_LATTICE_COEFS floats, row-major 3x3 blocks
 * unscaled by stiffness_scale: the 15 interior stencil blocks, then the 46 cell-pair blocks) and plane ([dims[2]] storage index of node (0, 0, k); NULL: not wanted) when it does, 0 when it
 * does not, a negative cwf_status code on bad arguments. `renumber` != 0 allows the lexicographic renumbering a handle
 * without CWF_DESC_KEEP_NODE_ORDER may apply. */
#define CWF_LATTICE_COEFS 549
int cwf_lattice_describe(const cwf_system_desc *desc, int renumber, uint32_t dims[3], float *coef, uint32_t *plane);
/* The same for layered blocks (host only, no device): a structured tet4 or hex8 block whose material is constant
 * within every k-layer of cells (cell layer kc: the cells between node planes kc and kc + 1) runs the per-plane
 * stencil tables of k_keff_lattice_layered; cwf_lattice_describe returns 0 for it. Returns 1 for a layered or a
 * one-material lattice and fills dims (nodes per axis, no flag bits) and info = {materials, plane classes, 1 when
 * hex8, 1 when the stencil pairs S_(-d) = S_d (one material only)}; 0 when the desc is no lattice (materials varying
 * inside a cell layer, more than CWF_LATTICE_MAX_MATERIALS materials or CWF_LATTICE_MAX_PLANE_CLASSES classes among
 * the reasons); CWF_ERR_SIZE when a wanted array's capacity is too small (dims and info are filled, so a caller can
 * size and call again); another negative cwf_status on bad arguments. Every array may be NULL (not wanted):
 *   plane [dims[2]] storage index of node (0, 0, k), plane_class [dims[2]], layer_material [dims[2] - 1] the desc's
 *   material index of each cell layer (capacity plane_capacity entries each);
 *   class_pair [2 classes] (material below, material above) of each class -- the end planes take their one layer
 *   twice --, class_coef [classes][offsets][3][3] row-major stencil blocks unscaled by stiffness_scale, offsets = 15
 *   (tet4) or 27 (hex8): S_d = sum over the node's corner positions c of Kc^m[c][c + d], m the material below for
 *   corners with z-bit 1 and above for z-bit 0, fp64 rounded to f32 once (capacity class_capacity classes);
 *   material_ids [materials] the desc's material index of each material slot, pair_coef [materials][pairs][3][3] the
 *   cell-pair blocks of each slot, pairs = 46 (tet4) or 64 (hex8) (capacity material_capacity slots).
 * A one-material block has one class whose tables are cwf_lattice_describe's, bit for bit. */
#define CWF_LATTICE_MAX_MATERIALS 8
#define CWF_LATTICE_MAX_PLANE_CLASSES 16
int cwf_lattice_describe_layers(const cwf_system_desc *desc, int renumber, uint32_t dims[3], uint32_t info[4],
                                uint32_t plane_capacity, uint32_t *plane, uint32_t *plane_class,
                                uint32_t *layer_material, uint32_t class_capacity, uint32_t *class_pair,
                                float *class_coef, uint32_t material_capacity, uint32_t *material_ids,
                                float *pair_coef);

/* Live kernel timing (measurement support, not a reference interface): when enabled, every
 * K_eff launch inside solve_pcg / stepper_step is bracketed by hipEvents on the handle's stream;
 * cwf_hip_system_timing returns the summed device time (ms) and launch count of the launches that
 * did work, and resets the accumulators. `enabled` > 1 samples every enabled-th launch (iteration
 * index multiple of it), so the event markers do not sit between every pair of kernels. */
int cwf_hip_system_set_timing(cwf_hip_system *h, int enabled);
int cwf_hip_system_timing(cwf_hip_system *h, double *keff_ms, uint64_t *keff_launches);
/* Standalone timed K_eff: `reps` launches of the PCG-loop SpMV (no sanitize) on device x -> y,
 * bracketed by one hipEvent pair; *avg_ms = elapsed / reps. */
int cwf_hip_keff_timed(cwf_hip_system *h, const float *x_dev, float *y_dev, int reps, double *avg_ms);

/* cwf::gpu::pcg::apply_keff (pcg.hpp:161-163, pcg.cpp:505-694): y = K_eff x with
 * Dirichlet identity rows. n = dof_count. */
int cwf_hip_apply_keff(cwf_hip_system *h, const float *x, float *y, uint64_t n, int ptr_kind);

/* cwf::gpu::pcg::build_block_jacobi_inverse (pcg.hpp:226-227, pcg.cpp:479-503):
 * inv_out[node*9 + 3*i + j], row-major f32. n = node_count * 9. This is the reference's inverse in
 * every mode (constrained rows = identity). A FAST solve applies a symmetrised, 16-B-packed form of
 * it instead; cwf_hip_fast_block_inverse exports that operator. */
int cwf_hip_build_block_jacobi_inverse(cwf_hip_system *h, float *inv_out, uint64_t n, int ptr_kind);

/* The preconditioner a FAST solve actually applies (no reference counterpart): the block inverse
 * above, symmetrised (upper triangle), restricted to the free axes (constrained rows and columns 0:
 * z and r are 0 there) and dequantised from the update pass's 16-B record (blockinv_pack.hpp).
 * inv_out as above (n = node_count * 9); packed_out (nullable, host) receives the 16-B records,
 * [node_count * 4] u32; *fallback_nodes (nullable) counts the nodes whose block is applied in fp32. */
int cwf_hip_fast_block_inverse(cwf_hip_system *h, float *inv_out, uint64_t n, int ptr_kind, uint32_t *packed_out,
                               uint64_t *fallback_nodes);

/* Host restatement of that packing for one node (the same code the device runs): v = the block's
 * upper triangle {a00 a01 a02 a11 a12 a22}, mask bit k = axis k constrained. Writes the 16-B record
 * (w[4]) and the applied upper triangle (d[6]); returns 1 for a packed block, 0 for an fp32 fallback. */
int cwf_pack_block_inverse(const float *v, uint32_t mask, uint32_t *w, float *d);

/* dot_accumulate (pcg.cpp:170-207): chunked fp64 dot of two f32 DOF vectors. partials may be
 * NULL; otherwise [reduction_partials] chunk partials are written (host or device by ptr_kind). */
int cwf_hip_dot(cwf_hip_system *h, const float *a, const float *b, uint64_t n, int ptr_kind, double *out,
                double *partials);

/* cwf::gpu::pcg::solve_pcg (pcg.hpp:210-212, pcg.cpp:696-918). x_inout is the warm start
 * (settings->warm_start) and receives the solution; residual_out (nullable) receives r. */
int cwf_hip_solve_pcg(cwf_hip_system *h, const float *rhs, const cwf_pcg_settings *settings, float *x_inout,
                      float *residual_out, uint64_t n, int ptr_kind, cwf_pcg_telemetry *telemetry);

/* Residual history of the last solve_pcg (|r| after each iteration, entry 0 = initial),
 * up to `capacity` entries. Returns the number written via *count. */
int cwf_hip_residual_history(cwf_hip_system *h, double *out, uint64_t capacity, uint64_t *count);

/* ---------------------------------------------------------------------------------------
 * Modal analysis (no reference counterpart): the `modes` lowest eigenpairs of K phi = lambda M phi, K the
 * handle's stiffness, M its lumped mass, Dirichlet DOFs held at zero. Subspace iteration with Rayleigh-Ritz
 * (Bathe) over a block of `block` vectors: each outer iteration solves (K + shift M) xbar_j = M x_j with the
 * handle's own PCG, in whatever schedule the handle's solves take, projects K and M onto the block on the device
 * (fp64 Gram matrices), solves the small problem on the host and rotates the block. A FAST tet4 handle ends with one
 * more Rayleigh-Ritz step in the PARITY operator's fp64 element math, so the eigenvalues returned are K's, not those
 * of FAST's f32 approximation of it (its PARITY node tiles are built at the first such call). For the duration of the call the
 * handle runs with scalars (1, shift); the caller's scalars are back on every return, errors included.
 * shift > 0 moves the spectrum, (K + shift M) phi = (lambda + shift) M phi, and makes a structure without enough
 * supports solvable; shift = 0 needs K definite on the free DOFs. A sharded handle (one attached to a communicator)
 * is refused with CWF_ERR_UNSUPPORTED: modal analysis across shards is not built.
 * ------------------------------------------------------------------------------------- */
#define CWF_MODAL_MAX_BLOCK 32
typedef struct cwf_modal_settings
{
    uint32_t modes, block, max_outer, reserved; /* block 0 = min(2 modes, modes + 8); max_outer 0 = 40; reserved
                                                   0 (bit 0, evaluation only: project K with `block` extra operator
                                                   applies per outer iteration instead of reusing the solves'
                                                   right-hand sides) */
    double tolerance, shift;                    /* tolerance 0 = 1e-6: largest relative change of the `modes`
                                                   lowest Ritz values lambda + shift between outer iterations */
    cwf_pcg_settings pcg; /* inner solves; relative_tolerance 0 = 1e-6, max_iterations 0 = 20000; warm_start is
                             the solver's own business (Ritz-scaled starts) and is ignored */
} cwf_modal_settings;
typedef struct cwf_modal_telemetry
{
    uint32_t outer_iterations, converged, block, reserved; /* converged 0 at max_outer is not an error */
    uint64_t pcg_iterations;                               /* over every inner solve */
    double max_change, solve_ms, block_ms; /* hipEvent time in the solves / in gram + fold + rotate */
} cwf_modal_telemetry;
/* eigenvalues [modes] ascending, fp64 (lambda_i = Ritz value - shift). modes_out (nullable) [modes * 3N], mode i at
 * [i * 3N], in the caller's node order, host or device by ptr_kind: M-orthonormal, constrained DOFs exactly 0, each
 * signed so that its component of largest magnitude (ties: the lowest DOF) is positive. The same handle and
 * settings give the same bits on every call. Errors: CWF_ERR_ARGUMENT naming the field for modes == 0, block <
 * modes, block > CWF_MODAL_MAX_BLOCK, shift < 0, tolerance < 0, 3N < block or a NULL pointer; CWF_ERR_UNSUPPORTED
 * for a sharded handle; a PCG failure keeps its code and text, its context extended by "outer=<i>" and
 * "column=<j>"; CWF_ERR_DENOM_ZERO "Ritz mass matrix is not positive definite" when the block lost rank. */
int cwf_hip_modal_solve(cwf_hip_system *h, const cwf_modal_settings *s, double *eigenvalues, float *modes_out,
                        int ptr_kind, cwf_modal_telemetry *tel);
/* G [qa x qb] row-major (host, fp64) = A^T W B for two blocks of contiguous f32 [3N] columns (column j at A + j 3N;
 * host or device by ptr_kind, caller's node order), 1 <= qa, qb <= CWF_MODAL_MAX_BLOCK. W = I, or with
 * mass_weighted the lumped mass on free DOFs and 0 on constrained ones. Products and sums are fp64; the rows are cut
 * into fixed chunks folded in ascending order, so the bits depend on the inputs alone. */
int cwf_hip_block_gram(cwf_hip_system *h, const float *A, uint32_t qa, const float *B, uint32_t qb,
                       int mass_weighted, double *G, int ptr_kind);
/* X_out [q_out columns] = X [q_in columns] Q, Q [q_in x q_out] row-major host fp64: fp64 accumulation rounded to f32
 * once; MX_out (nullable) = W X_out with the mass weight above (constrained rows 0). Out of place: X_out and MX_out
 * must not overlap X. */
int cwf_hip_block_rotate(cwf_hip_system *h, const float *X, uint32_t q_in, const double *Q, uint32_t q_out,
                         float *X_out, float *MX_out, int ptr_kind);

/* ---------------------------------------------------------------------------------------
 * Refined static solve (no reference counterpart): K_eff x = b to a tolerance on the TRUE residual
 * |b - K_eff x| / |b|, evaluated in fp64. cwf_hip_solve_pcg stops on the recurrence residual of an f32 iteration,
 * and f32 storage of x bounds the true residual at about cond(K) * 6e-8 however small the tolerance. Here x and b are
 * fp64 and classical iterative refinement runs around the handle's own PCG: each outer iteration forms
 * r = b - K_eff x on the device (fp64 element math on the handle's f32 element records, the PARITY operator's fold
 * order, no atomics: the same inputs give the same bits), scales it by a power of two into b's binade (the PCG's
 * guards are absolute), solves K_eff d = f32(2^e r) with an ordinary solve in the handle's mode and schedule, and
 * adds 2^(-e) d. Dirichlet DOFs: x_c = b_c exactly; a constrained row's residual is 0 and a constrained DOF enters
 * the operator as 0, as in the reference. |b| is taken over the free DOFs. The handle's mode and scalars are not
 * changed, and its own solves return afterwards what they returned before. tet4 handles of both modes (the PARITY
 * node tiles are built at the first such call); CWF_ERR_UNSUPPORTED for a handle attached to a communicator and for
 * a hex8 handle (no fp64 hex8 operator on the device).
 * ------------------------------------------------------------------------------------- */
typedef struct cwf_refine_settings
{
    uint32_t max_outer;          /* corrections at most; 0 -> 12, at most 31 */
    double relative_tolerance;   /* on the true fp64 residual |b - K_eff x| / |b|; 0 -> 1e-10 */
    double stagnation_ratio;     /* stop when |r_k| > ratio |r_(k-1)|; 0 -> 0.5 */
    cwf_pcg_settings inner;      /* inner.relative_tolerance 0 -> 1e-4, inner.max_iterations 0 -> 20000;
                                    inner.warm_start is ignored */
    int32_t warm_start;          /* x_inout holds a start value */
    int32_t reserved;
} cwf_refine_settings;
typedef struct cwf_refine_telemetry
{
    uint32_t outer_iterations;   /* corrections applied */
    uint64_t inner_iterations;   /* over every inner solve */
    double residual_norm, rhs_norm; /* fp64, true: of the returned x, and |b| over the free DOFs */
    int32_t converged, stagnated;   /* neither at max_outer; stagnated is reported, not an error */
    double history[32];          /* |r| before each inner solve, then the final one: outer_iterations + 1 entries */
    double residual_ms, solve_ms; /* hipEvent time in the fp64 kernels / in the inner solves */
} cwf_refine_telemetry;
/* rhs and x_inout are fp64 [n = 3N] in the caller's node order, host or device by ptr_kind; s == NULL: the defaults.
 * Stops converged (|r| <= tol |b|), stagnated (the rule above; the iterate with the smaller residual is returned) or
 * at max_outer; all three return CWF_OK. An inner solve that stops at its max_iterations still gave a correction and is
 * judged by the stagnation rule. A breakdown of an inner solve (CWF_ERR_RHO_ZERO, CWF_ERR_DENOM_ZERO) is the call's
 * status, its context extended by "outer=<k>"; x_inout then holds the iterate before that solve. |b| = 0 returns
 * the prescribed values, converged, with no inner solve. */
int cwf_hip_solve_refined(cwf_hip_system *h, const double *rhs, const cwf_refine_settings *s, double *x_inout,
                          uint64_t n, int ptr_kind, cwf_refine_telemetry *tel);
/* r_out (nullable) = b - K_eff x in fp64 with the handle's current scalars, *norm_out (nullable) = |r|: the kernel
 * of the refined solve on its own. The norm is folded from one share per node in a tree that depends on N alone. */
int cwf_hip_residual_f64(cwf_hip_system *h, const double *rhs, const double *x, double *r_out, uint64_t n,
                         int ptr_kind, double *norm_out);
/* Measurement support: `reps` launches of the fp64 residual's tile kernel alone (no norm fold, no copies) over the
 * handle's workspace vectors, bracketed by one hipEvent pair; *avg_ms = elapsed / reps. The yardstick is
 * cwf_hip_keff_timed on a PARITY handle of the same mesh: the same tile walk with f32 vectors. */
int cwf_hip_residual_f64_timed(cwf_hip_system *h, int reps, double *avg_ms);
/* Host only: the e with 2^e residual_norm in (rhs_norm / 2, 2 rhs_norm), the refined solve's scale. 0 for a zero
 * residual; a subnormal residual is counted from its leading bit; rhs_norm == 0 (only prescribed values load the
 * system) scales to the binade of 1. */
int cwf_refine_scale_exponent(double residual_norm, double rhs_norm);

/* ---------------------------------------------------------------------------------------
 * Newmark stepper: cwf::gpu::newmark::Stepper (newmark_stepper.hpp:92-190). Device-resident
 * node state (u, v, a, predictor, external force, bc values); one step = predictor -> RHS
 * (+ beta_R * K * d when beta_R != 0) -> Dirichlet clamp -> PCG -> corrector -> adaptive dt.
 * ------------------------------------------------------------------------------------- */

/* AdaptivePolicy (newmark_stepper.hpp:58-63) + config::SolverSettings / TimeSettings */
typedef struct cwf_stepper_desc
{
    double rayleigh_alpha, rayleigh_beta; /* RayleighCoefficients */
    double runtime_tolerance, pause_tolerance;
    uint64_t max_iterations;
    double initial_dt;
    int32_t adaptive;
    int32_t warm_start; /* Stepper::warm_start_enabled_ default true */
    double min_dt, max_dt;
    double low_iteration_ratio, increase_factor, decrease_factor; /* 0.3, 1.1, 0.5 */
    const float *external_force; /* [3N] interleaved dof = 3n+k (NodeBuffers::external_force) */
    const float *bc_value;       /* [3N] (NodeBuffers::bc_value) */
} cwf_stepper_desc;

/* StepTelemetry (newmark_stepper.hpp:68-79) */
typedef struct cwf_step_telemetry
{
    double simulation_time, time_step, applied_tolerance;
    int32_t paused_mode, dt_increased, dt_decreased, dt_clamped_min, dt_clamped_max, reserved;
    cwf_pcg_telemetry pcg;
} cwf_step_telemetry;

typedef struct cwf_hip_stepper cwf_hip_stepper;

int cwf_hip_stepper_create(cwf_hip_system *system, const cwf_stepper_desc *desc, cwf_hip_stepper **out);
void cwf_hip_stepper_destroy(cwf_hip_stepper *st);
/* Stepper::step(simulation_time_seconds, paused_mode) */
int cwf_hip_stepper_step(cwf_hip_stepper *st, double simulation_time, int paused, cwf_step_telemetry *tel);
/* which: 0 = displacement, 1 = velocity, 2 = acceleration, 3 = the last PCG solution x, 4 = external force
 * (get only); out [3N] */
int cwf_hip_stepper_get_state(cwf_hip_stepper *st, int which, float *out, uint64_t n, int ptr_kind);
int cwf_hip_stepper_set_state(cwf_hip_stepper *st, int which, const float *in, uint64_t n, int ptr_kind);
/* rewrite nodes.external_force between steps (viewer.cpp:262-266) */
int cwf_hip_stepper_set_external_force(cwf_hip_stepper *st, const float *f, uint64_t n, int ptr_kind);
/* Time-varying loads on the device (loads.cpp:87-174 evaluated for one curve-scaled pattern, cast as
 * pack.cpp:41-57): set_load_pattern uploads base = the loads no curve scales (gravity, unscaled tractions and
 * point loads) and pattern = the point-load values one curve scales, f64 [3N] host arrays in the caller's node
 * order; each set_load_scale(c) then writes external_force = safe_cast(base + c * pattern) on the handle's
 * stream, where c = evaluate_curve(curve, t) (loads.cpp:63-85). For point loads (at most one scaled group per
 * node) that is bitwise the external_force assemble_load_vector at t packs (loads.cpp:163-172 adds
 * scale * value[axis] after gravity); a scaled traction rounds as (area * scale / n) * value there and is not
 * covered. This is the viewer's per-step rewrite of nodes.external_force (viewer.cpp:262-266) without the
 * host round trip. */
int cwf_hip_stepper_set_load_pattern(cwf_hip_stepper *st, const double *base, const double *pattern, uint64_t n);
int cwf_hip_stepper_set_load_scale(cwf_hip_stepper *st, double scale);
int cwf_hip_stepper_set_warm_start(cwf_hip_stepper *st, int enabled);
int cwf_hip_stepper_time(const cwf_hip_stepper *st, double *current_time, double *time_step);

/* ---------------------------------------------------------------------------------------
 * Explicit stepper: central differences (leapfrog) on the lumped mass, for wave propagation, impact and blast-type
 * loads, where the physics wants a step near the mesh's stability limit anyway. No solve: a step is one operator
 * product and one node pass. State: u_n and the half-step velocity v_(n-1/2), f32 [3N]. Per step and free DOF, in
 * fp64, rounded to f32 only where stored:
 *     w     = f32(u_n + beta_R v_(n-1/2))                  the operator's input (u_n itself when beta_R == 0)
 *     y     = K w                                          the handle's operator at scalars (1, 0), f32; a constrained
 *                                                          DOF enters it as 0, as in cwf_hip_apply_keff
 *     f_n   = the external force at t_n = n dt             n = steps since create (not accumulated)
 *     v_new = f32(c1 v + c2 ((f_n - y) / m))               c1 = (1 - alpha_R dt / 2) / (1 + alpha_R dt / 2),
 *                                                          c2 = dt / (1 + alpha_R dt / 2)
 *     u_new = f32(u + dt v_new)
 * Constrained DOFs hold u = bc_value, v = 0. The stiffness-proportional damping force beta_R K v_(n-1/2) is lagged
 * half a step so that it rides in the same product; it lowers the stability limit to
 *     critical dt = (2 / omega_max) (sqrt(1 + xi^2) - xi),  xi = beta_R omega_max / 2,  omega_max^2 = lambda_max,
 * lambda_max the largest eigenvalue of M^-1 K over the free DOFs, estimated by cwf_hip_lambda_max. The handle's
 * scalars, mode, block inverse and solver vectors are left as they are: a Newmark stepper or a solve on the same
 * handle is unaffected. A handle attached to a communicator is refused with CWF_ERR_UNSUPPORTED.
 *
 * Absorbing boundaries (cwf_hip_explicit_set_dashpots): a dashpot node n carries a symmetric positive-semidefinite
 * 3x3 matrix C_n in N s / m -- a full matrix, not a diagonal: on a face with unit normal nu and tributary area a the
 * viscous (Lysmer-Kuhlemeyer) boundary is C = rho a (V_p nu nu^T + V_s (I - nu nu^T)), diagonal only on axis-aligned
 * faces (cwf_absorbing_dashpots). Its force takes the central average the mass-proportional term has,
 * (alpha_R M + C)(v_new + v) / 2, which is solved per node: with h = alpha_R dt / 2, B = C dt / (2 m) and
 * A = ((1 + h) I + B)^-1,
 *     P = A ((1 - h) I - B),   Q = dt A                      3x3 each, fp64, formed once on the host
 *                                                            (cwf_explicit_dashpot_update)
 *     g_j     = ((double)f_j - (double)y_j) / m              as above, m the f32 lumped mass widened to double
 *     v_new_k = f32(((P_k0 v_0 + P_k1 v_1) + P_k2 v_2) + ((Q_k0 g_0 + Q_k1 g_1) + Q_k2 g_2))
 *     u_new_k = f32(u_k + dt v_new_k)                        then constrained DOFs as above (u = bc_value, v = 0)
 * in exactly this association order, without fused multiply-adds. A node without a dashpot keeps the expression
 * above; with C = 0 the matrix form reduces to it (P = c1 I, Q = c2 I) up to the rounding of the products. beta_R != 0
 * keeps its lagged form, w = f32(u + beta_R v) as stored above. An incident wave enters through such a boundary as
 * the force 2 C_n v_inc(t) on the dashpot nodes (the compliant base): a load pattern of rows 2 C_n d with the load
 * curve c(t) gives the incident velocity d c(t).
 * The critical step is unchanged. C enters implicitly, through the average vbar = (v_new + v) / 2: with
 * M (v_new - v) / dt + (alpha_R M + C) vbar + K u = f the leapfrog energy
 * 1/2 v_new^T M v_new + 1/2 u_new^T K u_new - (dt / 2) v_new^T K u_new, which is positive definite exactly below the
 * critical step of M^-1 K alone, changes per unforced step by -dt vbar^T (alpha_R M + C) vbar <= 0 for every symmetric
 * C >= 0, however large; per node the eigenvalues of P are ((1 - h) - b) / ((1 + h) + b) with b >= 0 those of B, inside
 * (-1, 1]. So critical_dt and lambda_max are those of the stepper without dashpots, and dashpots scaled by 1e4 run at
 * the same step (tests/test_gpu_absorbing.py).
 *
 * Tied boundaries (cwf_hip_explicit_set_ties): the lateral boundary of a soil model. A tie set is a list of disjoint
 * groups of at least two nodes; the members of a group share one velocity in all three components -- every boundary
 * node of one elevation (a laminar shear box), or a node and its partner on the opposite face (periodic). With the
 * lumped mass the constraint has a closed form: the group moves as one node of mass M_G = sum m_i, net force
 * F_G = sum ((f_i - y_i) + p_i) and dashpot matrix C_G = sum C_i (p_i: plasticity's correction force where a set is in
 * force; C_i = 0 for a member without a dashpot). Per step, in fp64 without fused multiply-adds:
 *     term_j = ((double)f_j - (double)y_j) + (double)p_j     per member j and component (no "+ p" without plasticity);
 *                                                            f, y and p exactly as the update pass of the step reads them;
 *                                                            0 for a constrained component (the group has one mask), so
 *                                                            g_G is 0 there and no constrained row reaches a free one
 *     S      = the sum of the group's terms                  in the order below
 *     g_G    = S / M_G                                       M_G = (double)m_0, then M_G + (double)m_j in member order
 *     v_new_k = f32(((P_k0 v_0 + P_k1 v_1) + P_k2 v_2) + ((Q_k0 g_G0 + Q_k1 g_G1) + Q_k2 g_G2))     per member, v its own
 *     u_new_k = f32(u_k + dt v_new_k)                        then constrained DOFs as above
 * with P | Q = cwf_explicit_dashpot_update(C_G, M_G, alpha_R, dt), the rows associated as the dashpot rows above; C_G is
 * summed entry by entry in member order from the first member that has a dashpot. A group without dashpot members takes
 * the same rows with C_G = 0, P = c1 I and Q = c2 I up to the rounding of that function's products (the library's values
 * are the scheme's, not c1 and c2). Members that hold equal v run the same operations on the same operands, so they
 * keep bitwise equal v, and u_i - u_j stays what it was when the set was put in force: the tie constrains velocity.
 * The members of a group must have the same constraint mask; the mask wins on constrained components, as for dashpots.
 * Summation order of S, a function of the member count c alone (members in the order they were listed):
 *     c <= 8:  acc = 0, then acc = acc + term_j for j = 0 .. c - 1;
 *     c > 8:   64 lane sums L_l = 0, L_l = L_l + term_j for j = l, l + 64, ... (a lane without members keeps 0), then
 *              L_l = L_l + L_(l + s) for l < s, s = 32, 16, 8, 4, 2, 1; S = L_0.
 * One gather kernel per step forms g_G (one 64-lane wavefront per group, no atomics) after the operator launch, the
 * plasticity passes and the load sources' kernel and before the update pass, which then reads three f64 per tied node
 * instead of forming the node's own quotient. set_ties replaces every member's v by the group's mass-weighted mean
 * f32((sum (double)m_i (double)v_i) / M_G), the sum from the first term in member order (constrained components stay
 * 0), on the host; cwf_hip_explicit_set_state(1) does the same while a set is in force, which costs it three more
 * device round trips (mass, mask and v out, v in again). set_ties and set_dashpots read the mass back and rebuild and
 * upload every slot and tie array while a tie set is in force: set-time costs, none per step.
 * The critical step is unchanged: the tied system is (T^T K T, T^T M T) for the 0/1 map T from group DOFs to node DOFs,
 * whose eigenvalues are Rayleigh quotients of (K, M) on range(T), so its lambda_max does not exceed the untied one and
 * the stepper's dt stays valid without a new power iteration; C_G enters implicitly, as C_n does. The constraint
 * forces sum to zero within a group and its members share vbar, so they do no work: the energy ledger's per-node terms
 * stand as they are, and a member's dissipation term uses its own C_i as given to set_dashpots, never C_G.
 * A stepper without ties launches exactly the kernels it launches without this section.
 *
 * Monitors (cwf_hip_explicit_set_monitors): what a wave run takes home, recorded on the device while advance() queues
 * its steps. "Step count n" is the number of steps since create; after the update that makes it n the state is u_n and
 * v_(n-1/2). A stepper without monitors launches exactly the kernels it launches without this section.
 *   Receivers: after the update that makes the step count n, when n % receiver_every == 0 and a row is free, a gather
 *     kernel (one thread per receiver) writes u_n and v_(n-1/2) of the receiver nodes to row `held` of two device
 *     buffers [capacity][count][3], in the caller's receiver order. A full buffer drops the sample and counts it.
 *   Peak maps: three f32 per node, zero at set and at reset, raised in the update pass from the values it stores (a
 *     constrained DOF enters with u = bc_value, v = 0), each with max(p, x) = x > p ? x : p (a NaN never raises a peak):
 *       peak_u: x = f32(sqrt(((double)un_0 un_0 + (double)un_1 un_1) + (double)un_2 un_2))       un = u_(n+1)
 *       peak_v: the same of vn = v_(n+1/2)
 *       peak_a: the same of a_k = ((double)vn_k - (double)v_k) / dt, the central acceleration at t_n
 *   Energy ledger (needs beta_R == 0): per free DOF k of node n in the update of step i (step count i -> i + 1), in
 *     fp64 without fused multiply-adds, m = (double)mass[n], y = K u_i as the pass holds it (f32):
 *       vb   = 0.5 * ((double)vn_k + (double)v_k)
 *       kin  = 0.5 * (m * ((double)vn_k * (double)vn_k))
 *       pot  = 0.5 * ((double)un_k * (double)y_k)
 *       work = dt * (vb * (double)f_k)
 *       diss = dt * (alpha_R * (m * (vb * vb)))
 *            + (dashpot node) dt * (vb_k * ((C_k0 vb_0 + C_k1 vb_1) + C_k2 vb_2))     C as given to set_dashpots
 *     A constrained DOF contributes 0 to all four (its vb, from the stored vn = 0, still enters a dashpot row). With
 *     H_i = sum kin + sum pot = 1/2 v+^T M v+ + 1/2 u_(i+1)^T K u_i the scheme satisfies, in exact arithmetic,
 *     H_i - H_(i-1) = sum work_i - sum diss_i, dashpots and alpha_R included, so
 *     kinetic + potential - work_cum + dissipated_cum is constant along a run: the number the ledger exists to show.
 *     Summation order (a function of N alone): a node adds its components (t_0 + t_1) + t_2; a workgroup of the update
 *     pass holds nodes 256 b .. 256 b + 255 (internal order; lanes past N carry zeros) and reduces them in a fixed
 *     tree: within each 64-lane wave x += x[lane + 32], + 16, + 8, + 4, + 2, + 1, then (w_0 + w_1) + (w_2 + w_3) over
 *     its four waves. Work and dissipation are added every step to the workgroup's own two fp64 accumulators
 *     (acc = acc + share; no atomics); kinetic and potential are written to its two "current" slots on sampled steps.
 *     The update that makes the step count n is sampled when n % energy_every == 0 and a row is free; a one-workgroup
 *     kernel then folds the shares: thread t adds workgroups t, t + 256, ... in that order from 0, the 256 sums fold
 *     pairwise (s[t] += s[t + stride], stride 128 ... 1) into the row {kinetic, potential, work_cum, dissipated_cum}.
 *     The cumulative columns include the unsampled steps; a full buffer drops rows, not sums.
 *
 * Load sources (cwf_hip_explicit_set_sources): loads whose time function differs from node to node -- an obliquely
 * incident plane wave, a three-component ground motion, a travelling front. A source is a piecewise-linear curve and a
 * list of entries (node, amplitude A[3], delay tau in seconds, any sign); a set holds up to CWF_EXPLICIT_MAX_SOURCES
 * sources. At step n a node with entries (a loaded node) gets, per component k, in fp64 without fused multiply-adds,
 *     acc   = (double)f_ext_k                                f_ext: the external force as last set (create /
 *                                                            set_external_force)
 *     for each of the node's entries e, ascending source index s:
 *         c   = cwf_explicit_curve_value(curve_s, (double)n dt - tau_e)
 *         acc = acc + A_ek c
 *     f_n,k = safe_cast(acc)                                 cwf_hip_stepper_set_load_scale's rounding
 * and a node without entries reads f_ext as before. A kernel with one thread per loaded node runs before the update
 * pass of every step and stores these f_n into the stepper's force buffer, which the update pass reads as it reads the
 * external force: constrained DOFs are masked as always, and dashpots, peak maps and the ledger's work term see f_n.
 * n dt is formed on the host and passed to the launch; the kernel finds the curve's segment by bisection, the same
 * knot the linear scan of cwf_explicit_curve_value stops at (duplicate knots included), and evaluates it in the same
 * operations. cwf_hip_explicit_get_state(4) returns f_n of the last step; the loaded nodes' f_ext is kept in a side
 * array of 12 bytes per loaded node, which set_external_force refreshes and a removed set writes back. Sources and a
 * load pattern exclude each other. A stepper without sources launches exactly the kernels it launches without this
 * section and allocates nothing for it.
 *
 * Plasticity (cwf_hip_explicit_set_plasticity): rate-independent von Mises (J2) plasticity with linear isotropic
 * hardening on tet4 elements, by radial return, in the initial-stress form: the operator product stays the linear
 * y = K w on whichever path the handle takes, and the plastic strain enters as a correction force. A material m is
 * plastic when its yield stress sy_m is finite and > 0; its hardening modulus is H_m >= 0; its D must have the
 * isotropic Voigt pattern, mu = D[3][3] (engineering shears, as the post stack). An element of a plastic material is a
 * plastic element and owns a slot, slots in ascending element index; a node with at least one plastic incident element
 * is an affected node. State per slot, fp64: ep[6] (plastic strain, Voigt, engineering shears), abar (equivalent
 * plastic strain), wp (plastic work); all zero at set and at reset.
 * The step that takes the step count from n to n + 1 runs an element pass and a node pass before its operator launch.
 * The element pass reads u_n, the stored displacement (not the operator's input w). Per plastic element, in fp64
 * without fused multiply-adds:
 *     e      = strain of u_n                     the derived-fields element pass's statement order
 *     ee_r   = e_r - ep_r
 *     st     = D ee                              its isotropic row fold: a normal row adds its three normal columns
 *                                                from +0.0, a shear row is 0.0 + D_rr ee_r
 *     q      = von_mises(st)                     the derived fields' function
 *     Y      = sy + H * abar
 *     if q > Y:                                  (a NaN never yields)
 *         dg   = (q - Y) / (3.0 * mu + H)
 *         pm   = ((st_0 + st_1) + st_2) / 3.0
 *         s_r  = st_r - pm (r < 3),  s_r = st_r (r >= 3)
 *         fac  = (1.5 * dg) / q
 *         ep_r = ep_r + fac * s_r (r < 3);   ep_r = ep_r + (2.0 * fac) * s_r (r >= 3)
 *         abar = abar + dg
 *         wp   = wp + V * ((sy + H * abar) * dg)         abar already updated; V = (double)vol[e]
 *     sp     = D ep                              the same row fold
 *     corner a (gradient g = (gx, gy, gz), widened to double):
 *         c_a0 = V * ((gx*sp_0 + gy*sp_3) + gz*sp_5)
 *         c_a1 = V * ((gy*sp_1 + gx*sp_3) + gz*sp_4)
 *         c_a2 = V * ((gz*sp_2 + gy*sp_4) + gx*sp_5)     each stored as f32 (safe_cast)
 * Per affected node and component k the correction force is p_k = safe_cast(sum over the node's plastic incidences,
 * ascending element order, from +0.0, of (double)c). The update pass then takes
 *     g_k = (((double)f_k - (double)y_k) + (double)p_k) / m
 * in the plain form and in the dashpot form; everything else in the pass is unchanged, so M a = f - (K u - B^T D ep V).
 * Constrained DOFs are masked as always. An element whose abar is still 0 has ep = 0 and contributes corner forces of
 * magnitude 0, and adding a zero to a sum that starts at +0.0 leaves +0.0: a plastic material that never yields steps as
 * the elastic one up to the sign of a zero ((f - y) + 0.0 turns -0.0 into +0.0).
 * The critical step is unchanged: the elastoplastic tangent D - (3 mu)^2 / (3 mu + H) n n^T (n the unit flow direction)
 * is D minus a positive-semidefinite matrix, so the tangent stiffness is never stiffer than K and lambda_max of
 * M^-1 K bounds it; the return map itself is unconditionally stable.
 * On the device: per slot its element (4 B), 64 B of state, 16 B of corner positions and 48 B of corner forces; 16 B
 * of {sy, H} per material; 8 B per affected node (the node and its run); and the f32 [3N] vector p, zeroed at set, of
 * which only the affected rows are rewritten; all in the stepper's arena. The corner forces are stored node-major: an
 * affected node's plastic incidences are one contiguous run of 12-B entries in ascending element order, the element
 * pass pushes each corner's force to its position in that run, and the node pass reads runs, consecutive nodes
 * consecutive runs. No atomics, no second stream. The state is written only where an element yielded in that step,
 * and an element whose abar is still 0 stores no corner forces (its entries hold the +0.0 they were set to).
 * The energy ledger and plasticity exclude each other: the ledger's potential term 1/2 u . K u is the linear one, so its
 * balance would no longer be constant. Element monitors and gauges keep reporting D e, the stress of the total strain;
 * the stress D (e - ep) is formed on the host from cwf_hip_explicit_read_plasticity. A stepper without plasticity
 * launches exactly the kernels it launches without this section and allocates nothing for it.
 *
 * Soil plasticity (cwf_hip_explicit_set_soil_plasticity): rate-independent Drucker-Prager plasticity with linear
 * hardening of the cohesion on tet4 elements, in the same initial-stress form: the operator product stays y = K w,
 * plasticity enters through the correction force p alone, and the update pass, the node pass, slots, affected nodes and
 * the 64-B state record ep[6], abar, wp are those of "Plasticity". Small strain, tension positive, Voigt order with
 * engineering shears. A stepper holds one plasticity set: either setter replaces whichever is in force.
 * Per material m: an isotropic D (mu = D[3][3], lambda = D[0][1], Kb = lambda + (2/3) mu), alpha >= 0 (friction),
 * kappa >= 0 (cohesion), 0 <= beta <= alpha (dilation), H >= 0 (hardening of kappa with abar). kappa = +inf: the
 * material is elastic. alpha = 0 with kappa = 0 has no strength at all and is refused.
 * Per plastic element an optional stress at rest sig0[6] (fp64, Pa; zeros when no array is given). The dynamic run
 * models no gravity; sig0 is in equilibrium with the gravity that is not modelled, so it adds no force and enters the
 * yield function alone.
 * Per plastic element, in fp64 without fused multiply-adds, with e and ee as in "Plasticity":
 *     st     = D ee                              the same isotropic row fold
 *     st_r   = sig0_r + st_r                     every r, only when a stress at rest was given
 *     pm     = ((st_0 + st_1) + st_2) / 3.0
 *     s_r    = st_r - pm (r < 3),  s_r = st_r (r >= 3)
 *     j2     = 0.5 * ((s_0*s_0 + s_1*s_1) + s_2*s_2) + ((s_3*s_3 + s_4*s_4) + s_5*s_5)
 *     J      = sqrt(j2 < 0 ? 0 : j2)
 *     kc     = kappa + H * abar
 *     f      = (J + (3.0 * alpha) * pm) - kc
 *     if f > 0:                                  (a NaN never yields)
 *         Kb   = D_01 + (2.0 / 3.0) * mu
 *         dl   = f / ((mu + ((9.0 * Kb) * alpha) * beta) + H)
 *         Jn   = J - mu * dl
 *         if Jn >= 0 or not alpha > 0:           the cone (return value 1)
 *             half = (0.5 * dl) / J ;  bdl = beta * dl
 *             ep_r = ep_r + (half * s_r + bdl) (r < 3);   ep_r = ep_r + (2.0 * half) * s_r (r >= 3)
 *             abar = abar + dl
 *             wp   = wp + V * (dl * (Jn + (3.0 * beta) * (pm - ((3.0 * Kb) * beta) * dl)))
 *         else:                                  the apex (return value 2)
 *             pa   = kc / (3.0 * alpha) ;  dv = (pm - pa) / Kb ;  third = dv / 3.0
 *             ep_r = ep_r + (s_r / (2.0 * mu) + third) (r < 3);   ep_r = ep_r + s_r / mu (r >= 3)
 *             abar = abar + J / mu
 *             wp   = wp + V * (pa * dv)
 *     sp     = D ep                              then the corner forces and the node fold of "Plasticity"
 * With alpha = 0 the apex does not exist; "not alpha > 0" keeps a return whose Jn rounds below zero on the cone. The
 * apex branch holds kc at its value from the start of the step (the hardening during an apex return is not iterated):
 * a simplification. An apex return from a stress without a deviator changes ep and leaves abar at 0, so the element
 * pass stores corner forces where the element yielded in this step or abar > 0.
 * The device function, cwf_explicit_dp_update and the tests' numpy restatement each follow the lines above, not each
 * other.
 * Critical step: for beta = alpha (associated flow) the tangent is D minus a positive-semidefinite matrix and the
 * elastic critical step holds as for J2. For beta < alpha the tangent is unsymmetric; the elastic step is kept, and
 * its stability there is supposed, not proven.
 * On the device, beside what "Plasticity" lists: 32 B of {alpha, kappa, beta, H} per material in place of J2's 16 B,
 * and 48 B of sig0 per slot when one was given (slot-major, 16-B aligned; a set without it runs an instantiation of
 * the element kernel that reads nothing more than J2's). The soil set launches k_explicit_dp_elements and the node
 * pass k_explicit_plastic_nodes_coop: a wavefront copies the contiguous span of its 64 nodes' runs into LDS as
 * consecutive words, then each lane folds its own run from there, from +0.0 in ascending element order, so p has the
 * bits k_explicit_plastic_nodes gives (cwf_explicit_soil_desc.node_pass picks either for tests). J2 keeps its node pass.
 * A stepper without soil plasticity launches what it launched before this section.
 * ------------------------------------------------------------------------------------- */
typedef struct cwf_explicit_desc
{
    double rayleigh_alpha, rayleigh_beta;
    double dt;                 /* 0 -> safety * critical dt from the estimate */
    double safety;             /* 0 -> 0.9; in (0, 1] */
    uint32_t power_iterations; /* 0 -> 60 */
    uint32_t reserved;
    const float *external_force; /* [3N], as in cwf_stepper_desc; nullable: zero */
    const float *bc_value;       /* [3N] (nullable: zero) */
} cwf_explicit_desc;

typedef struct cwf_explicit_telemetry
{
    double time, dt, lambda_max, critical_dt;
    uint64_t steps;            /* steps taken since create */
    int32_t finite, reserved;  /* 0 when a non-finite value was stored */
} cwf_explicit_telemetry;

typedef struct cwf_hip_explicit cwf_hip_explicit;

#define CWF_EXPLICIT_MAX_CURVE_POINTS 4096

/* Estimates lambda_max with desc->power_iterations iterations. Errors: CWF_ERR_UNSUPPORTED "explicit stepping of a
 * sharded handle is not supported" {ranks=<n>} and "explicit stepping needs elements"; CWF_ERR_ARGUMENT "time step
 * exceeds the critical step" {dt=<dt>, critical_dt=<limit>} for a desc->dt above the estimated limit, and for a
 * negative coefficient or a safety outside (0, 1]. */
int cwf_hip_explicit_create(cwf_hip_system *system, const cwf_explicit_desc *desc, cwf_hip_explicit **out);
void cwf_hip_explicit_destroy(cwf_hip_explicit *ex);
/* Queues n_steps steps on the handle's stream (two launches each on a FAST handle: the operator's tile launch and the
 * update pass, which folds the node's partials itself; no hipGraph), synchronises once, then reads the device's
 * non-finite word. tel (nullable) is filled either way. A stored u or v that is not finite raised the word: the call
 * returns CWF_ERR_HIP "explicit step produced a non-finite value" {steps=<steps since create>} -- the device reported
 * the failure, not the host -- and so does every later call until set_state rewrites u or v. */
int cwf_hip_explicit_advance(cwf_hip_explicit *ex, uint64_t n_steps, cwf_explicit_telemetry *tel);
/* which: 0 = u, 1 = v (half step), 4 = external force at the last step (get only), 5 = plasticity's correction force p
 * of the last step (get only, while plasticity is set); [3N], the caller's node order */
int cwf_hip_explicit_get_state(cwf_hip_explicit *ex, int which, float *out, uint64_t n, int ptr_kind);
int cwf_hip_explicit_set_state(cwf_hip_explicit *ex, int which, const float *in, uint64_t n, int ptr_kind);
int cwf_hip_explicit_set_external_force(cwf_hip_explicit *ex, const float *f, uint64_t n, int ptr_kind);
/* base and pattern as cwf_hip_stepper_set_load_pattern. With a pattern and a curve set, the update pass forms
 * f_n = safe_cast(base + c(t_n) pattern) itself from the f64 arrays (cwf_hip_stepper_set_load_scale's rounding) and
 * external_force is not read; c(t_n) = cwf_explicit_curve_value of the curve at t_n, passed to step n's launch. */
int cwf_hip_explicit_set_load_pattern(cwf_hip_explicit *ex, const double *base, const double *pattern, uint64_t n);
/* piecewise-linear (times ascending), 1 <= count <= CWF_EXPLICIT_MAX_CURVE_POINTS; count == 0 removes the curve */
int cwf_hip_explicit_set_load_curve(cwf_hip_explicit *ex, const double *times, const double *values, uint64_t count);
int cwf_hip_explicit_time(const cwf_hip_explicit *ex, double *current_time, double *time_step);
/* Dashpots of the scheme above: `count` distinct nodes (the caller's numbering) and their C_n (f64, 9 per node,
 * row-major). P and Q are formed per node from the stepper's alpha_R, dt and the node's f32 mass and uploaded with a
 * u32 slot per node (0xFFFFFFFF: none) and one 144-byte fp64 P | Q record per dashpot node; the update pass reads the
 * slot only while a set is in force. u, v, the step count and the load state are kept; a later call replaces the set,
 * count == 0 removes it (the stepper then launches what a stepper that never had dashpots launches). Errors, all
 * CWF_ERR_ARGUMENT and leaving the previous set in force: "dashpot node out of range" {index=<i>, node=<id>},
 * "dashpot node listed twice" {index=<i>, node=<id>}, and a refused matrix (cwf_explicit_dashpot_update's texts)
 * {index=<i>}. A dashpot on a constrained DOF has no effect: the mask wins. While an energy ledger is set
 * (cwf_hip_explicit_set_monitors) the matrices as given are uploaded too, 72 bytes per dashpot node indexed by the same
 * slot and read only by the ledger, and a later set replaces them with the records. */
int cwf_hip_explicit_set_dashpots(cwf_hip_explicit *ex, uint64_t count, const uint32_t *node_ids, const double *C);
/* The set in force as it was given; node_ids and C are nullable (count only). */
int cwf_hip_explicit_get_dashpots(cwf_hip_explicit *ex, uint64_t *count, uint32_t *node_ids, double *C);
/* Tied boundaries of the scheme above: group g holds the nodes node_ids[offsets[g] .. offsets[g + 1]) (the caller's
 * numbering); group_count == 0 removes the set (the stepper then launches what a stepper that never had ties launches).
 * u, the step count, the load state, dashpots, monitors and plasticity are kept; v is projected as stated above. A tied
 * node owns a slot as a dashpot node does: the u32 slot per node and the 144-byte P | Q records are one set of arrays
 * for both (slots of the dashpot nodes first, in their order, then the other tied nodes in list order), with a u32
 * group word per slot, the groups' CSR in the handle's node order (4 B per group and per member), M_G and g_G (8 + 24 B
 * per group); set_dashpots and set_ties rebuild them together, so either call order gives the same arrays. Everything
 * refusable is checked on the host before anything changes; all refusals are CWF_ERR_ARGUMENT and leave the previous
 * set in force: "tie offsets must ascend from 0" {group=<g>}, "tie group needs at least two nodes" {group=<g>,
 * nodes=<n>}, "tied node out of range" / "tied node listed twice" {index=<i>, node=<id>} (across all groups), "tied
 * nodes differ in their constraints" {group=<g>, node=<id>, mask=<m>, first_mask=<m0>}, and what
 * cwf_explicit_dashpot_update refuses of a group's C_G {group=<g>} (set_dashpots answers the same while ties are in
 * force). */
typedef struct cwf_explicit_tie_info
{
    uint64_t group_count;
    uint64_t member_count;
    uint64_t dashed_groups; /* groups with at least one dashpot member */
    uint64_t device_bytes;  /* the slot arrays, records and tie arrays in the stepper's arena; 0 without a set */
} cwf_explicit_tie_info;
int cwf_hip_explicit_set_ties(cwf_hip_explicit *ex, uint64_t group_count, const uint64_t *offsets /* [group_count + 1] */,
                              const uint32_t *node_ids);
/* The set in force as it was given; offsets [group_count + 1] and node_ids [member_count] are nullable (counts only). */
int cwf_hip_explicit_get_ties(cwf_hip_explicit *ex, uint64_t *group_count, uint64_t *member_count, uint64_t *offsets,
                              uint32_t *node_ids);
int cwf_hip_explicit_tie_info(cwf_hip_explicit *ex, cwf_explicit_tie_info *out);
/* Monitors of the scheme above. Replaces the previous set; desc NULL or all zero removes everything and frees the
 * buffers (the stepper then launches what a stepper that never had monitors launches). u, v, the step count, loads and
 * dashpots are kept; peaks, cumulative sums and sample counts start at zero. May be called between advance calls. All
 * buffers are allocated here, in the stepper's arena. Everything refusable is checked before anything changes, and a
 * refusal leaves the previous set in force: CWF_ERR_ARGUMENT "receiver node out of range" {index=<i>, node=<id>},
 * "receiver node listed twice" {index=<i>, node=<id>}, "receiver_every must be at least 1", "monitor capacity must not
 * be zero" (a zero capacity with a non-zero count / every), "null pointer"; CWF_ERR_UNSUPPORTED "the energy ledger
 * needs rayleigh_beta == 0" {rayleigh_beta=<beta>}; CWF_ERR_ALLOC. */
typedef struct cwf_explicit_monitor_desc
{
    uint64_t receiver_count;
    const uint32_t *receiver_nodes; /* [receiver_count] distinct nodes, the caller's numbering */
    uint64_t receiver_every;        /* >= 1 when receiver_count > 0 */
    uint64_t receiver_capacity;     /* samples (rows) */
    uint64_t energy_every;          /* 0: no ledger */
    uint64_t energy_capacity;       /* samples (rows) */
    uint32_t peaks;                 /* 0 / 1 */
    uint32_t reserved;
} cwf_explicit_monitor_desc;

typedef struct cwf_explicit_monitor_info
{
    uint64_t receiver_count, receiver_every, receiver_capacity, receiver_samples, receiver_dropped;
    uint64_t energy_every, energy_capacity, energy_samples, energy_dropped;
    uint32_t peaks, reserved;
} cwf_explicit_monitor_info;

int cwf_hip_explicit_set_monitors(cwf_hip_explicit *ex, const cwf_explicit_monitor_desc *desc);
/* The same set: sample counts rewound, peaks and cumulative sums zeroed. */
int cwf_hip_explicit_reset_monitors(cwf_hip_explicit *ex);
/* Samples held and dropped (a full buffer drops further samples and counts them; stepping goes on). */
int cwf_hip_explicit_monitor_info(cwf_hip_explicit *ex, cwf_explicit_monitor_info *info);
/* Rows first .. first + count - 1 of the receiver buffers into host memory: steps [count] (the step count of each row;
 * time = steps x dt), u and v [count][receivers][3], each nullable. CWF_ERR_ARGUMENT "monitor rows out of range"
 * {first=<first>, count=<count>, held=<rows held>}. */
int cwf_hip_explicit_read_receivers(cwf_hip_explicit *ex, uint64_t first, uint64_t count, uint64_t *steps, float *u,
                                    float *v);
/* The peak maps, [N] each in the caller's node order, each nullable; n = N. CWF_ERR_ARGUMENT "no peak maps are set". */
int cwf_hip_explicit_read_peaks(cwf_hip_explicit *ex, float *peak_u, float *peak_v, float *peak_a, uint64_t n,
                                int ptr_kind);
/* Ledger rows into host memory: steps [count], rows [count][4] = {kinetic, potential, work_cum, dissipated_cum}. */
int cwf_hip_explicit_read_energy(cwf_hip_explicit *ex, uint64_t first, uint64_t count, uint64_t *steps, double *rows);
/* Element monitors: stresses and strains recorded on the device while advance() queues its steps, a set of its own next
 * to the node monitors above (neither touches the other). Both parts sample by the receivers' rule: after the update
 * that makes the step count n, when n % every == 0, u_n is sampled; the row and "this step is due" are launch
 * arguments, there are no device counters. A stepper without element monitors launches exactly the kernels it launches
 * without this section and allocates nothing for it.
 *   Gauges: one thread per gauge element writes the 13 floats {strain[6], stress[6], von_mises} of the element, bit for
 *     bit the row cwf_hip_derived_fields returns for the same u, to row `held` of a buffer [capacity][gauges][13] in the
 *     caller's gauge order. A full buffer drops the sample and counts it.
 *   Envelopes: one pass over all E elements per due step. With x the value the derived-fields element pass would store
 *     (f32) a stored value is replaced only where x > peak (maxima) or x < low (minima), so a NaN never enters:
 *       CWF_ENVELOPE_VON_MISES     peak von Mises stress, from +0.0
 *       CWF_ENVELOPE_SHEAR_STRAIN  peak effective shear strain, from +0.0: with the element's fp64 strain e[0..5], in
 *                                  fp64 without fused multiply-adds and with the IEEE square root,
 *                                    d0 = e0 - e1; d1 = e1 - e2; d2 = e2 - e0;
 *                                    sd = d0 d0 + d1 d1 + d2 d2; sg = e3 e3 + e4 e4 + e5 e5;
 *                                    g = sqrt(sd (2.0 / 3.0) + sg), stored as f32
 *                                  (2 sqrt(J2) of the strain deviator with engineering shears: |gamma| in pure shear)
 *       CWF_ENVELOPE_STRESS_RANGE  min (from +inf) and max (from -inf) of each of the six stresses
 *     On the device every map is a plane of one f32 per element, the stress range twelve of them (component-major), so
 *     that a wavefront's loads and stores are consecutive words; the caller sees [E] and [E][6]. */
#define CWF_ENVELOPE_VON_MISES 1u
#define CWF_ENVELOPE_SHEAR_STRAIN 2u
#define CWF_ENVELOPE_STRESS_RANGE 4u
typedef struct cwf_explicit_element_monitor_desc
{
    uint64_t gauge_count;
    const uint32_t *gauge_elements; /* [gauge_count] distinct elements, the caller's numbering */
    uint64_t gauge_every;           /* >= 1 when gauge_count > 0 */
    uint64_t gauge_capacity;        /* samples (rows) */
    uint64_t envelope_every;        /* 0: no envelopes */
    uint32_t envelope_maps;         /* CWF_ENVELOPE_* bits; non-zero exactly when envelope_every is */
    uint32_t reserved;
} cwf_explicit_element_monitor_desc;

typedef struct cwf_explicit_element_monitor_info
{
    uint64_t gauge_count, gauge_every, gauge_capacity, gauge_samples, gauge_dropped;
    uint64_t envelope_every, envelope_samples; /* envelope_samples: element passes since set or reset */
    uint32_t envelope_maps, reserved;
} cwf_explicit_element_monitor_info;

/* Replaces the previous set; desc NULL or all zero removes it and frees its buffers. u, v, the step count, loads,
 * dashpots, sources and the node monitors are kept; the maps start at their start values and the sample counts at
 * zero. All buffers are allocated here, in the stepper's arena. Everything refusable is checked before anything
 * changes, and a refusal leaves the previous set in force: CWF_ERR_ARGUMENT "gauge element out of range" {index=<i>,
 * element=<id>}, "gauge element listed twice" {index=<i>, element=<id>}, "gauge_every must be at least 1", "monitor
 * capacity must not be zero", "unknown envelope map" {maps=<bits>}, "envelope_maps without envelope_every",
 * "envelope_every without envelope_maps", "null pointer"; CWF_ERR_ALLOC. */
int cwf_hip_explicit_set_element_monitors(cwf_hip_explicit *ex, const cwf_explicit_element_monitor_desc *desc);
/* The same set: sample counts rewound, the maps back at their start values. */
int cwf_hip_explicit_reset_element_monitors(cwf_hip_explicit *ex);
int cwf_hip_explicit_element_monitor_info(cwf_hip_explicit *ex, cwf_explicit_element_monitor_info *info);
/* Rows first .. first + count - 1 of the gauge buffer into host memory: steps [count], rows [count][gauges][13], each
 * nullable. CWF_ERR_ARGUMENT "monitor rows out of range" {first=<first>, count=<count>, held=<rows held>}. */
int cwf_hip_explicit_read_gauges(cwf_hip_explicit *ex, uint64_t first, uint64_t count, uint64_t *steps, float *rows);
/* The envelope maps in the caller's element order: von_mises and shear_strain [E], stress_min and stress_max [E][6],
 * each nullable; n = E. CWF_ERR_ARGUMENT "envelope map is not set" for a map asked for that the set does not hold;
 * CWF_ERR_SIZE "envelope map span size mismatch" {span=<n>, elements=<E>}. */
int cwf_hip_explicit_read_envelopes(cwf_hip_explicit *ex, float *von_mises, float *shear_strain, float *stress_min,
                                    float *stress_max, uint64_t n, int ptr_kind);
/* Load sources of the scheme above. */
#define CWF_EXPLICIT_MAX_SOURCES 8
typedef struct cwf_explicit_source_desc
{
    uint64_t curve_points;   /* 1 .. CWF_EXPLICIT_MAX_CURVE_POINTS */
    const double *times;     /* [curve_points] ascending (equal neighbours: a step) */
    const double *values;    /* [curve_points] */
    uint64_t entry_count;    /* >= 1 */
    const uint32_t *node_ids; /* [entry_count] distinct within the source, the caller's numbering */
    const double *amplitude; /* [3 entry_count] A, in N per unit of the curve */
    const double *delay;     /* [entry_count] tau in seconds */
} cwf_explicit_source_desc;

typedef struct cwf_explicit_source_info
{
    uint32_t source_count, reserved;
    uint64_t entry_count;   /* over all sources */
    uint64_t loaded_nodes;  /* distinct nodes with an entry */
    uint64_t curve_points;  /* over all sources */
    uint64_t device_bytes;  /* what the set holds in the stepper's arena */
} cwf_explicit_source_info;

/* Replaces the set in force by `count` sources (1 .. CWF_EXPLICIT_MAX_SOURCES); count == 0 removes it, writes f_ext
 * back and frees its buffers (the stepper then launches what a stepper that never had sources launches). u, v, the step
 * count, f_ext, dashpots and monitors are kept. On the device: a CSR over the loaded nodes in the handle's node order
 * (the ids move through the permutation as set_dashpots' slots do), per entry a 32-byte record A | tau and 8 bytes of
 * curve directory, the curves' tables, and 12 bytes of f_ext per loaded node; all in the stepper's arena. Everything
 * refusable is checked on the host before anything changes, and a refusal leaves the previous set in force:
 * CWF_ERR_SIZE "too many load sources" {count=<n>, max=8} and "load source curve must have 1 to 4096 points"
 * {source=<s>, count=<n>}; CWF_ERR_ARGUMENT "null pointer" {source=<s>}, "load source has no entries" {source=<s>},
 * "load source curve is not finite" / "load source curve times must ascend" {source=<s>, index=<i>}, "load source node
 * out of range" / "load source node listed twice" {source=<s>, index=<i>, node=<id>}, "load source entry is not
 * finite" {source=<s>, index=<i>}; CWF_ERR_UNSUPPORTED "load sources and a load pattern exclude each other" when a load
 * pattern is set (cwf_hip_explicit_set_load_pattern answers the same while sources are in force); CWF_ERR_ALLOC. */
int cwf_hip_explicit_set_sources(cwf_hip_explicit *ex, const cwf_explicit_source_desc *sources, uint32_t count);
/* The set in force as it was given: *count sources; `sources` (nullable: count only; else room for
 * CWF_EXPLICIT_MAX_SOURCES) is filled with pointers into the stepper's own copies, valid until the next set_sources
 * or destroy. */
int cwf_hip_explicit_get_sources(cwf_hip_explicit *ex, uint32_t *count, cwf_explicit_source_desc *sources);
int cwf_hip_explicit_source_info(cwf_hip_explicit *ex, cwf_explicit_source_info *info);
/* Plasticity of the scheme above. yield_stress[m] = +inf or 0: material m is elastic. */
typedef struct cwf_explicit_plasticity_desc
{
    const double *yield_stress; /* [material_count] sy, Pa */
    const double *hardening;    /* [material_count] H >= 0, Pa */
    uint64_t material_count;    /* the handle's */
} cwf_explicit_plasticity_desc;

typedef struct cwf_explicit_plasticity_info
{
    uint64_t plastic_elements; /* slots */
    uint64_t affected_nodes;
    uint64_t yielded_elements; /* abar > 0, counted on read */
    uint64_t bytes;            /* what the set holds in the stepper's arena */
} cwf_explicit_plasticity_info;

/* Replaces the set in force, its state starting at zero; desc NULL, or a desc without a plastic element, removes
 * plasticity and frees its buffers (the stepper then launches what a stepper that never had it launches). u, v, the step
 * count, loads, dashpots, sources and monitors are kept. Everything refusable is checked before anything changes, and a
 * refusal leaves the previous set in force: CWF_ERR_UNSUPPORTED "plasticity needs tet4 elements" (a hex8 handle), "a
 * plastic material needs an isotropic stiffness" {material=<m>}, "the energy ledger and plasticity exclude each other"
 * (cwf_hip_explicit_set_monitors answers the same for a ledger while plasticity is in force); CWF_ERR_ARGUMENT
 * "plasticity material count mismatch" {material_count=<given>, materials=<the handle's>}, "yield stress and hardening
 * must be non-negative" {material=<m>, yield_stress=<sy>, hardening=<H>} (a NaN too), "null pointer"; CWF_ERR_ALLOC. */
int cwf_hip_explicit_set_plasticity(cwf_hip_explicit *ex, const cwf_explicit_plasticity_desc *desc);
/* The same set: ep, abar, wp and p zeroed. set_state leaves them alone. */
int cwf_hip_explicit_reset_plasticity(cwf_hip_explicit *ex);
int cwf_hip_explicit_plasticity_info(cwf_hip_explicit *ex, cwf_explicit_plasticity_info *info);
/* The state in the caller's element numbering into host memory: ep [E][6], abar [E], wp [E], each nullable; n = E.
 * Elastic elements read as zeros. CWF_ERR_ARGUMENT "no plasticity is set"; CWF_ERR_SIZE "plasticity span size
 * mismatch" {span=<n>, elements=<E>}. cwf_hip_explicit_get_state(which = 5) returns p of the last step taken, [3N] in
 * the caller's node order ("unknown state field" without plasticity). */
int cwf_hip_explicit_read_plasticity(cwf_hip_explicit *ex, double *ep, double *abar, double *wp, uint64_t n);
/* Host only, no GPU: the element update of the scheme above, the function the device pass runs. D row-major [36] with
 * the isotropic pattern, strain = e[6], state = ep[6], abar, wp (updated in place where the element yields), sigma_p
 * = D ep of the updated state. Returns 1 when the element yielded, else 0. */
int cwf_explicit_j2_update(const double D[36], double yield, double hardening, double volume, const double strain[6],
                           double state[8], double sigma_p[6]);
/* Soil plasticity of the scheme above. kappa[m] = +inf: material m is elastic. */
typedef struct cwf_explicit_soil_desc
{
    const double *alpha;          /* [material_count] friction coefficient, >= 0 */
    const double *kappa;          /* [material_count] cohesion, Pa, >= 0 */
    const double *beta;           /* [material_count] dilation coefficient, 0 <= beta <= alpha */
    const double *hardening;      /* [material_count] H >= 0, Pa */
    uint64_t material_count;      /* the handle's */
    const double *initial_stress; /* nullable; [element_count][6] the stress at rest, Pa, the caller's element order;
                                     rows of elastic elements are ignored */
    uint64_t element_count;       /* the handle's E (read only with initial_stress) */
    uint32_t node_pass;           /* 0: the library's choice; for tests and measurements 1: k_explicit_plastic_nodes,
                                     2: k_explicit_plastic_nodes_coop, 3: the latter with LDS rounds of 96 words, so
                                     that a small mesh takes many rounds (the same p, bit for bit, every way) */
    uint32_t reserved;
} cwf_explicit_soil_desc;
/* As cwf_hip_explicit_set_plasticity, for the Drucker-Prager set: replaces the set in force (J2 or soil), its state
 * starting at zero; desc NULL, or a desc without a plastic element, removes it. A refusal leaves the previous set in
 * force. Those of cwf_hip_explicit_set_plasticity with their codes and texts ("plasticity needs tet4 elements", "a
 * plastic material needs an isotropic stiffness", "the energy ledger and plasticity exclude each other", "plasticity
 * material count mismatch", "null pointer"), and CWF_ERR_ARGUMENT "soil plasticity parameters out of range"
 * {material=<m>, alpha=, kappa=, beta=, hardening=} (a NaN too; alpha = kappa = 0), "initial stress is not finite"
 * {element=<e>, component=<c>} (a plastic element's row); CWF_ERR_SIZE "initial stress span size mismatch"
 * {span=<element_count>, elements=<E>}, CWF_ERR_ARGUMENT "unknown node pass" {node_pass=<n>}; CWF_ERR_ALLOC. cwf_hip_explicit_reset_plasticity, _plasticity_info,
 * _read_plasticity and cwf_hip_explicit_get_state(which = 5) serve both models. For a soil set
 * cwf_explicit_plasticity_info.yielded_elements counts the elements with abar > 0 or a plastic strain that is not zero
 * (an apex return from a stress without a deviator leaves abar at 0). */
int cwf_hip_explicit_set_soil_plasticity(cwf_hip_explicit *ex, const cwf_explicit_soil_desc *desc);
/* *model: 0 no plasticity set, 1 J2, 2 soil */
int cwf_hip_explicit_plasticity_model(cwf_hip_explicit *ex, int *model);
/* Host only, no GPU: the element update of "Soil plasticity", the function the device pass runs. params = {alpha,
 * kappa, beta, H}; sig0 nullable; the other arguments as cwf_explicit_j2_update. Returns 0 when the element stayed
 * elastic, 1 when it returned to the cone, 2 to the apex. */
int cwf_explicit_dp_update(const double D[36], const double params[4], const double *sig0, double volume,
                           const double strain[6], double state[8], double sigma_p[6]);
/* Host only: Drucker-Prager parameters out = {alpha, kappa, beta} from a Mohr-Coulomb cohesion c (Pa), friction angle
 * phi and dilation angle psi (radians, 0 <= psi <= phi < pi/2). match 0, the compression cone: alpha = 2 sin phi /
 * (sqrt3 (3 - sin phi)), kappa = 6 c cos phi / (sqrt3 (3 - sin phi)); match 1, the extension cone: 3 + sin phi in the
 * denominators; match 2, plane strain: alpha = tan phi / sqrt(9 + 12 tan^2 phi), kappa = 3 c / sqrt(9 + 12 tan^2 phi).
 * beta is alpha's formula at psi. CWF_ERR_ARGUMENT "Mohr-Coulomb parameters out of range", "unknown Drucker-Prager
 * match". */
int cwf_soil_dp_from_mohr_coulomb(double cohesion, double phi, double psi, int match, double out[3]);
/* Host only: the stress at rest sig0 [element_count][6] of a horizontally layered deposit under its own weight, for
 * cwf_explicit_soil_desc.initial_stress. centroids [element_count][3]; material [element_count] indexes density and
 * k0 [material_count]; axis (0, 1, 2) is the vertical, pointing up; surface: the elevation of the free surface (NULL:
 * the largest coordinate along axis of coords [node_count][3], which is read in that case only). Elements whose
 * centroid elevations lie within 1e-9 of the deposit's height of each other form a bin; runs of bins of one material
 * from the top down are the layers, two layers meeting midway between their adjacent bins. Per element
 *     sigma_v = -gravity * (sum over the layers above of rho_l * thickness_l + rho * (top of its layer - centroid))
 * on the vertical component, sigma_h = k0 * sigma_v on the two others, zero shears: for one material exactly
 * -gravity * (rho * depth). CWF_ERR_ARGUMENT "the deposit is not horizontally layered" {element=, material=,
 * layer_material=} for a bin of two materials, "a centroid lies above the surface", "null pointer" and non-finite or
 * negative inputs; CWF_ERR_INDEX "material index out of range". */
int cwf_soil_geostatic_stress(uint64_t element_count, const double *centroids, const uint32_t *material,
                              uint64_t material_count, const double *density, const double *k0, double gravity,
                              int axis, const double *surface, uint64_t node_count, const double *coords,
                              double *sig0);
/* Host only, no GPU: P and Q of the scheme above from C (row-major), the node's mass, alpha_R and dt, by the
 * closed-form 3x3 inverse. CWF_ERR_ARGUMENT for a C that is not finite ("dashpot matrix is not finite"), not symmetric
 * (|C_ij - C_ji| > 1e-12 trace: "dashpot matrix is not symmetric") or not positive semidefinite (a principal minor
 * below -1e-12 in units of the trace: "dashpot matrix is not positive semidefinite"), for mass <= 0 ("dashpot node
 * mass must be positive") and for a negative or non-finite alpha or dt. */
int cwf_explicit_dashpot_update(const double C[9], double mass, double alpha, double dt, double P[9], double Q[9]);
/* Host only, no GPU: tie sets for cwf_hip_explicit_set_ties from the node coordinates (f64 [3 node_count]). The
 * results go to *group_count, offsets (room for one more than the largest possible group count) and out_ids. tolerance
 * is relative to the model's extent along the axis compared; 0 means 1e-9. Errors are CWF_ERR_ARGUMENT in the thread's
 * record: "tied node out of range" / "tied node listed twice" {index, node}, "tie axis must be 0, 1 or 2" {axis},
 * "tie tolerance must be finite and not negative", "null pointer".
 * cwf_tie_levels (the laminar box): the listed nodes (distinct) are sorted by their coordinate along `axis`; a level is
 * the run of nodes within the tolerance of its lowest node, and each level of at least two nodes becomes one group.
 * Groups ascend in coordinate, members in node id. offsets [count / 2 + 1], out_ids [count].
 * cwf_tie_periodic: each node of face A is paired with the one node of face B whose coordinates in the two axes other
 * than `axis` agree within the tolerance; group i is {ids_a[i], its partner}. A node of either face without exactly one
 * partner is refused: "periodic faces do not match" {node, face=A|B}. offsets [count_a + 1], out_ids [2 count_a].
 * cwf_tie_merge: groups that may share nodes (the edges that an x-pair set and a y-pair set share) become the disjoint
 * groups of their union (union-find): groups ordered by smallest member, members ascending, a group of one node
 * dropped. offsets [members / 2 + 1], out_ids [members]; also "tie offsets must ascend from 0" {group}. */
int cwf_tie_levels(uint64_t node_count, const double *coords, uint64_t count, const uint32_t *node_ids, int axis,
                   double tolerance, uint64_t *group_count, uint64_t *offsets, uint32_t *out_ids);
int cwf_tie_periodic(uint64_t node_count, const double *coords, uint64_t count_a, const uint32_t *ids_a,
                     uint64_t count_b, const uint32_t *ids_b, int axis, double tolerance, uint64_t *group_count,
                     uint64_t *offsets, uint32_t *out_ids);
int cwf_tie_merge(uint64_t node_count, uint64_t in_groups, const uint64_t *in_offsets, const uint32_t *in_ids,
                  uint64_t *group_count, uint64_t *offsets, uint32_t *out_ids);
/* Host only, no GPU: the viscous-boundary matrices of a face list. coords f64 [3 node_count]; connectivity u32
 * [nodes_per_element (4: tet4, 8: hex8 in Gmsh corner order) x element_count]; element_material [element_count] indexes
 * rho, lame_lambda, lame_mu [material_count]; faces u32 [nodes_per_face (3 or 4) x face_count]. Every face must be a
 * face of exactly one element, whose material gives V_p = sqrt((lambda + 2 mu) / rho) and V_s = sqrt(mu / rho): a
 * layered block gets its strata's impedances. Area and unit normal come from the face's nodes (a quad: its triangles
 * (0,1,2) + (0,2,3), the normal along the sum of their cross products); each of the face's k nodes gets
 * rho (a / k)(V_p nu nu^T + V_s (I - nu nu^T)). Out: *count distinct nodes touched, ascending, in node_ids, and their
 * accumulated C_n in C (9 per node, row-major); both need room for min(node_count, nodes_per_face x face_count)
 * entries. Errors: CWF_ERR_ARGUMENT "absorbing face is not a boundary face of the mesh" {face=<i>} and "absorbing
 * face has zero area" {face=<i>}; CWF_ERR_NODE_RANGE "absorbing face references node out of range" {face=<i>,
 * node=<id>}. */
int cwf_absorbing_dashpots(uint64_t node_count, const double *coords, uint64_t element_count,
                           uint32_t nodes_per_element, const uint32_t *connectivity,
                           const uint32_t *element_material, uint64_t material_count, const double *rho,
                           const double *lame_lambda, const double *lame_mu, uint64_t face_count,
                           uint32_t nodes_per_face, const uint32_t *faces, uint64_t *count, uint32_t *node_ids,
                           double *C);
/* Host only, no GPU: an obliquely incident plane wave through the viscous boundary of a face list, as entries of a load
 * source. The wave has particle velocity d g(t - tau), tau = khat . (x - x0) / c, khat = propagation / |propagation|,
 * d = polarisation as given (not normalised), c = V_p when d is parallel to khat and V_s when it is perpendicular:
 * with q = |d . khat| / (|d| |khat|), q >= 1 - CWF_PLANE_WAVE_TOLERANCE is a P wave, q <= CWF_PLANE_WAVE_TOLERANCE an
 * S wave, anything between is refused. Its stress is sigma = -(g / c) [lambda (d . khat) I + mu (d khat^T + khat
 * d^T)]. A boundary node gets the dashpot's share plus the free-field traction,
 *     A_n = sum over its faces (a_f / k_f) [rho (V_p nu nu^T + V_s (I - nu nu^T)) d + S nu],   S = sigma / g,
 * nu the face's outward unit normal (away from the owning element's centroid, whatever the face's winding), a_f and
 * k_f as in cwf_absorbing_dashpots; the first term sums to C_n d. tau_n = khat . (x_n - x0) / c. For khat = -nu on a
 * flat face this is 2 C_n d with equal delays, cwf.absorbing.incident_pattern. Mesh, materials and faces as in
 * cwf_absorbing_dashpots, and its errors; all owning elements must share one material: CWF_ERR_UNSUPPORTED "plane wave
 * faces span more than one material" {face=<i>, material=<m>, first_material=<m0>}. CWF_ERR_ARGUMENT "propagation
 * must be a non-zero finite vector", "polarisation must be a non-zero finite vector", "polarisation is neither
 * parallel nor perpendicular to the propagation" {cosine=<q>}. Out: *count nodes ascending in node_ids, A (3 per
 * node), tau (1 per node), room as in cwf_absorbing_dashpots; *wave_speed (nullable) = c. */
#define CWF_PLANE_WAVE_TOLERANCE 1e-9
int cwf_absorbing_incident_plane(uint64_t node_count, const double *coords, uint64_t element_count,
                                 uint32_t nodes_per_element, const uint32_t *connectivity,
                                 const uint32_t *element_material, uint64_t material_count, const double *rho,
                                 const double *lame_lambda, const double *lame_mu, uint64_t face_count,
                                 uint32_t nodes_per_face, const uint32_t *faces, const double polarisation[3],
                                 const double propagation[3], const double origin[3], uint64_t *count,
                                 uint32_t *node_ids, double *A, double *tau, double *wave_speed);
/* lambda_max of M^-1 K over the free DOFs by `iterations` (0 -> 60) power iterations from a fixed start vector (a hash
 * of the node index), the handle's operator at scalars (1, 0) and fp64 dots in a fixed order: the same handle gives
 * the same bits on every call. The estimate is the quotient (K x . M^-1 K x) / (x . K x), which approaches lambda_max
 * from below; *last_change (nullable) is the last iteration's relative change of it. */
int cwf_hip_lambda_max(cwf_hip_system *h, uint32_t iterations, double *lambda_max, double *last_change);
/* Host only, no GPU: the damped stability limit above (2 / sqrt(lambda_max) when rayleigh_beta == 0). */
double cwf_explicit_critical_dt(double lambda_max, double rayleigh_beta);
/* Host only, no GPU: evaluate_curve (loads.cpp:63-85) on n points; 1.0 for n == 0. */
double cwf_explicit_curve_value(const double *times, const double *values, uint64_t n, double t);

/* ---------------------------------------------------------------------------------------
 * Multi-GPU: node-range shards with a ghost element layer (the north
 * star's "mesh shards ... RCCL all-reduce for the PCG dot products and halo-DOF exchange").
 * The reference itself is single-device; its src/gpu/sharding.cpp:38-144 (plan_shards) only
 * splits packed buffers under Vulkan's 2 GiB cap, which HBM handles do not need.
 * ------------------------------------------------------------------------------------- */

/* Host-only (no GPU needed). Rank `rank` of `nranks` owns global nodes
 * [rank_node_begin[rank], rank_node_begin[rank+1]). `desc` is the global mesh or any sub-mesh
 * holding every element that touches an owned node (in ascending global element order);
 * node_global_ids maps desc node -> global id (NULL = identity). The shard's local system has
 * the owned nodes first (ascending global id), then the ghosts grouped by owner rank. */
typedef struct cwf_shard cwf_shard;
typedef struct cwf_shard_info
{
    uint64_t owned_nodes;          /* local ids [0, owned_nodes) */
    uint64_t local_nodes;          /* owned + ghost */
    uint64_t local_elements;
    uint32_t neighbor_count;
    uint32_t reserved;
    const int32_t *neighbor_ranks; /* [neighbor_count], ascending */
    const uint64_t *send_offsets;  /* [neighbor_count + 1] into send_nodes */
    const uint32_t *send_nodes;    /* owned local ids each neighbour needs, ascending global id */
    const uint64_t *recv_offsets;  /* [neighbor_count + 1]: ghosts of neighbour k are local ids
                                      owned_nodes + [recv_offsets[k], recv_offsets[k+1]) */
    const uint64_t *node_global;   /* [local_nodes] global node id */
    const uint64_t *element_source; /* [local_elements] element index in the input desc */
    const uint64_t *node_source;    /* [local_nodes] node index in the input desc */
} cwf_shard_info;

int cwf_shard_build(const cwf_system_desc *desc, const uint64_t *node_global_ids, const uint64_t *rank_node_begin,
                    int32_t nranks, int32_t rank, cwf_shard **out);
/* local_desc: the shard's local system (arrays owned by the shard; adjacency NULL) */
int cwf_shard_get(const cwf_shard *shard, cwf_system_desc *local_desc, cwf_shard_info *info);
void cwf_shard_destroy(cwf_shard *shard);

/* Communicators. RCCL: one process per GPU (ncclCommInitRank; the 128-byte unique id is made by
 * rank 0 and broadcast by the caller, e.g. over torch.distributed). LOCAL: every rank's handle
 * lives in this process on one device (exchanges are device copies on one shared stream); it runs
 * the identical sharded kernels and exists to test the decomposition on a single GPU. */
#define CWF_COMM_ID_BYTES 128
typedef struct cwf_hip_comm cwf_hip_comm;
int cwf_hip_comm_unique_id(uint8_t *id);
int cwf_hip_comm_create_rccl(int32_t nranks, int32_t rank, const uint8_t *id, int device, cwf_hip_comm **out);
int cwf_hip_comm_create_local(int32_t nranks, int device, cwf_hip_comm **out);
void cwf_hip_comm_destroy(cwf_hip_comm *comm); /* after every attached handle is destroyed */

/* PEER: one process per rank, as RCCL, but the FAST exchange steps (the per-rank scalar all-gathers and the
 * halos) are device-initiated stores into the peers' IPC-mapped mailboxes plus a flag per step (peer.hip; the
 * "one-shot P2P" of SURVEY.md section 7 (iv)); PARITY's chunk-partial all-gathers are refused
 * (CWF_ERR_UNSUPPORTED: use RCCL). Setup: create, cwf_hip_system_attach (allocates this rank's mailbox),
 * cwf_hip_comm_peer_handle, exchange the handles between the processes (e.g. torch.distributed
 * all_gather_object), cwf_hip_comm_peer_connect with every rank's handle in rank order. Replaces the RCCL
 * group calls comm.cpp issues where pcg.cpp:170-207's dots would cross ranks. <= 16 ranks. */
#define CWF_IPC_HANDLE_BYTES 64
int cwf_hip_comm_create_peer(int32_t nranks, int32_t rank, int device, cwf_hip_comm **out);
int cwf_hip_comm_peer_handle(cwf_hip_comm *comm, uint8_t *handle /* [CWF_IPC_HANDLE_BYTES] */);
int cwf_hip_comm_peer_connect(cwf_hip_comm *comm, const uint8_t *handles /* [nranks * CWF_IPC_HANDLE_BYTES] */);
/* `steps` exchange steps shaped like the FAST PCG iteration's second one (the {r.r, r.z} all-gather and the z
 * halo) on the attached handle's stream, hipEvent-timed: microseconds per step (collective: every rank calls);
 * any communicator kind. An untimed first step carries a known pattern in z (owned rows = f(global id), the
 * plan's node_global) and every ghost row must arrive as its owner's value, else CWF_ERR_COMM "halo check failed"
 * {ghost, global}; z is clobbered (the next solve recomputes it). */
int cwf_hip_comm_time_exchange(cwf_hip_system *h, int32_t steps, double *us_per_step);
/* the memory this rank's PEER mailbox was allocated in (after attach): uncached device memory
 * (hipDeviceMallocUncached: another device's xGMI stores are visible without trusting the receiver's L2), else
 * fine-grained, else plain device memory when neither allocation can be IPC-exported. A PEER step whose wait times
 * out marks the communicator dead (a sticky device word): every later step returns CWF_ERR_COMM at once, and
 * cwf_hip_comm_time_exchange reports such a trial as CWF_ERR_COMM. */
#define CWF_PEER_MAILBOX_DEVICE 0
#define CWF_PEER_MAILBOX_FINEGRAINED 1
#define CWF_PEER_MAILBOX_UNCACHED 2
int cwf_hip_comm_peer_mailbox_kind(const cwf_hip_comm *comm, int *kind);

/* Make `h` (created from a shard's local desc with CWF_DESC_KEEP_NODE_ORDER) rank `rank` of `comm` with the
 * shard's halo plan. Afterwards solve_pcg / stepper_step are collective: scalars are all-gathered and folded
 * in rank order on every rank (identical control flow everywhere), ghost DOFs are refreshed by the halo
 * exchange, and vectors are local [3 * local_nodes] with only the owned rows meaningful on output (x is
 * halo-consistent). Both modes: FAST all-gathers one fp64 per rank per scalar (p.Ap; r.r and r.z with the z
 * halo in one RCCL group). PARITY all-gathers every rank's 256-DOF chunk partials and folds them in global
 * chunk order (pcg.cpp:170-207), so x, r and the residual history equal one handle's PARITY solve bit for
 * bit; it requires owned ranges that are contiguous, ascending by rank from node 0, and (all but the last)
 * whole reduction blocks: 3 * owned_nodes % reduction_block == 0 (cwf/shard.py slab_ranges(align=256)),
 * else CWF_ERR_UNSUPPORTED at the first solve. */
int cwf_hip_system_attach(cwf_hip_system *h, cwf_hip_comm *comm, int32_t rank, const cwf_shard_info *plan);
/* solve_pcg over all ranks of a LOCAL communicator (members in rank order); for RCCL call
 * cwf_hip_solve_pcg on each rank's handle. Telemetry is identical on every rank. residual_out (nullable, or
 * NULL entries) receives each member's local r (owned rows meaningful). */
int cwf_hip_solve_pcg_group(cwf_hip_system *const *members, int32_t count, const float *const *rhs,
                            const cwf_pcg_settings *settings, float *const *x_inout, float *const *residual_out,
                            int ptr_kind, cwf_pcg_telemetry *telemetry);

/* ---------------------------------------------------------------------------------------
 * Host-side preprocessing (no GPU needed): tet gradients/volume/lumped mass/CSR exactly as
 * mesh::pre::run + pack::build_packed_buffers (preprocess.cpp:268-405, pack.cpp:41-200).
 * Outputs are caller-allocated: grads[E*24], volume[E], mass[N] (f64) and mass32[N],
 * offsets[N+1], adj_elem[4E], adj_local[4E], conn8[8E].
 * ------------------------------------------------------------------------------------- */
int cwf_preprocess_tets(uint64_t node_count, uint64_t element_count, const double *coords, const uint32_t *tets,
                        const uint32_t *material_index, const double *density, uint64_t material_count,
                        float *grads24, float *volume, double *mass64, float *mass32, uint32_t *offsets,
                        uint32_t *adj_elem, uint8_t *adj_local, uint32_t *conn8);

/* Native hex8 (no reference counterpart: the reference rejects hex8 in
 * preprocess.cpp:326-330, so parity is unpinned). Trilinear isoparametric element, Gmsh/VTK corner
 * order, 2x2x2 Gauss: volume = sum_gp det J, lumped mass rho V / 8 per corner, grads24 = dN_a/dx at
 * the element centre; CSR with 8E incidences (adj_local 0..7); conn8 = hexes. A system_desc whose
 * connectivity fills all 8 slots is a hex8 system: CWF_MODE_FAST only, node_coords required.
 * Errors: "hexahedron Jacobian non-positive (inverted or degenerate)" {"elements [e]"} (CWF_ERR_SIZE). */
int cwf_preprocess_hex8(uint64_t node_count, uint64_t element_count, const double *coords, const uint32_t *hexes,
                        const uint32_t *material_index, const double *density, uint64_t material_count,
                        float *grads24, float *volume, double *mass64, float *mass32, uint32_t *offsets,
                        uint32_t *adj_elem, uint8_t *adj_local, uint32_t *conn8);

/* ---- post stack ---------------------------------------------------------- */

/* cwf::post::compute_derived_fields (src/post/derived_fields.cpp:139-211), on the device and bit-exact:
 * u = displacement f32 [3N] node-interleaved (n = dof_count); outputs are 13 floats per element /
 * node {strain[6] (Voigt, engineering shear), stress[6], von_mises} -- the memory layout of
 * cwf::post::ElementField / NodeField (derived_fields.hpp:37-55). `elements` [13E] or `nodes` [13N] may
 * be NULL. */
int cwf_hip_derived_fields(cwf_hip_system *h, const float *u, uint64_t n, int u_kind, float *elements,
                           float *nodes, int out_kind);

/* One output frame, host memory (the PackingResult node buffers + DerivedFieldSet the reference
 * writers read). Vectors are node-interleaved f32 [3N]; connectivity is the packed u32 [8E] with
 * UINT32_MAX padding (4 valid slots = tet4 / VTK 10, otherwise hex8 / VTK 12). */
typedef struct cwf_frame_view
{
    uint64_t node_count;
    uint64_t element_count;
    const float *position0;      /* pack.hpp:96 Float3SoA position0 (f32) */
    const float *displacement;
    const float *velocity;
    const float *acceleration;
    const float *element_fields; /* [13E] */
    const float *node_fields;    /* [13N] */
    const uint32_t *connectivity;
    /* the explicit stepper's plasticity (both NULL: none): two more Float32 cell arrays of the VTU frame,
     * plastic_strain (6 components) and equivalent_plastic_strain; the probe logger does not read them */
    const float *plastic_strain;            /* [6E] */
    const float *equivalent_plastic_strain; /* [E] */
} cwf_frame_view;

/* cwf::post::write_vtu (vtu_writer.cpp:171-297): binary-appended UnstructuredGrid, byte-identical to
 * the reference writer; parent directories are created. Errors: CWF_ERR_IO "failed to open VTU file"
 * {path}. cwf_hip_last_error(NULL) holds the message. */
int cwf_write_vtu(const char *path, const cwf_frame_view *frame, double simulation_time, uint32_t frame_index);

/* cwf::post::ProbeLogger::log_frame (probe_logger.cpp:91-124): appends one CSV row per probe node;
 * *header_written is the logger's header_written_ flag (0 -> truncate + header first, then set to 1).
 * Errors: "probe index out of range" {index} (CWF_ERR_INDEX), "failed to open probe CSV" (CWF_ERR_IO). */
int cwf_probe_log_frame(const char *path, int *header_written, const uint32_t *probes, uint64_t probe_count,
                        const cwf_frame_view *frame, double simulation_time, uint32_t frame_index);

/* ---- scenario front-end ------------------------------------------------------- */
/* Error contexts of these calls are the reference's breadcrumb vectors joined with '\n'. */

/* cwf::config::load_config_from_file / load_config_from_string (src/config/config.cpp:118-146) with
 * parse_config_node's validation (:148-605): same messages and breadcrumbs, e.g. "material.E must be
 * > 0" {"materials", "[0]", "E"} (CWF_ERR_PARSE). The YAML subset is parsed natively (no yaml-cpp). */
typedef struct cwf_config cwf_config;
int cwf_config_load_file(const char *path, cwf_config **out);
int cwf_config_load_string(const char *yaml_text, cwf_config **out);
/* the validated Config as canonical JSON (field names of config.hpp:41-237, doubles %.17g) */
const char *cwf_config_json(const cwf_config *cfg);
void cwf_config_destroy(cwf_config *cfg);

/* cwf::mesh::load_gmsh_file / load_gmsh_from_string (src/mesh/mesh.cpp:459-566): Gmsh MSH 4.1 ASCII. */
typedef struct cwf_mesh cwf_mesh;
typedef struct cwf_mesh_info
{
    uint64_t node_count;
    uint64_t element_count; /* volume elements (tet4 / hex8) */
    uint64_t surface_count; /* tri3 / quad4 boundary faces */
    uint64_t group_count;   /* physical groups */
} cwf_mesh_info;
int cwf_mesh_load_file(const char *path, cwf_mesh **out);
int cwf_mesh_load_string(const char *text, cwf_mesh **out);
void cwf_mesh_destroy(cwf_mesh *mesh);
int cwf_mesh_get_info(const cwf_mesh *mesh, cwf_mesh_info *info);
/* coords f64 [3N] (xyz per node, file order), original_ids u32 [N]; either may be NULL */
int cwf_mesh_nodes(const cwf_mesh *mesh, double *coords, uint32_t *original_ids);
/* nodes8 u32 [8E] (UINT32_MAX padded), geometry u8 [E] (4 = tet4, 8 = hex8), physical_group u32 [E] */
int cwf_mesh_elements(const cwf_mesh *mesh, uint32_t *nodes8, uint8_t *geometry, uint32_t *physical_group,
                      uint32_t *original_ids);
/* nodes4 u32 [4S] (UINT32_MAX padded), geometry u8 [S] (3 = tri3, 4 = quad4), physical_group u32 [S] */
int cwf_mesh_surfaces(const cwf_mesh *mesh, uint32_t *nodes4, uint8_t *geometry, uint32_t *physical_group);
/* physical group `index` (0 .. group_count-1, ascending id); *name stays valid until destroy */
int cwf_mesh_group(const cwf_mesh *mesh, uint64_t index, uint32_t *dimension, uint32_t *id, const char **name);
/* node indices tagged with physical group `group_id` through $Entities (Mesh::node_groups) */
int cwf_mesh_node_group(const cwf_mesh *mesh, uint32_t group_id, const uint32_t **nodes, uint64_t *count);

/* ---- native scenario driver ----------------------------------------------------
 * The viewer backend's sequence (src/ui/viewer.cpp:200-277) in C++: load_config_from_file ->
 * load_gmsh_file -> pre::run + pack::build_packed_buffers (loads at t = 0) -> Stepper; per frame
 * step(simulation_time) with simulation_time = telemetry.simulation_time + time_step, then
 * OutputManager::handle_frame (output_manager.cpp:49-87). The mesh path is taken as given, else
 * next to the YAML file. An all-hex8 mesh runs as native hex8 in CWF_MODE_FAST. Errors carry the
 * reference's texts prefixed "config: ", "mesh: " or "preprocess: "; every call leaves its message in
 * cwf_hip_last_error(NULL) / cwf_hip_last_context(NULL). */
typedef struct cwf_scenario cwf_scenario;
#define CWF_SCENARIO_TIME_VARYING_LOADS 1 /* re-evaluate load curves at each step's start time */
#define CWF_SCENARIO_PACK_ONLY 2          /* build the packed buffers only, no device handle (host tests) */
int cwf_scenario_create(const char *yaml_path, int mode, int device, int flags, cwf_scenario **out);
int cwf_scenario_info(const cwf_scenario *sc, uint64_t *nodes, uint64_t *elements, uint64_t *dofs);
/* one Newmark frame (Stepper::step errors, e.g. "CG denominator approached zero") */
int cwf_scenario_step(cwf_scenario *sc, int paused, cwf_step_telemetry *telemetry);
/* derived fields of the last stepped frame -> <out_root>/vtu/frame_%05u.vtu every vtu_stride frames
 * and one probe row per probe to <out_root>/probes/probes.csv */
int cwf_scenario_output_frame(cwf_scenario *sc, const char *out_root);
/* the Stepper's state after the last step (newmark_stepper.hpp:92-190: the pack's displacement / velocity /
 * acceleration node buffers, f32 [3N] each) and the derived fields OutputManager::handle_frame computes from it
 * (output_manager.cpp:49-87 -> derived_fields.cpp:139-211: element f32 [13E], node f32 [13N], the layout of
 * cwf_hip_derived_fields); any pointer may be NULL */
int cwf_scenario_state(cwf_scenario *sc, float *u, float *v, float *a, float *element_fields, float *node_fields);
/* read-only view of one packed host buffer (pack.hpp:93-183 names): position0, external_force, bc_mask,
 * bc_value, lumped_mass, lumped_mass64, connectivity, gradients, volume, material_index, offsets,
 * element_indices, local_indices. Unknown name: CWF_ERR_ARGUMENT. */
int cwf_scenario_packed(const cwf_scenario *sc, const char *name, const void **data, uint64_t *bytes);
/* loads.cpp:87-174 assemble_load_vector at `time`, cast like pack.cpp:41-57 -> out f32 [3N] */
int cwf_scenario_external_force(const cwf_scenario *sc, double time, float *out, uint64_t n);
void cwf_scenario_destroy(cwf_scenario *sc);

#ifdef __cplusplus
}
#endif
#endif /* CWF_HIP_H */
