// cwf_hip.hpp -- C++20 host mirror of CiviWave's L4 solver-core interface over the C-ABI.
//
// Same names, argument meaning and error behaviour as the reference headers:
//   cwf::hip::pcg::{MatrixFreeSystem, MatrixFreeWorkspace, PcgVectors, PcgSettings, PcgTelemetry,
//                   PcgError, apply_keff, solve_pcg, build_block_jacobi_inverse}
//       <- include/cwf/gpu/pcg.hpp:47-227
//   cwf::hip::newmark::{Stepper, StepTelemetry, StepError, AdaptivePolicy}
//       <- include/cwf/gpu/newmark_stepper.hpp:49-190
// Results are cwf::hip::expected<T, E> (std::expected is C++23; this header targets C++20 so it
// builds with the image's g++ 11). Header-only; link libcwf_hip.so.
//
// Device state: the first call with a workspace uploads the system's spans to HBM and keeps the
// handle in the workspace (the reference reuses one workspace per system, pcg.hpp:91-97), so
// a workspace must not be shared between different meshes. stiffness_scale / mass_factor are
// pushed on every call.
#pragma once

#include <array>
#include <cstdint>
#include <span>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "cwf_hip.h"

namespace cwf::hip
{

template <class E> struct unexpected
{
    E error;
};

template <class T, class E> class expected
{
public:
    expected(T v) : v_(std::in_place_index<0>, std::move(v)) {}
    expected(unexpected<E> u) : v_(std::in_place_index<1>, std::move(u.error)) {}
    bool has_value() const noexcept { return v_.index() == 0; }
    explicit operator bool() const noexcept { return has_value(); }
    T &value() { return std::get<0>(v_); }
    const T &value() const { return std::get<0>(v_); }
    T &operator*() { return value(); }
    T *operator->() { return &value(); }
    const E &error() const { return std::get<1>(v_); }

private:
    std::variant<T, E> v_;
};

template <class E> class expected<void, E>
{
public:
    expected() = default;
    expected(unexpected<E> u) : err_(std::move(u.error)), ok_(false) {}
    bool has_value() const noexcept { return ok_; }
    explicit operator bool() const noexcept { return ok_; }
    const E &error() const { return err_; }

private:
    E err_{};
    bool ok_ = true;
};

namespace pcg
{

struct PcgError
{
    std::string message;
    std::vector<std::string> context;
};

// materials[m] = ElasticProperties::stiffness (6x6 Voigt, row-major)
struct MatrixFreeSystem
{
    std::span<const std::uint32_t> element_connectivity;
    std::span<const float> element_gradients;
    std::span<const float> element_volume;
    std::span<const std::uint32_t> element_material_index;
    std::span<const std::array<double, 36>> materials;
    std::span<const float> lumped_mass;
    std::span<const std::uint32_t> bc_mask;
    std::size_t node_count{};
    std::size_t element_count{};
    std::size_t dof_count{};
    double stiffness_scale{};
    double mass_factor{};
    std::size_t reduction_block{};
    std::size_t reduction_partials{};
    int mode = CWF_MODE_PARITY;  // build extension: PARITY (bit-exact) or FAST
    int device = 0;              // build extension: HIP device ordinal
};

struct MatrixFreeWorkspace
{
    cwf_hip_system *handle = nullptr;
    MatrixFreeWorkspace() = default;
    MatrixFreeWorkspace(const MatrixFreeWorkspace &) = delete;
    MatrixFreeWorkspace &operator=(const MatrixFreeWorkspace &) = delete;
    MatrixFreeWorkspace(MatrixFreeWorkspace &&o) noexcept : handle(std::exchange(o.handle, nullptr)) {}
    ~MatrixFreeWorkspace() { cwf_hip_system_destroy(handle); }
};

struct PcgVectors
{
    std::span<float> solution;
    std::span<float> residual;
    std::span<float> search_direction;  // scratch lives in HBM; kept for signature parity
    std::span<float> preconditioned;
    std::span<float> matvec;
    std::span<double> partials;
};

struct PcgSettings
{
    std::size_t max_iterations{128U};
    double relative_tolerance{3.0e-4};
    bool warm_start{false};
};

struct PcgTelemetry
{
    std::size_t iterations{};
    double residual_norm{};
    double rhs_norm{};
    double alpha_last{};
    double beta_last{};
    bool converged{};
};

namespace detail
{
// breadcrumb vectors cross the ABI joined with '\n'
inline std::vector<std::string> split_context(const std::string &ctx)
{
    std::vector<std::string> out;
    if (ctx.empty())
        return out;
    size_t b = 0;
    for (;;)
    {
        const size_t e = ctx.find('\n', b);
        out.push_back(ctx.substr(b, e == std::string::npos ? std::string::npos : e - b));
        if (e == std::string::npos)
            return out;
        b = e + 1;
    }
}

inline PcgError last(const cwf_hip_system *h)
{
    return PcgError{cwf_hip_last_error(h), split_context(cwf_hip_last_context(h))};
}

inline expected<cwf_hip_system *, PcgError> bind(const MatrixFreeSystem &s, MatrixFreeWorkspace &ws)
{
    if (!ws.handle)
    {
        std::vector<double> mats;
        for (const auto &m : s.materials)
            mats.insert(mats.end(), m.begin(), m.end());
        cwf_system_desc d{};
        d.node_count = s.node_count;
        d.element_count = s.element_count;
        d.dof_count = s.dof_count;
        d.element_connectivity = s.element_connectivity.data();
        d.element_gradients = s.element_gradients.data();
        d.element_volume = s.element_volume.data();
        d.element_material_index = s.element_material_index.data();
        d.material_stiffness = mats.empty() ? nullptr : mats.data();
        d.material_count = s.materials.size();
        d.lumped_mass = s.lumped_mass.data();
        d.bc_mask = s.bc_mask.data();
        d.stiffness_scale = s.stiffness_scale;
        d.mass_factor = s.mass_factor;
        d.reduction_block = s.reduction_block;
        d.reduction_partials = s.reduction_partials;
        d.mode = s.mode;
        if (s.element_connectivity.size() != s.element_count * 8U)
            return unexpected<PcgError>{{"connectivity size mismatch",
                                         {"expected=" + std::to_string(s.element_count * 8U),
                                          "actual=" + std::to_string(s.element_connectivity.size())}}};
        if (s.element_gradients.size() != s.element_count * 24U)
            return unexpected<PcgError>{{"gradient table size mismatch",
                                         {"expected=" + std::to_string(s.element_count * 24U),
                                          "actual=" + std::to_string(s.element_gradients.size())}}};
        if (s.element_volume.size() != s.element_count || s.element_material_index.size() != s.element_count ||
            s.bc_mask.size() != s.node_count || s.lumped_mass.size() != s.node_count)
            return unexpected<PcgError>{{"system table size mismatch", {}}};
        if (cwf_hip_system_create(&d, s.device, &ws.handle) != 0)
            return unexpected<PcgError>{last(nullptr)};
    }
    cwf_hip_system_set_scalars(ws.handle, s.stiffness_scale, s.mass_factor);
    cwf_hip_system_set_mode(ws.handle, s.mode);
    return ws.handle;
}
}  // namespace detail

// pcg.hpp:161-163
[[nodiscard]] inline auto apply_keff(const MatrixFreeSystem &system, std::span<const float> input,
                                     std::span<float> output, MatrixFreeWorkspace &workspace)
    -> expected<void, PcgError>
{
    if (input.size() != system.dof_count || output.size() != system.dof_count)
        return unexpected<PcgError>{{"input/output span size mismatch",
                                     {"input=" + std::to_string(input.size()),
                                      "output=" + std::to_string(output.size()),
                                      "dofs=" + std::to_string(system.dof_count)}}};
    auto h = detail::bind(system, workspace);
    if (!h)
        return unexpected<PcgError>{h.error()};
    if (cwf_hip_apply_keff(*h, input.data(), output.data(), input.size(), CWF_PTR_HOST) != 0)
        return unexpected<PcgError>{detail::last(*h)};
    return {};
}

// pcg.hpp:210-212
[[nodiscard]] inline auto solve_pcg(const MatrixFreeSystem &system, std::span<const float> rhs,
                                    const PcgSettings &settings, PcgVectors vectors, MatrixFreeWorkspace &workspace)
    -> expected<PcgTelemetry, PcgError>
{
    if (rhs.size() != system.dof_count)
        return unexpected<PcgError>{{"rhs span size mismatch", {"rhs=" + std::to_string(rhs.size()),
                                                                 "dofs=" + std::to_string(system.dof_count)}}};
    if (vectors.solution.size() != system.dof_count)
        return unexpected<PcgError>{{"solver vector span size mismatch", {}}};
    auto h = detail::bind(system, workspace);
    if (!h)
        return unexpected<PcgError>{h.error()};
    cwf_pcg_settings cs{settings.max_iterations, settings.relative_tolerance, settings.warm_start ? 1 : 0, 0};
    cwf_pcg_telemetry t{};
    float *res = vectors.residual.size() == system.dof_count ? vectors.residual.data() : nullptr;
    if (cwf_hip_solve_pcg(*h, rhs.data(), &cs, vectors.solution.data(), res, rhs.size(), CWF_PTR_HOST, &t) != 0)
        return unexpected<PcgError>{detail::last(*h)};
    return PcgTelemetry{t.iterations, t.residual_norm, t.rhs_norm, t.alpha_last, t.beta_last, t.converged != 0};
}

// pcg.hpp:226-227
[[nodiscard]] inline auto build_block_jacobi_inverse(const MatrixFreeSystem &system, MatrixFreeWorkspace &workspace,
                                                     std::span<float> out_inverse) -> expected<void, PcgError>
{
    const auto required = system.node_count * 9U;
    if (out_inverse.size() < required)
        return unexpected<PcgError>{{"block inverse span too small", {"required=" + std::to_string(required),
                                                                      "available=" +
                                                                          std::to_string(out_inverse.size())}}};
    auto h = detail::bind(system, workspace);
    if (!h)
        return unexpected<PcgError>{h.error()};
    if (cwf_hip_build_block_jacobi_inverse(*h, out_inverse.data(), out_inverse.size(), CWF_PTR_HOST) != 0)
        return unexpected<PcgError>{detail::last(*h)};
    return {};
}

// Refined static solve (cwf_hip_solve_refined; no reference counterpart): fp64 x and b, the tolerance on the true
// residual |b - K_eff x| / |b|, iterative refinement around the handle's own PCG.
struct RefineSettings
{
    std::uint32_t max_outer{12};
    double relative_tolerance{1.0e-10};
    double stagnation_ratio{0.5};
    PcgSettings inner{20000, 1.0e-4, false};  // inner solves (warm_start is ignored)
    bool warm_start{false};                   // solution holds a start value
};

struct RefineTelemetry
{
    std::uint32_t outer_iterations{0};
    std::uint64_t inner_iterations{0};
    double residual_norm{0.0}, rhs_norm{0.0};  // fp64, true
    bool converged{false}, stagnated{false};
    std::vector<double> history;               // |r| before each inner solve, then the final one
    double residual_ms{0.0}, solve_ms{0.0};
};

[[nodiscard]] inline auto solve_refined(const MatrixFreeSystem &system, std::span<const double> rhs,
                                        const RefineSettings &settings, std::span<double> solution,
                                        MatrixFreeWorkspace &workspace) -> expected<RefineTelemetry, PcgError>
{
    if (rhs.size() != system.dof_count || solution.size() != system.dof_count)
        return unexpected<PcgError>{{"rhs span size mismatch", {"rhs=" + std::to_string(rhs.size()),
                                                                 "dofs=" + std::to_string(system.dof_count)}}};
    auto h = detail::bind(system, workspace);
    if (!h)
        return unexpected<PcgError>{h.error()};
    cwf_refine_settings cs{};
    cs.max_outer = settings.max_outer;
    cs.relative_tolerance = settings.relative_tolerance;
    cs.stagnation_ratio = settings.stagnation_ratio;
    cs.inner = cwf_pcg_settings{settings.inner.max_iterations, settings.inner.relative_tolerance, 0, 0};
    cs.warm_start = settings.warm_start ? 1 : 0;
    cwf_refine_telemetry t{};
    if (cwf_hip_solve_refined(*h, rhs.data(), &cs, solution.data(), rhs.size(), CWF_PTR_HOST, &t) != 0)
        return unexpected<PcgError>{detail::last(*h)};
    RefineTelemetry r{t.outer_iterations, t.inner_iterations, t.residual_norm, t.rhs_norm, t.converged != 0,
                      t.stagnated != 0,   {},                 t.residual_ms,   t.solve_ms};
    r.history.assign(t.history, t.history + t.outer_iterations + 1);
    return r;
}

// r = b - K_eff x in fp64 (cwf_hip_residual_f64): the value is |r|; residual (dof_count, or empty) receives r
[[nodiscard]] inline auto residual_f64(const MatrixFreeSystem &system, std::span<const double> rhs,
                                       std::span<const double> x, std::span<double> residual,
                                       MatrixFreeWorkspace &workspace) -> expected<double, PcgError>
{
    if (rhs.size() != system.dof_count || x.size() != system.dof_count ||
        (!residual.empty() && residual.size() != system.dof_count))
        return unexpected<PcgError>{{"rhs span size mismatch", {"rhs=" + std::to_string(rhs.size()),
                                                                 "dofs=" + std::to_string(system.dof_count)}}};
    auto h = detail::bind(system, workspace);
    if (!h)
        return unexpected<PcgError>{h.error()};
    double norm = 0.0;
    if (cwf_hip_residual_f64(*h, rhs.data(), x.data(), residual.empty() ? nullptr : residual.data(), rhs.size(),
                             CWF_PTR_HOST, &norm) != 0)
        return unexpected<PcgError>{detail::last(*h)};
    return norm;
}

}  // namespace pcg

// Modal analysis (cwf_hip_modal_solve; no reference counterpart): the lowest eigenpairs of K phi = lambda M phi.
namespace modal
{

struct ModalSettings
{
    std::uint32_t modes{6};
    std::uint32_t block{0};       // 0: min(2 modes, modes + 8)
    std::uint32_t max_outer{40};
    double tolerance{1.0e-6};
    double shift{0.0};
    pcg::PcgSettings pcg{20000, 1.0e-6, false};  // inner solves
};

struct ModalTelemetry
{
    std::uint32_t outer_iterations{0};
    bool converged{false};
    std::uint32_t block{0};
    std::uint64_t pcg_iterations{0};
    double max_change{0.0}, solve_ms{0.0}, block_ms{0.0};
};

struct ModalResult
{
    std::vector<double> eigenvalues;  // lambda, ascending
    std::vector<float> modes;         // [modes * dof_count], M-orthonormal, mode i at [i * dof_count]
    ModalTelemetry telemetry;
};

[[nodiscard]] inline auto solve(const pcg::MatrixFreeSystem &system, const ModalSettings &settings,
                                pcg::MatrixFreeWorkspace &workspace) -> expected<ModalResult, pcg::PcgError>
{
    auto h = pcg::detail::bind(system, workspace);
    if (!h)
        return unexpected<pcg::PcgError>{h.error()};
    cwf_modal_settings cs{};
    cs.modes = settings.modes;
    cs.block = settings.block;
    cs.max_outer = settings.max_outer;
    cs.tolerance = settings.tolerance;
    cs.shift = settings.shift;
    cs.pcg = cwf_pcg_settings{settings.pcg.max_iterations, settings.pcg.relative_tolerance, 0, 0};
    ModalResult r;
    r.eigenvalues.resize(settings.modes);
    r.modes.resize(static_cast<std::size_t>(settings.modes) * system.dof_count);
    cwf_modal_telemetry t{};
    if (cwf_hip_modal_solve(*h, &cs, r.eigenvalues.data(), r.modes.data(), CWF_PTR_HOST, &t) != 0)
        return unexpected<pcg::PcgError>{pcg::detail::last(*h)};
    r.telemetry = ModalTelemetry{t.outer_iterations, t.converged != 0, t.block, t.pcg_iterations,
                                 t.max_change,       t.solve_ms,       t.block_ms};
    return r;
}

}  // namespace modal

namespace newmark
{

struct StepError
{
    std::string message;
    std::vector<std::string> context;
};

struct AdaptivePolicy
{
    double low_iteration_ratio{0.3};
    double increase_factor{1.1};
    double decrease_factor{0.5};
};

struct StepTelemetry
{
    double simulation_time{};
    double time_step{};
    double applied_tolerance{};
    bool paused_mode{};
    bool dt_increased{};
    bool dt_decreased{};
    bool dt_clamped_min{};
    bool dt_clamped_max{};
    pcg::PcgTelemetry pcg{};
};

struct SolverSettings  // config::SolverSettings subset (config.hpp:100-107)
{
    double runtime_tolerance{3.0e-4};
    double pause_tolerance{1.0e-5};
    std::uint32_t max_iterations{128};
};

struct TimeSettings  // config::TimeSettings (config.hpp:88-94)
{
    double initial_dt{0.01};
    bool adaptive{false};
    double min_dt{0.0};
    double max_dt{0.0};
};

struct Rayleigh
{
    double alpha{};
    double beta{};
};

// Stepper(packing, materials, rayleigh, solver_settings, time_settings, policy): the packing is
// the MatrixFreeSystem spans plus the node external force / Dirichlet values (dof = 3n+k).
class Stepper
{
public:
    Stepper(const pcg::MatrixFreeSystem &system, std::span<const float> external_force,
            std::span<const float> bc_value, Rayleigh rayleigh, const SolverSettings &solver,
            const TimeSettings &time, AdaptivePolicy policy = {})
    {
        auto h = pcg::detail::bind(system, ws_);
        if (!h)
        {
            init_error_ = StepError{h.error().message, h.error().context};
            return;
        }
        cwf_stepper_desc d{};
        d.rayleigh_alpha = rayleigh.alpha;
        d.rayleigh_beta = rayleigh.beta;
        d.runtime_tolerance = solver.runtime_tolerance;
        d.pause_tolerance = solver.pause_tolerance;
        d.max_iterations = solver.max_iterations;
        d.initial_dt = time.initial_dt;
        d.adaptive = time.adaptive ? 1 : 0;
        d.warm_start = 1;
        d.min_dt = time.min_dt;
        d.max_dt = time.max_dt;
        d.low_iteration_ratio = policy.low_iteration_ratio;
        d.increase_factor = policy.increase_factor;
        d.decrease_factor = policy.decrease_factor;
        d.external_force = external_force.data();
        d.bc_value = bc_value.data();
        if (cwf_hip_stepper_create(*h, &d, &st_) != 0)
            init_error_ = StepError{cwf_hip_last_error(*h), {cwf_hip_last_context(*h)}};
        dofs_ = system.dof_count;
    }
    ~Stepper() { cwf_hip_stepper_destroy(st_); }
    Stepper(const Stepper &) = delete;
    Stepper &operator=(const Stepper &) = delete;

    [[nodiscard]] auto step(double simulation_time_seconds, bool paused_mode = false)
        -> expected<StepTelemetry, StepError>
    {
        if (!st_)
            return unexpected<StepError>{init_error_};
        cwf_step_telemetry t{};
        if (cwf_hip_stepper_step(st_, simulation_time_seconds, paused_mode ? 1 : 0, &t) != 0)
            return unexpected<StepError>{{cwf_hip_last_error(ws_.handle), {cwf_hip_last_context(ws_.handle)}}};
        return StepTelemetry{t.simulation_time, t.time_step, t.applied_tolerance, t.paused_mode != 0,
                             t.dt_increased != 0, t.dt_decreased != 0, t.dt_clamped_min != 0, t.dt_clamped_max != 0,
                             pcg::PcgTelemetry{t.pcg.iterations, t.pcg.residual_norm, t.pcg.rhs_norm,
                                               t.pcg.alpha_last, t.pcg.beta_last, t.pcg.converged != 0}};
    }
    [[nodiscard]] auto current_time() const noexcept -> double
    {
        double c = 0.0;
        cwf_hip_stepper_time(st_, &c, nullptr);
        return c;
    }
    [[nodiscard]] auto time_step() const noexcept -> double
    {
        double d = 0.0;
        cwf_hip_stepper_time(st_, nullptr, &d);
        return d;
    }
    void set_warm_start(bool enabled) noexcept { cwf_hip_stepper_set_warm_start(st_, enabled ? 1 : 0); }
    // node state (0 displacement, 1 velocity, 2 acceleration), dof = 3n+k
    bool state(int which, std::span<float> out) const
    {
        return cwf_hip_stepper_get_state(st_, which, out.data(), out.size(), CWF_PTR_HOST) == 0;
    }
    bool set_external_force(std::span<const float> f)
    {
        return cwf_hip_stepper_set_external_force(st_, f.data(), f.size(), CWF_PTR_HOST) == 0;
    }
    // one curve-scaled point-load pattern on the device: after set_load_pattern(base, pattern), each
    // set_load_scale(evaluate_curve(curve, t)) writes external_force = safe_cast(base + c * pattern), bitwise
    // what assemble_load_vector packs at t (loads.cpp:63-172), without the host round trip of set_external_force
    bool set_load_pattern(std::span<const double> base, std::span<const double> pattern)
    {
        return base.size() == pattern.size() &&
               cwf_hip_stepper_set_load_pattern(st_, base.data(), pattern.data(), base.size()) == 0;
    }
    bool set_load_scale(double scale) { return cwf_hip_stepper_set_load_scale(st_, scale) == 0; }
    [[nodiscard]] auto dof_count() const noexcept -> std::size_t { return dofs_; }

private:
    pcg::MatrixFreeWorkspace ws_{};
    cwf_hip_stepper *st_ = nullptr;
    StepError init_error_{"stepper not initialised", {}};
    std::size_t dofs_ = 0;
};

}  // namespace newmark

// ---- post stack: include/cwf/post/{derived_fields,vtu_writer,probe_logger}.hpp ----------------------
namespace post
{
struct PostError
{
    std::string message;
    std::vector<std::string> context;
};

// derived_fields.hpp:37-55 (13 floats each; the C-ABI writes these layouts directly)
struct ElementField
{
    std::array<float, 6> strain{};
    std::array<float, 6> stress{};
    float von_mises{0.0F};
};
struct NodeField
{
    std::array<float, 6> strain{};
    std::array<float, 6> stress{};
    float von_mises{0.0F};
};
static_assert(sizeof(ElementField) == 13 * sizeof(float) && sizeof(NodeField) == 13 * sizeof(float));

struct DerivedFieldSet
{
    std::vector<ElementField> elements;
    std::vector<NodeField> nodes;
};

// derived_fields.hpp:97-99 compute_derived_fields(packing, materials): the system's element tables
// (bound to `workspace` on first use) and the packing's node displacement (dof = 3n+k)
[[nodiscard]] inline auto compute_derived_fields(const pcg::MatrixFreeSystem &system,
                                                 pcg::MatrixFreeWorkspace &workspace,
                                                 std::span<const float> displacement)
    -> expected<DerivedFieldSet, PostError>
{
    auto h = pcg::detail::bind(system, workspace);
    if (!h)
        return unexpected<PostError>{{h.error().message, h.error().context}};
    DerivedFieldSet d;
    d.elements.resize(system.element_count);
    d.nodes.resize(system.node_count);
    if (cwf_hip_derived_fields(*h, displacement.data(), displacement.size(), CWF_PTR_HOST,
                               reinterpret_cast<float *>(d.elements.data()), reinterpret_cast<float *>(d.nodes.data()),
                               CWF_PTR_HOST) != 0)
        return unexpected<PostError>{{cwf_hip_last_error(*h), pcg::detail::split_context(cwf_hip_last_context(*h))}};
    return d;
}

// the PackingResult node buffers the writers read (pack.hpp:95-105), node-interleaved f32 [3N]
struct FrameData
{
    std::span<const float> position0, displacement, velocity, acceleration;
    std::span<const std::uint32_t> connectivity;  // [8E] packed, UINT32_MAX padded
};

namespace detail
{
inline cwf_frame_view view(const FrameData &f, const DerivedFieldSet &d)
{
    return cwf_frame_view{f.position0.size() / 3,
                          f.connectivity.size() / 8,
                          f.position0.data(),
                          f.displacement.data(),
                          f.velocity.data(),
                          f.acceleration.data(),
                          reinterpret_cast<const float *>(d.elements.data()),
                          reinterpret_cast<const float *>(d.nodes.data()),
                          f.connectivity.data()};
}
}  // namespace detail

// vtu_writer.hpp:43-48
[[nodiscard]] inline auto write_vtu(const std::string &path, const FrameData &frame, const DerivedFieldSet &derived,
                                    double simulation_time, std::uint32_t frame_index) -> expected<void, PostError>
{
    const cwf_frame_view v = detail::view(frame, derived);
    if (cwf_write_vtu(path.c_str(), &v, simulation_time, frame_index) != 0)
        return unexpected<PostError>{{cwf_hip_last_error(nullptr), pcg::detail::split_context(cwf_hip_last_context(nullptr))}};
    return {};
}

// probe_logger.hpp:29-45
class ProbeLogger
{
public:
    ProbeLogger(std::string path, std::vector<std::uint32_t> probes) : path_(std::move(path)), probes_(std::move(probes)) {}
    [[nodiscard]] auto log_frame(double simulation_time, std::uint32_t frame_index, const FrameData &frame,
                                 const DerivedFieldSet &derived) -> expected<void, PostError>
    {
        const cwf_frame_view v = detail::view(frame, derived);
        if (cwf_probe_log_frame(path_.c_str(), &header_written_, probes_.data(), probes_.size(), &v, simulation_time,
                                frame_index) != 0)
            return unexpected<PostError>{{cwf_hip_last_error(nullptr), pcg::detail::split_context(cwf_hip_last_context(nullptr))}};
        return {};
    }

private:
    std::string path_;
    std::vector<std::uint32_t> probes_;
    int header_written_ = 0;
};
}  // namespace post

// ---- scenario front-end: include/cwf/{config/config,mesh/mesh}.hpp --------------------------------
namespace config
{
struct ConfigError
{
    std::string message;
    std::vector<std::string> context;
};
// config.hpp:272-285: the validated Config as canonical JSON (field names of config.hpp); the typed
// records are built by the host mirror that consumes it (civiwave-fem_amd/cwf/config.py)
[[nodiscard]] inline auto load_config_from_file(const std::string &path) -> expected<std::string, ConfigError>
{
    cwf_config *c = nullptr;
    if (cwf_config_load_file(path.c_str(), &c) != 0)
        return unexpected<ConfigError>{{cwf_hip_last_error(nullptr), pcg::detail::split_context(cwf_hip_last_context(nullptr))}};
    std::string j = cwf_config_json(c);
    cwf_config_destroy(c);
    return j;
}
[[nodiscard]] inline auto load_config_from_string(const std::string &yaml) -> expected<std::string, ConfigError>
{
    cwf_config *c = nullptr;
    if (cwf_config_load_string(yaml.c_str(), &c) != 0)
        return unexpected<ConfigError>{{cwf_hip_last_error(nullptr), pcg::detail::split_context(cwf_hip_last_context(nullptr))}};
    std::string j = cwf_config_json(c);
    cwf_config_destroy(c);
    return j;
}
}  // namespace config

namespace mesh
{
struct MeshError
{
    std::string message;
    std::vector<std::string> context;
};
struct PhysicalGroup
{
    std::uint32_t dimension{}, id{};
    std::string name;
};
// mesh.hpp:120-146, flattened: nodes xyz [3N]; elements [8E] UINT32_MAX padded with geometry 4 / 8
struct Mesh
{
    std::vector<double> positions;
    std::vector<std::uint32_t> node_ids;
    std::vector<std::uint32_t> elements;
    std::vector<std::uint8_t> geometry;
    std::vector<std::uint32_t> element_group;
    std::vector<std::uint32_t> surfaces;  // [4S]
    std::vector<std::uint8_t> surface_geometry;
    std::vector<std::uint32_t> surface_group;
    std::vector<PhysicalGroup> physical_groups;
    std::vector<std::pair<std::uint32_t, std::vector<std::uint32_t>>> node_groups;
};
namespace detail
{
inline auto take(int rc, cwf_mesh *m) -> expected<Mesh, MeshError>
{
    if (rc != 0)
        return unexpected<MeshError>{{cwf_hip_last_error(nullptr), pcg::detail::split_context(cwf_hip_last_context(nullptr))}};
    cwf_mesh_info i{};
    cwf_mesh_get_info(m, &i);
    Mesh out;
    out.positions.resize(3 * i.node_count);
    out.node_ids.resize(i.node_count);
    cwf_mesh_nodes(m, out.positions.data(), out.node_ids.data());
    out.elements.resize(8 * i.element_count);
    out.geometry.resize(i.element_count);
    out.element_group.resize(i.element_count);
    cwf_mesh_elements(m, out.elements.data(), out.geometry.data(), out.element_group.data(), nullptr);
    out.surfaces.resize(4 * i.surface_count);
    out.surface_geometry.resize(i.surface_count);
    out.surface_group.resize(i.surface_count);
    cwf_mesh_surfaces(m, out.surfaces.data(), out.surface_geometry.data(), out.surface_group.data());
    for (std::uint64_t g = 0; g < i.group_count; ++g)
    {
        PhysicalGroup pg;
        const char *name = nullptr;
        cwf_mesh_group(m, g, &pg.dimension, &pg.id, &name);
        pg.name = name ? name : "";
        const std::uint32_t *nodes = nullptr;
        std::uint64_t n = 0;
        cwf_mesh_node_group(m, pg.id, &nodes, &n);
        if (n)
            out.node_groups.emplace_back(pg.id, std::vector<std::uint32_t>(nodes, nodes + n));
        out.physical_groups.push_back(std::move(pg));
    }
    cwf_mesh_destroy(m);
    return out;
}
}  // namespace detail
// mesh.hpp:148-160
[[nodiscard]] inline auto load_gmsh_file(const std::string &path) -> expected<Mesh, MeshError>
{
    cwf_mesh *m = nullptr;
    const int rc = cwf_mesh_load_file(path.c_str(), &m);
    return detail::take(rc, m);
}
[[nodiscard]] inline auto load_gmsh_from_string(const std::string &text) -> expected<Mesh, MeshError>
{
    cwf_mesh *m = nullptr;
    const int rc = cwf_mesh_load_string(text.c_str(), &m);
    return detail::take(rc, m);
}
}  // namespace mesh

// ---- the viewer backend's scenario sequence (viewer.cpp:200-277) over cwf_scenario_* -------------
namespace scenario
{
struct ScenarioError
{
    std::string message;
    std::vector<std::string> context;
};
class Scenario
{
  public:
    [[nodiscard]] static auto create(const std::string &yaml_path, int mode = CWF_MODE_PARITY, int device = 0,
                                     int flags = 0) -> expected<Scenario, ScenarioError>
    {
        cwf_scenario *s = nullptr;
        if (cwf_scenario_create(yaml_path.c_str(), mode, device, flags, &s) != 0)
            return unexpected<ScenarioError>{{cwf_hip_last_error(nullptr), pcg::detail::split_context(cwf_hip_last_context(nullptr))}};
        return Scenario(s);
    }
    Scenario(Scenario &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Scenario &operator=(Scenario &&o) noexcept
    {
        std::swap(s_, o.s_);
        return *this;
    }
    Scenario(const Scenario &) = delete;
    Scenario &operator=(const Scenario &) = delete;
    ~Scenario() { cwf_scenario_destroy(s_); }
    // Stepper::step at the scenario clock (simulation_time = telemetry.simulation_time + time_step)
    [[nodiscard]] auto step(bool paused = false) -> expected<cwf_step_telemetry, ScenarioError>
    {
        cwf_step_telemetry t{};
        if (cwf_scenario_step(s_, paused ? 1 : 0, &t) != 0)
            return unexpected<ScenarioError>{{cwf_hip_last_error(nullptr), pcg::detail::split_context(cwf_hip_last_context(nullptr))}};
        return t;
    }
    // OutputManager::handle_frame of the last stepped frame under `root` (vtu/, probes/)
    [[nodiscard]] auto output_frame(const std::string &root) -> expected<void, ScenarioError>
    {
        if (cwf_scenario_output_frame(s_, root.c_str()) != 0)
            return unexpected<ScenarioError>{{cwf_hip_last_error(nullptr), pcg::detail::split_context(cwf_hip_last_context(nullptr))}};
        return {};
    }
    [[nodiscard]] std::uint64_t dof_count() const
    {
        std::uint64_t d = 0;
        cwf_scenario_info(s_, nullptr, nullptr, &d);
        return d;
    }

  private:
    explicit Scenario(cwf_scenario *s) : s_(s) {}
    cwf_scenario *s_ = nullptr;
};
}  // namespace scenario
}  // namespace cwf::hip
