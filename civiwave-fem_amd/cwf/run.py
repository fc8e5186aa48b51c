"""Scenario driver: YAML scenario -> Gmsh mesh -> preprocess/pack -> device Newmark steps -> VTU/probes.

    python -m cwf.run scenario.yaml [--steps N] [--out DIR] [--mode parity|fast] [--paused]
                                    [--time-varying-loads] [--device K]
                                    [--integrator newmark|explicit] [--safety 0.9]
                                    [--trace-every K] [--peaks] [--energy-every K] [--mass-damping-only]
                                    [--envelope-every K] [--gauges e0,e1,... [--gauge-every K]]

The reference has no such executable (its only binary is the viewer demo);
this wires its pieces in the order the viewer backend does (src/ui/viewer.cpp:200-277):
load_config_from_file -> load_gmsh_file -> pre::run + pack::build_packed_buffers -> Stepper, then per
frame ``step(simulation_time)``, ``simulation_time = telemetry.simulation_time + telemetry.time_step``
and OutputManager::handle_frame. The external force is evaluated once at pack time (t = 0), as in the
reference (newmark_stepper.cpp:1369-1379); ``--time-varying-loads`` re-evaluates the load curves at
every step's start time instead (the viewer's custom-load path, viewer.cpp:262-266).

``--integrator explicit`` runs the central-difference stepper (cwf.explicit) at ``--safety`` x its estimated critical
step instead: ``--steps`` still counts output frames, one every ceil(dt_scenario / dt_explicit) explicit steps (the
scenario's ``time.dt`` is the output interval), through the same VTU and probe writers; loads are those of t = 0.
A scenario's ``absorbing:`` entries (explicit only) put viscous dashpots on their groups' faces; an entry's
``incident: {direction, velocity_curve}`` feeds that curve in through the dashpots as an incident wave. With
``propagation: [x, y, z]`` (and ``origin``) the wave is a plane wave travelling obliquely along it, each boundary node
with its own arrival delay; such entries, and entries naming different curves, run as the stepper's load sources.
A top-level ``tied:`` list (explicit only) ties lateral boundaries: ``{group: NAME, axis: k}`` ties the group's nodes
level by level along axis k (a laminar box), ``{pair: [A, B], axis: k}`` the nodes of two opposite faces normal to axis
k pairwise (periodic); all entries are merged into one set, applied after the dashpots.
``--trace-every K``, ``--peaks`` and ``--energy-every K`` (explicit only) turn on the stepper's monitors: receiver
traces at ``output.probes`` every K explicit steps (``probes/traces.csv``), the peak |u|, |v|, |a| maps
(``monitors/peaks.npy``, [N,3]) and the energy ledger (``monitors/energy.csv``), written after the last frame. The
ledger needs beta_R == 0, which no scenario's ``damping:`` gives: ``--mass-damping-only`` keeps alpha_R and drops beta_R.
``--envelope-every K`` and ``--gauges e0,e1,... [--gauge-every K]`` (explicit only) turn on its element monitors: every
K explicit steps the peak von Mises stress, the peak effective shear strain and the min / max of the six stresses per
element (``monitors/envelope_von_mises.npy``, ``envelope_shear_strain.npy`` [E]; ``envelope_stress_min.npy``,
``envelope_stress_max.npy`` [E,6]), and the strain / stress / von Mises rows of the gauge elements
(``monitors/gauges.csv``, one line per sample and gauge).

Materials with a ``yield_stress`` yield by J2 plasticity (explicit only); materials with a ``friction_angle`` (degrees;
``cohesion``, ``dilation_angle``, ``hardening_modulus``) by the Drucker-Prager soil model, with the stress at rest of a
top-level ``geostatic: {gravity, k0, axis, surface}``. Either way the VTU frames carry ``plastic_strain`` and
``equivalent_plastic_strain`` per cell, and ``--plastic-summary`` logs the yielded elements and the plastic work.

Mesh paths are resolved like the reference (relative to the working directory) and, failing that,
relative to the YAML file's directory. One JSON line per step is printed; the last line is a summary.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

from . import _lib, config, mesh, pack, post
from .physics import compute_rayleigh, make_properties
from .stepper import Stepper


class ScenarioError(RuntimeError):
    pass


def resolve_mesh_path(cfg_path: str, mesh_path: str) -> str:
    if os.path.isabs(mesh_path) or os.path.exists(mesh_path):
        return mesh_path
    here = os.path.dirname(os.path.abspath(cfg_path))
    for cand in (os.path.join(here, mesh_path), os.path.join(here, os.path.basename(mesh_path))):
        if os.path.exists(cand):
            return cand
    return mesh_path


def load_scenario(cfg_path: str, allow_hex8: bool = False):
    """-> (config, tet mesh, packing, materials). Raises ScenarioError with the reference's texts.
    allow_hex8: an all-hex8 Gmsh mesh runs as native hex8 (FAST mode only)."""
    rc = config.load_config_from_file(cfg_path)
    if not rc.has_value():
        raise ScenarioError(f"config: {rc.error().message} {rc.error().context}")
    cfg = rc.value()
    rm = mesh.load_gmsh_file(resolve_mesh_path(cfg_path, cfg.mesh_path))
    if not rm.has_value():
        raise ScenarioError(f"mesh: {rm.error().message} {rm.error().context}")
    try:
        m = rm.value().to_tet_mesh(allow_hex8)
        P = pack.build_packed_buffers(m, cfg)
    except pack.PackError as e:
        raise ScenarioError(f"preprocess: {e.message} {e.context}") from None
    return cfg, m, P, [make_properties(x) for x in cfg.materials]


def run_scenario(cfg_path: str, steps: int, out_dir: str | None, mode: int = _lib.MODE_PARITY, device: int = 0,
                 paused: bool = False, time_varying_loads: bool = False, log=print) -> dict:
    cfg, m, P, materials = load_scenario(cfg_path, allow_hex8=mode == _lib.MODE_FAST)
    if cfg.absorbing:
        raise ScenarioError("absorbing boundaries need the explicit integrator")
    if cfg.tied:
        raise ScenarioError("tied boundaries need the explicit integrator")
    if any(x.yield_stress > 0.0 or x.friction_angle is not None for x in cfg.materials):
        raise ScenarioError("plastic materials need the explicit integrator")
    st = Stepper(P, materials, compute_rayleigh(cfg.damping), cfg.solver, cfg.time, mode=mode, device=device)
    om = post.OutputManager(out_dir, m, P, materials, cfg.output, stepper=st) if out_dir else None
    t_sim, total_iters, wall0 = 0.0, 0, time.perf_counter()
    last = None
    try:
        for frame in range(steps):
            if time_varying_loads:
                f = pack._safe_f32(pack.assemble_load_vector(m, cfg, P.lumped_mass64, t_sim))
                st.set_external_force(f)
            r = st.step(t_sim, paused)
            if not r.has_value():
                raise ScenarioError(f"step {frame}: {r.error().message} {r.error().context}")
            tel = r.value()
            t_sim = tel.simulation_time + tel.time_step
            total_iters += tel.pcg.iterations
            if om is not None:
                o = om.handle_frame(t_sim, frame)
                if not o.has_value():
                    raise ScenarioError(f"output frame {frame}: {o.error().message} {o.error().context}")
            last = dict(frame=frame, time=t_sim, dt=tel.time_step, iterations=tel.pcg.iterations,
                        residual=tel.pcg.residual_norm, converged=tel.pcg.converged,
                        dt_increased=tel.dt_increased, dt_decreased=tel.dt_decreased)
            log(json.dumps(last))
        wall = time.perf_counter() - wall0
        return dict(scenario=cfg_path, nodes=P.node_count, tets=P.element_count, dofs=P.dof_count, steps=steps,
                    pcg_iterations=total_iters, wall_s=wall, final_time=t_sim, last=last,
                    mode="fast" if mode == _lib.MODE_FAST else "parity")
    finally:
        if om is not None:
            om.close()
        st.close()
        st.system.close()


def set_soil_plasticity(st, cfg, P):
    """The scenario's soil model on an explicit stepper: materials with a ``friction_angle`` become Drucker-Prager
    cones through the Mohr-Coulomb compression corners, ``hardening_modulus`` hardening the cohesion; materials
    without one stay elastic. A stepper holds one plasticity set, so J2 materials (``yield_stress``) of the same
    scenario enter as the cone without friction that is the same surface (alpha = beta = 0, kappa = sy / sqrt3,
    H / 3), which is said on stderr. ``geostatic:`` gives the stress at rest; without it there is none."""
    import math

    import numpy as np

    from . import soil

    alpha, kappa, beta, H = [], [], [], []
    for x in cfg.materials:
        if x.friction_angle is not None:
            a, k, b = soil.from_mohr_coulomb(x.cohesion, x.friction_angle, x.dilation_angle)
            h = x.hardening_modulus
        elif x.yield_stress > 0.0:
            a, k, b, h = 0.0, x.yield_stress / math.sqrt(3.0), 0.0, x.hardening_modulus / 3.0
            print(f"material {x.name}: yield_stress {x.yield_stress:g} enters the soil plasticity set as "
                  f"alpha = beta = 0, kappa = {k:g}, hardening = {h:g}", file=sys.stderr)
        else:
            a, k, b, h = 0.0, math.inf, 0.0, 0.0
        alpha.append(a), kappa.append(k), beta.append(b), H.append(h)
    sig0 = None
    if cfg.geostatic is not None:
        g = cfg.geostatic
        k0 = g.k0 if g.k0 is not None else [1.0 - math.sin(math.radians(x.friction_angle or 0.0))
                                            for x in cfg.materials]
        sig0 = soil.geostatic_stress(P, cfg.materials, gravity=g.gravity, k0=k0, axis=g.axis, surface=g.surface)
        mat = np.asarray(P.material_index, np.int64)
        soft = np.isfinite(np.asarray(kappa))[mat]
        bad = soil.overstressed(sig0[soft], np.asarray(alpha)[mat][soft], np.asarray(kappa)[mat][soft])
        if bad.size:
            print(f"geostatic: the stress at rest of {bad.size} elements lies outside their cone (K0 too far from 1 "
                  f"for the friction angle); they yield in the first step", file=sys.stderr)
    st.set_soil_plasticity(alpha, kappa, beta, H, initial_stress=sig0)


def run_scenario_explicit(cfg_path: str, steps: int, out_dir: str | None, mode: int = _lib.MODE_PARITY,
                          device: int = 0, safety: float = 0.9, log=print, trace_every: int = 0, peaks: bool = False,
                          energy_every: int = 0, mass_damping_only: bool = False, envelope_every: int = 0,
                          gauges=(), gauge_every: int = 1, plastic_summary: bool = False) -> dict:
    """`steps` output frames of the explicit stepper, ceil(cfg.time.initial_dt / dt) explicit steps each.
    trace_every / peaks / energy_every: the stepper's monitors (receivers at cfg.output.probes), written under
    out_dir after the last frame; their capacities follow from `steps`. mass_damping_only: the stepper gets the
    scenario's alpha_R and beta_R = 0 (a scenario's damping always has beta_R > 0, which the energy ledger refuses).
    envelope_every / gauges, gauge_every: the stepper's element monitors (all three envelope maps; gauge elements in
    the mesh's numbering), written under out_dir after the last frame. Materials with a ``yield_stress`` yield (J2
    plasticity): the VTU frames then carry plastic_strain and equivalent_plastic_strain per cell, and
    plastic_summary logs one line with the yielded elements and the total plastic work after the last frame."""
    import math

    from .explicit import ExplicitStepper

    cfg, m, P, materials = load_scenario(cfg_path, allow_hex8=mode == _lib.MODE_FAST)
    rayleigh = compute_rayleigh(cfg.damping)
    if mass_damping_only:
        rayleigh = type(rayleigh)(rayleigh.alpha, 0.0)
    try:
        st = ExplicitStepper(P, materials, rayleigh, cfg.solver, cfg.time, safety=safety, mode=mode, device=device)
    except RuntimeError as e:
        raise ScenarioError(str(e)) from None
    om = post.OutputManager(out_dir, m, P, materials, cfg.output, stepper=st) if out_dir else None
    wall0, last = time.perf_counter(), None
    try:
        absorbing_nodes = set_absorbing(st, cfg, m, P)
        tied = set_tied(st, cfg, m, P)  # dashpots first, ties second; either order gives the same arrays
        soil_model = any(x.friction_angle is not None for x in cfg.materials)
        plastic = soil_model or any(x.yield_stress > 0.0 for x in cfg.materials)
        if cfg.geostatic is not None and not soil_model:
            raise ScenarioError("geostatic needs a material with a friction_angle")
        if plastic:
            try:
                if soil_model:
                    set_soil_plasticity(st, cfg, P)
                else:
                    st.set_plasticity([x.yield_stress for x in cfg.materials],
                                      [x.hardening_modulus for x in cfg.materials])
            except (RuntimeError, ValueError) as e:
                raise ScenarioError(str(e)) from None
            if om is not None:
                om.plasticity = st.plasticity
        info = st.source_info()
        sources = dict(sources=info.source_count, source_nodes=info.loaded_nodes) if info.source_count else {}
        tel = st.telemetry()
        per_frame = max(1, math.ceil(cfg.time.initial_dt / tel.dt))
        monitored = trace_every > 0 or peaks or energy_every > 0
        if monitored:
            total = steps * per_frame
            if trace_every > 0 and not cfg.output.probes:
                raise ScenarioError("--trace-every needs output.probes")
            try:
                st.set_monitors(receivers=list(cfg.output.probes) if trace_every > 0 else None,
                                receiver_every=max(trace_every, 1), receiver_capacity=max(total // max(trace_every, 1), 1),
                                peaks=peaks, energy_every=max(energy_every, 0),
                                energy_capacity=max(total // max(energy_every, 1), 1))
            except RuntimeError as e:
                raise ScenarioError(str(e)) from None
        element_monitored = envelope_every > 0 or len(gauges) > 0
        if element_monitored:
            every = max(gauge_every, 1)
            try:
                st.set_element_monitors(gauges=list(gauges) or None, gauge_every=every,
                                        gauge_capacity=max(steps * per_frame // every, 1),
                                        envelope_every=max(envelope_every, 0), von_mises=envelope_every > 0,
                                        shear_strain=envelope_every > 0, stress_range=envelope_every > 0)
            except RuntimeError as e:
                raise ScenarioError(str(e)) from None
        for frame in range(steps):
            r = st.advance(per_frame)
            if not r.has_value():
                raise ScenarioError(f"frame {frame}: {r.error().message} {r.error().context}")
            tel = r.value()
            if om is not None:
                o = om.handle_frame(tel.time, frame)
                if not o.has_value():
                    raise ScenarioError(f"output frame {frame}: {o.error().message} {o.error().context}")
            last = dict(frame=frame, time=tel.time, dt=tel.dt, steps=tel.steps)
            log(json.dumps(last))
        written = write_monitors(st, out_dir, cfg.output.probes, trace_every > 0, peaks, energy_every > 0) \
            if monitored and out_dir else {}
        if element_monitored:
            written.update(write_element_monitors(st, out_dir, gauges, envelope_every > 0))
        if plastic:
            pi = st.plasticity_info()
            written.update(plastic_elements=pi.plastic_elements, yielded_elements=pi.yielded_elements,
                           plastic_work=float(st.plasticity().plastic_work.sum()))
            if plastic_summary:
                log(json.dumps(dict(plastic_summary=dict(plastic_elements=pi.plastic_elements,
                                                         yielded_elements=pi.yielded_elements,
                                                         plastic_work=written["plastic_work"]))))
        wall = time.perf_counter() - wall0
        return dict(scenario=cfg_path, nodes=P.node_count, tets=P.element_count, dofs=P.dof_count, steps=steps,
                    integrator="explicit", explicit_steps=tel.steps, steps_per_frame=per_frame, dt=tel.dt,
                    critical_dt=tel.critical_dt, lambda_max=tel.lambda_max, wall_s=wall, final_time=tel.time,
                    last=last, mode="fast" if mode == _lib.MODE_FAST else "parity", absorbing_nodes=absorbing_nodes,
                    **tied, **sources, **written)
    finally:
        if om is not None:
            om.close()
        st.close()
        st.system.close()


def write_monitors(st, out_dir, probes, traces: bool, peaks: bool, energy: bool) -> dict:
    """The stepper's monitors as files under out_dir: probes/traces.csv (step,time,node,ux,uy,uz,vx,vy,vz; one row per
    sample and probe), monitors/peaks.npy ([N,3]: |u|, |v|, |a|) and monitors/energy.csv -> the summary's entries."""
    import os

    import numpy as np

    out = {}
    if traces:
        os.makedirs(os.path.join(out_dir, "probes"), exist_ok=True)
        tr = st.receiver_traces()
        with open(os.path.join(out_dir, "probes", "traces.csv"), "w") as f:
            f.write("step,time,node,ux,uy,uz,vx,vy,vz\n")
            for i in range(tr.steps.size):
                for r, node in enumerate(probes):
                    vals = ",".join(repr(float(x)) for x in (*tr.u[i, r], *tr.v[i, r]))
                    f.write(f"{int(tr.steps[i])},{float(tr.time[i])!r},{int(node)},{vals}\n")
        out["trace_samples"] = int(tr.steps.size)
    if peaks or energy:
        os.makedirs(os.path.join(out_dir, "monitors"), exist_ok=True)
    if peaks:
        np.save(os.path.join(out_dir, "monitors", "peaks.npy"), np.stack(st.peaks(), axis=1))
    if energy:
        e = st.energy()
        with open(os.path.join(out_dir, "monitors", "energy.csv"), "w") as f:
            f.write("step,time,kinetic,potential,work,dissipated,balance\n")
            for row in zip(e.steps, e.time, e.kinetic, e.potential, e.work, e.dissipated, e.balance()):
                f.write(f"{int(row[0])}," + ",".join(repr(float(x)) for x in row[1:]) + "\n")
        out["energy_samples"] = int(e.steps.size)
    return out


def write_element_monitors(st, out_dir, gauges, envelopes: bool) -> dict:
    """The stepper's element monitors as files under out_dir/monitors (out_dir None: no files): the four envelope_*.npy
    maps and gauges.csv (one row per sample and gauge) -> the summary's entries."""
    import os

    import numpy as np

    info = st.element_monitor_info()
    out = {}
    if out_dir:
        os.makedirs(os.path.join(out_dir, "monitors"), exist_ok=True)
    if envelopes:
        out["envelope_samples"] = info.envelope_samples
        if out_dir:
            env = st.envelopes()
            for name in ("von_mises", "shear_strain", "stress_min", "stress_max"):
                np.save(os.path.join(out_dir, "monitors", f"envelope_{name}.npy"), getattr(env, name))
    if len(gauges):
        out["gauge_samples"] = info.gauge_samples
        if out_dir:
            tr = st.gauge_traces()
            comps = ("xx", "yy", "zz", "xy", "yz", "xz")
            with open(os.path.join(out_dir, "monitors", "gauges.csv"), "w") as f:
                f.write("step,time,element," + ",".join(f"strain_{c}" for c in comps) + "," +
                        ",".join(f"stress_{c}" for c in comps) + ",von_mises\n")
                for i in range(tr.steps.size):
                    for g, elem in enumerate(gauges):
                        vals = ",".join(repr(float(x)) for x in tr.rows[i, g])
                        f.write(f"{int(tr.steps[i])},{float(tr.time[i])!r},{int(elem)},{vals}\n")
    return out


class AbsorbingSetup(tuple):
    """(node_ids, C summed per node, load base, load pattern, curve), as absorbing_setup always returned it; ``sources``
    holds the load sources of a scenario that needs them (then base, pattern and curve are None)."""
    sources = ()


def absorbing_setup(cfg, m, P):
    """The scenario's ``absorbing:`` entries -> AbsorbingSetup (node_ids, C summed per node, load base, load pattern,
    curve); the last three are None without an incident wave. Entries of the plain form (no ``propagation``) that
    name one curve between them: base is the static load vector, pattern the entries' incident patterns summed, curve
    the one they name. An entry with ``propagation``, or more than one curve: every incident entry becomes a load
    source instead (.sources; a plain entry's is 2 C_n d with zero delays)."""
    import numpy as np

    from . import absorbing
    from .explicit import MAX_SOURCES, LoadSource

    parts, pattern, names, sources = [], np.zeros(P.dof_count, np.float64), [], []
    for i, entry in enumerate(cfg.absorbing):
        try:
            faces = absorbing.faces_of_group(m, entry.group)
            ids, Cn = absorbing.dashpots(m, cfg, faces)
            if not ids.size:
                raise ScenarioError(f"absorbing [{i}]: group '{entry.group}' has no boundary faces")
            inc = entry.incident
            if inc is not None and inc.propagation is not None:
                sid, A, tau, _ = absorbing.incident_plane_wave(m, cfg, faces, inc.direction, inc.propagation,
                                                               inc.origin or (0.0, 0.0, 0.0))
                sources.append(LoadSource(cfg.curves[inc.velocity_curve], sid, A, tau))
            elif inc is not None:
                sources.append(LoadSource(cfg.curves[inc.velocity_curve], ids,
                                          2.0 * (Cn @ np.asarray(inc.direction, np.float64)), np.zeros(ids.size)))
        except (KeyError, ValueError, RuntimeError) as e:
            if isinstance(e, ScenarioError):
                raise
            raise ScenarioError(f"absorbing [{i}]: {e.args[0] if e.args else e}") from None
        parts.append((ids, Cn))
        if entry.incident is not None:
            pattern += absorbing.incident_pattern(ids, Cn, entry.incident.direction, P.node_count)
            if entry.incident.velocity_curve not in names:
                names.append(entry.incident.velocity_curve)
    ids, Cn = absorbing.merge(parts)
    if not names:
        return AbsorbingSetup((ids, Cn, None, None, None))
    if len(names) > 1 or any(e.incident is not None and e.incident.propagation is not None for e in cfg.absorbing):
        if len(sources) > MAX_SOURCES:
            raise ScenarioError(f"explicit stepper takes at most {MAX_SOURCES} load sources")
        out = AbsorbingSetup((ids, Cn, None, None, None))
        out.sources = sources
        return out
    base = pack.assemble_load_vector(m, cfg, P.lumped_mass64)
    return AbsorbingSetup((ids, Cn, base, pattern, cfg.curves[names[0]]))


def tied_setup(cfg, m, P):
    """The scenario's ``tied:`` entries merged into one tie set -> (offsets, node_ids): a ``group`` entry by levels
    along its axis, a ``pair`` entry pairwise across the two faces; groups that share nodes (the edges of an x pair and a
    y pair) become one."""
    import numpy as np

    from . import ties

    def nodes_of(i, name):
        gid = m.group_names.get(name)
        if gid is None or gid not in m.node_groups:
            raise ScenarioError(f"tied [{i}]: unknown group '{name}'")
        return np.asarray(m.node_groups[gid], np.uint32)

    sets = []
    for i, entry in enumerate(cfg.tied):
        try:
            if entry.group is not None:
                sets.append(ties.levels(m.coords, nodes_of(i, entry.group), entry.axis))
            else:
                sets.append(ties.periodic(m.coords, nodes_of(i, entry.pair[0]), nodes_of(i, entry.pair[1]), entry.axis))
        except ValueError as e:
            raise ScenarioError(f"tied [{i}]: {e.args[0] if e.args else e}") from None
    return ties.merge(P.node_count, *sets)


def set_tied(st, cfg, m, P) -> dict:
    """Put the scenario's tied boundaries on an ExplicitStepper -> the summary's entries ({} without ``tied:``)."""
    if not cfg.tied:
        return {}
    off, ids = tied_setup(cfg, m, P)
    try:
        st.set_ties(off, ids)
    except RuntimeError as e:
        raise ScenarioError(f"tied: {e}") from None
    return dict(tie_groups=int(off.size - 1), tied_nodes=int(ids.size))


def set_absorbing(st, cfg, m, P) -> int:
    """Put the scenario's absorbing boundaries and incident waves on an ExplicitStepper -> dashpot nodes."""
    if not cfg.absorbing:
        return 0
    setup = absorbing_setup(cfg, m, P)
    ids, Cn, base, pattern, curve = setup
    if curve is not None:
        st.set_load_pattern(base, pattern)
        st.set_load_curve(curve)
    try:
        st.set_dashpots(ids, Cn)
        if setup.sources:
            st.set_sources(setup.sources)
    except RuntimeError as e:
        raise ScenarioError(str(e)) from None
    return int(ids.size)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m cwf.run", description=__doc__.split("\n\n")[0])
    ap.add_argument("scenario")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None, help="output root (vtu/, probes/); omitted: no files")
    ap.add_argument("--mode", choices=["parity", "fast"], default="parity")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--paused", action="store_true")
    ap.add_argument("--time-varying-loads", action="store_true")
    ap.add_argument("--integrator", choices=["newmark", "explicit"], default="newmark")
    ap.add_argument("--safety", type=float, default=0.9, help="explicit: fraction of the critical step")
    ap.add_argument("--trace-every", type=int, default=0, metavar="K",
                    help="explicit: receiver traces at output.probes every K steps -> <out>/probes/traces.csv")
    ap.add_argument("--peaks", action="store_true", help="explicit: peak |u|, |v|, |a| maps -> <out>/monitors/peaks.npy")
    ap.add_argument("--energy-every", type=int, default=0, metavar="K",
                    help="explicit: energy ledger every K steps -> <out>/monitors/energy.csv (needs beta_R == 0: "
                         "--mass-damping-only)")
    ap.add_argument("--mass-damping-only", action="store_true",
                    help="explicit: keep the scenario's alpha_R and drop its stiffness-proportional beta_R")
    ap.add_argument("--envelope-every", type=int, default=0, metavar="K",
                    help="explicit: peak von Mises, peak effective shear strain and stress min / max per element, "
                         "raised every K steps -> <out>/monitors/envelope_*.npy")
    ap.add_argument("--gauges", default="", metavar="E0,E1,...",
                    help="explicit: strain / stress / von Mises rows of these elements -> <out>/monitors/gauges.csv")
    ap.add_argument("--gauge-every", type=int, default=1, metavar="K", help="explicit: a gauge row every K steps")
    ap.add_argument("--plastic-summary", action="store_true",
                    help="explicit, materials with a yield_stress: one line with the yielded elements and the total "
                         "plastic work after the last frame")
    a = ap.parse_args(argv)
    try:
        gauges = [int(x) for x in a.gauges.split(",") if x.strip()]
    except ValueError:
        print("error: --gauges takes element numbers separated by commas", file=sys.stderr)
        return 1
    try:
        if a.integrator == "explicit":
            if a.time_varying_loads or a.paused:
                raise ScenarioError("--time-varying-loads and --paused belong to the newmark integrator")
            s = run_scenario_explicit(a.scenario, a.steps, a.out,
                                      _lib.MODE_FAST if a.mode == "fast" else _lib.MODE_PARITY, a.device, a.safety,
                                      trace_every=a.trace_every, peaks=a.peaks, energy_every=a.energy_every,
                                      mass_damping_only=a.mass_damping_only, envelope_every=a.envelope_every,
                                      gauges=gauges, gauge_every=a.gauge_every, plastic_summary=a.plastic_summary)
            print(json.dumps(dict(summary=s)))
            return 0
        if a.trace_every or a.peaks or a.energy_every or a.mass_damping_only:
            raise ScenarioError("--trace-every, --peaks, --energy-every and --mass-damping-only belong to the explicit "
                                "integrator")
        if a.envelope_every or gauges or a.gauge_every != 1:
            raise ScenarioError("--envelope-every, --gauges and --gauge-every belong to the explicit integrator")
        if a.plastic_summary:
            raise ScenarioError("--plastic-summary belongs to the explicit integrator")
        s = run_scenario(a.scenario, a.steps, a.out, _lib.MODE_FAST if a.mode == "fast" else _lib.MODE_PARITY,
                         a.device, a.paused, a.time_varying_loads)
    except ScenarioError as e:
        print(f"error: {e}", file=sys.stderr)
        return 1
    print(json.dumps(dict(summary=s)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
