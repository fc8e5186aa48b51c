"""The explicit stepper's monitors, host side (no GPU): the exported entry points, the struct layouts, and the ledger's
definition -- its terms summed over an all-float64 run of the scheme keep kinetic + potential - work + dissipated
constant."""
import ctypes as C
import math

import absorbing_common as ac
import monitors_common as mc
from cwf import _lib
from explicit_common import header_struct_size

SYMBOLS = {
    "cwf_hip_explicit_set_monitors", "cwf_hip_explicit_reset_monitors", "cwf_hip_explicit_monitor_info",
    "cwf_hip_explicit_read_receivers", "cwf_hip_explicit_read_peaks", "cwf_hip_explicit_read_energy",
}


def test_library_declares_and_exports_the_monitor_entry_points():
    L = _lib.load()
    assert SYMBOLS <= set(_lib.declared_symbols())
    for n in SYMBOLS:
        assert hasattr(L, n), n
    assert L.cwf_hip_abi_version() == 1


def test_monitor_struct_sizes_match_the_header():
    assert C.sizeof(_lib.ExplicitMonitorDescC) == header_struct_size("cwf_explicit_monitor_desc") == 6 * 8 + 2 * 4 == 56
    assert C.sizeof(_lib.ExplicitMonitorInfoC) == header_struct_size("cwf_explicit_monitor_info") == 9 * 8 + 2 * 4 == 80
    assert _lib.ExplicitMonitorDescC.receiver_nodes.offset == 8 and _lib.ExplicitMonitorDescC.peaks.offset == 48
    assert _lib.ExplicitMonitorInfoC.energy_every.offset == 40 and _lib.ExplicitMonitorInfoC.peaks.offset == 72
    # the structs this feature must not move
    assert C.sizeof(_lib.ExplicitDescC) == 56 and C.sizeof(_lib.ExplicitTelemetryC) == 48


def test_null_handles_are_refused_before_any_device_call():
    L = _lib.load()
    assert L.cwf_hip_explicit_set_monitors(None, None) == -11
    assert L.cwf_hip_explicit_reset_monitors(None) == -11
    assert L.cwf_hip_explicit_monitor_info(None, None) == -11
    assert L.cwf_hip_explicit_read_energy(None, 0, 0, None, None) == -11


MEASURED_DRIFT = 4.7e-14  # measured: 4.749e-14 over the 150 steps of the run below
BOUND = 100.0 * MEASURED_DRIFT


def test_the_ledger_is_the_conserved_quantity_of_the_scheme():
    """Soil column P (225 nodes, dashpots at the base, incident Gaussian), all float64 with the dense K, at 0.9 of the
    critical step: max |balance_i - balance_0| / max total measured 4.749e-14 over 150 steps (pure fp64 summation and
    rounding noise; work and dissipation each reach twice the peak total); bounded at 100 x that, 4.7e-12. Without the
    dissipation term the same figure is 2.0."""
    ref = ac.column_dense("P")
    dt = 0.9 * 2.0 / math.sqrt(ref["lam_max"])
    rows = mc.ledger_of_f64_run("P", dt)
    drift = mc.balance_drift(rows)
    total = rows[:, 0] + rows[:, 1]
    print(f"ledger drift on the fp64 column: {drift:.3e} over {len(rows)} steps (bound {BOUND:.1e}); "
          f"work {rows[-1, 2]:.6e} dissipated {rows[-1, 3]:.6e} max total {total.max():.6e}")
    assert rows[-1, 2] > 0.0 and total.max() > 0.0
    assert drift <= BOUND, drift
    broken = mc.balance_drift(mc.ledger_of_f64_run("P", dt, with_dissipation=False))
    print(f"the same without the dissipation term: {broken:.3e}")
    assert broken >= 1e6 * BOUND, broken
