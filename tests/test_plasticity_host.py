"""The explicit stepper's J2 plasticity on the host (include/cwf_hip.h "Plasticity"; no GPU).

1. cwf_explicit_j2_update -- the inline function the device pass runs -- equals the numpy restatement of the header's
   block bit for bit, over 1,000 random strains and states of three materials, yielded and elastic outcomes both.
2. Return-map properties in fp64: consistency (the returned stress lies on the hardened yield surface), abar and wp
   never decrease, hydrostatic strain never yields.
"""
import numpy as np

import plasticity_common as pc
from cwf import _lib, explicit
from cwf.physics import Material, make_properties

SYMBOLS = {"cwf_hip_explicit_set_plasticity", "cwf_hip_explicit_reset_plasticity", "cwf_hip_explicit_plasticity_info",
           "cwf_hip_explicit_read_plasticity", "cwf_explicit_j2_update"}
# steel-like, a soft soil, a stiffer soil: (material, yield stress, hardening modulus)
MATERIALS = [(Material("m0", 30.0e9, 0.2, 2500.0), 40.0e6, 0.0),
             (Material("m1", 3.0e9, 0.3, 1800.0), 2.0e6, 3.0e8),
             (Material("m2", 12.0e9, 0.25, 2200.0), 15.0e6, 4.0e9)]
COUNT = 1000


def inputs():
    """COUNT elements: D [n,6,6], sy, H, V, strain e, and a state (ep, abar, wp); a third start from the zero state."""
    rng = np.random.Generator(np.random.PCG64(11))
    which = rng.integers(0, 3, COUNT)
    Dm = np.stack([np.asarray(make_properties(m).stiffness, np.float64).reshape(6, 6) for m, _, _ in MATERIALS])
    D = Dm[which]
    sy = np.array([s for _, s, _ in MATERIALS])[which]
    H = np.array([h for _, _, h in MATERIALS])[which]
    V = np.float32(rng.uniform(1e-4, 1e-2, COUNT)).astype(np.float64)
    # strains around the yield strain sy / (3 mu) of each material, so that both outcomes occur
    scale = (sy / (3.0 * D[:, 3, 3]))[:, None]
    e = scale * rng.standard_normal((COUNT, 6)) * 0.8
    ep = scale * rng.standard_normal((COUNT, 6)) * 0.3
    ep[:, :3] -= ep[:, :3].mean(1, keepdims=True)  # plastic strain is deviatoric
    abar = np.abs(scale[:, 0] * rng.standard_normal(COUNT))
    wp = np.abs(rng.standard_normal(COUNT))
    fresh = rng.random(COUNT) < 1.0 / 3.0
    ep[fresh], abar[fresh], wp[fresh] = 0.0, 0.0, 0.0
    return D, sy, H, V, e, ep, abar, wp


def library(D, sy, H, V, e, ep, abar, wp):
    L = _lib.load()
    n = e.shape[0]
    y = np.zeros(n, bool)
    state = np.ascontiguousarray(np.concatenate([ep, abar[:, None], wp[:, None]], 1))
    sp = np.zeros((n, 6))
    for i in range(n):
        Di, ei = np.ascontiguousarray(D[i]), np.ascontiguousarray(e[i])
        y[i] = L.cwf_explicit_j2_update(_lib.ptr(Di), sy[i], H[i], V[i], _lib.ptr(ei), _lib.ptr(state[i]),
                                        _lib.ptr(sp[i])) == 1
    return y, state[:, :6], state[:, 6], state[:, 7], sp


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_symbols_are_declared_and_exported():
    assert SYMBOLS <= set(_lib.declared_symbols())
    L = _lib.load()
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_j2_update_is_the_restatement_bit_for_bit():
    args = inputs()
    y, ep, abar, wp, sp = pc.j2_update(*args)
    assert 100 < np.count_nonzero(y) < COUNT - 100, np.count_nonzero(y)  # both outcomes, before comparing
    ly, lep, labar, lwp, lsp = library(*args)
    assert np.array_equal(ly, y)
    for name, a, b in (("ep", lep, ep), ("abar", labar, abar), ("wp", lwp, wp), ("sigma_p", lsp, sp)):
        assert np.array_equal(bits(a), bits(b)), (name, np.argwhere(bits(a) != bits(b))[:5])
    # where nothing yielded the state is the input's
    for a, b in ((lep, args[5]), (labar, args[6]), (lwp, args[7])):
        assert np.array_equal(bits(a[~y]), bits(b[~y]))
    # the Python wrapper is the same function
    i = int(np.flatnonzero(y)[0])
    yy, st, spp = explicit.j2_update(args[0][i], args[1][i], args[2][i], args[3][i], args[4][i],
                                     np.concatenate([args[5][i], [args[6][i], args[7][i]]]))
    assert yy and np.array_equal(bits(st[:6]), bits(ep[i])) and np.array_equal(bits(spp), bits(sp[i]))


def consistency_residual(update):
    """max over the yielding inputs of |von_mises(D (e - ep_new)) - (sy + H abar_new)| / (sy + H abar_new)."""
    D, sy, H, V, e, ep, abar, wp = inputs()
    y, epn, abarn, _, _ = update(D, sy, H, V, e, ep, abar, wp)[:5]
    q = pc.von_mises(pc.iso_row_fold(D, e - epn))
    Y = sy + H * abarn
    return float(np.max(np.abs(q - Y)[y] / Y[y]))


def test_return_map_lands_on_the_yield_surface():
    """Tolerance: 4 x the numpy restatement's own residual on the same inputs. The restatement's residual is
    6.5e-16 relative (a few fp64 roundings of the radial scaling and the square root), so the bound is 2.6e-15;
    the library, which is the same operations, shows the same residual."""
    ref = consistency_residual(pc.j2_update)
    print(f"restatement residual {ref:.3e}")
    assert 0.0 < ref < 1e-13  # a rounding-level number, or the inputs are not what this test thinks
    got = consistency_residual(library)
    print(f"library residual {got:.3e}")
    assert got <= 4.0 * ref


def test_abar_and_wp_never_decrease_and_hydrostatic_strain_never_yields():
    D, sy, H, V, e, ep, abar, wp = inputs()
    y, epn, abarn, wpn, _ = library(D, sy, H, V, e, ep, abar, wp)
    assert np.all(abarn >= abar) and np.all(wpn >= wp)
    assert np.all(abarn[y] > abar[y]) and np.all(wpn[y] > wp[y])
    # a second update at the same strain finds every element on or inside its surface up to rounding: what it adds
    # is rounding-sized
    y2, _, abar2, wp2, _ = library(D, sy, H, V, e, epn, abarn, wpn)
    assert np.all(abar2 >= abarn) and np.all(wp2 >= wpn)
    assert np.all(abar2 - abarn <= 1e-12 * np.maximum(abarn, 1e-30))
    # pure hydrostatic strain of any size, from the zero state
    rng = np.random.Generator(np.random.PCG64(3))
    mag = 10.0 ** rng.uniform(-12, 2, COUNT) * rng.choice([-1.0, 1.0], COUNT)
    eh = np.zeros((COUNT, 6))
    eh[:, :3] = mag[:, None]
    zero6, zero = np.zeros((COUNT, 6)), np.zeros(COUNT)
    yh, eph, abarh, wph, sph = library(D, sy, H, V, eh, zero6, zero, zero)
    assert not yh.any() and not eph.any() and not abarh.any() and not wph.any() and not sph.any()


# ---- the scenario keys ----------------------------------------------------------------------------------------------
def _yaml(extra=""):
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "tests", "golden", "data", "cantilever.yaml")).read()
    assert text.count("    rho: 2500.0\n") == 1
    return text.replace("    rho: 2500.0\n", "    rho: 2500.0\n" + extra)


def _json_of(text):
    import ctypes as C

    L = _lib.load()
    h = C.c_void_p()
    assert L.cwf_config_load_string(text.encode(), C.byref(h)) == 0, _lib.last_error(None)
    try:
        return L.cwf_config_json(h).decode()
    finally:
        L.cwf_config_destroy(h)


def test_config_takes_the_two_keys_and_keeps_configs_without_them():
    from cwf import config

    plain = config.load_config_from_string(_yaml())
    assert plain.has_value(), plain.error()
    m = plain.value().materials[0]
    assert (m.yield_stress, m.hardening_modulus) == (0.0, 0.0)
    r = config.load_config_from_string(_yaml("    yield_stress: 4.0e7\n    hardening_modulus: 3.0e9\n"))
    assert r.has_value(), r.error()
    m = r.value().materials[0]
    assert (m.name, m.youngs_modulus, m.yield_stress, m.hardening_modulus) == ("concrete", 3.0e10, 4.0e7, 3.0e9)
    only = config.load_config_from_string(_yaml("    yield_stress: 4.0e7\n"))
    assert only.has_value() and only.value().materials[0].hardening_modulus == 0.0
    # the serialised config: the keys appear only when the document has them, in the material's entry, and a document
    # without them serialises to the text it always did (the entry closes right after rho)
    without, with_keys = _json_of(_yaml()), _json_of(_yaml("    yield_stress: 4.0e7\n    hardening_modulus: 3.0e9\n"))
    assert "yield_stress" not in without and "hardening_modulus" not in without
    assert '"rho": 2500}' in without.replace("2500.0", "2500")
    head, tail = with_keys.split(', "yield_stress": ')
    value, rest = tail.split(', "hardening_modulus": ')
    assert float(value) == 4.0e7 and float(rest.split("}")[0]) == 3.0e9
    assert head + "}" + rest.split("}", 1)[1] == without


def test_config_refuses_a_negative_yield_stress_with_its_path():
    from cwf import config

    for extra, msg, key in (("    yield_stress: -1.0\n", "material.yield_stress must be >= 0", "yield_stress"),
                            ("    yield_stress: 1.0e6\n    hardening_modulus: -2.0\n",
                             "material.hardening_modulus must be >= 0", "hardening_modulus"),
                            ("    hardening_modulus: 2.0\n", "material.hardening_modulus needs material.yield_stress",
                             "hardening_modulus")):
        r = config.load_config_from_string(_yaml(extra))
        assert not r.has_value()
        assert r.error().message == msg and r.error().context == ["materials", "[0]", key], r.error()
    r = config.load_config_from_string(_yaml("    yield_stress: soft\n"))
    assert not r.has_value() and r.error().context == ["materials", "[0]", "yield_stress"], r.error()
