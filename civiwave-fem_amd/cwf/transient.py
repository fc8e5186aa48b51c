"""What cwf.stepper.Stepper and cwf.explicit.ExplicitStepper share: state and load access over the C functions
``<prefix>_get_state`` / ``_set_state`` / ``_set_external_force`` / ``_set_load_pattern`` / ``_time`` / ``_destroy``
(one state core in the library too: csrc/abi_transient.cpp).

A subclass names its C prefix (``_PREFIX``) and the attribute holding its handle (``_HANDLE``), and sets ``system``
and ``dof_count``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _f32_span(values):
    """-> (values as the library reads them, their pointer kind)."""
    if isinstance(values, np.ndarray):
        return np.ascontiguousarray(values, np.float32), _lib.PTR_HOST
    return values, _lib.PTR_DEVICE


class TransientState:
    _PREFIX = ""
    _HANDLE = ""

    def _fn(self, name: str):
        return getattr(_lib.load(), f"{self._PREFIX}_{name}")

    def _raw(self):
        return getattr(self, self._HANDLE)

    def _check(self, rc):
        if rc:
            raise RuntimeError(_lib.last_error(self.system._h))

    def _times(self):
        ct, dt = C.c_double(), C.c_double()
        self._fn("time")(self._raw(), C.byref(ct), C.byref(dt))
        return ct.value, dt.value

    def current_time(self) -> float:
        return self._times()[0]

    def time_step(self) -> float:
        return self._times()[1]

    def get_state(self, which: int, out=None):
        if out is None:
            out = np.zeros(self.dof_count, np.float32)
        kind = _lib.PTR_HOST if isinstance(out, np.ndarray) else _lib.PTR_DEVICE
        self._check(self._fn("get_state")(self._raw(), which, _lib.ptr(out), self.dof_count, kind))
        return out

    def set_state(self, which: int, values):
        values, kind = _f32_span(values)
        self._check(self._fn("set_state")(self._raw(), which, _lib.ptr(values), self.dof_count, kind))

    def set_external_force(self, force):
        """Rewrite nodes.external_force between steps (the viewer does this, viewer.cpp:262-266)."""
        force, kind = _f32_span(force)
        self._check(self._fn("set_external_force")(self._raw(), _lib.ptr(force), self.dof_count, kind))

    def set_load_pattern(self, base: np.ndarray, pattern: np.ndarray):
        """Device-side time-varying load: f64 [3N] loads no curve scales (base) and the point-load values one curve
        scales (pattern). Stepper.set_load_scale(c) then packs f32(base + c * pattern); with
        ExplicitStepper.set_load_curve the update pass forms f32(base + curve(t_n) * pattern) itself at every step."""
        self._lbase = np.ascontiguousarray(base, np.float64)
        self._lpat = np.ascontiguousarray(pattern, np.float64)
        self._check(self._fn("set_load_pattern")(self._raw(), _lib.ptr(self._lbase), _lib.ptr(self._lpat),
                                                 self.dof_count))

    def close(self):
        if getattr(self, self._HANDLE, None) is not None:
            self._fn("destroy")(self._raw())
            setattr(self, self._HANDLE, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
