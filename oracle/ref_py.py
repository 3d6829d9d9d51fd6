"""ctypes binding of oracle/_ref/librebvio_ref.so: the reference's own hot-path sources behind oracle/ref_driver.cpp
(TEST INFRASTRUCTURE - may be imported only by tests/).

`Ref` and `RefMap` have the method names and return shapes of oracle_py.Oracle and oracle_py.Map for the part of the interface the
reference's public classes can serve, so that one test body drives either library. Parameters are oracle_py.Params; keylines are
oracle_py.KEYLINE_DTYPE records. Differences, all forced by the reference's interface (oracle/ref_driver.cpp):
  - minimize_vel returns F, vel and Rvel only (no accept mask, no quantile); ext_rot_vel returns ok, Wx and X only (no JtF);
  - EdgeMapConfig stays at its defaults (regularize is regularize1Iter at 0.5, the match thresholds 2.0 / 1.0 / 45 degrees);
  - there is no auto_threshold accessor (a map's threshold carries it) and no dense detector mask (RefMap.mask is the map's own).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from .oracle_py import KEYLINE_DTYPE, Params

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "librebvio_ref.so")


def reference_root() -> str:
    """The reference checkout `make ref` would read (the Makefile's REBVIO_REFERENCE, overridable from the environment)."""
    return subprocess.run(["make", "-s", "-C", _HERE, "ref-root"], capture_output=True, text=True, check=True).stdout.strip()


def have_reference() -> bool:
    root = reference_root()
    return bool(root) and os.path.exists(os.path.join(root, "rebvio", "src", "core.cpp"))


def build() -> str:
    """`make -C oracle ref` under the oracle's build lock. Without a reference checkout the target does nothing and an existing
    library is left as it is. Returns the library's path (which may not exist: see have_reference)."""
    import fcntl
    os.makedirs(os.path.join(_HERE, "_build"), exist_ok=True)
    with open(os.path.join(_HERE, "_build", ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            subprocess.run(["make", "-s", "-C", _HERE, "ref"], check=True)
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)
    return LIB_PATH


def default_params(rows: int, cols: int, **over) -> Params:
    """oracle_py.default_params: one parameter record serves both libraries"""
    from . import oracle_py
    return oracle_py.default_params(rows, cols, **over)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = C.CDLL(LIB_PATH)
    fp = C.POINTER(C.c_float)
    ip = C.POINTER(C.c_int)
    vp = C.c_void_p
    sig = {
        "ref_create": (vp, [C.POINTER(Params)]),
        "ref_destroy": (None, [vp]),
        "ref_scale_space": (None, [vp, fp, fp, fp, fp, fp]),
        "ref_filter_width": (C.c_int, [vp, C.c_int, C.c_int]),
        "ref_smooth_n": (None, [vp, fp, C.c_float, C.c_int, fp, ip]),
        "ref_detect": (vp, [vp, fp, C.c_uint64]),
        "ref_detector_threshold": (C.c_float, [vp]),
        "ref_map_size": (C.c_int, [vp]),
        "ref_map_threshold": (C.c_float, [vp]),
        "ref_map_set_threshold": (None, [vp, C.c_float]),
        "ref_map_get_keylines": (None, [vp, vp]),
        "ref_map_set_keylines": (None, [vp, vp, C.c_int]),
        "ref_map_get_mask": (None, [vp, vp, ip]),
        "ref_map_clone": (vp, [vp]),
        "ref_map_free": (None, [vp]),
        "ref_build_distance_field": (None, [vp, vp]),
        "ref_distance_field": (None, [vp, ip, ip]),
        "ref_rotate_keylines": (None, [vp, vp, fp]),
        "ref_estimate_quantile": (C.c_float, [vp, C.c_float, C.c_int]),
        "ref_try_vel": (C.c_float, [vp, vp, fp, C.c_float, fp, fp, fp]),
        "ref_minimize_vel": (C.c_float, [vp, vp, fp, fp]),
        "ref_forward_match": (C.c_int, [vp, vp]),
        "ref_ext_rot_vel": (C.c_int, [vp, vp, fp, fp, fp]),
        "ref_directed_match": (C.c_int, [vp, vp, vp, fp, fp, fp, ip, C.c_float]),
        "ref_regularize": (C.c_int, [vp]),
        "ref_update_inverse_depth": (None, [vp, fp]),
        "ref_gyro_bias_correction": (None, [vp, fp, fp, fp, fp, fp, fp]),
        "ref_search_match": (C.c_int, [vp, vp, vp, fp, fp, fp, C.c_float]),
        "ref_calculate_fj": (C.c_float, [vp, vp, C.c_int, fp, fp, vp, C.c_float, C.c_float, ip, fp]),
        "ref_update_inverse_depth_arlu": (None, [vp, vp, fp]),
    }
    for name, (res, args) in sig.items():
        # A library that travelled with the tree may have been built from an earlier oracle/ref_driver.cpp and cannot be rebuilt
        # where there is no reference checkout: it still serves every entry it has. An entry it lacks is reported by the call
        # that needs it (has_entry; Ref.gyro_bias_correction), not by every test that loads the library.
        if name in LATER_ENTRIES and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


LATER_ENTRIES = ("ref_gyro_bias_correction",)   # added to the driver after the library's first version


def has_entry(name: str) -> bool:
    return hasattr(lib(), name)


def _f(a):
    a = np.ascontiguousarray(a, np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


class RefMap:
    def __init__(self, L, ctx, h):
        self.L, self.ctx, self.h = L, ctx, h   # ctx: the Ref that made the map (kept alive; the dense mask needs its size)

    def __del__(self):
        if self.h:
            self.L.ref_map_free(self.h)
            self.h = None

    def size(self):
        return self.L.ref_map_size(self.h)

    @property
    def threshold(self):
        return self.L.ref_map_threshold(self.h)

    @threshold.setter
    def threshold(self, t):
        self.L.ref_map_set_threshold(self.h, float(t))

    def keylines(self) -> np.ndarray:
        out = np.zeros(self.size(), KEYLINE_DTYPE)
        if out.size:
            self.L.ref_map_get_keylines(self.h, out.ctypes.data)
        return out

    def set_keylines(self, kl: np.ndarray):
        kl = np.ascontiguousarray(kl, KEYLINE_DTYPE)
        self.L.ref_map_set_keylines(self.h, kl.ctypes.data, len(kl))

    def mask(self, rows, cols) -> np.ndarray:
        assert (rows, cols) == (self.ctx.rows, self.ctx.cols)
        out = np.empty((rows, cols), np.int32)
        self.L.ref_map_get_mask(self.ctx.h, self.h, out.ctypes.data_as(C.POINTER(C.c_int)))
        return out

    def clone(self) -> "RefMap":
        return RefMap(self.L, self.ctx, self.L.ref_map_clone(self.h))


class Ref:
    """The reference's EdgeDetector, ScaleSpace, Core and a DistanceField of its own for one camera and one set of parameters."""

    def __init__(self, params: Params):
        self.L = lib()
        self.p = params
        self.rows, self.cols = params.rows, params.cols
        self.h = self.L.ref_create(C.byref(params))
        self._field_map = None

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ref_destroy(self.h)
            self.h = None

    # --- detection -------------------------------------------------------------------------
    def scale_space(self, img):
        img, pi = _f(img)
        assert img.shape == (self.rows, self.cols)
        outs = [np.empty((self.rows, self.cols), np.float32) for _ in range(4)]
        self.L.ref_scale_space(self.h, pi, *[o.ctypes.data_as(C.POINTER(C.c_float)) for o in outs])
        return dict(scale0=outs[0], scale1=outs[1], dog=outs[2], mag=outs[3])

    def filter_width(self, filt, k):
        return self.L.ref_filter_width(self.h, filt, k)

    def smooth(self, img, sigma, n=3):
        img, pi = _f(img)
        assert img.shape == (self.rows, self.cols)
        out = np.empty((self.rows, self.cols), np.float32)
        w = (C.c_int * n)()
        self.L.ref_smooth_n(self.h, pi, sigma, n, out.ctypes.data_as(C.POINTER(C.c_float)), w)
        return out, list(w)

    def detect(self, img, ts_us=0) -> RefMap:
        img, pi = _f(img)
        assert img.shape == (self.rows, self.cols)
        return RefMap(self.L, self, self.L.ref_detect(self.h, pi, ts_us))

    def detect_u8(self, frame_u8, ts_us=0) -> RefMap:
        return self.detect(frame_u8.astype(np.float32) * np.float32(3.0), ts_us)

    @property
    def threshold(self):
        return self.L.ref_detector_threshold(self.h)

    # --- tracking --------------------------------------------------------------------------
    def build_distance_field(self, m: RefMap):
        self._field_map = m
        self.L.ref_build_distance_field(self.h, m.h)

    def distance_field(self):
        ids = np.empty((self.rows, self.cols), np.int32)
        dist = np.empty((self.rows, self.cols), np.int32)
        ip = C.POINTER(C.c_int)
        self.L.ref_distance_field(self.h, ids.ctypes.data_as(ip), dist.ctypes.data_as(ip))
        return ids, dist

    def rotate(self, m: RefMap, R):
        R, pr = _f(np.asarray(R).reshape(9))
        self.L.ref_rotate_keylines(self.h, m.h, pr)

    def quantile(self, m: RefMap, pct=0.9, bins=100):
        return self.L.ref_estimate_quantile(m.h, pct, bins)

    def try_vel(self, m: RefMap, vel, sigma_rho_min, residuals):
        vel, pv = _f(vel)
        assert residuals.dtype == np.float32 and residuals.flags.c_contiguous
        JtJ = np.zeros(9, np.float32)
        JtF = np.zeros(3, np.float32)
        fp = C.POINTER(C.c_float)
        s = self.L.ref_try_vel(self.h, m.h, pv, sigma_rho_min, residuals.ctypes.data_as(fp), JtJ.ctypes.data_as(fp),
                               JtF.ctypes.data_as(fp))
        return s, JtJ.reshape(3, 3), JtF

    def minimize_vel(self, m: RefMap, vel0=(0, 0, 0)):
        vel = np.array(vel0, np.float32)
        Rvel = np.zeros(9, np.float32)
        fp = C.POINTER(C.c_float)
        F = self.L.ref_minimize_vel(self.h, m.h, vel.ctypes.data_as(fp), Rvel.ctypes.data_as(fp))
        return dict(F=F, vel=vel, Rvel=Rvel.reshape(3, 3))

    def forward_match(self, old: RefMap, new: RefMap):
        return self.L.ref_forward_match(old.h, new.h)

    def ext_rot_vel(self, vel):
        """on the map of the last build_distance_field, like the oracle (the reference's own map argument is unused)"""
        vel, pv = _f(vel)
        Wx = np.zeros(36, np.float32)
        X = np.zeros(6, np.float32)
        fp = C.POINTER(C.c_float)
        ok = self.L.ref_ext_rot_vel(self.h, self._field_map.h, pv, Wx.ctypes.data_as(fp), X.ctypes.data_as(fp))
        return dict(ok=ok, Wx=Wx.reshape(6, 6), X=X)

    def directed_match(self, new: RefMap, old: RefMap, vel, Rvel, Rback, max_radius=40.0):
        vel, pv = _f(vel)
        Rvel, prv = _f(np.asarray(Rvel).reshape(9))
        Rback, prb = _f(np.asarray(Rback).reshape(9))
        kf = C.c_int(0)
        n = self.L.ref_directed_match(self.h, new.h, old.h, pv, prv, prb, C.byref(kf), max_radius)
        return n, kf.value

    def regularize(self, m: RefMap):
        return self.L.ref_regularize(m.h)

    def search_match(self, searched: RefMap, query_keyline, vel, Rvel, Rback, max_radius=40.0) -> int:
        q = np.ascontiguousarray(np.asarray(query_keyline, KEYLINE_DTYPE).reshape(1))
        vel, pv = _f(vel)
        Rvel, prv = _f(np.asarray(Rvel).reshape(9))
        Rback, prb = _f(np.asarray(Rback).reshape(9))
        return self.L.ref_search_match(self.h, searched.h, q.ctypes.data, pv, prv, prb, max_radius)

    def update_inverse_depth(self, vel):
        vel, pv = _f(vel)
        self.L.ref_update_inverse_depth(self.h, pv)

    def gyro_bias_correction(self, X, Wx, Wb, Rg, Rb):
        """Core::gyroBiasCorrection of this context's Core on copies of the inputs: (X[6], Wx[6, 6], Wb[3, 3], dgbias[3])
        afterwards, the shapes of oracle_py.gyro_bias_correction."""
        if not has_entry("ref_gyro_bias_correction"):
            raise RuntimeError(f"{LIB_PATH} was built from an earlier oracle/ref_driver.cpp and has no ref_gyro_bias_correction: "
                               "rebuild it with `make -C oracle ref` where the reference checkout is")
        X, px = _f(np.array(X, np.float32).reshape(6))
        Wx, pwx = _f(np.array(Wx, np.float32).reshape(36))
        Wb, pwb = _f(np.array(Wb, np.float32).reshape(9))
        Rg, prg = _f(np.asarray(Rg).reshape(9))
        Rb, prb = _f(np.asarray(Rb).reshape(9))
        dg = np.zeros(3, np.float32)
        self.L.ref_gyro_bias_correction(self.h, px, pwx, pwb, prg, prb, dg.ctypes.data_as(C.POINTER(C.c_float)))
        return X, Wx.reshape(6, 6), Wb.reshape(3, 3), dg

    # --- single-keyline forms (oracle_py has no wrapper of these: tests call orc_calculate_fj / orc_update_inverse_depth_arlu) ---
    def calculate_fj(self, f_inx, keyline, px, py):
        """Core::calculatefJ on the field of the last build_distance_field: (f, df_dx, df_dy, mnum, fi, the keyline afterwards);
        df_dx, df_dy, fi start at 0 and mnum at 0, so an output the call leaves unset reads 0."""
        q = np.ascontiguousarray(np.asarray(keyline, KEYLINE_DTYPE).reshape(1)).copy()
        dx, dy, fi, mnum = C.c_float(0), C.c_float(0), C.c_float(0), C.c_int(0)
        f = self.L.ref_calculate_fj(self.h, self._field_map.h, f_inx, C.byref(dx), C.byref(dy), q.ctypes.data, px, py, C.byref(mnum),
                                    C.byref(fi))
        return f, dx.value, dy.value, mnum.value, fi.value, q[0]

    def update_inverse_depth_arlu(self, keyline, vel):
        q = np.ascontiguousarray(np.asarray(keyline, KEYLINE_DTYPE).reshape(1)).copy()
        vel, pv = _f(vel)
        self.L.ref_update_inverse_depth_arlu(self.h, q.ctypes.data, pv)
        return q[0]
