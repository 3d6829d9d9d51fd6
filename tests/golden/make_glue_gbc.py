#!/usr/bin/env python3
"""Generates tests/golden/glue_gbc_reference.npz: what the reference's Core::gyroBiasCorrection (oracle/_ref/librebvio_ref.so)
returns for the pair glue's own Xv and W_Xv on support.glue_family_cases() x support.DT_GRID. Two steps, because the inputs come
from the device and the reference library can be built only where the reference checkout is:
  python tests/golden/make_glue_gbc.py dump inputs.npz     on a GPU: Xv, W_Xv of rebvio_hip_test_glue, case by case
  python tests/golden/make_glue_gbc.py oracle-inputs inputs.npz   or, without a GPU, from the oracle's restatement of the solve
  python tests/golden/make_glue_gbc.py record inputs.npz [out.npz]   where oracle/_ref/librebvio_ref.so is current (`make -C oracle
                                                                      ref`, or a library built there): the reference's X, Wx, Wb, dgbias
tests/test_reference_pin.py holds the recorded results to the live library, tests/test_reference_pin_gpu.py the device to them
(and the device's Xv, W_Xv to the recorded inputs). Re-run when glue_family, DT_GRID or the glue's 6x6 solve change."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import support as S  # noqa: E402

SIZE = (96, 128)   # rows, cols of the context the probe runs in (no image is involved)


def cases():
    return [(fam, decade, dt) for fam, decade in S.glue_family_cases() for dt in S.DT_GRID]


def dump(path):
    import torch  # noqa: F401
    from rebvio_amd import backend as B
    ctx = B.Context(B.default_params(*SIZE, keylines_ref=3000, keylines_max=4000))
    Xv, W = [], []
    for fam, decade, dt in cases():
        g = S.glue_family(fam, decade)
        dev, _ = ctx.test_glue(g["vel"], g["JtJ6"], 100.0, 1.0, 1, g["xrv"], g["n_new"], float(np.float32(dt)), g["Bg"], g["W_Bg"], g["R_prior"])
        Xv.append(np.array(dev[0].Xv, np.float32))
        W.append(np.array(dev[0].W_Xv, np.float32))
    ctx.close()
    np.savez(path, Xv=np.array(Xv), W_Xv=np.array(W))
    print("dumped", len(Xv), "cases")


def oracle_inputs(path):
    """the same two arrays without a GPU: the block records summed as glue.hpp sums them (in double, block by block, rounded once)
    and the oracle's 6x6 solve of them - the device test fails at its first assertion if these are not the device's"""
    import ctypes as C
    from oracle import oracle_py as O
    O.build()
    fp = C.POINTER(C.c_float)
    Xv, W = [], []
    iu = np.triu_indices(6)
    for fam, decade, dt in cases():
        xrv = S.glue_family(fam, decade)["xrv"]
        acc = np.zeros(27)
        for b in range(len(xrv)):
            acc += xrv[b, :27].astype(np.float64)
        Wx = np.zeros((6, 6), np.float32)
        Wx[iu] = acc[:21].astype(np.float32)
        Wx = np.ascontiguousarray(np.triu(Wx) + np.triu(Wx, 1).T)
        JtF, X = acc[21:].astype(np.float32), np.zeros(6, np.float32)
        O.lib().orc_sym6_solve(Wx.ctypes.data_as(fp), JtF.ctypes.data_as(fp), X.ctypes.data_as(fp))
        Xv.append(X)
        W.append(Wx.ravel())
    np.savez(path, Xv=np.array(Xv), W_Xv=np.array(W))
    print("formed", len(Xv), "cases on the oracle")


def record(path, out_path=os.path.join(HERE, "glue_gbc_reference.npz")):
    from oracle import ref_py
    ref_py.build()
    inp = np.load(path)
    p = ref_py.default_params(*SIZE)
    ref = ref_py.Ref(p)
    out = dict(Xv=inp["Xv"], W_Xv=inp["W_Xv"], X=[], Wx=[], Wb=[], dgbias=[])
    for k, (fam, decade, dt) in enumerate(cases()):
        s_g, s_b = S.gyro_noise(p, dt)
        X, Wx, Wb, dg = ref.gyro_bias_correction(inp["Xv"][k], inp["W_Xv"][k], S.glue_family(fam, decade)["W_Bg"],
                                                 np.eye(3, dtype=np.float32) * s_g, np.eye(3, dtype=np.float32) * s_b)
        for name, v in (("X", X), ("Wx", Wx), ("Wb", Wb), ("dgbias", dg)):
            out[name].append(np.ravel(v))
    np.savez_compressed(out_path, **{k: np.array(v, np.float32) for k, v in out.items()})
    print("recorded", len(out["X"]), "cases")


if __name__ == "__main__":
    {"dump": dump, "oracle-inputs": oracle_inputs, "record": record}[sys.argv[1]](*sys.argv[2:])
