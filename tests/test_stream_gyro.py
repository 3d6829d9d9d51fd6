"""Gyro rotations for the streaming and batch drivers, the parts that need no GPU: the new entries are exported, and
rebvio_hip_gyro_integrate - one step of IntegratedImu::add (types/imu.hpp:72), R <- R * exp(gyro * dt) - follows a float64
Rodrigues product."""
import ctypes

import numpy as np

from support import backend  # noqa: F401
from support import rodrigues


NEW_SYMBOLS = ("rebvio_hip_push_frame_px_gyro_device", "rebvio_hip_push_frame_px_gyro", "rebvio_hip_batch_push_px_gyro_device",
               "rebvio_hip_gyro_integrate")


def test_gyro_entries_are_exported_and_bound(backend):
    lib = ctypes.CDLL(backend.LIB_PATH)
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    assert all(n in backend.SIGNATURES for n in NEW_SYMBOLS)
    assert backend.lib().rebvio_hip_abi_version() == 3            # additions only
    for name in ("push_frame_px_gyro_device", "push_frame_px_gyro"):
        assert callable(getattr(backend.Context, name))
    assert callable(backend.Batch.push_px_gyro_device) and callable(backend.gyro_integrate)


def test_gyro_integrate_follows_a_float64_rodrigues_product(backend):
    """200 steps of dt = 0.005 at rates up to 2 rad/s. Bound 2e-5 per entry: 200 steps, each a handful of fp32 roundings of 2^-24
    relative on entries <= 1 (200 * 8 * 6e-8 ~ 1e-5), with a factor 2 of slack."""
    rng = np.random.Generator(np.random.PCG64(11))
    dt = 0.005
    for trial in range(4):
        R = np.eye(3, dtype=np.float32)
        want = np.eye(3)
        worst = 0.0
        mean = np.array([1.0, -0.8, 0.6]) * (1 if trial % 2 else -1)     # a steady turn under the noise: |rate| <= 2 rad/s per axis
        for _ in range(200):
            g = (mean + rng.uniform(-1.0, 1.0, 3)).astype(np.float32)
            R = backend.gyro_integrate(R, g, dt)
            want = want @ rodrigues(g.astype(np.float64) * np.float64(np.float32(dt)))
            worst = max(worst, np.abs(R.astype(np.float64) - want).max())
        assert R.dtype == np.float32 and R.shape == (3, 3)
        assert worst <= 2e-5, (trial, worst)
        assert np.abs(R.astype(np.float64) @ R.astype(np.float64).T - np.eye(3)).max() <= 4e-5   # still a rotation
        assert np.abs(want - np.eye(3)).max() > 0.1                                             # ... and it went somewhere


def test_gyro_integrate_single_step_and_zero_rate(backend):
    rng = np.random.Generator(np.random.PCG64(12))
    for _ in range(50):
        g = rng.uniform(-2.0, 2.0, 3).astype(np.float32)
        one = backend.gyro_integrate(np.eye(3, dtype=np.float32), g, 0.005)
        want = rodrigues(g.astype(np.float64) * np.float64(np.float32(0.005)))
        assert np.abs(one.astype(np.float64) - want).max() <= 1e-6, (g, one)
    # the three ranges of the exponential's series (|w|^2 below 1e-8, below 1e-6, above), each a single step
    for rate in (0.01, 0.15, 1.9):
        one = backend.gyro_integrate(np.eye(3, dtype=np.float32), [rate, 0.0, 0.0], 0.005)
        assert np.abs(one.astype(np.float64) - rodrigues([np.float64(np.float32(rate)) * np.float64(np.float32(0.005)), 0, 0])).max() <= 1e-6
    # a zero rate leaves R as it is, bit for bit (a generic rotation and the identity)
    for R in (rodrigues([0.4, -0.3, 0.2]).astype(np.float32), np.eye(3, dtype=np.float32)):
        for dt in (0.005, 0.0):
            out = backend.gyro_integrate(R, [0.0, 0.0, 0.0], dt)
            assert np.array_equal(out.view(np.uint32), R.view(np.uint32))
    # ... and the caller's array is not written
    R = np.eye(3, dtype=np.float32)
    backend.gyro_integrate(R, [1.0, 1.0, 1.0], 0.005)
    assert np.array_equal(R, np.eye(3, dtype=np.float32))
