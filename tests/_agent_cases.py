"""Shared by tests/test_agent_host.py and tests/test_gpu_agent.py: the numpy restatement of the sensor contract (include/ngp_hip.h: ngp_agent_sensor), its
test input, and the golden file of the agent's step (tests/golden/agent.npz, written by tests/golden/make_agent_golden.py)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GOLD = None


def gold():
    global _GOLD
    if _GOLD is None:
        _GOLD = dict(np.load(os.path.join(ROOT, "tests", "golden", "agent.npz")))
    return _GOLD


def names():
    return [str(n) for n in gold()["names"]]


def sensor_restated(image):
    """c = clamp(image, 0, 1); png = (uint8)(c * 255.0f), a float32 product truncated; target = (float)((double)png / 255.0)"""
    image = np.asarray(image)
    assert image.dtype == np.float32
    c = np.minimum(np.maximum(image, np.float32(0)), np.float32(1))
    product = c * np.float32(255.0)
    assert product.dtype == np.float32
    png = product.astype(np.uint8)
    target = (png.astype(np.float64) / 255.0).astype(np.float32)
    return png, target


def sensor_values():
    """every k / 255 as float32 with its two float32 neighbours, 0 and 1, and values just outside [0, 1]: 783 values"""
    k = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    inside = np.stack([np.nextafter(k, np.float32(-1)), k, np.nextafter(k, np.float32(2))], -1).reshape(-1)
    tiny = np.float32(np.finfo(np.float32).tiny)
    outside = np.array([0.0, 1.0, -tiny, np.nextafter(np.float32(0), np.float32(-1)), -1e-7, -0.5, -3.0, np.nextafter(np.float32(1), np.float32(2)),
                        1.0 + 1e-6, 1.5, 255.0, 1e30, -1e30, -0.0, 0.5], np.float32)
    return np.concatenate([inside, outside]).astype(np.float32)


def sensor_input(N):
    """[N,3] float32 from sensor_values(): all of them when 3 N >= 783 (then repeated), else a window that starts at another place for every N"""
    v = sensor_values()
    return np.resize(np.roll(v, -7 * N), 3 * N).reshape(N, 3).astype(np.float32)
