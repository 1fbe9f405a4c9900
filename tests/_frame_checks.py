"""Conditions on a rendered frame that do not depend on which frame kernel rendered it, shared by test_gpu_frame_inside.py (render_fused.hip, half
precision) and test_gpu_default_frame_inside.py (nav_frame.hip, float32)."""
import numpy as np
import torch


def _written(out, what):
    for key in ("image", "weights_sum"):
        assert not bool(torch.isnan(out[key]).any()), f"{what}: {key}: {int(torch.isnan(out[key]).sum())} values were not written"
    assert bool((out["stats"] >= 0).all()), (what, out["stats"])


def _same_count_same_weight(ws, n, what):
    """constant density and constant step: a ray's weights_sum depends on its sample count alone and strictly increases with it
    (test_gpu_fullsize.test_fused_march_gives_every_ray_the_single_march_sample_count), here against the CPU oracle's per-ray counts"""
    order = np.argsort(n, kind="stable")
    n_s, ws_s = n[order], ws[order]
    same = n_s[1:] == n_s[:-1]
    bad = np.flatnonzero(same & (ws_s[1:] != ws_s[:-1]))
    assert bad.size == 0, f"{what}: rays {order[bad[:4] + 1].tolist()} and {order[bad[:4]].tolist()} have {n_s[bad[:4]].tolist()} samples each but differ in weights_sum"
    bad = np.flatnonzero(~same & ~(ws_s[1:] > ws_s[:-1]))
    assert bad.size == 0, (f"{what}: weights_sum does not increase with the sample count: rays {order[bad[:4] + 1].tolist()} "
                           f"({n_s[bad[:4] + 1].tolist()} samples in the oracle) against {order[bad[:4]].tolist()} ({n_s[bad[:4]].tolist()})")
    assert bool((ws[n == 0] == 0).all()), f"{what}: a ray without samples has weight"
