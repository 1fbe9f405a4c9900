"""The frame kernel's tile order off and on (ngp_render_set_tile_order), and with it the pick among an XCD's bands by their next tile's estimate
(ngp_render_set_band_merge; NGP_BAND_HYSTERESIS sets its h): ms per 800x800 frame of the hand-set scene for a camera on bench's orbit, one below the
scene and one above it:  python tools/time_tile_order.py [frames] [res]
Each (pose, setting) is timed twice, interleaved, with HIP events around every launch (mean of the launches after 5 warm-up frames)."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("nerf-navigation_amd")
import ngp_hip  # noqa: E402
from ngp import workload as W  # noqa: E402
from ngp.field import NGPFieldFF  # noqa: E402
from ngp.render import NGPRenderer  # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 100
res = int(sys.argv[2]) if len(sys.argv) > 2 else 800
dev = torch.device("cuda:0")
field = NGPFieldFF(bound=W.BOUND).to(dev).load_arrays(W.make_model(0))
ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
ren.load_density_grid(W.density_grid())
intr = W.intrinsics(res, res)
L = ngp_hip.lib()
poses = {"orbit(1)": W.orbit_pose(1), "below(z=-1.2)": W.orbit_pose(1, height=-1.2), "above(z=1.5)": W.orbit_pose(1, height=1.5)}


SETTINGS = {"row-major": (0, 0), "cost order": (1, 0), "cost order + band merge": (1, 1)}       # (tile order, band merge)


def time_pose(pose, order, merge):
    previous = L.ngp_render_set_tile_order(order)
    previous_merge = L.ngp_render_set_band_merge(merge)
    try:
        for _ in range(5):
            ren.render_fused_camera(pose, intr, res, res, bg_color=1)
        ev = []
        for _ in range(frames):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = ren.render_fused_camera(pose, intr, res, res, bg_color=1)
            b.record()
            ev.append((a, b))
        torch.cuda.synchronize()
    finally:
        L.ngp_render_set_tile_order(previous)
        L.ngp_render_set_band_merge(previous_merge)
    return float(np.mean([a.elapsed_time(b) for a, b in ev])), int(out["stats"][0])


for name, pose in poses.items():
    t = {k: [] for k in SETTINGS}
    for _ in range(2):
        for k, (order, merge) in SETTINGS.items():
            ms, smp = time_pose(pose, order, merge)
            t[k].append(ms)
    base = np.mean(t["row-major"])
    print("%-14s samples %9d  " % (name, smp) + "  ".join(
        "%s %s ms%s" % (k, " / ".join("%.3f" % v for v in t[k]), "" if k == "row-major" else " (%+.1f %%)" % (100.0 * (np.mean(t[k]) / base - 1.0))) for k in SETTINGS))
