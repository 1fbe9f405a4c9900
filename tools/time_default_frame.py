"""Time an occupancy-grid frame of the DEFAULT float32 field (nerf/network.py, the model the nav loop flies in) on cuda:0, both ways, on the same renderer in
the same process:
   (a) NGPRenderer.render_fused_camera: one launch per frame (csrc/nav_frame.hip);
   (b) NGPRenderer.run_cuda in eval mode: the reference's loop, op by op, no autocast.
bench.py's nav model (workload.make_model(0) table + workload.nav_weights(0)), the S-ring density grid (density_thresh 10), 800 x 800, bench.py's
orbit of 8 poses.  Timed with events after a warm-up.  Prints ms per frame for both, samples per ray (stats[0]), the achieved fraction of the gather
roofline (1,024 B of float32 table per sample against 8 TB/s: bench.py's nav convention) and the FLOP floor (9,344 MAC per sample at 157.3 TFLOPS),
then one JSON line.
   python tools/time_default_frame.py [--frames 100] [--warmup 5] [--loop-frames 16] [--res 800]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("nerf-navigation_amd")
from ngp import workload as W  # noqa: E402
from ngp.field import NGPField  # noqa: E402
from ngp.render import NGPRenderer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=100, help="timed frames of the one-launch route (short runs scatter by +-10 %%)")
ap.add_argument("--loop-frames", type=int, default=16, help="timed frames of run_cuda (tens of milliseconds each); 0 = time the one-launch route only")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--res", type=int, default=800)
args = ap.parse_args()

BYTES_PER_SAMPLE, HBM_BPS = 1024.0, 8.0e12               # 16 levels x 8 corners x 8 B; bench.py's nav roofline
MAC_PER_SAMPLE, FLOPS = 9344.0, 157.3e12                 # 32x64 + 64x16 + 31x64 + 64x64 + 64x3; float32 vector / matrix peak

dev = torch.device("cuda:0")
model = W.make_model(0)
sw, cw = W.nav_weights(0)
field = NGPField(bound=W.BOUND).to(dev)
with torch.no_grad():
    field.encoder.embeddings.copy_(torch.from_numpy(model["embeddings"]))
    for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
        layer.weight.copy_(torch.from_numpy(w))
ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
ren.load_density_grid(W.density_grid())

H = Wd = args.res
intr = W.intrinsics(H, Wd)
radius, height = W.scene_orbit("ring")
poses = [W.orbit_pose(view, 8, radius, height).astype(np.float32) for view in range(8)]
rays = [tuple(torch.from_numpy(a).to(dev)[None] for a in W.get_rays(p, intr, H, Wd)) for p in poses]


def fused(k):
    return ren.render_fused_camera(poses[k % 8], intr, H, Wd, dt_gamma=0, bg_color=1, max_steps=1024)


def loop(k):
    o, d = rays[k % 8]
    with torch.no_grad():
        return ren.run_cuda(o, d, dt_gamma=0, bg_color=1, perturb=False, max_steps=1024)


def timeit(fn, n, warmup):
    for k in range(max(warmup, 1)):
        fn(k)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(n):
        fn(k)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / n


samples = float(np.mean([int(fused(k)["stats"][0]) for k in range(8)]))            # per frame, over the orbit
ms_fused = timeit(fused, max(args.frames, 100), args.warmup)
if args.loop_frames <= 0:
    print("(a) render_fused_camera, one launch per frame: %.3f ms per %dx%d frame (%d frames), %.1f samples per ray" % (ms_fused, H, Wd, max(args.frames, 100), samples / (H * Wd)))
    sys.exit(0)
d_image = float((fused(2)["image"].reshape(-1, 3) - loop(2)["image"].reshape(-1, 3)).abs().max())
ms_loop = timeit(loop, args.loop_frames, max(args.warmup // 2, 1))
per_ray = samples / (H * Wd)
gather_floor_ms = samples * BYTES_PER_SAMPLE / HBM_BPS * 1e3
flop_floor_ms = samples * 2.0 * MAC_PER_SAMPLE / FLOPS * 1e3
print("(a) render_fused_camera, one launch per frame: %.3f ms per %dx%d frame (%d frames)" % (ms_fused, H, Wd, max(args.frames, 100)))
print("(b) run_cuda, eval mode, op by op:             %.3f ms per frame (%d frames)   (a) is %.2fx faster; images differ by %.2g" %
      (ms_loop, args.loop_frames, ms_loop / ms_fused, d_image))
print("samples per ray %.1f (%.0f per frame)" % (per_ray, samples))
print("gather: 1,024 B per sample at 8 TB/s = %.3f ms per frame: (a) reaches %.1f %% of it" % (gather_floor_ms, 100.0 * gather_floor_ms / ms_fused))
print("FLOP floor: 9,344 MAC per sample at 157.3 TFLOPS = %.3f ms per frame: (a) reaches %.1f %% of it" % (flop_floor_ms, 100.0 * flop_floor_ms / ms_fused))
print(json.dumps({"metric": "default float32 field, occupancy-grid frame, ms", "ms_per_frame_fused": round(ms_fused, 4), "ms_per_frame_run_cuda": round(ms_loop, 4),
                  "speedup": round(ms_loop / ms_fused, 3), "samples_per_ray": round(per_ray, 2), "gather_fraction": round(gather_floor_ms / ms_fused, 4),
                  "flop_floor_ms": round(flop_floor_ms, 4), "frames": max(args.frames, 100), "loop_frames": args.loop_frames, "res": H}))
