"""Time a training step of the DEFAULT float32 field (ngp.field.NGPField) through NGPTrainer(fp16=False): the op-by-op autograd chain against the
native forward / backward of csrc/nav_train.hip (`fused_training=True`), and against the same with the table gradient from the float32 binned scatter
(`reproducible=True`: route `fused_reproducible`).  bench.py's training workload (ngp.workload's scene, teacher-rendered
200 x 200 views, 4,096 rays per step, the seed fixed), in two phases: the first steps on the initial, nearly full occupancy grid, and after
`--settle` further steps, when the grid has converged to the scene.  Every step is timed with its own pair of events; printed are the median, the
quartiles and the extremes of `--steps` steps after `--warmup` untimed ones, and the points per step.  The routes run in ONE process, phase by
phase in alternation, so that clocks and neighbours are shared.
   python tools/time_default_train.py [--steps 30] [--warmup 5] [--settle 1460] [--routes op_chain,fused,fused_reproducible]"""
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
from ngp.field import NGPField, NGPFieldFF  # noqa: E402
from ngp.render import NGPRenderer  # noqa: E402
from ngp.train import NGPTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--settle", type=int, default=1460)
ap.add_argument("--rays", type=int, default=4096)
ap.add_argument("--routes", default="op_chain,fused,fused_reproducible")
args = ap.parse_args()
dev = torch.device("cuda:0")
res = 200

teacher = NGPRenderer(NGPFieldFF(bound=W.BOUND).to(dev).load_arrays(W.make_model(0)), bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
teacher.load_density_grid(W.density_grid())
pool = []
for view in range(8):
    o, d = W.get_rays(W.orbit_pose(view, 8), W.intrinsics(res, res), res, res)
    to, td = torch.from_numpy(o).to(dev)[None], torch.from_numpy(d).to(dev)[None]
    pool.append((to, td, teacher.render_fused(to, td, bg_color=1, image_width=res)["image"]))


class Route:
    def __init__(self, name):
        torch.manual_seed(0)                                              # the same initial parameters for every route
        field = NGPField(bound=W.BOUND, fused_training=name != "op_chain", reproducible=name == "fused_reproducible")
        self.ren = NGPRenderer(field.to(dev), bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev)
        self.tr = NGPTrainer(self.ren, lr=1e-2, iters=30000, fp16=False, steps_per_epoch=len(pool))
        self.gen = torch.Generator(device=dev).manual_seed(1)
        self.k = 0

    def step(self):
        to, td, tc = pool[self.k % len(pool)]
        idx = torch.randint(0, res * res, (args.rays,), device=dev, generator=self.gen)
        self.k += 1
        return self.tr.step(to[:, idx], td[:, idx], tc[:, idx], bg_color=1, max_steps=1024)

    def points(self):
        n = min(16, self.ren.local_step)
        return float(self.ren.step_counter[:n, 0].float().mean().item())

    def timed(self, count):
        ms = []
        for _ in range(count):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            loss = self.step()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        q = np.percentile(ms, [0, 25, 50, 75, 100])
        return dict(median_ms=float(q[2]), q25_ms=float(q[1]), q75_ms=float(q[3]), min_ms=float(q[0]), max_ms=float(q[4]), steps=count,
                    points_per_step=self.points(), loss=float(loss))


routes = {name: Route(name) for name in args.routes.split(",")}
for phase, untimed in (("initial grid", args.warmup), (f"after {args.settle} more steps", args.settle)):
    for name, r in routes.items():
        for _ in range(untimed):
            r.step()
        torch.cuda.synchronize()
    for name, r in routes.items():
        out = r.timed(args.steps)
        print(json.dumps(dict(route=name, phase=phase, rays=args.rays, **out)), flush=True)
