"""Time the multi-start pose filter (NativePoseFilter.estimate_relative_pose_multi: K hypotheses of B rays as one K B-ray launch sequence, csrc/nav_filter.hip)
on cuda:0 against the existing single-hypothesis route, on tools/time_filter.py's field and sizes (bench.py's nav field, 32 x 32 pixels, 512 steps, 300 Adam
iterations), in ms per iteration:

  (a) K in {2, 4, 8} at B = 1,024: one multi-start call against K successive estimate_relative_pose calls (ngp_filter_iterations, K times);
  (b) packing: 8 x 128, 4 x 256 and 2 x 512 rays in one call against one 1,024-ray single run and against K successive single runs at the small B; the single
      run at B in {128, 256, 512, 1,024} is the fill curve;
  (c) what a multi-start call costs beyond its iterations: the extra measurement pass (update = 0) and the selection, in ms per call.

A multi-start call is timed whole (iterations + the extra pass + the selection) and divided by the 300 iterations.  Everything runs in one process in
alternating rounds (clocks and caches drift over a process' life), wall time between two synchronisations; medians with quartiles over the rounds.  One JSON line."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
importlib.import_module("nerf-navigation_amd")
from ngp import nav  # noqa: E402
from oracle import nav_oracle as NO  # noqa: E402
from time_filter import ITERS, SIDE, START_OFFSET, TRUE_STATE, make_queries  # noqa: E402

SAME_B = [(2, 1024), (4, 1024), (8, 1024)]
PACKED = [(8, 128), (4, 256), (2, 512)]
CURVE = [128, 256, 512, 1024]


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(values, digits=4):
    q = statistics.quantiles(values, n=4) if len(values) > 1 else [values[0]] * 3
    return {"median": round(statistics.median(values), digits), "quartiles": [round(q[0], digits), round(q[2], digits)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=ITERS)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    q = make_queries(dev)
    true_state = torch.tensor(TRUE_STATE, device=dev)
    start = true_state + torch.tensor(START_OFFSET, device=dev)
    sig = 0.1 * torch.eye(12, device=dev)
    with torch.no_grad():
        rays = q.get_rays_fn(NO.camera_pose_from_state(true_state).reshape(1, 4, 4))
        target = q.render_fn(rays["rays_o"], rays["rays_d"])["image"].reshape(SIDE, SIDE, 3).contiguous()
    rows, cols = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    pixels = np.stack([rows.ravel(), cols.ravel()], -1)
    n = args.iters
    filt, batches = {}, {}
    for B in CURVE:
        filt[B] = nav.NativePoseFilter({"batch_size": B, "lrate": 1e-3, "N_iter": n, "sig0": sig, "Q": sig}, q)
        batches[B] = filt[B].draw_batches(pixels, n, np.random.default_rng(B))
    offsets = 0.01 * torch.randn(8, 12, generator=torch.Generator().manual_seed(0))
    offsets[0] = 0.0                                                # hypothesis 0 is the single route's start

    def single(B, times=1):
        for _ in range(times):
            filt[B].estimate_relative_pose(target, start, sig, batches[B], check=False)

    def multi(K, B):
        filt[B].estimate_relative_pose_multi(target, start, sig, batches[B], offsets[:K], check=False)

    for K, B in SAME_B + PACKED:                                   # first launches, LDS attribute, workspaces
        multi(K, B)
        single(B)
    torch.cuda.synchronize()
    times = {}
    extra = {f"{K}x{B}": {"pass": [], "select": []} for K, B in SAME_B + PACKED}
    for _ in range(args.rounds):
        for B in CURVE:
            times.setdefault(f"single {B}", []).append(wall_ms(lambda: single(B)) / n)
        for K, B in SAME_B + PACKED:
            times.setdefault(f"multi {K}x{B}", []).append(wall_ms(lambda: multi(K, B)) / n)
            times.setdefault(f"successive {K}x{B}", []).append(wall_ms(lambda: single(B, K)) / n)
            m = filt[B].multi
            states, adam, final = m["states"].clone(), filt[B].new_adam_state_multi(K), torch.empty(1, K, device=dev)
            c = filt[B]._cfg_struct(B, start, sig)                  # estimate_relative_pose_multi builds it once for the iterations and the extra pass
            extra[f"{K}x{B}"]["pass"].append(wall_ms(lambda: filt[B]._iterations_multi(c, n - 1, 1, adam, states, target, batches[B], False, final, None, None)))
            extra[f"{K}x{B}"]["select"].append(wall_ms(lambda: filt[B].select(final[0], states)))
    out = {"case": f"{SIDE} x {SIDE} pixels, 512 steps, {n} iterations, {args.rounds} rounds", "launches_per_iteration": 5,
           "ms_per_iteration": {k: summary(v) for k, v in times.items()},
           "ms_per_call_beyond_the_iterations": {k: {p: summary(v[p]) for p in v} for k, v in extra.items()}}
    ratios = {}
    for K, B in SAME_B + PACKED:
        med = lambda key: statistics.median(times[key])             # noqa: E731
        ratios[f"{K}x{B}"] = {"successive_over_multi": round(med(f"successive {K}x{B}") / med(f"multi {K}x{B}"), 3),
                              "multi_over_single_1024": round(med(f"multi {K}x{B}") / med("single 1024"), 3)}
    out["ratios"] = ratios
    out["winner_of_8x128"] = int(filt[128].multi["index"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
