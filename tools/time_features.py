"""Time the front of the pose filter's time step (find_POI, the dilation, coords[mask] and the draws: nav/estimator_helpers.py:181-204, 229-230) on cuda:0
at simulate.py's sizes: an 800 x 800 sensor image rendered from bench.py's nav field (tools/time_filter.py's field and camera), kernel_size 5, dil_iter 3,
1,024 rays, N_iter 300, 512 steps.  In ms:

  detect, regions, draw     NativePoseFilter.detect / ngp_features_regions / draw_batches_native, each alone (the mean of REPEAT back-to-back calls
                            between two synchronisations: the one synchronisation's latency is shared by the REPEAT calls); *_single is one call
                            between two synchronisations, which is what a caller who waits for the result sees
  host_draw                 the route the tree had: draw_batches over the same list on the host (300 draws of rng.choice(M, 1024, replace=False)) with its
                            copy to the device -- the one part with a like-for-like baseline
  step_native, step_host    estimate_state(features="native") against estimate_state(interest_regions=<the same list, on the host>)

All in one process, in alternating rounds (clocks and caches drift over a process' life), wall time between two synchronisations; median and quartiles over
the rounds.  The detector has no baseline here (no OpenCV): its time stands beside the bytes its launches move at the least (every level read once and
written once, the image read once), computed from the level sizes.  --sleep-us puts a host sleep between timed calls.  One JSON line."""
import argparse
import ctypes
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
import ngp_hip  # noqa: E402
from ngp import nav  # noqa: E402
from oracle import nav_oracle as NO  # noqa: E402
import time_filter as TF  # noqa: E402
from time_filter_step import ACTION, AGENT, quartiles  # noqa: E402

SIDE, RAYS, STEPS, ITERS = 800, 1024, 512, 300
KERNEL, DIL_ITER = 5, 3
REPEAT = 20


def wall(fn, repeat=1, sleep_us=0):
    """ms per call: `repeat` calls queued back to back between two synchronisations (after `sleep_us` of host sleep)"""
    if sleep_us:
        time.sleep(sleep_us * 1e-6)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeat):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / repeat, out


def render_target(q, state, dev):
    """the sensor image at `state`, a band of rows at a time"""
    with torch.no_grad():
        rays = q.get_rays_fn(NO.camera_pose_from_state(state).reshape(1, 4, 4))
        o, d = rays["rays_o"].reshape(-1, 3), rays["rays_d"].reshape(-1, 3)
        rows = []
        for a in range(0, o.shape[0], 1 << 16):
            rows.append(q.render_fn(o[None, a:a + (1 << 16)], d[None, a:a + (1 << 16)])["image"].reshape(-1, 3))
        return torch.cat(rows).reshape(SIDE, SIDE, 3).clamp(0.0, 1.0).contiguous()


def pyramid_bytes(H, W):
    """what the detector's launches move at the least: the image once; per level one read of its source and one write; per octave the six levels once
    more for the extrema; the mask once"""
    out = np.zeros(40, np.uint64)
    ngp_hip.lib().ngp_features_layout(H, W, out.ctypes.data_as(ctypes.c_void_p))
    total = 12 * H * W + H * W
    for o in range(int(out[0])):
        hw = int(out[4 + 3 * o]) * int(out[5 + 3 * o])
        total += 4 * hw * (2 * 6 + 6)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=ITERS)
    ap.add_argument("--sleep-us", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    TF.SIDE = SIDE                                            # time_filter.py's field behind an 800 x 800 sensor
    q = TF.make_queries(dev)
    true_state = torch.tensor(TF.TRUE_STATE, device=dev)
    start = true_state + torch.tensor(TF.START_OFFSET, device=dev)
    sig0, Q = 0.1 * torch.eye(12, device=dev), 0.01 * torch.eye(12, device=dev)
    action = torch.tensor(ACTION, device=dev)
    AGENT["I"] = AGENT["I"].to(dev)
    target = render_target(q, true_state, dev)
    cfg = {"batch_size": RAYS, "lrate": 1e-3, "N_iter": args.iters, "sig0": sig0, "Q": Q, "kernel_size": KERNEL, "dil_iter": DIL_ITER}
    filt = nav.NativePoseFilter(cfg, q, start.clone(), AGENT)

    def reset():
        filt.xt, filt.sig, filt.iteration = start.clone(), sig0.clone(), 0

    mask = filt.detect(target)
    regions = filt.interest_regions(target)
    M = int(regions.shape[0])
    if M < RAYS:
        raise SystemExit(f"the image yields {M} interest pixels, fewer than a batch of {RAYS}")
    regions_host = regions.cpu().numpy()
    ws = filt._features_workspace()
    list_out = torch.empty(SIDE * SIDE, 2, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)

    def regions_alone():
        ngp_hip.check(ngp_hip.lib().ngp_features_regions(ngp_hip.ptr(mask), SIDE, SIDE, KERNEL, DIL_ITER, ngp_hip.ptr(list_out), ngp_hip.ptr(count), ngp_hip.ptr(ws),
                                                         ws.numel(), ngp_hip.stream()), "features_regions")

    rng = np.random.default_rng(0)
    # warm-up: every route once
    reset(); filt.estimate_state(target, action, features="native", seed=1)
    reset(); filt.estimate_state(target, action, interest_regions=regions_host, rng=rng)
    regions_alone()
    times = {k: [] for k in ("detect", "regions", "draw", "detect_single", "regions_single", "draw_single", "host_draw", "step_native", "step_host")}
    s = args.sleep_us
    for _ in range(args.rounds):
        times["detect"].append(wall(lambda: filt.detect(target), REPEAT, s)[0])
        times["regions"].append(wall(regions_alone, REPEAT, s)[0])
        times["draw"].append(wall(lambda: filt.draw_batches_native(regions, args.iters, 7), REPEAT, s)[0])
        times["detect_single"].append(wall(lambda: filt.detect(target), 1, s)[0])
        times["regions_single"].append(wall(regions_alone, 1, s)[0])
        times["draw_single"].append(wall(lambda: filt.draw_batches_native(regions, args.iters, 7), 1, s)[0])
        times["host_draw"].append(wall(lambda: filt.draw_batches(regions_host, args.iters, rng), 1, s)[0])
        reset(); times["step_native"].append(wall(lambda: filt.estimate_state(target, action, features="native", seed=1), 1, s)[0])
        reset(); times["step_host"].append(wall(lambda: filt.estimate_state(target, action, interest_regions=regions_host, rng=rng), 1, s)[0])
    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = pyramid_bytes(SIDE, SIDE)
    out = {"case": f"{SIDE} x {SIDE} image, kernel {KERNEL} x {KERNEL} x {DIL_ITER}, {RAYS} rays x {STEPS} steps, {args.iters} iterations, {args.rounds} alternating rounds"
                   + (f", {s} us of host sleep between timed calls" if s else ""),
           "keypoint_pixels": int(mask.sum()), "M": M,
           "ms": {k: quartiles(v) for k, v in times.items()},
           "detect_min_bytes": nbytes, "detect_GBps_of_min_bytes": round(nbytes / (med["detect"] * 1e-3) / 1e9, 1),
           "draw_speedup_over_host": round(med["host_draw"] / med["draw_single"], 1),
           "front_native_ms": round(med["detect"] + med["regions"] + med["draw"], 4),
           "step_native_over_step_host": round(med["step_native"] / med["step_host"], 4)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
