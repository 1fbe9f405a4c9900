"""Time the pose filter's loop on its "resampled" route on cuda:0 (ngp_filter_iterations_res: NeRFRenderer.run's importance resampling on the device, DESIGN 3.5
"Resampled run") against the dense 512-step loop of the same build, on tools/time_filter_occ.py's field, views, states and protocol: ngp.workload's scene,
32 x 32 pixels, 1,024 rays, 300 Adam iterations, the two views "across" and "orbit", alternating rounds in one process, medians over the rounds.

Reported per view:

  ms_per_iteration     one iteration = one C call with n_iter = 1 between two events on the stream (five launches dense, six resampled); median and quartiles
                       over the 300 iterations of every round, for dense 512 and resampled (128, 128), (64, 64), (256, 256)
  loop_ms_per_iteration the whole estimate_relative_pose call (one C call queues all 300), wall time between two synchronisations, per iteration
  multi_8x1024         the per-iteration figure of the 8 x 1,024-ray multi-start loop, dense and resampled (128, 128)
  op_chain             NavQueries' torch op chain with the same upsample_steps (the only route before this one): the restated measurement function + backward
                       + torch's Adam, wall time per iteration over --chain-iters iterations
  kernels              k_nav_resample, k_nav_run_fwd<true>, k_nav_run_bwd<true> at 1,024 rays, each between two events (ngp_hip.TIMERS), medians
  minimiser            how far each resampled shape's final state after the 300 iterations sits from the dense 512-step run's, and both from the state the
                       target was rendered at.  Reported, not judged: the resampled objective is another function.

One JSON line."""
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
import ngp_hip as H  # noqa: E402
from ngp import nav  # noqa: E402
from ngp import workload as W  # noqa: E402
from oracle import nav_oracle as NO  # noqa: E402
from time_filter import ITERS, RAYS, SIDE, START_OFFSET, STEPS, TRUE_STATE, make_queries  # noqa: E402  (a cuda_ray=False renderer: no occupancy grid)
from time_filter_occ import iterations_by_events, loop_wall, state_of_pose, summary  # noqa: E402

SHAPES = [(128, 128), (64, 64), (256, 256)]
MULTI_K = 8


def chain_ms(ren, target, start, sig, batches, Nc, Nf, n, lr):
    """tools/time_filter.py's torch route over NavQueries(upsample_steps = Nf): ms per iteration"""
    q = nav.NavQueries(ren, W.intrinsics(SIDE, SIDE), SIDE, SIDE, num_steps=Nc, upsample_steps=Nf)
    state = (start.clone().detach() + 1e-6).requires_grad_(True)
    opt = torch.optim.Adam(params=[state], lr=lr, betas=(0.9, 0.999), capturable=True)

    def one(k):
        opt.zero_grad()
        loss = NO.measurement_loss(state, start, sig, target, batches[k].long(), q.get_rays_fn, q.render_fn)
        loss.item()                                              # nav/estimator_helpers.py:237-238
        loss.backward()
        opt.step()
    one(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(1, n + 1):
        one(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def kernel_ms(q, rays, Nf, repeat=20):
    """medians of the three launches of _nav_run_resampled (forward with a gradient asked, then backward) at these rays"""
    H.TIMERS = {}
    for _ in range(repeat + 2):
        o, d = rays["rays_o"].clone().requires_grad_(True), rays["rays_d"].clone().requires_grad_(True)
        q.render_fn_resampled(o[None], d[None], Nf)["image"].sum().backward()
    torch.cuda.synchronize()
    out = {}
    for name, ev in H.TIMERS.items():
        out[name] = round(statistics.median([a.elapsed_time(b) for a, b in ev[2:]]), 4)
    H.TIMERS = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=ITERS)
    ap.add_argument("--chain-iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dense_q = make_queries(dev)
    ren = dense_q.renderer
    n = args.iters
    queries = {"dense": dense_q}
    for Nc, Nf in SHAPES:
        queries[(Nc, Nf)] = nav.NativeNavQueries(ren, W.intrinsics(SIDE, SIDE), SIDE, SIDE, num_steps=Nc)
    views = {"across": torch.tensor(TRUE_STATE, device=dev), "orbit": state_of_pose(W.orbit_pose(1), dev)}
    result = {}
    for view, true_state in views.items():
        start = true_state + torch.tensor(START_OFFSET, device=dev)
        sig = 0.1 * torch.eye(12, device=dev)
        with torch.no_grad():
            rays = dense_q.get_rays_fn(NO.camera_pose_from_state(true_state).reshape(1, 4, 4))
            target = dense_q.render_fn(rays["rays_o"], rays["rays_d"])["image"].reshape(SIDE, SIDE, 3).contiguous()
        rows, cols = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
        pixels = np.stack([rows.ravel(), cols.ravel()], -1)
        cfg = {"batch_size": RAYS, "lrate": 1e-3, "N_iter": n, "sig0": sig, "Q": sig}
        filt = {"dense": nav.NativePoseFilter(cfg, dense_q)}
        for Nc, Nf in SHAPES:
            filt[(Nc, Nf)] = nav.NativePoseFilter(cfg, queries[(Nc, Nf)], sampling="resampled", upsample_steps=Nf)
        batches = filt["dense"].draw_batches(pixels, n + 1, np.random.default_rng(RAYS))
        offsets = 0.01 * torch.randn(MULTI_K, 12, generator=torch.Generator().manual_seed(0))
        offsets[0] = 0.0
        routes = list(filt)
        multi_routes = ["dense", SHAPES[0]]
        for r in routes:                                                 # first launches, LDS attribute, workspaces
            loop_wall(filt[r], target, start, sig, batches)
            iterations_by_events(filt[r], 1, target, start, sig, batches, offsets, min(n, 5))
        for r in multi_routes:
            iterations_by_events(filt[r], MULTI_K, target, start, sig, batches, offsets, min(n, 5))
        per_iter, loop, multi, finals = {r: [] for r in routes}, {r: [] for r in routes}, {r: [] for r in multi_routes}, {}
        for _ in range(args.rounds):
            for r in routes:
                ms, finals[r] = loop_wall(filt[r], target, start, sig, batches)
                loop[r].append(ms)
                per_iter[r] += iterations_by_events(filt[r], 1, target, start, sig, batches, offsets, n)[0]
            for r in multi_routes:
                multi[r] += iterations_by_events(filt[r], MULTI_K, target, start, sig, batches, offsets, n)[0]
        name = lambda r: f"dense_{STEPS}" if r == "dense" else f"resampled_{r[0]}_{r[1]}"      # noqa: E731
        tr = true_state.double().cpu()
        dist = lambda a, b: {"position": float((a[:3] - b[:3]).norm()), "rotation_vector": float((a[6:9] - b[6:9]).norm()), "all_12": float((a - b).norm())}   # noqa: E731
        d = finals["dense"].double().cpu()
        some = filt["dense"].rays(start + 1e-6, pixels)
        out = {"case": f"{SIDE} x {SIDE} pixels, {RAYS} rays, {n} iterations, {args.rounds} rounds",
               "ms_per_iteration": {name(r): summary(per_iter[r]) for r in routes},
               "loop_ms_per_iteration": {name(r): summary(loop[r]) for r in routes},
               f"multi_{MULTI_K}x{RAYS}": {name(r): summary(multi[r]) for r in multi_routes},
               "op_chain": {f"NavQueries_{Nc}_{Nf}": round(chain_ms(ren, target, start, sig, batches, Nc, Nf, args.chain_iters, 1e-3), 3) for Nc, Nf in SHAPES[:1]},
               "kernels": {name(r): kernel_ms(queries[r], some, r[1]) for r in SHAPES},
               "minimiser": {"start_from_true": dist(start.double().cpu(), tr), "dense_from_true": dist(d, tr),
                             **{name(r): {"minus_dense": dist(finals[r].double().cpu(), d), "from_true": dist(finals[r].double().cpu(), tr),
                                          "final_loss": float(filt[r].losses[-1])} for r in SHAPES},
                             "dense_final_loss": float(filt["dense"].losses[-1])}}
        result[view] = out
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
