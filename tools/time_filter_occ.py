"""Time the pose filter's loop on its two sampling routes on cuda:0 -- "dense" (every lattice sample: ngp_filter_iterations, unchanged) against "occupied"
(the samples in occupied grid cells only: ngp_filter_iterations_occ, DESIGN 3.5 "Occupancy-masked pose filter") -- on tools/time_filter.py's field, states
and sizes: ngp.workload's scene and its settled occupancy grid (density_thresh 10), 32 x 32 pixels, 1,024 rays x 512 steps, 300 Adam iterations.

Two views, because what the route saves is the empty part of the rays and that depends on where the camera looks: "across" is tools/time_filter.py's state
(a camera inside the box that looks across the ring: most of its rays meet no occupied cell), "orbit" the state whose camera is workload.orbit_pose(1),
the frame benchmark's kind of view (it looks at the scene's centre from outside the ring).

Both routes run in one process on the same queries, target, start and batches, in alternating rounds.  Reported per view:

  ms_per_iteration          one iteration = the five launches of one C call with n_iter = 1, between two events on the stream; median and quartiles over
                            the 300 iterations of every round (the state moves along the loop, so these are the iterations a filter step runs)
  loop_ms_per_iteration     the whole estimate_relative_pose call, wall time between two synchronisations, divided by the iterations (tools/time_filter.py's
                            number: one C call queues all 300)
  occupied_samples_per_ray  counts of ngp_nav_run_occ_forward over the 1,024 pixels at the start state and at the occupied route's final state
  multi                     the same per-iteration figures at 8 x 128 and 8 x 1,024 rays through the multi-start entry points
  minimiser                 the two routes' final states after the 300 iterations from the same start and batches: their difference (position, rotation
                            vector) and each one's distance from the state the target was rendered at.  Reported, not judged: the masked objective is
                            another function.

One JSON line."""
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
import ngp_hip as H  # noqa: E402
from ngp import nav  # noqa: E402
from ngp import workload as W  # noqa: E402
from ngp.field import NGPField  # noqa: E402
from ngp.render import NGPRenderer  # noqa: E402
from oracle import nav_oracle as NO  # noqa: E402
from time_filter import ITERS, RAYS, SIDE, START_OFFSET, STEPS, TRUE_STATE  # noqa: E402

MULTI = [(8, 128), (8, 1024)]


def make_queries(dev):
    """tools/time_filter.py's queries on a renderer that holds the workload's grid (the dense route never looks at it)"""
    model = W.make_model(0)
    sw, cw = W.nav_weights(0)
    field = NGPField(bound=W.BOUND).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(model["embeddings"]))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            layer.weight.copy_(torch.from_numpy(w))
    ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
    ren.load_density_grid(W.density_grid())
    return nav.NativeNavQueries(ren, W.intrinsics(SIDE, SIDE), SIDE, SIDE, num_steps=STEPS)


def state_of_pose(pose, dev):
    """the filter state (zero velocity and rate) whose measurement pose is `pose` [4,4]: the inverse of ngp.nav._measurement_pose's chain"""
    pose = torch.as_tensor(pose, dtype=torch.float32)
    about_x = nav._rot_x(torch.pi / 2)
    neg_yz = torch.tensor([[1., 0, 0], [0, -1, 0], [0, 0, -1]])
    flip_yz = torch.tensor([[0., 1, 0], [0, 0, 1], [1, 0, 0]])
    R = about_x.T @ (flip_yz.T @ pose[:3, :3] @ neg_yz)
    state = torch.zeros(12)
    state[:3] = flip_yz.T @ pose[:3, 3]
    state[6:9] = nav._rot_matrix_to_vec(R)
    state = state.to(dev)
    back = nav._measurement_pose(state)
    assert float((back[:3] - pose[:3].to(dev)).abs().max()) < 1e-5, float((back[:3] - pose[:3].to(dev)).abs().max())
    return state


def summary(values, digits=4):
    q = statistics.quantiles(values, n=4) if len(values) > 1 else [values[0]] * 3
    return {"median": round(statistics.median(values), digits), "quartiles": [round(q[0], digits), round(q[2], digits)]}


def iterations_by_events(filt, K, target, start, sig, batches, offsets, n):
    """n iterations, one C call each, an event before the first and after every one -> (ms per iteration [n], final states [K,12])"""
    B = int(batches.shape[1])
    c = filt._cfg_struct(B, start, sig)                              # once: it inverts the covariance and reads it back
    states = ((filt._vec(start)[None] + offsets[:K].to(filt.device)) + 1e-6).contiguous()
    st, prep = filt.queries.native.struct()
    if K == 1 and filt.sampling == "dense":                          # the single loop's own entry point: the route every filter step takes today
        adam, ws, state = filt.new_adam_state(), filt._workspace(B), states[0].clone()
        call = lambda k: H.check(H.lib().ngp_filter_iterations(ctypes.byref(st), H.ptr(prep), ctypes.byref(c), H.ptr(state), H.ptr(adam), H.ptr(target),   # noqa: E731
                                                               H.ptr(batches), k, 1, 1, None, None, None, H.ptr(ws), ws.numel(), H.stream()), "filter_iterations")
    else:
        adam, state = filt.new_adam_state_multi(K), states
        call = lambda k: filt._iterations_multi(c, k, 1, adam, state, target, batches, True, None, None, None)       # noqa: E731
    events = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    torch.cuda.synchronize()
    events[0].record()
    for k in range(n):
        call(k)
        events[k + 1].record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in zip(events, events[1:])], state.reshape(-1, 12).clone()


def loop_wall(filt, target, start, sig, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    final = filt.estimate_relative_pose(target, start, sig, batches, check=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / filt.iter, final


def occupied_counts(filt, state, pixels):
    rays = filt.rays(state, pixels)
    counts = torch.empty(pixels.shape[0], dtype=torch.int32, device=filt.device)
    with torch.no_grad():
        filt.queries.render_fn_occupied(rays["rays_o"], rays["rays_d"], counts)
    c = counts.float()
    return {"mean": round(float(c.mean()), 2), "median": float(c.median()), "max": int(c.max()), "rays_without_a_sample": int((counts == 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=ITERS)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    q = make_queries(dev)
    n = args.iters
    views = {"across": torch.tensor(TRUE_STATE, device=dev), "orbit": state_of_pose(W.orbit_pose(1), dev)}
    result = {}
    for view, true_state in views.items():
        start = true_state + torch.tensor(START_OFFSET, device=dev)
        sig = 0.1 * torch.eye(12, device=dev)
        with torch.no_grad():
            rays = q.get_rays_fn(NO.camera_pose_from_state(true_state).reshape(1, 4, 4))
            target = q.render_fn(rays["rays_o"], rays["rays_d"])["image"].reshape(SIDE, SIDE, 3).contiguous()
        rows, cols = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
        pixels = np.stack([rows.ravel(), cols.ravel()], -1)
        routes = ("dense", "occupied")
        sizes = sorted({RAYS} | {B for _, B in MULTI})
        filt = {(r, B): nav.NativePoseFilter({"batch_size": B, "lrate": 1e-3, "N_iter": n, "sig0": sig, "Q": sig}, q, sampling=r) for r in routes for B in sizes}
        batches = {B: filt[("dense", B)].draw_batches(pixels, n, np.random.default_rng(B)) for B in sizes}
        offsets = 0.01 * torch.randn(8, 12, generator=torch.Generator().manual_seed(0))
        offsets[0] = 0.0
        shapes = [(1, RAYS)] + MULTI
        for r in routes:                                                 # first launches, LDS attribute, workspaces
            loop_wall(filt[(r, RAYS)], target, start, sig, batches[RAYS])
            for K, B in shapes:
                iterations_by_events(filt[(r, B)], K, target, start, sig, batches[B], offsets, min(n, 5))
        per_iter = {(r, K, B): [] for r in routes for K, B in shapes}
        loop = {r: [] for r in routes}
        finals = {}
        for _ in range(args.rounds):
            for r in routes:
                ms, finals[r] = loop_wall(filt[(r, RAYS)], target, start, sig, batches[RAYS])
                loop[r].append(ms)
                for K, B in shapes:
                    ms_k, _ = iterations_by_events(filt[(r, B)], K, target, start, sig, batches[B], offsets, n)
                    per_iter[(r, K, B)] += ms_k
        med = lambda key: statistics.median(per_iter[key])               # noqa: E731
        out = {"case": f"{SIDE} x {SIDE} pixels, {RAYS} rays x {STEPS} steps, {n} iterations, {args.rounds} rounds",
               "ms_per_iteration": {r: summary(per_iter[(r, 1, RAYS)]) for r in routes},
               "dense_over_occupied": round(med(("dense", 1, RAYS)) / med(("occupied", 1, RAYS)), 3),
               "loop_ms_per_iteration": {r: summary(loop[r]) for r in routes},
               "loop_dense_over_occupied": round(statistics.median(loop["dense"]) / statistics.median(loop["occupied"]), 3),
               "occupied_samples_per_ray": {"at_the_start": occupied_counts(filt[("occupied", RAYS)], start + 1e-6, pixels),
                                            "at_the_occupied_final_state": occupied_counts(filt[("occupied", RAYS)], finals["occupied"], pixels), "of": STEPS},
               "multi": {f"{K}x{B}": {"ms_per_iteration": {r: summary(per_iter[(r, K, B)]) for r in routes},
                                      "dense_over_occupied": round(med(("dense", K, B)) / med(("occupied", K, B)), 3)} for K, B in MULTI}}
        d, o, tr = finals["dense"].double().cpu(), finals["occupied"].double().cpu(), true_state.double().cpu()
        dist = lambda a, b: {"position": float((a[:3] - b[:3]).norm()), "rotation_vector": float((a[6:9] - b[6:9]).norm()), "all_12": float((a - b).norm())}   # noqa: E731
        out["minimiser"] = {"occupied_minus_dense": dist(o, d), "dense_from_true": dist(d, tr), "occupied_from_true": dist(o, tr),
                            "start_from_true": dist(start.double().cpu(), tr),
                            "final_loss": {r: float(filt[(r, RAYS)].losses[-1]) for r in routes}}
        result[view] = out
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
