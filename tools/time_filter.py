"""Time the pose filter's optimisation loop (Estimator.estimate_relative_pose, nav/estimator_helpers.py:227-241) on cuda:0 at simulate.py's sizes --
1,024 rays x 512 steps, 300 Adam iterations -- on bench.py's nav field (NGPField + workload.nav_weights(0), float32, 32 x 32 pixels), in ms per
iteration:

  (a) the native loop: NativePoseFilter.estimate_relative_pose (csrc/nav_filter.hip; 5 launches per iteration, all 300 queued by one C call);
  (b) the route available without it: the restated measurement function (oracle/nav_oracle.py: measurement_loss) over NativeNavQueries + backward
      + torch.optim.Adam(capturable=True), with the reference's per-iteration loss.item() and copy of the state to the host.

Both in one process, in alternating rounds (a b a b ...; clocks and caches drift over a process' life), wall time between two synchronisations; the
median over the rounds is reported, every round is listed.  (b) runs ITERS_B iterations per round (default 100).  One JSON line.  For the split of the five
launches run it under `rocprofv3 --kernel-trace --stats -- python tools/time_filter.py --native-only`."""
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
importlib.import_module("nerf-navigation_amd")
from ngp import nav  # noqa: E402
from ngp import workload as W  # noqa: E402
from ngp.field import NGPField  # noqa: E402
from ngp.render import NGPRenderer  # noqa: E402
from oracle import nav_oracle as NO  # noqa: E402

SIDE, RAYS, STEPS, ITERS = 32, 1024, 512, 300
# a camera inside the box that looks across the ring (position, velocity, rotation vector, rate); the start is what the dynamics would predict
TRUE_STATE = [0.93, -1.11, 0.44, 0.1, -0.03, 0.02, 0.117, -0.221, 2.267, 0.0, 0.02, 0.005]
START_OFFSET = [0.016, 0.008, 0.012, 0.003, -0.02, -0.003, 0.003, 0.02, 0.033, 0.01, 0.0, -0.035]


def make_queries(dev):
    model = W.make_model(0)
    sw, cw = W.nav_weights(0)
    field = NGPField(bound=W.BOUND).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(model["embeddings"]))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            layer.weight.copy_(torch.from_numpy(w))
    ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=False).to(dev).eval()
    return nav.NativeNavQueries(ren, W.intrinsics(SIDE, SIDE), SIDE, SIDE, num_steps=STEPS)


def time_native(filt, target, start, sig, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    filt.estimate_relative_pose(target, start, sig, batches)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3 / filt.iter, (t1 - t0) * 1e3 / filt.iter


def time_torch_route(q, target, start, sig, batches, n, lr):
    state = (start.clone().detach() + 1e-6).requires_grad_(True)
    opt = torch.optim.Adam(params=[state], lr=lr, betas=(0.9, 0.999), capturable=True)
    losses, states = [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        opt.zero_grad()
        loss = NO.measurement_loss(state, start, sig, target, batches[k].long(), q.get_rays_fn, q.render_fn)
        losses.append(loss.item())                              # nav/estimator_helpers.py:237-238
        states.append(state.clone().cpu().detach().numpy().tolist())
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters-b", type=int, default=int(os.environ.get("ITERS_B", "100")))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    q = make_queries(dev)
    true_state = torch.tensor(TRUE_STATE, device=dev)
    start = true_state + torch.tensor(START_OFFSET, device=dev)
    sig = 0.1 * torch.eye(12, device=dev)
    with torch.no_grad():
        rays = q.get_rays_fn(NO.camera_pose_from_state(true_state).reshape(1, 4, 4))
        target = q.render_fn(rays["rays_o"], rays["rays_d"])["image"].reshape(SIDE, SIDE, 3).contiguous()
    filt = nav.NativePoseFilter({"batch_size": RAYS, "lrate": 1e-3, "N_iter": ITERS, "sig0": sig, "Q": sig}, q)
    rows, cols = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
    batches = filt.draw_batches(np.stack([rows.ravel(), cols.ravel()], -1), ITERS, np.random.default_rng(0))
    warm = nav.NativePoseFilter({"batch_size": RAYS, "lrate": 1e-3, "N_iter": 10, "sig0": sig, "Q": sig}, q)
    warm.estimate_relative_pose(target, start, sig, batches)     # first launches, LDS attribute, workspace
    if not args.native_only:
        time_torch_route(q, target, start, sig, batches, 10, 1e-3)
    native, enqueue, torch_route = [], [], []
    for _ in range(args.rounds):
        ms, enq = time_native(filt, target, start, sig, batches)
        native.append(ms); enqueue.append(enq)
        if not args.native_only:
            torch_route.append(time_torch_route(q, target, start, sig, batches, args.iters_b, 1e-3))
    out = {"case": f"{RAYS} rays x {STEPS} steps, {ITERS} iterations", "launches_per_iteration": 5,
           "native_ms_per_iteration": round(statistics.median(native), 4), "native_rounds": [round(v, 4) for v in native],
           "native_enqueue_ms_per_iteration": round(statistics.median(enqueue), 4),
           "loss_first_last": [round(float(filt.losses[0]), 6), round(float(filt.losses[-1]), 6)]}
    if not args.native_only:
        out.update(torch_route_ms_per_iteration=round(statistics.median(torch_route), 4), torch_route_rounds=[round(v, 4) for v in torch_route],
                   torch_route_iterations=args.iters_b, speedup=round(statistics.median(torch_route) / statistics.median(native), 2))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
