"""Time the planner's optimisation epoch (Planner.learn_init, nav/quad_plot.py:256-280) on cuda:0 at simulate.py's sizes (steps 20, body
10 x 10 x 5 = 500 points, 2,500 epochs) and with R = 40 rows of states (steps 42), in ms per epoch:

  (a) the reference structure: the restated planner (oracle/nav_oracle.py: planner_costs) + backward + torch.optim.Adam(capturable=True) over
      NativeNavQueries.density_fn, once with the per-epoch `print(it, loss)` sync the reference makes (here: loss.item()) and once without;
  (b) the native loop: NativePlanner.run_epochs (csrc/nav_plan.hip; 3 launches per epoch, no synchronisation).

The field is tests/test_gpu_nav_golden.py's (NGPField + workload.nav_weights(0), float32).  Wall time between two synchronisations; (a) runs
EPOCHS_A epochs (default 250) after 20 of warm-up, (b) the full 2,500 after one warm-up call.  One JSON line per case.  For the split of the three
launches run it under `rocprofv3 --kernel-trace --stats -- python tools/time_nav_plan.py --native-only`."""
import argparse
import importlib
import json
import os
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

SIM_START, SIM_END = [0.39, -0.67, 0.2], [-0.4, 0.55, 0.16]
BODY = [[-0.05, 0.05], [-0.05, 0.05], [-0.02, 0.02]]


def make_queries(dev):
    model = W.make_model(0)
    sw, cw = W.nav_weights(0)
    field = NGPField(bound=W.BOUND).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(model["embeddings"]))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            layer.weight.copy_(torch.from_numpy(w))
    ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=False).to(dev).eval()
    return nav.NativeNavQueries(ren, (20., 20., 10., 10.), 20, 20, num_steps=64)


def cfg_for(steps):
    return {"T_final": 2., "steps": steps, "lr": 0.001, "epochs_init": 2500, "epochs_update": 250, "fade_out_epoch": 0, "fade_out_sharpness": 10,
            "mass": 1., "I": torch.eye(3), "g": 10., "body": np.array(BODY), "nbins": [10, 10, 5]}


def time_reference(q, plan, n, sync_every_epoch):
    st = plan.states.detach().clone().requires_grad_(True)
    ia = plan.initial_accel.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([ia, st], lr=plan.cfg["lr"], capturable=True)

    def epochs(k):
        for it in range(k):
            opt.zero_grad()
            loss = NO.planner_costs(st, ia, plan.start_state, plan.end_state, plan.cfg, plan.robot_body, q.density_fn, epoch=it)["total"]
            if sync_every_epoch:
                loss.item()                                 # what print(it, loss) costs (nav/quad_plot.py:264)
            loss.backward()
            opt.step()
    epochs(20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    epochs(n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def time_native(plan, n):
    adam = plan.new_adam_state()
    losses = torch.empty(n, device=plan.device)
    states0, ia0 = plan.states.clone(), plan.initial_accel.clone()
    plan.run_epochs(0, 50, adam, losses=losses)             # warm-up (first launches, LDS attribute)
    torch.cuda.synchronize()
    plan.states.copy_(states0); plan.initial_accel.copy_(ia0); adam.zero_()
    t0 = time.perf_counter()
    plan.run_epochs(0, n, adam, losses=losses)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3 / n, (t1 - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--epochs", type=int, default=2500)
    ap.add_argument("--epochs-a", type=int, default=int(os.environ.get("EPOCHS_A", "250")))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    q = make_queries(dev)
    start, end = NO.state18(SIM_START), NO.state18(SIM_END)
    for steps in (20, 42):
        cfg = cfg_for(steps)
        plan = nav.NativePlanner(start, end, cfg, q)
        out = {"case": f"steps{steps}", "R": plan.R, "B": int(plan.robot_body.shape[0]), "points": plan.S * int(plan.robot_body.shape[0])}
        ms, enqueue = time_native(plan, args.epochs)
        out.update(native_ms_per_epoch=round(ms, 4), native_enqueue_ms_per_epoch=round(enqueue, 4), native_epochs=args.epochs)
        if not args.native_only:
            plan = nav.NativePlanner(start, end, cfg, q)
            out["reference_ms_per_epoch_sync"] = round(time_reference(q, plan, args.epochs_a, True), 4)
            out["reference_ms_per_epoch_nosync"] = round(time_reference(q, plan, args.epochs_a, False), 4)
            out["reference_epochs"] = args.epochs_a
            out["speedup_vs_sync"] = round(out["reference_ms_per_epoch_sync"] / ms, 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
