"""Time the multi-start planner (NativePlanner.run_epochs_multi: K trajectories as one sequence of three launches per epoch, csrc/nav_plan.hip) on cuda:0
against the existing single-trajectory route, on tools/time_nav_plan.py's field at simulate.py's sizes (steps 20, body 10 x 10 x 5 = 500 points, 250 epochs: one
replan), in ms per epoch:

  (a) K in {1, 2, 4, 8, 16, 64}: one run_epochs_multi call against K successive run_epochs calls (ngp_plan_epochs, K times);
  (b) K = 1 multi against the single entry point: what the multi entry point itself costs;
  (c) what the multi-start route adds to its epochs: the measurement pass (update = 0) and the selection, in ms per call.

--baseline-lib PATH: a libngp_hip.so built from another commit (the parent's); its ngp_plan_epochs is timed in the same rounds on the same tensors, so that
"the single path as it was" is a measurement and not a number from a document.

(a) and (b) queue their epochs through the C ABI with the cfg struct and the workspace built once, so that both entry points and both builds are timed by the
same code; NativePlanner.run_epochs / run_epochs_multi add one cfg struct (two small host reads) per call.  (c) goes through the Python methods.

Everything runs in one process in alternating rounds (clocks and caches drift over a process' life), wall time between two synchronisations; medians with
quartiles over the rounds.  One JSON line."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
importlib.import_module("nerf-navigation_amd")
import ngp_hip as _hip  # noqa: E402
from ngp import nav  # noqa: E402
from oracle import nav_oracle as NO  # noqa: E402
from time_nav_plan import SIM_END, SIM_START, cfg_for, make_queries  # noqa: E402

KS = [1, 2, 4, 8, 16, 64]
EPOCHS = 250
AMPLITUDE = 0.05


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(values, digits=4):
    q = statistics.quantiles(values, n=4) if len(values) > 1 else [values[0]] * 3
    return {"median": round(statistics.median(values), digits), "quartiles": [round(q[0], digits), round(q[2], digits)]}


def library(path):
    """a build of the library by path, with the planner's entry points prototyped (the multi ones where the build has them)"""
    handle = ctypes.CDLL(os.path.abspath(path))
    for name in ("ngp_plan_workspace", "ngp_plan_epochs", "ngp_plan_multi_workspace", "ngp_plan_epochs_multi"):
        if hasattr(handle, name):
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = _hip._SIGNATURES[name]
    return handle


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def single_call(handle, plan, adam, losses, n):
    """ngp_plan_epochs of `handle` on plan's tensors, cfg struct and workspace built once -> a function queueing n epochs"""
    B = int(plan.robot_body.shape[0])
    ws = _hip.workspace(handle.ngp_plan_workspace(plan.R, B), plan.device)
    st, prep = plan.queries.native.struct()
    c = plan._cfg_struct()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        rc = handle.ngp_plan_epochs(ctypes.byref(st), p(prep), ctypes.byref(c), p(plan.states), p(plan.initial_accel), p(adam), p(plan.robot_body), B, plan.R,
                                    0, n, 1, p(losses), None, p(ws), ws.numel(), stream)
        if rc != 0:
            raise RuntimeError(f"ngp_plan_epochs failed ({rc})")
    return run


def multi_call(handle, plan, b, K, n):
    """ngp_plan_epochs_multi of `handle` on the K-hypothesis buffers b -> a function queueing n epochs"""
    B = int(plan.robot_body.shape[0])
    ws = _hip.workspace(handle.ngp_plan_multi_workspace(K, plan.R, B), plan.device)
    st, prep = plan.queries.native.struct()
    c = plan._cfg_struct()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        rc = handle.ngp_plan_epochs_multi(ctypes.byref(st), p(prep), ctypes.byref(c), K, p(b["states"]), p(b["accel"]), p(b["adam"]), p(plan.robot_body), B,
                                          plan.R, 0, n, 1, p(b["losses"]), None, p(ws), ws.numel(), stream)
        if rc != 0:
            raise RuntimeError(f"ngp_plan_epochs_multi failed ({rc})")
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)           # even: the order of a pair alternates
    ap.add_argument("--epochs", type=int, default=EPOCHS)
    ap.add_argument("--baseline-lib", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    q = make_queries(dev)
    n = args.epochs
    plan = nav.NativePlanner(NO.state18(SIM_START), NO.state18(SIM_END), cfg_for(20), q)
    R, B = plan.R, int(plan.robot_body.shape[0])
    offsets = plan.draw_offsets(max(KS), AMPLITUDE, torch.Generator().manual_seed(0))   # hypothesis 0 is the single route's start
    starts = (plan.states[None] + offsets).contiguous()
    accel0 = plan.initial_accel.clone()
    adam1, losses1 = plan.new_adam_state(), torch.empty(n, device=dev)
    buf = {K: dict(states=torch.empty(K, R, 4, device=dev), accel=torch.empty(K, 2, device=dev), adam=plan.new_adam_state_multi(K),
                   losses=torch.empty(n, K, device=dev), final=torch.empty(1, K, device=dev)) for K in KS}

    this = library(_hip.LIB_PATH)
    this_single = single_call(this, plan, adam1, losses1, n)
    parent = single_call(library(args.baseline_lib), plan, adam1, losses1, n) if args.baseline_lib else None
    multi_run = {K: multi_call(this, plan, buf[K], K, n) for K in KS}

    def single(times=1, run=this_single):
        for k in range(times):
            plan.states.copy_(starts[k]); plan.initial_accel.copy_(accel0); adam1.zero_()
            run()

    def multi(K):
        b = buf[K]
        b["states"].copy_(starts[:K]); b["accel"].copy_(accel0[None].expand(K, 2)); b["adam"].zero_()
        multi_run[K]()

    for K in KS:                                                    # first launches, LDS attribute, workspaces
        multi(K)
    single()
    if parent:
        single(run=parent)
    torch.cuda.synchronize()
    times = {}
    extra = {K: {"pass": [], "select": []} for K in KS}

    def pair(name, times_k, first_this_build):
        """this build's single route and the baseline library's, in the given order: whichever runs second finds the clocks up"""
        order = [(name, this_single)] + ([(f"{name}, baseline library", parent)] if parent else [])
        for key, run in order if first_this_build else reversed(order):
            times.setdefault(key, []).append(wall_ms(lambda: single(times_k, run)) / n)

    for r in range(args.rounds):
        single()                                                    # unrecorded: the round's first measurement does not start from idle clocks
        pair("single", 1, r % 2 == 0)
        for K in KS:
            times.setdefault(f"multi {K}", []).append(wall_ms(lambda: multi(K)) / n)
            pair(f"successive {K}", K, r % 2 == 0)
            b = buf[K]
            scratch = plan.new_adam_state_multi(K)
            extra[K]["pass"].append(wall_ms(lambda: plan.run_epochs_multi(b["states"], b["accel"], n - 1, 1, scratch, update=False, losses=b["final"])))
            extra[K]["select"].append(wall_ms(lambda: plan.select(b["final"][0], b["states"], b["accel"])))
    med = lambda key: statistics.median(times[key])                 # noqa: E731
    base = ", baseline library" if parent else ""
    out = {"case": f"steps 20, R = {R}, B = {B}, {n} epochs, {args.rounds} rounds", "launches_per_epoch": 3, "points_per_hypothesis": plan.S * B,
           "baseline": "ngp_plan_epochs of --baseline-lib" if parent else "ngp_plan_epochs of this build",
           "ms_per_epoch": {k: summary(v) for k, v in times.items()},
           "ms_per_call_beyond_the_epochs": {str(K): {p: summary(v[p]) for p in v} for K, v in extra.items()},
           "ratios": {str(K): {"successive_over_multi": round(med(f"successive {K}{base}") / med(f"multi {K}"), 3),
                               "multi_over_single": round(med(f"multi {K}") / med(f"single{base}"), 3)} for K in KS}}
    if parent:
        out["single_over_baseline_single"] = round(med("single") / med("single, baseline library"), 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
