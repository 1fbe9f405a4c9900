"""Time one MPC step of the closed navigation loop (ngp.nav.simulate) on cuda:0 at simulate.py's sizes -- an 800 x 800 sensor, 1,024 rays x 512 steps and
300 iterations in the filter, 250 epochs per replan (steps 20, body 10 x 10 x 5) -- on bench.py's nav field (NGPField + workload.nav_weights(0), float32;
the sensor marches the S-ring occupancy grid, density_thresh 10), phase by phase, in ms:

  agent_step_rays    ngp_agent_step + ngp_agent_rays (two launches)
  observation_frame  NGPRenderer.render_fused over the agent's rays: the one-launch frame (csrc/nav_frame.hip)
  observation_chunks NativeNavQueries.render_fn over the same rays in max_ray_batch chunks: the image the filter predicts (157 launches)
  sensor             ngp_agent_sensor over the 640,000 pixels
  agent_step_frame / agent_step_chunks   NativeAgent.step as a whole, both routes
  filter_step        NativePoseFilter.estimate_state(target, action, features="native"): regions, draw, propagate, loop, Hessian, covariance
  replan             NativePlanner.update_state + learn_update

Without --phase this is a driver: every phase group runs in a child process of its own under `timeout -k 10 <limit>`, one after the other, and the driver
stops at the first child that does not end with status 0.  In a child: every shape is warmed up first; a measurement is wall time between two device
synchronisations around REPEAT back-to-back calls; median and quartiles over the rounds are reported.  One JSON line per group, one summary line."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
importlib.import_module("nerf-navigation_amd")

SIDE, RAYS, STEPS, ITERS, EPOCHS = 800, 1024, 512, 300, 250
GROUPS = ("agent", "filter", "replan")
AGENT = {"dt": 0.1, "mass": 1.0, "g": 10.0}
ACTION = [10.1, 0.01, -0.02, 0.015]
NOISE_STD = [2e-2, 2e-2, 2e-2, 1e-2, 1e-2, 1e-2, 2e-2, 2e-2, 2e-2, 1e-2, 1e-2, 1e-2]           # simulate.py:264


def wall(fn, repeat=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeat):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / repeat, out


def quartiles(v):
    q = statistics.quantiles(v, n=4) if len(v) > 1 else [v[0]] * 3
    return {"median": round(statistics.median(v), 4), "q1": round(q[0], 4), "q3": round(q[2], 4)}


def scene(dev, side, queries_hold_the_grid=False):
    """(queries over the map, sensor renderer with the occupancy grid loaded, the true state).  queries_hold_the_grid: the queries' renderer is the
    sensor's (what NativePoseFilter(sampling="occupied") needs); the dense routes never look at the grid"""
    from ngp import nav
    from ngp import workload as W
    from ngp.field import NGPField
    from ngp.render import NGPRenderer
    from time_filter import TRUE_STATE
    model = W.make_model(0)
    sw, cw = W.nav_weights(0)
    field = NGPField(bound=W.BOUND).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(model["embeddings"]))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            layer.weight.copy_(torch.from_numpy(w))
    ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=False).to(dev).eval()
    q = nav.NativeNavQueries(ren, W.intrinsics(side, side), side, side, num_steps=STEPS)
    sensor = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
    sensor.load_density_grid(W.density_grid())
    if queries_hold_the_grid:
        q = nav.NativeNavQueries(sensor, W.intrinsics(side, side), side, side, num_steps=STEPS)
    return q, sensor, torch.tensor(TRUE_STATE, device=dev)


def group_agent(args, dev):
    from ngp import nav
    q, sensor, x0 = scene(dev, args.side)
    cfg = dict(AGENT, I=torch.eye(3), x0=x0)
    frame, chunks = nav.NativeAgent(cfg, q, sensor), nav.NativeAgent(cfg, q)
    action = torch.tensor(ACTION, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    noise = torch.normal(torch.zeros(12, device=dev), torch.tensor(NOISE_STD, device=dev), generator=gen)
    scratch = torch.empty(12, device=dev)
    poses = torch.empty(2, 4, 4, device=dev)
    import ctypes
    import ngp_hip as H

    def step_rays():
        H.check(H.lib().ngp_agent_step(ctypes.byref(frame._dyn), H.ptr(x0), H.ptr(action), H.ptr(noise), H.ptr(scratch), H.ptr(poses[0]), H.ptr(poses[1]),
                                       H.stream()), "agent_step")
        return frame.rays(scratch)

    def whole(agent):
        agent.x = x0                                         # the same step every time: the camera stays inside the scene
        return agent.step(action, noise)

    rays_o, rays_d = step_rays()
    image = frame.render(rays_o, rays_d)
    d_routes = float((image - chunks.render(rays_o, rays_d)).abs().max())
    parts = {"agent_step_rays": (step_rays, 50), "observation_frame": (lambda: frame.render(rays_o, rays_d), 10),
             "observation_chunks": (lambda: chunks.render(rays_o, rays_d), 2), "sensor": (lambda: frame.sense(image), 50),
             "agent_step_frame": (lambda: whole(frame), 10), "agent_step_chunks": (lambda: whole(chunks), 2)}
    for fn, _ in parts.values():                             # warm-up: every shape once more
        fn()
    times = {k: [] for k in parts}
    for _ in range(args.rounds):
        for k, (fn, repeat) in parts.items():
            times[k].append(wall(fn, repeat)[0])
    png = frame.sense(image)[0]
    return {"group": "agent", "case": f"{args.side} x {args.side} sensor, {STEPS} steps per ray on the chunked route, {args.rounds} rounds",
            "ms": {k: quartiles(v) for k, v in times.items()}, "levels_in_the_observation": int(torch.unique(png).numel()),
            "frame_vs_chunks_max_abs_difference": d_routes}


def group_filter(args, dev):
    from ngp import nav
    from time_filter import START_OFFSET
    q, sensor, x0 = scene(dev, args.side, queries_hold_the_grid=args.filter_sampling == "occupied")
    cfg = dict(AGENT, I=torch.eye(3), x0=x0)
    agent = nav.NativeAgent(cfg, q, sensor)
    action = torch.tensor(ACTION, device=dev)
    agent.step(action)
    target = agent.target
    start = x0 + torch.tensor(START_OFFSET, device=dev)
    sig0, Q = 0.1 * torch.eye(12, device=dev), 0.01 * torch.eye(12, device=dev)
    qf, steps, kw = q, f"{STEPS} steps", {}
    if args.filter_sampling == "resampled":                  # the filter's own queries: num_steps coarse samples, then upsample_steps more; the sensor keeps q
        qf = nav.NativeNavQueries(q.renderer, q.intrinsics, q.H, q.W, num_steps=args.filter_num_steps)
        steps, kw = f"{args.filter_num_steps} + {args.filter_upsample_steps} steps", {"upsample_steps": args.filter_upsample_steps}
    filt = nav.NativePoseFilter({"batch_size": RAYS, "lrate": 1e-3, "N_iter": args.iters, "sig0": sig0, "Q": Q}, qf, start.clone(), cfg,
                                sampling=args.filter_sampling, **kw)

    # the front (keypoints, dilation, pixel list) is timed on the observation as it is.  The loop needs batch_size distinct pixels: where this synthetic
    # scene gives the detector fewer, the batches are drawn (natively, on the device) from every pixel of the image instead, and the output says so
    found = int(filt.interest_regions(target).shape[0])
    native_front = found >= RAYS
    rows, cols = torch.meshgrid(torch.arange(args.side, device=dev), torch.arange(args.side, device=dev), indexing="ij")
    every_pixel = torch.stack([rows.reshape(-1), cols.reshape(-1)], -1).to(torch.int32).contiguous()

    def step():
        filt.xt, filt.sig, filt.iteration = start.clone(), sig0.clone(), 0
        if native_front:
            return filt.estimate_state(target, action, features="native", seed=7)
        regions = filt.interest_regions(target)              # still paid: the loop looks for them every step
        return filt.estimate_state(target, action, batches=filt.draw_batches_native(every_pixel if regions.shape[0] < RAYS else regions, args.iters, 7))

    step()
    times = {"filter_step": [], "interest_regions": []}
    for _ in range(args.rounds):
        times["filter_step"].append(wall(step)[0])
        times["interest_regions"].append(wall(lambda: filt.interest_regions(target))[0])
    return {"group": "filter", "case": f"{RAYS} rays x {steps}, {args.iters} iterations, {args.side} x {args.side} target, {args.rounds} rounds, "
                                       f"{args.filter_sampling} sampling",
            "ms": {k: quartiles(v) for k, v in times.items()}, "interest_pixels": found,
            "batches_drawn_from": "the interest regions (features='native')" if native_front else "every pixel (fewer interest pixels than rays per batch)",
            "loop_ran": bool(len(filt.losses))}


def group_replan(args, dev):
    from ngp import nav
    from oracle import nav_oracle as NO
    from time_nav_plan import SIM_END, SIM_START, cfg_for
    q, _, _ = scene(dev, 20)
    cfg = dict(cfg_for(20), epochs_init=50, epochs_update=args.epochs)
    plan = nav.NativePlanner(NO.state18(SIM_START), NO.state18(SIM_END), cfg, q)
    plan.learn_init()                                        # from the straight line between start and end (tools/time_nav_plan.py): 18 states, as steps = 20 gives
    states0, accel0, start0 = plan.states.clone(), plan.initial_accel.clone(), plan.start_state.clone()
    measured = plan.get_full_states()[1].clone()

    def replan():
        plan.states, plan.initial_accel, plan.start_state = states0.clone(), accel0.clone(), start0
        action = plan.get_next_action().clone()
        plan.update_state(measured)
        plan.learn_update(0)
        return action

    replan()
    times = {"replan": [wall(replan)[0] for _ in range(args.rounds)]}
    return {"group": "replan", "case": f"{args.epochs} epochs, R = {plan.R} states after update_state, {int(plan.robot_body.shape[0])} body points, {args.rounds} rounds",
            "ms": {k: quartiles(v) for k, v in times.items()}, "ms_per_epoch": round(statistics.median(times["replan"]) / max(args.epochs, 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", choices=GROUPS, help="run one group in this process (what the driver starts)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--side", type=int, default=SIDE)
    ap.add_argument("--iters", type=int, default=ITERS)
    ap.add_argument("--epochs", type=int, default=EPOCHS)
    ap.add_argument("--limit", type=int, default=300, help="seconds a group may take")
    ap.add_argument("--filter-sampling", choices=("dense", "occupied", "resampled"), default="dense", help="NativePoseFilter's sampling in the filter group")
    ap.add_argument("--filter-num-steps", type=int, default=128, help="coarse samples per ray of --filter-sampling resampled")
    ap.add_argument("--filter-upsample-steps", type=int, default=128, help="importance samples per ray of --filter-sampling resampled")
    args = ap.parse_args()
    if args.phase:
        dev = torch.device("cuda:0")
        out = {"agent": group_agent, "filter": group_filter, "replan": group_replan}[args.phase](args, dev)
        print(json.dumps(out), flush=True)
        return 0
    summary = {}
    for group in GROUPS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--phase", group, "--rounds", str(args.rounds), "--side",
               str(args.side), "--iters", str(args.iters), "--epochs", str(args.epochs), "--filter-sampling", args.filter_sampling,
               "--filter-num-steps", str(args.filter_num_steps), "--filter-upsample-steps", str(args.filter_upsample_steps)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:
            print(json.dumps({"group": group, "status": done.returncode, "stopped": "no further group is started"}), flush=True)
            return done.returncode or 1
        line = [l for l in done.stdout.splitlines() if l.startswith("{")][-1]
        summary.update({k: v["median"] for k, v in json.loads(line)["ms"].items()})
    step = summary["agent_step_frame"] + summary["filter_step"] + summary["replan"]
    print(json.dumps({"metric": "one MPC step of the closed loop, ms (medians)", **summary, "mpc_step_frame_route_sum": round(step, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
