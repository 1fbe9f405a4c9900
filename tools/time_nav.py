"""Time BASELINE config 4 (nav loop pieces, fp32, no autocast) on cuda:0:
   (ii) density + backward on [20,500,3] body points (planner, nav/quad_plot.py:224-250);
   (iii) run() render + backward, 1024 rays x 512 steps (pose filter, nav/estimator_helpers.py:293-327);
   planner_astar_init: the planner's A* initialisation at the reference's sizes (100^3 lattice, pool 5, 20^3 cells; nav/quad_plot.py:64-115).
Prints one line per variant and a final JSON line (`ms_per_step` = the frozen-model filter iteration).
   python tools/time_nav.py [--steps 20] [--warmup 1] [--torch-profile]"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("nerf-navigation_amd")
from ngp import nav  # noqa: E402
from ngp import workload as W  # noqa: E402
from ngp.field import NGPField  # noqa: E402
from ngp.render import NGPRenderer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--torch-profile", action="store_true", help="print torch.profiler's kernel table for the filter iteration")
ap.add_argument("--only", default="", help="comma list of: planner, filter, planner_frozen, filter_frozen, planner_graphed, planner_native, filter_native, planner_native_graphed, astar, planner_astar_init")
args = ap.parse_args()
only = set(filter(None, args.only.split(",")))

dev = torch.device("cuda:0")
torch.manual_seed(0)
field = NGPField(bound=W.BOUND).to(dev)
with torch.no_grad():
    field.encoder.embeddings.uniform_(-0.5, 0.5)
ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=False).to(dev).eval()
rot = torch.tensor(nav.ROT, device=dev)


def timeit(fn, n):
    for _ in range(max(args.warmup, 1)):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


pts = (torch.rand(20, 500, 3, device=dev) * 2 - 1)
o, d = W.get_rays(W.orbit_pose(1), W.intrinsics(32, 32), 32, 32)
o, d = torch.from_numpy(o).to(dev)[None], torch.from_numpy(d).to(dev)[None]
res = {}


def planner():
    p = pts.clone().requires_grad_(True)
    ren.density(p.reshape(-1, 3) @ rot)["sigma"].sum().backward()


def filt():
    ro, rd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    out = ren.render(ro, rd, staged=True, bg_color=1.0, perturb=False, num_steps=512, upsample_steps=0, max_ray_batch=4096)
    out["image"].sum().backward()


def want(name):
    return not only or name in only


if want("planner"):
    res["planner"] = timeit(planner, 2 * args.steps)
    print("(ii) density+backward on 10,000 points, reference structure (trainable model): %.3f ms" % res["planner"])
if want("filter"):
    res["filter"] = timeit(filt, args.steps)
    print("(iii) run() 1024 rays x 512 steps + backward, reference structure: %.3f ms" % res["filter"])

q = nav.NavQueries(ren, W.intrinsics(32, 32), 32, 32)


def planner_frozen():
    p = pts.clone().requires_grad_(True)
    q.density_fn(p).sum().backward()


def filt_frozen():
    ro, rd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    q.render_fn(ro, rd)["image"].sum().backward()


if want("planner_frozen"):
    res["planner_frozen"] = timeit(planner_frozen, 2 * args.steps)
if want("filter_frozen"):
    res["filter_frozen"] = timeit(filt_frozen, args.steps)
    print("frozen model: (ii) %.3f ms   (iii) %.3f ms" % (res.get("planner_frozen", float("nan")), res["filter_frozen"]))
if args.torch_profile:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(3):
            filt_frozen()
        torch.cuda.synchronize()
    print(prof.key_averages().table(sort_by="cuda_time_total", row_limit=14, max_name_column_width=60))
if want("planner_graphed"):
    dens = nav.GraphedDensity(q, n_points=pts.numel() // 3)

    def planner_graphed():
        p = pts.clone().requires_grad_(True)
        dens(p).sum().backward()
    res["planner_graphed"] = timeit(planner_graphed, 10 * args.steps)
    print("frozen model, one graph replay per planner query: (ii) %.3f ms" % res["planner_graphed"])
if hasattr(nav, "NativeNavQueries"):
    nq = nav.NativeNavQueries(ren, W.intrinsics(32, 32), 32, 32)

    def planner_native():
        p = pts.clone().requires_grad_(True)
        nq.density_fn_native(p).sum().backward()

    def filt_native():
        ro, rd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        nq.render_fn(ro, rd)["image"].sum().backward()
    if want("planner_native"):
        res["planner_native"] = timeit(planner_native, 10 * args.steps)
    if want("filter_native"):
        res["filter_native"] = timeit(filt_native, args.steps)
    print("native fused fp32 queries: (ii) %.3f ms   (iii) %.3f ms" % (res.get("planner_native", float("nan")), res.get("filter_native", float("nan"))))
    if want("planner_native_graphed"):
        class _N:
            renderer = nq.renderer
            density_fn = staticmethod(nq.density_fn_native)
        dens_n = nav.GraphedDensity(_N, n_points=pts.numel() // 3)

        def planner_native_graphed():
            p = pts.clone().requires_grad_(True)
            dens_n(p).sum().backward()
        res["planner_native_graphed"] = timeit(planner_native_graphed, 10 * args.steps)
        print("native queries, one graph replay per planner query: (ii) %.3f ms" % res["planner_native_graphed"])
if want("astar"):
    big = torch.rand(1000000, 3, device=dev) * 2 - 1                       # the A* occupancy query: 100^3 lattice, no gradient (nav/quad_plot.py:65-79)
    with torch.no_grad():
        res["astar_torch"] = timeit(lambda: q.density_fn(big), args.steps)
        if hasattr(nav, "NativeNavQueries"):
            res["astar_native"] = timeit(lambda: nq.density_fn(big), args.steps)
    print("A* query, 10^6 points, no gradient: op chain %.3f ms, fused %.3f ms" % (res["astar_torch"], res.get("astar_native", float("nan"))))
if want("planner_astar_init") and hasattr(nav, "NativeNavQueries"):
    import ctypes
    import numpy as np
    import ngp_hip
    side, k, G = 100, 5, 20
    lin = torch.linspace(-1, 1, side)
    coods = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), dim=-1).to(dev)
    pool = torch.nn.MaxPool3d(kernel_size=k)
    cfg = {"T_final": 2., "steps": 20, "lr": 0.001, "epochs_init": 1, "epochs_update": 1, "fade_out_epoch": 0, "fade_out_sharpness": 10, "mass": 1.,
           "I": torch.eye(3), "g": 10., "body": np.array([[-0.05, 0.05], [-0.05, 0.05], [-0.02, 0.02]]), "nbins": [10, 10, 5]}
    state = lambda cell: torch.cat([torch.tensor([-1 + 2 * (c + 0.5) / G for c in cell]), torch.zeros(3), torch.eye(3).reshape(-1), torch.zeros(3)])  # noqa: E731
    with torch.no_grad():
        pooled = pool(nq.density_fn_native(coods)[None, None])[0, 0]
        thr = float(torch.quantile(pooled.flatten(), 0.7))                  # this field is random: a threshold that leaves 70 % of the cells free
        plan = nav.NativePlanner(state((0, 0, 0)), state((G - 1,) * 3), cfg, nq)
        occ = plan.occupancy(side, k, thr)
        assert torch.equal(occ != 0, pooled > thr)
    spread = {}

    def rounds(legs, reps=5):
        """the legs in turn, `reps` times over: res gets each leg's median, `spread` its smallest and largest round"""
        times = {name: [] for name in legs}
        for _ in range(reps):
            for name, fn in legs.items():
                times[name].append(timeit(fn, args.steps))
        for name, ts in times.items():
            res[name], spread[name] = sorted(ts)[len(ts) // 2], (min(ts), max(ts))
    with torch.no_grad():
        rounds({"astar_init_occupancy_unfused": lambda: pool(nq.density_fn_native(coods)[None, None])[0, 0] > thr,
                "astar_init_occupancy_fused": lambda: plan.occupancy(side, k, thr)})
    # two free cells with a path between them: the first free cell, and the last one the host twin reaches from it
    occ_h = np.ascontiguousarray(occ.cpu().numpy())
    free = [tuple(int(v) for v in c) for c in np.argwhere(occ_h == 0)]
    dims, cap = (ctypes.c_uint32 * 3)(G, G, G), G ** 3
    path_h, result_h = np.zeros((cap, 3), np.int32), np.zeros(2, np.int32)
    L = ngp_hip.lib()

    def host_search(a, b):
        L.raw.ngp_plan_astar_host(occ_h.ctypes.data, dims, (ctypes.c_int32 * 3)(*a), (ctypes.c_int32 * 3)(*b), path_h.ctypes.data, cap, result_h.ctypes.data)
        return int(result_h[0]), int(result_h[1])

    def joined(a, b):
        status, n = host_search(a, b)
        return status == 0 and 2 <= n <= 255
    a = free[0]
    b = next(c for c in reversed(free) if joined(a, c))
    n_cells = host_search(a, b)[1]
    path_d = torch.empty((cap, 3), dtype=torch.int32, device=dev)
    result_d = torch.empty(2, dtype=torch.int32, device=dev)
    rounds({"astar_init_search_host": lambda: host_search(a, b),
            "astar_init_search_kernel": lambda: ngp_hip.check(L.ngp_plan_astar(ngp_hip.ptr(occ), dims, (ctypes.c_int32 * 3)(*a), (ctypes.c_int32 * 3)(*b),
                                                                               ngp_hip.ptr(path_d), cap, ngp_hip.ptr(result_d), ngp_hip.stream()))})
    assert result_d.cpu().tolist() == [0, n_cells] and np.array_equal(path_d[:n_cells].cpu().numpy(), path_h[:n_cells])
    plan = nav.NativePlanner(state(a), state(b), cfg, nq)
    rounds({"astar_init_whole": lambda: plan.a_star_init(side, k, thr)})
    assert plan.R == n_cells
    print("planner A* initialisation, 100^3 lattice / pool 5 / 20^3 cells, path of %d cells: occupancy fused %.3f ms (unfused native route %.3f ms), "
          "search kernel %.3f ms (host twin %.3f ms), a_star_init with its host read %.3f ms"
          % (n_cells, res["astar_init_occupancy_fused"], res["astar_init_occupancy_unfused"], res["astar_init_search_kernel"], res["astar_init_search_host"],
             res["astar_init_whole"]))
    print("  medians of 5 alternating rounds of %d calls; smallest - largest round: " % args.steps
          + ", ".join("%s %.3f - %.3f" % (name[len("astar_init_"):], lo, hi) for name, (lo, hi) in spread.items()))
main = res.get("filter_native", res.get("filter_frozen", float("nan")))
print(json.dumps({"metric": "nav-loop query times (BASELINE config 4), ms", "ms_per_step": main, "steps": args.steps, **{k: round(v, 4) for k, v in res.items()}}))
