"""GPU: the planner's native A* initialisation (csrc/nav_astar.hip; ngp.nav.NativePlanner.occupancy / find_path / a_star_init).

  * k_plan_occupancy is BIT-IDENTICAL to the unfused native route MaxPool3d(k)(density_fn_native(lattice)) > t: the fused kernel evaluates every lattice
    point with the device functions of k_nav_density_fwd, and a maximum is exact whatever its order.  (The density values themselves are held to the
    pinned float64 oracle by tests/test_gpu_nav_pinned.py; this file is about the fusion.)
  * k_plan_astar equals the host twin ngp_plan_astar_host -- the same functions of csrc/ngp_plan_path.h run cell after cell -- path for path and status
    for status; the twin is held to the executed reference and to a restatement of the contract on the CPU (tests/test_plan_path_host.py,
    tests/test_astar_golden.py).
  * a_star_init composes them as Planner.a_star_init does (nav/quad_plot.py:64-115) and leaves a planner whose epochs run."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

import _astar_cases as AC  # noqa: E402
import _nav_cases as NC  # noqa: E402

BODY = [[-0.05, 0.05], [-0.05, 0.05], [-0.02, 0.02]]
UNIT = ((-1., -1., -1.), (1., 1., 1.))
WIDE = ((-2.5, -2.25, -2.75), (2.5, 2.75, 2.25))                       # reaches outside the field's bound (2): sigma = exp(0) there, like the unfused query


@pytest.fixture(scope="module")
def queries(dev):
    """test_gpu_nav_plan.py's field: NGPField + workload.nav_weights(0), float32"""
    from ngp import nav
    from ngp import workload as W
    from ngp.field import NGPField
    from ngp.render import NGPRenderer
    g = NC.gold()
    model = W.make_model(0)
    sw, cw = W.nav_weights(0)
    field = NGPField(bound=W.BOUND).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(model["embeddings"]))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            layer.weight.copy_(torch.from_numpy(w))
    ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=False).to(dev).eval()
    H, Wd = (int(v) for v in g["mf_HW"])
    return nav.NativeNavQueries(ren, g["mf_intrinsics"], H, Wd, num_steps=int(g["mf_num_steps"]))


def cfg(**kw):
    c = {"T_final": 2., "steps": 20, "lr": 0.001, "epochs_init": 3, "epochs_update": 2, "fade_out_epoch": 0, "fade_out_sharpness": 10, "mass": 1.,
         "I": torch.eye(3), "g": 10., "body": np.array(BODY), "nbins": [3, 3, 2]}
    c.update(kw)
    return c


def state(pos):
    return torch.cat([torch.tensor(pos, dtype=torch.float32), torch.zeros(3), torch.eye(3).reshape(-1), torch.zeros(3)])


def make_planner(queries, start=(0.39, -0.67, 0.2), end=(-0.4, 0.55, 0.16), **kw):
    from ngp import nav
    return nav.NativePlanner(state(start), state(end), cfg(**kw), queries)


# ------------------------------------------------------------------------------------------------------------------------
# 1. occupancy: the fusion is exact
# ------------------------------------------------------------------------------------------------------------------------
_POOLED = {}


def pooled_unfused(queries, dev, side, k, box):
    """MaxPool3d(k) of the unfused native density over the reference's lattice (nav/quad_plot.py:74-80), computed once per case"""
    key = (side, k, box)
    if key not in _POOLED:
        lo, hi = box
        axes = [torch.linspace(lo[a], hi[a], side) for a in range(3)]
        coods = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).to(dev)
        with torch.no_grad():
            sigma = queries.density_fn_native(coods)
            _POOLED[key] = torch.nn.MaxPool3d(kernel_size=k)(sigma[None, None, ...])[0, 0, ...]
    return _POOLED[key]


def thresholds(pooled):
    """midpoints between adjacent sorted pooled values at about the 30 % and 70 % quantiles (as float32 values strictly between their neighbours, so
    that no value sits on the threshold and the grid is neither empty nor full), one above the maximum, one below the minimum"""
    v = np.unique(pooled.cpu().numpy().astype(np.float32))
    assert len(v) >= 4 and np.all(np.isfinite(v))
    out = []
    for quantile in (0.3, 0.7):
        i = int(quantile * (len(v) - 1))
        while i + 1 < len(v):
            mid = np.float32((np.float64(v[i]) + np.float64(v[i + 1])) / 2)
            if v[i] < mid < v[i + 1]:
                break
            i += 1
        else:
            raise AssertionError("no float32 fits between adjacent pooled values")
        out.append(float(mid))
    return out + [float(v[-1]) * 2 + 1, float(v[0]) / 2 - 1]


CASES = [(20, 5, UNIT), (20, 5, WIDE), (12, 3, UNIT), (12, 3, WIDE), (13, 4, UNIT), (13, 4, WIDE),      # 13 / 4: a remainder that MaxPool3d's floor drops
         (6, 1, UNIT), (14, 7, UNIT),                                                                     # kernel^3 = 1 (256 cells per workgroup) and 343 > 256 (two passes per cell)
         (100, 5, UNIT)]                                                                                  # the reference's own sizes, once


@pytest.mark.parametrize("side,k,box", CASES, ids=[f"{s}-{k}-{'unit' if b is UNIT else 'wide'}" for s, k, b in CASES])
def test_occupancy_is_the_unfused_route_bit_for_bit(queries, dev, side, k, box):
    plan = make_planner(queries)
    pooled = pooled_unfused(queries, dev, side, k, box)
    G = side // k
    assert tuple(pooled.shape) == (G, G, G)
    ts = thresholds(pooled)
    for n, t in enumerate(ts):
        occ = plan.occupancy(side=side, kernel_size=k, threshold=t, lo=box[0], hi=box[1])
        assert occ.dtype == torch.uint8 and tuple(occ.shape) == (G, G, G) and occ.device == pooled.device
        want = pooled > t
        assert torch.equal(occ != 0, want), (side, k, t, int((occ != 0).sum()), int(want.sum()))
        assert int(occ.max()) <= 1
        filled = int(want.sum())
        if n < 2:
            assert 0 < filled < G ** 3
        else:
            assert filled == (0 if n == 2 else G ** 3)


def test_occupancy_at_the_references_threshold(queries, dev):
    """the defaults are the reference's: 100^3 lattice over [-1, 1]^3, pool 5, sigma > 0.3"""
    plan = make_planner(queries)
    occ = plan.occupancy()
    assert tuple(occ.shape) == (20, 20, 20)
    assert torch.equal(occ != 0, pooled_unfused(queries, dev, 100, 5, UNIT) > 0.3)


# ------------------------------------------------------------------------------------------------------------------------
# 2. the search kernel against the host twin
# ------------------------------------------------------------------------------------------------------------------------
def device_search(dev, occupied, start, goal, cap=None):
    """ngp_plan_astar -> (status, n_cells, path [cap,3]); buffers pre-filled with -7"""
    import ngp_hip as H
    occ = torch.from_numpy(np.ascontiguousarray(np.asarray(occupied) != 0, np.uint8)).to(dev)
    cap = int(occ.numel()) if cap is None else int(cap)
    path = torch.full((cap, 3), -7, dtype=torch.int32, device=dev)
    result = torch.full((2,), -7, dtype=torch.int32, device=dev)
    H.check(H.lib().ngp_plan_astar(H.ptr(occ), (ctypes.c_uint32 * 3)(*occ.shape), (ctypes.c_int32 * 3)(*start), (ctypes.c_int32 * 3)(*goal), H.ptr(path), cap,
                                   H.ptr(result), H.stream()), "plan_astar")
    status, n = (int(v) for v in result.cpu().tolist())
    return status, n, path.cpu().numpy()


def kernel_equals_twin(dev, occ, start, goal, cap=None):
    rc, status_h, n_h, path_h = AC.host_search(occ, start, goal, cap)
    assert rc == 0
    status, n, path = device_search(dev, occ, start, goal, cap)
    assert (status, n) == (status_h, n_h)
    assert np.array_equal(path, path_h[:len(path)])                   # the cells, and -7 wherever the twin wrote nothing
    if status == AC.OK:
        AC.check_path(occ, start, goal, path[:n])
    return status, n


@pytest.mark.parametrize("name", AC.names())
def test_search_kernel_equals_the_host_twin_on_the_fixture_grids(dev, name):
    occ, start, goal, ref = AC.case(name)
    status, n = kernel_equals_twin(dev, occ, start, goal)
    assert (status, n) == ((AC.OK, len(ref)) if ref is not None else (AC.NO_PATH, 0))


def test_search_kernel_on_the_largest_grid_and_random_ones(dev):
    occ, start, goal = AC.free30()
    assert kernel_equals_twin(dev, occ, start, goal) == (AC.OK, 88)
    for occ, start, goal in AC.random_cases(12, seed=9):
        kernel_equals_twin(dev, occ, start, goal)


def test_search_kernel_statuses(dev):
    free = np.zeros((3, 4, 5), bool)
    assert kernel_equals_twin(dev, free, (0, 0, 0), (2, 3, 4), cap=9) == (AC.TOO_LONG, 10)      # 10 cells do not fit 9 rows: nothing written
    assert kernel_equals_twin(dev, free, (0, 0, 0), (2, 3, 4), cap=10) == (AC.OK, 10)
    occ = free.copy()
    occ[0, 0, 0] = True
    assert kernel_equals_twin(dev, occ, (0, 0, 0), (2, 3, 4)) == (AC.START_OCCUPIED, 0)
    assert kernel_equals_twin(dev, occ, (2, 3, 4), (0, 0, 0)) == (AC.GOAL_OCCUPIED, 0)
    assert kernel_equals_twin(dev, occ, (1, 1, 1), (1, 1, 1)) == (AC.OK, 1)


def test_find_path_raises_a_value_error_per_status(queries, dev):
    plan = make_planner(queries)
    occ = torch.zeros((4, 4, 4), dtype=torch.uint8, device=dev)
    occ[0, 0, 0] = 1
    occ[2] = 1
    with pytest.raises(ValueError, match="start cell .* is occupied"):
        plan.find_path(occ, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="goal cell .* is occupied"):
        plan.find_path(occ, (1, 1, 1), (0, 0, 0))
    with pytest.raises(ValueError, match="Failed to find path"):
        plan.find_path(occ, (1, 1, 1), (3, 3, 3))
    with pytest.raises(ValueError, match="outside the grid"):
        plan.find_path(occ, (1, 1, 1), (4, 3, 3))
    path = plan.find_path(occ > 0, (1, 0, 0), (1, 3, 3))             # a bool grid serves too
    assert path.dtype == torch.int32 and path.is_cuda and tuple(path.shape) == (7, 3)
    assert np.array_equal(path.cpu().numpy(), AC.restated(occ.cpu().numpy(), (1, 0, 0), (1, 3, 3))[1])


# ------------------------------------------------------------------------------------------------------------------------
# 3. a_star_init on the field
# ------------------------------------------------------------------------------------------------------------------------
SIDE, K = 40, 5
G = SIDE // K


def far_apart(occ, at_least=4):
    """two free cells of the grid joined by a path of `at_least` .. 255 cells, and that path by the restated contract: a free cell and the cell of its
    connected region that is farthest from it (flood fill), for the first region that is large enough"""
    import collections
    seen = np.zeros(occ.shape, bool)
    for start in (tuple(int(v) for v in c) for c in np.argwhere(~occ)):
        if seen[start]:
            continue
        seen[start] = True
        queue, dist, last = collections.deque([start]), {start: 1}, start
        while queue:
            c = queue.popleft()
            last = c if dist[c] <= 255 else last
            for step in AC.NEIGHBOURS:
                n = tuple(a + b for a, b in zip(c, step))
                if all(0 <= v < s for v, s in zip(n, occ.shape)) and not occ[n] and not seen[n]:
                    seen[n] = True
                    dist[n] = dist[c] + 1
                    queue.append(n)
        if dist[last] >= at_least:
            status, path = AC.restated(occ, start, last)
            assert status == AC.OK and len(path) == dist[last]
            return start, last, path
    raise AssertionError("no two connected free cells far enough apart in the test scene")


@pytest.fixture(scope="module")
def scene(queries, dev):
    """a threshold at which the 8^3 grid of the field is about 30 % occupied, and two free cells with a path of at least 4 cells between them"""
    t = thresholds(pooled_unfused(queries, dev, SIDE, K, UNIT))[1]                      # above 70 % of the pooled values
    occ = (pooled_unfused(queries, dev, SIDE, K, UNIT) > t).cpu().numpy()
    start, goal, path = far_apart(occ)
    return dict(t=t, occ=occ, start=start, goal=goal, path=path)


def centre(cell):
    return tuple(-1.0 + 2.0 * (c + 0.5) / G for c in cell)


def test_a_star_init_without_noise(queries, dev, scene):
    from ngp import nav
    plan = make_planner(queries, centre(scene["start"]), centre(scene["goal"]))
    straight = plan.states.clone()
    plan._workspace()                                                 # laid out for the 18 rows of the straight line
    path = plan.a_star_init(side=SIDE, kernel_size=K, threshold=scene["t"], noise_std=0)
    assert np.array_equal(path.cpu().numpy(), scene["path"])          # the restated contract on the unfused grid
    assert np.array_equal(plan.occupied.cpu().numpy() != 0, scene["occ"]) and plan.path is path
    n = len(scene["path"])
    want = nav.astar_states(plan.find_path(plan.occupancy(SIDE, K, scene["t"]), scene["start"], scene["goal"]), G, *UNIT, None)
    assert plan.states.dtype == torch.float32 and plan.states.is_cuda and plan.states.is_contiguous()
    assert torch.equal(plan.states, want) and plan.R == n and tuple(plan.states.shape) != tuple(straight.shape)
    assert plan._ws is None                                           # dropped: laid out again for the new R
    losses = plan.learn_init()
    assert tuple(losses.shape) == (3,) and bool(torch.isfinite(losses).all())
    assert plan._ws is not None and plan.R == n and bool(torch.isfinite(plan.states).all())


def test_a_star_init_noise_is_seeded_on_the_host(queries, dev, scene):
    from ngp import nav
    plans = []
    for _ in range(2):
        plan = make_planner(queries, centre(scene["start"]), centre(scene["goal"]))
        plan.a_star_init(side=SIDE, kernel_size=K, threshold=scene["t"], generator=torch.Generator().manual_seed(3))
        plans.append(plan)
    assert torch.equal(plans[0].states, plans[1].states)
    n = plans[0].R
    noise = torch.randn(n, 4, generator=torch.Generator().manual_seed(3)) * 0.001
    assert torch.equal(plans[0].states, nav.astar_states(plans[0].path, G, *UNIT, noise))
    assert not torch.equal(plans[0].states, nav.astar_states(plans[0].path, G, *UNIT, None))


def test_a_star_init_refusals_leave_the_states(queries, dev, scene, monkeypatch):
    plan = make_planner(queries, (1.5, 0.0, 0.0), centre(scene["goal"]))
    before = plan.states.clone()
    launched = []
    monkeypatch.setattr(plan, "occupancy", lambda *a, **k: launched.append(a))
    with pytest.raises(ValueError, match="start state lies in cell .* outside"):
        plan.a_star_init(side=SIDE, kernel_size=K, threshold=scene["t"])
    assert not launched and torch.equal(plan.states, before)
    monkeypatch.undo()
    c = centre(scene["start"])
    plan = make_planner(queries, c, (c[0] + 0.01, c[1], c[2]))       # start and end in one cell: a path of one cell, R = 1
    before = plan.states.clone()
    with pytest.raises(ValueError, match="has 1 cells"):
        plan.a_star_init(side=SIDE, kernel_size=K, threshold=scene["t"], noise_std=0)
    assert torch.equal(plan.states, before) and not hasattr(plan, "path")


def test_stand_alone_start_up_at_the_references_sizes(queries, dev):
    """plan = NativePlanner(...); plan.a_star_init(); plan.learn_init() with no reference object: the 100^3 lattice, pool 5, a threshold at which a path
    exists in this scene"""
    pooled = pooled_unfused(queries, dev, 100, 5, UNIT)
    t = thresholds(pooled)[1]
    occ = (pooled > t).cpu().numpy()
    start, goal, want = far_apart(occ)
    plan = make_planner(queries, tuple(-1.0 + 2.0 * (c + 0.5) / 20 for c in start), tuple(-1.0 + 2.0 * (c + 0.5) / 20 for c in goal))
    path = plan.a_star_init(threshold=t)
    assert np.array_equal(path.cpu().numpy(), want)
    assert bool(torch.isfinite(plan.learn_init()).all())
