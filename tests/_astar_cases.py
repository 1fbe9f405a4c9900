"""The A* cases of tests/golden/astar.npz (the executed reference: tests/golden/make_astar_golden.py) and a numpy restatement of the native search's
contract, shared by the CPU tests (ngp_plan_astar_host) and the GPU tests (k_plan_astar).

The contract (csrc/ngp_plan_path.h): the path is a shortest 6-connected path through the free cells, so it has the length of the
reference's; among equally short paths it is the one that from every cell moves to the first neighbour in the order +x, -x, +y, -y, +z, -z that is one
step closer to the goal.  Restated here as a breadth-first search from the goal followed by that descent."""
import collections
import ctypes
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "astar.npz")
NEIGHBOURS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
OK, START_OCCUPIED, GOAL_OCCUPIED, NO_PATH, TOO_LONG = 0, 1, 2, 3, 4
MAX_CELLS = 27000

_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(GOLD) as z:
            _gold = {k: z[k] for k in z.files}
    return _gold


def names():
    return [str(n) for n in gold()["names"]]


def unique_names():
    return [str(n) for n in gold()["unique"]]


def case(name):
    """(occupied bool [gx,gy,gz], start, goal, the reference's path [n,3] or None where it raised ValueError)"""
    g = gold()
    path = g.get(f"{name}_path")
    if path is None:
        assert str(g[f"{name}_raised"]) == "ValueError"
    return g[f"{name}_occupied"], tuple(int(v) for v in g[f"{name}_start"]), tuple(int(v) for v in g[f"{name}_goal"]), path


def restated(occupied, start, goal):
    """(status, path [n,3] int32 or None) by the contract, in plain Python"""
    occ = np.asarray(occupied) != 0
    start, goal = tuple(start), tuple(goal)
    if occ[start]:
        return START_OCCUPIED, None
    if occ[goal]:
        return GOAL_OCCUPIED, None
    dist = np.full(occ.shape, -1, np.int64)
    dist[goal] = 0
    queue = collections.deque([goal])
    while queue and dist[start] < 0:
        c = queue.popleft()
        for step in NEIGHBOURS:
            n = tuple(a + b for a, b in zip(c, step))
            if all(0 <= v < s for v, s in zip(n, occ.shape)) and not occ[n] and dist[n] < 0:
                dist[n] = dist[c] + 1
                queue.append(n)
    if dist[start] < 0:
        return NO_PATH, None
    path, c = [start], start
    while c != goal:
        for step in NEIGHBOURS:
            n = tuple(a + b for a, b in zip(c, step))
            if all(0 <= v < s for v, s in zip(n, occ.shape)) and dist[n] == dist[c] - 1:
                c = n
                break
        else:
            raise AssertionError("a labelled cell without a neighbour one step closer")
        path.append(c)
    return OK, np.array(path, np.int32).reshape(-1, 3)


def random_cases(count=30, seed=5):
    """seeded random grids with dims drawn from {1..8}^3, 0 - 40 % occupied; start and goal are any two cells (occupied ones included: statuses 1 - 3 occur)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        dims = tuple(int(v) for v in rng.integers(1, 9, 3))
        occ = rng.random(dims) < rng.uniform(0.0, 0.4)
        start = tuple(int(rng.integers(0, d)) for d in dims)
        goal = tuple(int(rng.integers(0, d)) for d in dims)
        if rng.random() < 0.8:
            occ[start] = occ[goal] = False
        out.append((occ, start, goal))
    return out


def free30():
    return np.zeros((30, 30, 30), bool), (0, 0, 0), (29, 29, 29)


def check_path(occupied, start, goal, path):
    """what every returned path holds: starts at the start, ends at the goal, unit steps, free cells only"""
    occ = np.asarray(occupied) != 0
    path = np.asarray(path)
    assert path.ndim == 2 and path.shape[1] == 3 and len(path) >= 1
    assert tuple(path[0]) == tuple(start) and tuple(path[-1]) == tuple(goal)
    assert np.all(np.abs(np.diff(path, axis=0)).sum(axis=1) == 1)
    assert np.all(path >= 0) and np.all(path < np.array(occ.shape))
    assert not occ[path[:, 0], path[:, 1], path[:, 2]].any()


def host_search(occupied, start, goal, cap=None):
    """ngp_plan_astar_host -> (return code, status, n_cells, path [cap,3]); the buffers are pre-filled with -7 so that a test sees what was written"""
    import ngp_hip
    L = ngp_hip.lib()
    occ = np.ascontiguousarray(np.asarray(occupied) != 0, np.uint8)
    dims = (ctypes.c_uint32 * 3)(*occ.shape)
    cap = int(occ.size) if cap is None else int(cap)
    path = np.full((max(cap, 1), 3), -7, np.int32)
    result = np.full(2, -7, np.int32)
    rc = L.raw.ngp_plan_astar_host(occ.ctypes.data, dims, (ctypes.c_int32 * 3)(*start), (ctypes.c_int32 * 3)(*goal), path.ctypes.data, cap,
                                   result.ctypes.data)
    return rc, int(result[0]), int(result[1]), path
