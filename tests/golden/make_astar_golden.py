"""Golden vectors for the planner's A* initialisation, produced by EXECUTING THE REFERENCE'S OWN PYTHON.

Build container only (needs /root/reference); run as `python -B tests/golden/make_astar_golden.py` from the repository root.
Writes data only: tests/golden/astar.npz.  Running it again gives the same bytes (fixed seeds, fixed archive timestamps).

What executes: `astar` (nav/quad_helpers.py:201-258) on grids built here, and `Planner.a_star_init` (nav/quad_plot.py:64-115) over an analytic density
written here.  Like make_callers_golden.py, the third-party modules the `nav` package imports but these paths never use (cv2, imageio, trimesh,
tensorboardX, mcubes, torch_ema, lpips) are EMPTY placeholder modules; nothing is written under /root/reference (python -B).

astar cases (`names`): per case <name>_occupied (bool [gx,gy,gz]), _start, _goal (cells) and _path ([n,3], start -> goal), or _raised = "ValueError"
when the reference found no path.  `unique` lists the cases whose free cells form a simple chain, so that the shortest path is unique.
Planner.a_star_init cases (`init_names`): the lattice-derived occupied [20,20,20], the start and end states, the cells and path `astar` was called with,
the noise `torch.normal` returned (replaced for the call by a reader of a seeded array, or by zeros) and the resulting states.
"""
import io
import os
import sys
import types
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

import numpy as np  # noqa: E402
import torch  # noqa: E402


def import_reference():
    for name in ("cv2", "trimesh", "imageio", "tensorboardX", "mcubes", "torch_ema", "lpips"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["cv2"].transform = None
    sys.modules["torch_ema"].ExponentialMovingAverage = object
    sys.path.insert(0, REF)
    import nav.quad_helpers as QH
    import nav.quad_plot as QP
    assert QH.__file__.startswith(REF) and QP.__file__.startswith(REF)
    return QH, QP


# ------------------------------------------------------------------------------------------------------------------------
# grids
# ------------------------------------------------------------------------------------------------------------------------
def random_grid(side, fraction, seed, start, goal):
    occ = np.random.default_rng(seed).random((side, side, side)) < fraction
    occ[start] = occ[goal] = False
    return occ


def walls_grid():
    """two walls across x with gaps at opposite corners: the path has to go through both"""
    occ = np.zeros((20, 20, 20), bool)
    occ[6] = True
    occ[6, 2:5, 2:5] = False
    occ[13] = True
    occ[13, 15:18, 14:17] = False
    return occ


def serpentine_layer(nx, ny):
    """free cells of a corridor one cell wide that snakes through an nx x ny layer: the even columns, joined at alternating ends"""
    free = np.zeros((nx, ny), bool)
    free[0::2] = True
    for x in range(1, nx, 2):
        free[x, ny - 1 if (x // 2) % 2 == 0 else 0] = True
    return free


def chain_ends(occ):
    """the two ends of the free cells, after checking that they form one simple chain (every cell has at most two free neighbours, two cells have one)"""
    free = ~occ
    ends = []
    for c in np.argwhere(free):
        deg = 0
        for axis in range(3):
            for step in (1, -1):
                n = c.copy()
                n[axis] += step
                if 0 <= n[axis] < occ.shape[axis] and free[tuple(n)]:
                    deg += 1
        assert 1 <= deg <= 2, (c, deg)
        if deg == 1:
            ends.append(tuple(int(v) for v in c))
    assert len(ends) == 2, ends
    return ends


def serpentine_5():
    occ = np.ones((5, 5, 5), bool)
    layer = serpentine_layer(5, 5)
    for z in (0, 2, 4):
        occ[:, :, z] = ~layer
    occ[4, 4, 1] = False                                               # layer 0 ends at (4, 4), layer 2 is walked back to (0, 0)
    occ[0, 0, 3] = False
    return occ


def serpentine_20():
    occ = np.ones((20, 3, 3), bool)
    occ[:, :, 1] = ~serpentine_layer(20, 3)
    return occ


def astar_cases():
    cases = []                                                         # (name, occupied, start, goal, unique)
    cases.append(("empty4", np.zeros((4, 4, 4), bool), (0, 0, 0), (3, 3, 3), False))
    cases.append(("same_cell", random_grid(4, 0.2, 11, (1, 2, 3), (1, 2, 3)), (1, 2, 3), (1, 2, 3), True))
    cases.append(("walls20", walls_grid(), (1, 10, 10), (18, 9, 10), False))
    cases.append(("random7", random_grid(7, 0.20, 1, (0, 0, 0), (6, 6, 6)), (0, 0, 0), (6, 6, 6), False))
    cases.append(("random20a", random_grid(20, 0.20, 2, (1, 1, 1), (18, 17, 19)), (1, 1, 1), (18, 17, 19), False))
    cases.append(("random20b", random_grid(20, 0.35, 3, (2, 3, 4), (17, 15, 16)), (2, 3, 4), (17, 15, 16), False))
    box = np.zeros((3, 5, 7), bool)
    box[1, 1:, 2] = True
    box[:, 2, 4] = True
    box[0, :4, 5] = True
    cases.append(("box357", box, (0, 0, 0), (2, 4, 6), False))
    for name, occ in (("serpentine5", serpentine_5()), ("serpentine20", serpentine_20())):
        a, b = chain_ends(occ)
        cases.append((name, occ, a, b, True))
    cases.append(("line9", np.zeros((1, 1, 9), bool), (0, 0, 8), (0, 0, 0), True))
    walled = np.zeros((7, 7, 7), bool)
    for axis in range(3):
        for step in (1, -1):
            n = [5, 5, 5]
            n[axis] += step
            walled[tuple(n)] = True
    cases.append(("walled_goal", walled, (1, 1, 1), (5, 5, 5), False))
    return cases


def run_astar(QH):
    out, names, unique = {}, [], []
    for name, occ, start, goal, uniq in astar_cases():
        names.append(name)
        out[f"{name}_occupied"] = occ
        out[f"{name}_start"] = np.array(start, np.int64)
        out[f"{name}_goal"] = np.array(goal, np.int64)
        try:
            path = QH.astar(occ, start, goal)
        except ValueError:
            out[f"{name}_raised"] = np.array("ValueError")
            assert name == "walled_goal", name
            continue
        assert name != "walled_goal"
        out[f"{name}_path"] = np.array(path, np.int64).reshape(-1, 3)
        if uniq:
            unique.append(name)
    out["names"] = np.array(names)
    out["unique"] = np.array(unique)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# Planner.a_star_init over an analytic density
# ------------------------------------------------------------------------------------------------------------------------
SIDE, KERNEL = 100, 5
# The scene is solid (sigma = 1) except for a corridor one coarse cell wide (sigma = 0), the union of three axis-aligned boxes given in coarse cells
# (inclusive): along x, then along y, then along z.  Its free cells form a simple chain from the start's cell to the end's, so the path is unique.
CORRIDOR = (((2, 3, 10), (12, 3, 10)), ((12, 3, 10), (12, 15, 10)), ((12, 15, 4), (12, 15, 10)))
START_POS, END_POS = (-0.75, -0.65, 0.05), (0.25, 0.55, -0.55)        # the centres of cells (2, 3, 10) and (12, 15, 4)


def corridor_density(coods):
    """sigma [..] for points [.., 3]: 0 inside the corridor's boxes, 1 elsewhere.  A box of cells c0 .. c1 spans the lattice points 5 c0 .. 5 c1 + 4 of
    linspace(-1, 1, 100); its faces lie half a lattice step beyond them, so a pooled cell is free exactly when it belongs to the corridor."""
    h = 2.0 / (SIDE - 1)
    free = torch.zeros(coods.shape[:-1], dtype=torch.bool)
    for c0, c1 in CORRIDOR:
        inside = torch.ones(coods.shape[:-1], dtype=torch.bool)
        for a in range(3):
            lo = -1.0 + (KERNEL * c0[a] - 0.5) * h
            hi = -1.0 + (KERNEL * c1[a] + KERNEL - 0.5) * h
            inside &= (coods[..., a] > lo) & (coods[..., a] < hi)
        free |= inside
    return torch.where(free, torch.zeros(()), torch.ones(()))


def planner_cfg():
    return {"T_final": 2., "steps": 20, "lr": 0.001, "epochs_init": 1, "epochs_update": 1, "fade_out_epoch": 0, "fade_out_sharpness": 10,
            "I": torch.eye(3), "g": 10., "mass": 1., "body": np.array([[-0.05, 0.05], [-0.05, 0.05], [-0.02, 0.02]]), "nbins": [3, 3, 2]}


def full_state(pos):
    return torch.cat([torch.tensor(pos, dtype=torch.float32), torch.zeros(3), torch.eye(3).reshape(-1), torch.zeros(3)])


def run_a_star_init(QP):
    out, names = {}, []
    real_normal, real_astar = torch.normal, QP.astar
    for name, seed in (("init_noise", 7), ("init_zero", None)):
        names.append(name)
        seen = {}

        def normal(mean, std, seed=seed, seen=seen):
            shape = tuple(std.shape)
            noise = np.zeros(shape, np.float32) if seed is None else np.random.default_rng(seed).normal(0.0, 0.001, shape).astype(np.float32)
            seen["noise"] = noise
            return torch.from_numpy(noise.copy())

        def astar(occupied, start, goal, seen=seen):
            path = real_astar(occupied, start, goal)
            seen.update(occupied=occupied.numpy().copy(), start=np.array(start, np.int64), goal=np.array(goal, np.int64),
                        path=np.array(path, np.int64).reshape(-1, 3))
            return path

        start, end = full_state(START_POS), full_state(END_POS)
        pl = QP.Planner(start, end, planner_cfg(), corridor_density)
        torch.normal, QP.astar = normal, astar
        try:
            pl.a_star_init()
        finally:
            torch.normal, QP.astar = real_normal, real_astar
        assert seen["occupied"].shape == (20, 20, 20) and seen["occupied"].dtype == np.bool_
        chain_ends(seen["occupied"])
        out.update({f"{name}_start_state": start.numpy(), f"{name}_end_state": end.numpy(), f"{name}_occupied": seen["occupied"],
                    f"{name}_start": seen["start"], f"{name}_goal": seen["goal"], f"{name}_path": seen["path"], f"{name}_noise": seen["noise"],
                    f"{name}_states": pl.states.detach().numpy().copy()})
    out["init_names"] = np.array(names)
    out["init_side_kernel_threshold"] = np.array([SIDE, KERNEL, 0.3])
    return out


def save(path, data):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(data):
            raw = io.BytesIO()
            np.lib.format.write_array(raw, np.asanyarray(data[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, raw.getvalue())


def main():
    cache = os.path.join(REF, "nav", "__pycache__")
    before = sorted(os.listdir(cache)) if os.path.isdir(cache) else None
    QH, QP = import_reference()
    data = run_astar(QH)
    data.update(run_a_star_init(QP))
    path = os.path.join(HERE, "astar.npz")
    save(path, data)
    print(f"astar: {len(data)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")
    assert (sorted(os.listdir(cache)) if os.path.isdir(cache) else None) == before, "bytecode was written into the reference tree"


if __name__ == "__main__":
    main()
