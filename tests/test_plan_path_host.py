"""CPU: the planner's path search (csrc/ngp_plan_path.h) through the host export that runs the functions the kernel calls (ngp_plan_astar_host),
against the numpy restatement of its contract (tests/_astar_cases.py), and the argument checks of the two device entry points."""
import ctypes
import os

import numpy as np
import pytest

import _astar_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import ngp_hip
    return ngp_hip, ngp_hip.lib()


def _agrees(occ, start, goal):
    """the host twin against the restatement: status for status, path for path; returns (status, path)"""
    rc, status, n, path = AC.host_search(occ, start, goal)
    assert rc == 0
    want_status, want = AC.restated(occ, start, goal)
    assert status == want_status
    if status != AC.OK:
        assert n == 0 and np.all(path == -7)                         # nothing written but the result
        return status, None
    assert n == len(want) and np.array_equal(path[:n], want)
    assert np.all(path[n:] == -7)
    AC.check_path(occ, start, goal, path[:n])
    return status, path[:n]


def test_entry_points_are_exported_and_declared():
    ngp_hip, L = _lib()
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    for name in ("ngp_plan_occupancy", "ngp_plan_astar", "ngp_plan_astar_host"):
        assert name in ngp_hip.EXPORTS and f"{name}(" in header
        assert hasattr(L.raw, name)


@pytest.mark.parametrize("name", AC.names())
def test_fixture_grids_against_the_restatement(name):
    occ, start, goal, _ = AC.case(name)
    _agrees(occ, start, goal)


def test_random_grids_against_the_restatement():
    seen = set()
    for occ, start, goal in AC.random_cases():
        seen.add(_agrees(occ, start, goal)[0])
    assert {AC.OK, AC.NO_PATH} <= seen                                # the draw covers found and not found


def test_the_largest_grid_all_free():
    occ, start, goal = AC.free30()
    status, path = _agrees(occ, start, goal)
    assert status == AC.OK and len(path) == 3 * 29 + 1
    # the rule on an empty grid: +x until x matches, then +y, then +z
    want = [(x, 0, 0) for x in range(30)] + [(29, y, 0) for y in range(1, 30)] + [(29, 29, z) for z in range(1, 30)]
    assert np.array_equal(path, np.array(want, np.int32))


def test_each_status_on_a_grid_built_for_it():
    occ = np.zeros((3, 4, 5), bool)
    occ[0, 0, 0] = True
    assert AC.host_search(occ, (0, 0, 0), (2, 3, 4))[1:3] == (AC.START_OCCUPIED, 0)
    assert AC.host_search(occ, (2, 3, 4), (0, 0, 0))[1:3] == (AC.GOAL_OCCUPIED, 0)
    both = occ.copy()
    both[2, 3, 4] = True
    assert AC.host_search(both, (0, 0, 0), (2, 3, 4))[1] == AC.START_OCCUPIED        # the start is looked at first, as the reference asserts it first
    wall = np.zeros((3, 4, 5), bool)
    wall[1] = True
    assert AC.host_search(wall, (0, 1, 1), (2, 1, 1))[1:3] == (AC.NO_PATH, 0)
    free = np.zeros((3, 4, 5), bool)
    rc, status, n, path = AC.host_search(free, (0, 0, 0), (2, 3, 4), cap=9)             # the path has 2 + 3 + 4 + 1 = 10 cells
    assert (rc, status, n) == (0, AC.TOO_LONG, 10) and np.all(path == -7)
    rc, status, n, path = AC.host_search(free, (0, 0, 0), (2, 3, 4), cap=10)
    assert (rc, status, n) == (0, AC.OK, 10)
    rc, status, n, path = AC.host_search(occ, (1, 2, 3), (1, 2, 3))                     # start == goal: one cell
    assert (rc, status, n) == (0, AC.OK, 1) and tuple(path[0]) == (1, 2, 3) and np.all(path[1:] == -7)


def _astar_rc(fn, occ, dims, start, goal, path, cap, result, device):
    args = [occ, (ctypes.c_uint32 * 3)(*dims) if dims is not None else None, (ctypes.c_int32 * 3)(*start) if start is not None else None,
            (ctypes.c_int32 * 3)(*goal) if goal is not None else None, path, cap, result]
    return fn(*args, None) if device else fn(*args)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_argument_errors_return_a_code_and_write_nothing(device):
    """every refusal happens before anything is read, written or launched: on the device entry point the pointers are never dereferenced, so host
    arrays serve (and no GPU is needed)"""
    ngp_hip, L = _lib()
    fn = L.raw.ngp_plan_astar if device else L.raw.ngp_plan_astar_host
    occ = np.zeros((4, 4, 4), np.uint8)
    path = np.full((64, 3), -7, np.int32)
    result = np.full(2, -7, np.int32)
    o, p, r = occ.ctypes.data, path.ctypes.data, result.ctypes.data
    good = dict(occ=o, dims=(4, 4, 4), start=(0, 0, 0), goal=(3, 3, 3), path=p, cap=64, result=r, device=device)
    bad = [dict(occ=None), dict(dims=None), dict(start=None), dict(goal=None), dict(path=None), dict(result=None),
           dict(dims=(0, 4, 4)), dict(dims=(4, 0, 4)), dict(dims=(4, 4, 0)), dict(dims=(31, 31, 31)), dict(dims=(27001, 1, 1)), dict(dims=(65536, 65536, 1)),
           dict(start=(4, 0, 0)), dict(start=(0, -1, 0)), dict(goal=(0, 0, 4)), dict(goal=(-1, 3, 3)), dict(cap=0)]
    for change in bad:
        assert _astar_rc(fn, **dict(good, **change)) == -1, change
        assert L.ngp_last_error()
        assert np.all(path == -7) and np.all(result == -7), change
    if not device:
        assert _astar_rc(fn, **good) == 0 and tuple(result) == (AC.OK, 10)


def test_31_cubed_is_refused_and_30_cubed_is_not():
    occ = np.zeros((31, 31, 31), bool)
    rc, status, n, path = AC.host_search(occ, (0, 0, 0), (30, 30, 30))
    assert rc == -1 and (status, n) == (-7, -7)
    ngp_hip, L = _lib()
    assert b"27000" in L.ngp_last_error()
    assert AC.host_search(np.zeros((30, 30, 30), bool), (0, 0, 0), (0, 0, 1))[:3] == (0, AC.OK, 2)


def test_occupancy_argument_errors_need_no_gpu():
    ngp_hip, L = _lib()
    one = ctypes.c_void_p(16)                                         # non-null dummy: validation rejects before any dereference
    offsets = (ctypes.c_int32 * 17)(*range(0, 17 * 8, 8))
    f = ngp_hip.ngp_nav_field_t(16, ctypes.cast(offsets, ctypes.c_void_p), 16, 16, 16, 16, 16, 16, 16, 0.5, 1.0, 1.0)
    fn = L.raw.ngp_plan_occupancy
    args = dict(f=ctypes.byref(f), prep=one, ax=one, ay=one, az=one, side=20, kernel=5, rot=None, thr=0.3, occ=one)

    def rc(**change):
        a = dict(args, **change)
        return fn(a["f"], a["prep"], a["ax"], a["ay"], a["az"], a["side"], a["kernel"], a["rot"], a["thr"], a["occ"], None)
    for change, said in ((dict(f=None), b"null field pointer"), (dict(prep=None), b"null field pointer"), (dict(ax=None), b"null pointer"),
                         (dict(ay=None), b"null pointer"), (dict(az=None), b"null pointer"), (dict(occ=None), b"null pointer"),
                         (dict(kernel=0), b"kernel must be at least 1"), (dict(side=4), b"smaller than kernel"), (dict(side=0), b"smaller than kernel"),
                         (dict(side=2048, kernel=1), b"supported up to 1024")):
        assert rc(**change) == -1, change
        assert said in L.ngp_last_error(), (change, L.ngp_last_error())
