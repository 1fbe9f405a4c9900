"""Record what the host side of libngp_hip.so promises about workspaces: every size function over a grid of shapes, the two offsets
ngp_field_train_live_list hands out, and the return code and message of every entry point that refuses a workspace one byte short before it
touches the device.  Needs no GPU.  `python tools/workspace_sizes.py` writes tests/golden/workspace_sizes.json from the library NGP_HIP_LIB
selects (default: the tree's own build); tests/test_workspace_host.py calls collect() on the built library and compares.  The size functions of the
occupancy-masked run and filter route have a fixture of their own, tests/golden/workspace_sizes_run_occ.json (tests/test_run_occ_host.py), written too."""
import ctypes
import importlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
importlib.import_module("nerf-navigation_amd")
import ngp_hip as H  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 4096, 1 << 22, (1 << 22) + 1]
GRID_H, GRID_C = [8, 16, 64, 128], [1, 2, 3]
LEVELS = [1, 16, 32]
PLAN_R, PLAN_B = [1, 2, 255, 256], [0, 1, 65536, 65537]
MESH_SIDES = [1, 2, 17, 1024, 1025]
STEPS = [1, 16, 1024]
FFMLP_SHAPES = [(32, 16, 64, 2), (16, 16, 64, 3), (64, 16, 64, 4), (32, 16, 128, 2), (48, 32, 32, 5), (16, 16, 16, 2)]   # in, out, hidden, layers
FRAMES = [(1, 64), (2, 64), (2, 100), (8, 4096), (64, 640000 // 64)]                                                         # P, rays per frame

# function -> list of argument tuples
SIZE_CALLS = {
    "ngp_march_rays_train_workspace": [(n,) for n in COUNTS],
    "ngp_march_rays_train_workspace_full": list(itertools.product(COUNTS, STEPS)),
    "ngp_march_rays_workspace": list(itertools.product(GRID_C, GRID_H)),
    "ngp_compact_alive_workspace": [(n,) for n in COUNTS],
    "ngp_density_grid_workspace": list(itertools.product(GRID_C, GRID_H)),
    "ngp_grid_scatter_binned_workspace": list(itertools.product(COUNTS, LEVELS)),
    "ngp_mse_head_workspace": [()],
    "ngp_ffmlp_backward_workspace": FFMLP_SHAPES,
    "ngp_field_density_workspace": [(n,) for n in COUNTS],
    "ngp_field_train_saved_bytes": [(n,) for n in COUNTS],
    "ngp_field_train_workspace": [(n,) for n in COUNTS],
    "ngp_render_frame_workspace": [(n,) for n in COUNTS],
    "ngp_render_frames_workspace": FRAMES,
    "ngp_nav_field_workspace": [()],
    "ngp_nav_run_saved_bytes": list(itertools.product(COUNTS, STEPS)),
    "ngp_marching_cubes_workspace": list(itertools.product(MESH_SIDES, repeat=3)),
    "ngp_plan_workspace": list(itertools.product(PLAN_R, PLAN_B)),
}

# the occupancy-masked run and the filter route over it (a fixture of their own: the one above is compared whole)
RUN_OCC_GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes_run_occ.json")
RUN_OCC_CALLS = {
    "ngp_nav_run_occ_saved_bytes": [(0, 64), (16, 0), (1, 1), (1, 64), (8, 64), (16, 257), (152, 257), (8, 513), (8, 4096), (1024, 512), (8192, 512), (3, 4095)],
    "ngp_filter_occ_workspace": [(1, 16, 64), (3, 16, 64), (64, 16, 64), (1, 64, 64), (3, 64, 64), (1, 1024, 512), (8, 128, 512), (8, 1024, 512), (1, 257, 64),
                                 (0, 16, 64), (65, 16, 64), (1, 16, 4097)],
}

LIVE_BASE = 1 << 20            # dummy workspace address: ngp_field_train_live_list only adds offsets to it


def sizes(L):
    return {name: [list(a) + [int(getattr(L, name)(*a))] for a in calls] for name, calls in SIZE_CALLS.items()}


def run_occ_sizes(L):
    return {name: [list(a) + [int(getattr(L, name)(*a))] for a in calls] for name, calls in RUN_OCC_CALLS.items()}


def live_list(L):
    out = []
    for m in COUNTS:
        lst, cnt = ctypes.c_void_p(0), ctypes.c_void_p(0)
        rc = L.ngp_field_train_live_list(ctypes.c_void_p(LIVE_BASE), m, ctypes.byref(lst), ctypes.byref(cnt))
        out.append([m, rc, (cnt.value or LIVE_BASE) - LIVE_BASE, (lst.value or LIVE_BASE) - LIVE_BASE])     # M, return code, offset of count, of list
    return out


def refusals(L):
    """name -> [return code, ngp_last_error()] of a call whose workspace (or kept buffer) is one byte short.  Every pointer is a dummy: each of
    these entry points refuses before it dereferences anything or asks the runtime for anything."""
    one = ctypes.c_void_p(16)
    offsets = (ctypes.c_int32 * 17)(*[i * 4096 for i in range(17)])
    field = H.ngp_field_t(16, 16, 16, 16, 16, 16, 0.5, 2.0, 1.0)
    nav = H.ngp_nav_field_t(16, ctypes.cast(offsets, ctypes.c_void_p), 16, 16, 16, 16, 16, 16, 16, 0.5, 2.0, 1.0)
    aabb = ctypes.cast((ctypes.c_float * 6)(-2, -2, -2, 2, 2, 2), ctypes.c_void_p)     # read on the host
    cfg = H.ngp_plan_cfg_t()
    cfg.dt = 0.1
    fp, nv, cf = ctypes.byref(field), ctypes.byref(nav), ctypes.byref(cfg)
    out = {}

    def note(name, rc):
        out[name] = [int(rc), L.ngp_last_error().decode()]

    n = L.ngp_compact_alive_workspace(257) - 1
    note("compact_alive", L.ngp_compact_alive(one, 257, one, one, one, n, None))
    note("compact_alive_publish", L.ngp_compact_alive_publish(one, 257, one, one, one, 1, one, n, None))
    n = L.ngp_march_rays_train_workspace(65) - 1
    args = (one, one, one, 1.0, 0.0, 16, 65, 1, 16, 1024, one, one, one, one, one, one, one, 0, one, n, None)
    note("march_rays_train", L.ngp_march_rays_train(*args))
    note("march_rays_train_filled", L.ngp_march_rays_train_filled(*args))
    n = L.ngp_density_grid_workspace(2, 8) - 1
    note("density_grid_update", L.ngp_density_grid_update(one, one, 16, 1.0, 0.95, 10.0, 2, 8, one, one, one, one, n, None))
    note("density_grid_sample_partial", L.ngp_density_grid_sample(one, 2, 8, 2.0, 1, 1, 1, one, one, one, n, None))
    n = L.ngp_grid_scatter_binned_workspace(1025, 2) - 1
    note("grid_scatter_binned", L.ngp_grid_scatter_binned(one, one, one, one, 1025, 2, 1.0, 16, 4096, 0, 0, 0, 1.0, one, n, None))
    note("grid_scatter_binned_listed", L.ngp_grid_scatter_binned_listed(one, one, one, one, 1025, 2, 1.0, 16, 4096, 0, 0, 0, 1.0, one, one, one, n, None))
    note("grid_scatter_binned_phase", L.ngp_grid_scatter_binned_phase(1, one, one, one, one, 1025, 2, 0, 2, 1.0, 16, 4096, 0, 0, 0, 1.0, one, n, None))
    note("field_train_forward", L.ngp_field_train_forward(fp, one, one, 33, one, one, one, L.ngp_field_train_saved_bytes(33) - 1, None))
    note("field_train_backward", L.ngp_field_train_backward(fp, one, one, 33, one, one, one, one, one, one, L.ngp_field_train_workspace(33) - 1, 1, None))
    note("field_density", L.ngp_field_density(fp, one, 33, one, one, L.ngp_field_density_workspace(33) - 1, None))
    n = L.ngp_marching_cubes_workspace(17, 17, 17) - 1
    note("marching_cubes_count", L.ngp_marching_cubes_count(one, 17, 17, 17, 0.5, one, n, one, one, None))
    note("marching_cubes_emit", L.ngp_marching_cubes_emit(one, 17, 17, 17, 0.5, one, n, one, 3, one, 1, None))
    note("nav_field_prepare", L.ngp_nav_field_prepare(nv, one, L.ngp_nav_field_workspace() - 1, None))
    n = L.ngp_nav_run_saved_bytes(3, 8) - 1
    note("nav_run_forward", L.ngp_nav_run_forward(nv, one, one, one, one, one, 3, 8, aabb, None, one, one, one, one, n, None))
    note("nav_run_backward", L.ngp_nav_run_backward(nv, one, one, one, one, one, 3, 8, aabb, None, one, None, None, one, n, one, one, None))
    note("plan_epochs", L.ngp_plan_epochs(nv, one, cf, one, one, one, one, 3, 2, 0, 1, 1, None, None, one, L.ngp_plan_workspace(2, 3) - 1, None))
    # (the register-resident path uses the head of the workspace only: the partial sums, without the 2 bytes per weight and the 256 spare bytes behind)
    n = L.ngp_ffmlp_backward_workspace(32, 16, 64, 2) - 2 * 64 * (32 + 64 + 16) - 256 - 1
    note("ffmlp_backward", L.ngp_ffmlp_backward(one, one, one, one, 128, 32, 16, 64, 2, 0, 6, 0, one, None, one, one, n, None))
    n = L.ngp_ffmlp_backward_workspace(32, 16, 128, 2) - 1
    note("ffmlp_backward_layer_by_layer", L.ngp_ffmlp_backward(one, one, one, one, 128, 32, 16, 128, 2, 0, 6, 0, one, None, one, one, n, None))
    n = L.ngp_mse_head_workspace() - 1
    note("mse_head_forward", L.ngp_mse_head_forward(one, one, 300, None, one, one, one, n, None))
    note("train_head_direct", L.ngp_train_head_direct(one, one, None, 0, 1.0, one, None, 100, one, one, one, one, None, None, 0, one, n, None))
    note("render_frame", L.ngp_render_frame(fp, one, one, 64, 8, one, 0.2, one, 1, 16, 0.0, 64, one, one, one, one, one, one, 255, None))
    return out


def collect():
    L = H.lib()
    return {"sizes": sizes(L), "live_list": live_list(L), "refusals": refusals(L)}


if __name__ == "__main__":
    data = collect()
    with open(GOLDEN, "w") as f:
        json.dump(data, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", GOLDEN, "from", H.LIB_PATH)
    with open(RUN_OCC_GOLDEN, "w") as f:
        json.dump(run_occ_sizes(H.lib()), f, indent=1)
        f.write("\n")
    print("wrote", RUN_OCC_GOLDEN)
