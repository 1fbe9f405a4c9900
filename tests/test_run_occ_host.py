"""CPU: the occupancy-masked run and filter route (include/ngp_hip.h: ngp_nav_run_occ_*, ngp_filter_*_occ; DESIGN.md 3.5 "Occupancy-masked pose filter").

  * the reference tests/test_gpu_run_occ.py judges against is a fair yardstick for every case and bitfield used there: the pinned float64 run, the
    float32 run and the numpy restatement of the kernel's samples see the same mask; left_out leaves out rows with an exactly zero reference gradient
    (the GPU test asks for exact zeros there) and at most 2 % of the others;
  * the numpy cell rule against the oracle's C march: every sample the march emits lies in a cell whose bit the rule finds set;
  * the new size functions against tests/golden/workspace_sizes_run_occ.json;
  * every refusal, none of which touches a device."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

importlib.import_module("nerf-navigation_amd")
import ngp_hip  # noqa: E402

import _nav_pinned_cases as C  # noqa: E402
import _run_occ_cases as RO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -3
GPU_CASES = ("tiny_1", "tiny_2", "tiny_3", "chunk_255", "chunk_256", "contrast", "long_513", "bound_1", "scale_2")
NEW = ("ngp_nav_run_occ_saved_bytes", "ngp_nav_run_occ_forward", "ngp_nav_run_occ_backward", "ngp_filter_occ_workspace", "ngp_filter_iterations_occ",
       "ngp_filter_hessian_occ")


def test_symbols_are_declared_exported_and_prototyped():
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    for name in NEW:
        assert name in ngp_hip.EXPORTS and f"{name}(" in header
        assert getattr(ngp_hip.lib().raw, name).argtypes == ngp_hip._SIGNATURES[name][1]
    sig = ngp_hip._SIGNATURES
    assert len(sig["ngp_nav_run_occ_forward"][1]) == len(sig["ngp_nav_run_forward"][1]) + 2            # the grid and counts
    assert len(sig["ngp_nav_run_occ_backward"][1]) == len(sig["ngp_nav_run_backward"][1]) + 1          # the grid
    assert len(sig["ngp_filter_iterations_occ"][1]) == len(sig["ngp_filter_iterations_multi"][1]) + 1
    assert len(sig["ngp_filter_hessian_occ"][1]) == len(sig["ngp_filter_hessian"][1]) + 1
    assert ctypes.sizeof(ngp_hip.ngp_occ_grid_t) == 16 and "} ngp_occ_grid_t;" in header


# ------------------------------------------------------------------------------------------------------------------------
# the reference is a fair yardstick
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", RO.BITFIELDS)
@pytest.mark.parametrize("name", GPU_CASES + ("base",))
def test_the_masked_reference_is_a_fair_yardstick(name, bf):
    r = RO.occ_reference(name, bf)
    case, ref, f32 = r["case"], r["ref"], r["f32"]
    # one mask: the pinned float64 run, the float32 run and the restatement of the kernel's own samples
    restated = RO.case_mask(case, r["bits"])
    assert np.array_equal(ref["occupied"], f32["occupied"]) and np.array_equal(ref["occupied"], restated)
    assert np.array_equal(r["counts"], restated.sum(axis=1))
    if bf == "ones":
        assert restated.all()
        dense = C.run_reference(name)["ref"]                        # the all-ones mask changes nothing: the dense reference, bit for bit
        for k in ("image", "weights_sum", "grad_o", "grad_d"):
            assert np.array_equal(ref[k], dense[k]), k
    else:
        assert not restated.all() and (restated.any() or case["T"] <= 3)
    # a masked sample carries no weight
    assert np.all(ref["weights"][~ref["occupied"]] == 0)
    # rows whose reference gradient is exactly zero are not left out: the kernel must give exact zeros there (a relative error has no meaning on them);
    # of the rest left_out leaves out at most 2 %
    hit, left = r["hit"], r["left"]
    zero = r["zero"]["grad_o"] & r["zero"]["grad_d"]
    assert np.array_equal(r["zero"]["grad_o"][hit], r["zero"]["grad_d"][hit])          # a ray's two gradients vanish together
    others = hit & ~zero
    print(f"{name} {bf}: {int((zero & hit).sum())} of {int(hit.sum())} rays with a zero gradient, {int((left & others).sum())} other rows left out; "
          f"float32 oracle: image {np.nanmax(r['e32']['image']):.2e}, grad_o {np.nanmax(r['e32']['grad_o'][r['judged']], initial=0):.2e}")
    assert (left & others).sum() <= 0.02 * others.sum()
    assert np.nanmax(r["e32"]["image"]) <= 1e-6                                       # what every case has to meet to serve as a yardstick


def test_straddle_cases_straddle_the_chunk_width():
    for name, bf in sorted(RO.STRADDLE):
        assert C.RUN_CASES[name]["T"] > RO.CHUNK and bf == "rand50"
        rows = RO.straddle_rays(name)
        for count in (RO.CHUNK - 1, RO.CHUNK, RO.CHUNK + 1):
            assert len(rows[count]) >= 1, (name, count)
        changed = np.count_nonzero(RO.straddle_bits(name) != RO.bitfield("rand50", C.RUN_CASES[name]["bound"]))
        assert 0 < changed < 300                                                      # still rand50 but for three rays' cells
    assert RO.carry_floor(64) == 0 and RO.carry_floor(65) == 2.0 ** -24 * 7 ** 0.5 and RO.carry_floor(4096) == 2.0 ** -24 * (7 * 63) ** 0.5


# ------------------------------------------------------------------------------------------------------------------------
# the cell rule against the oracle's march
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [1.0, 2.0, 4.0])
def test_cell_rule_against_the_oracle_march(oracle, bound):
    """The C march emits a sample only where the cell of its position, by its own arithmetic, has its bit set.  With dt_gamma = 0 and 1,024 steps the
    step (2 sqrt(3) / 1024, 0.054 cells of a 32-grid) has a negative frexp exponent, so the step's cascade is 0 and the march's level is the position's
    alone -- the rule of the masked run.  So every emitted sample must be occupied by the numpy rule under the marched bitfield, and empty under the
    bitfield's complement, through which the march walks the other half of the cells."""
    cascade, H = RO.cascades(bound), RO.H_GRID
    o, d, miss = C.rays(bound)
    aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
    nears, fars = oracle.near_far_from_aabb(o, d, aabb, 0.05)
    N = o.shape[0]
    alive = np.arange(N, dtype=np.int32)
    bits = RO.bitfield("rand50", bound)
    seen_levels = set()
    for marched, expect in ((bits, True), (~bits, False)):
        x, _, deltas = oracle.march_rays(N, 64, alive, nears.copy(), o, d, bound, marched, cascade, H, nears, fars, 128, False, 0.0, 1024)
        x, deltas = x.reshape(-1, 3), deltas.reshape(-1, 2)
        emitted = deltas[:, 0] > 0
        assert emitted.sum() > 1000
        got = RO.occupied(x[emitted], bits, bound, cascade, H)
        assert (got == expect).all(), (bound, expect, int((got != expect).sum()))
        seen_levels |= set(RO.cell_bits(x[emitted], bound, cascade, H)[1].tolist())
    assert seen_levels == set(range(cascade))                                         # every cascade was exercised


def test_cell_rule_on_chosen_positions():
    f = np.float32
    H, bound, cascade = 32, 2.0, 2
    x = np.array([[0, 0, 0], [-1, -1, -1], [1, 1, 1], [0.999, 0, 0], [1.0, 0, 0], [2, 2, 2], [-2, 0.3, 0], [np.nextafter(f(1), f(0)), 0, 0]], f)
    bit, level, n = RO.cell_bits(x, bound, cascade, H)
    # frexp: |x| < 1 -> exponent <= 0 -> level 0; 1 <= |x| < 2 -> exponent 1 -> level 1; 2 -> exponent 2, clamped to C - 1 = 1
    assert level.tolist() == [0, 1, 1, 0, 1, 1, 1, 0]
    assert n[0].tolist() == [16, 16, 16] and n[1].tolist() == [8, 8, 8]               # -1 at level 1 (half-width 2): (-0.5 + 1) * 16
    assert n[2].tolist() == [24, 24, 24] and n[5].tolist() == [31, 31, 31] and n[6].tolist() == [0, 18, 16]
    assert n[3].tolist() == [31, 16, 16] and n[4].tolist() == [24, 16, 16]
    assert bit[0] == int(W_morton(16, 16, 16)) and bit[2] == H ** 3 + int(W_morton(24, 24, 24))


def W_morton(x, y, z):
    from ngp import workload as W
    return W.morton3(np.array([x], np.uint32), np.array([y], np.uint32), np.array([z], np.uint32))[0]


# ------------------------------------------------------------------------------------------------------------------------
# sizes
# ------------------------------------------------------------------------------------------------------------------------
def test_size_functions_against_the_fixture():
    L = ngp_hip.lib()
    fixture = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_sizes_run_occ.json")))
    assert len(fixture["ngp_nav_run_occ_saved_bytes"]) >= 8 and len(fixture["ngp_filter_occ_workspace"]) >= 8
    for N, T, want in fixture["ngp_nav_run_occ_saved_bytes"]:
        assert L.ngp_nav_run_occ_saved_bytes(N, T) == want, (N, T)
        if N and T:
            # the dense record (every sample occupied), the counts and the lists, each piece after the first on a 256-byte boundary
            dense = L.ngp_nav_run_saved_bytes(N, T)
            assert dense == 108 * N * T
            a = lambda v: (v + 255) // 256 * 256                                      # noqa: E731
            assert want == a(a(a(dense) + 4 * N) + 2 * N * T)
    for K, B, T, want in fixture["ngp_filter_occ_workspace"]:
        assert L.ngp_filter_occ_workspace(K, B, T) == want, (K, B, T)
        if want:
            extra = L.ngp_nav_run_occ_saved_bytes(K * B, T) - L.ngp_nav_run_saved_bytes(K * B, T)
            assert abs(want - L.ngp_filter_multi_workspace(K, B, T) - extra) < 512    # the same pieces around a longer record
    assert L.ngp_nav_run_occ_saved_bytes(0, 64) == 0 and L.ngp_nav_run_occ_saved_bytes(16, 0) == 0
    for K, B, T in ((0, 16, 64), (65, 16, 64), (2, (1 << 19) + 1, 64), (1, 0, 64), (1, 16, 0), (1, 16, 4097)):
        assert L.ngp_filter_occ_workspace(K, B, T) == 0, (K, B, T)


# ------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------
def _fake(n=16):
    return ctypes.c_void_p(n)                                                         # never dereferenced: every call below is refused first


_KEEP = []


def _field():
    """a field nav_fill accepts (the default field's level table on the host); its device pointers are fakes"""
    from ngp.field import NGPField
    enc = NGPField(bound=2.0).encoder
    offsets = (ctypes.c_int32 * 17)(*[int(v) for v in enc.offsets.tolist()])
    _KEEP.append(offsets)
    f = 16
    return ngp_hip.ngp_nav_field_t(f, ctypes.cast(offsets, ctypes.c_void_p), f, f, f, f, f, 16, enc.base_resolution, float(np.log2(enc.per_level_scale)), 2.0, 1.0)


def _grid(C=2, H=32, bits=True):
    return ngp_hip.ngp_occ_grid_t(16 if bits else None, C, H)


def _run(L, grid="default", T=64, N=8, saved_bytes=None, backward=False, field=None):
    f = _fake()
    fld = _field() if field is None else field
    g = _grid() if grid == "default" else grid
    gp = ctypes.byref(g) if g is not None else None
    aabb, bg = (ctypes.c_float * 6)(-2, -2, -2, 2, 2, 2), (ctypes.c_float * 3)(1, 1, 1)
    need = L.ngp_nav_run_occ_saved_bytes(N, T) if saved_bytes is None else saved_bytes
    if backward:
        return L.ngp_nav_run_occ_backward(ctypes.byref(fld), f, gp, f, f, f, f, N, T, aabb, bg, f, None, None, f, need, f, f, None)
    return L.ngp_nav_run_occ_forward(ctypes.byref(fld), f, gp, f, f, f, f, N, T, aabb, bg, f, f, f, None, f, need, None)


@pytest.mark.parametrize("backward", [False, True])
def test_run_refusals_need_no_device(backward):
    L = ngp_hip.lib().raw
    err = L.ngp_last_error
    assert _run(L, grid=None, backward=backward) == EINVAL and b"null occupancy grid" in err()
    assert _run(L, grid=_grid(bits=False), backward=backward) == EINVAL and b"null occupancy grid" in err()
    assert _run(L, grid=_grid(C=0), backward=backward) == EINVAL and b"C = 0" in err()
    for H in (0, 1, 24, 33, 100, 2048):
        assert _run(L, grid=_grid(H=H), backward=backward) == EINVAL and b"power of two" in err(), H
    assert _run(L, grid=_grid(C=8, H=1024), backward=backward) == EINVAL and b"32-bit index" in err()
    for T in (0, 4097):
        assert _run(L, T=T, saved_bytes=1 << 40, backward=backward) == EINVAL and b"num_steps must be in [1, 4096]" in err(), T
    need = L.ngp_nav_run_occ_saved_bytes(8, 64)
    assert _run(L, saved_bytes=need - 1, backward=backward) == EINVAL and (b"saved" in err())
    assert _run(L, saved_bytes=L.ngp_nav_run_saved_bytes(8, 64), backward=backward) == EINVAL      # the dense record alone is too short
    assert _run(L, field=ngp_hip.ngp_nav_field_t(), backward=backward) == EINVAL and b"null field" in err()
    # the grid is judged even when there is nothing to render; a good one with no rays is fine
    assert _run(L, grid=_grid(H=33), N=0, backward=backward) == EINVAL
    assert _run(L, N=0, backward=backward) == 0


def _cfg(B=16, num_steps=64):
    c = ngp_hip.ngp_filter_cfg_t()
    c.H, c.W, c.num_steps, c.B = 20, 20, num_steps, B
    c.intrinsics[:] = [27.8, 27.8, 10.0, 10.0]
    c.aabb[:] = [-2, -2, -2, 2, 2, 2]
    c.min_near = 0.2
    c.bg[:] = [1, 1, 1]
    c.sig_inv[:] = [1.0 if k % 13 == 0 else 0.0 for k in range(144)]
    c.lr, c.beta1, c.beta2, c.eps = 1e-3, 0.9, 0.999, 1e-8
    return c


def _iterations(L, c, grid="default", K=3, ws_bytes=1 << 40, field=None, n_iter=1):
    f = _fake()
    fld = _field() if field is None else field
    g = _grid() if grid == "default" else grid
    return L.ngp_filter_iterations_occ(ctypes.byref(fld), f, ctypes.byref(c), ctypes.byref(g) if g is not None else None, K, f, f, f, f, 0, n_iter, 1,
                                       None, None, None, f, ws_bytes, None)


def _hessian(L, c, grid="default", ws_bytes=1 << 40, field=None):
    f = _fake()
    fld = _field() if field is None else field
    g = _grid() if grid == "default" else grid
    return L.ngp_filter_hessian_occ(ctypes.byref(fld), f, ctypes.byref(c), ctypes.byref(g) if g is not None else None, f, f, f, f, None, None, None, f,
                                    ws_bytes, None)


def test_filter_refusals_need_no_device():
    L = ngp_hip.lib().raw
    err = L.ngp_last_error
    for call in (_iterations, _hessian):
        assert call(L, _cfg(), grid=None) == EINVAL and b"null occupancy grid" in err()
        assert call(L, _cfg(), grid=_grid(H=48)) == EINVAL and b"power of two" in err()
        assert call(L, _cfg(), grid=_grid(C=0)) == EINVAL and b"C = 0" in err()
        for T in (0, 4097):
            assert call(L, _cfg(num_steps=T)) == EINVAL and b"num_steps" in err(), T
        assert call(L, _cfg(), field=ngp_hip.ngp_nav_field_t()) == EINVAL and b"null field" in err()
    for K in (1, 3, 64):
        need = L.ngp_filter_occ_workspace(K, 16, 64)
        assert need > L.ngp_filter_multi_workspace(K, 16, 64)
        assert _iterations(L, _cfg(), K=K, ws_bytes=need - 1) == EWORKSPACE and b"ngp_filter_occ_workspace" in err()
        assert _iterations(L, _cfg(), K=K, ws_bytes=L.ngp_filter_multi_workspace(K, 16, 64)) == EWORKSPACE     # the dense route's workspace is too short
        assert _iterations(L, _cfg(), K=K, ws_bytes=need, n_iter=0) == 0                                         # everything judged, nothing queued
    assert _iterations(L, _cfg(), K=0) == EINVAL and b"K = 0" in err()
    assert _iterations(L, _cfg(), K=65) == EINVAL and b"K = 65" in err()
    need = L.ngp_filter_occ_workspace(1, 16, 64)
    assert _hessian(L, _cfg(), ws_bytes=need - 1) == EWORKSPACE and b"ngp_filter_occ_workspace(1, B, num_steps)" in err()


def test_python_interface_refuses_without_a_grid():
    """render_fn_occupied and sampling="occupied" need the renderer's grid (cuda_ray=True); "dense" is the default and any other word is refused"""
    import inspect
    import torch
    from ngp import nav
    from ngp.field import NGPField
    from ngp.render import NGPRenderer
    ren = NGPRenderer(NGPField(bound=2.0), bound=2.0, cuda_ray=False)
    q = nav.NativeNavQueries(ren, (27.8, 27.8, 10.0, 10.0), 20, 20, num_steps=64)
    cfg = {"batch_size": 16, "lrate": 1e-3, "N_iter": 2, "sig0": torch.eye(12), "Q": torch.eye(12)}
    assert nav.NativePoseFilter(cfg, q).sampling == "dense" and nav.NativePoseFilter(cfg, q, sampling="dense").sampling == "dense"
    with pytest.raises(ValueError, match="cuda_ray=True"):
        nav.NativePoseFilter(cfg, q, sampling="occupied")
    with pytest.raises(ValueError, match="sampling must be"):
        nav.NativePoseFilter(cfg, q, sampling="sparse")
    with pytest.raises(ValueError, match="cuda_ray=True"):
        q.render_fn_occupied(torch.zeros(4, 3), torch.zeros(4, 3))
    assert inspect.signature(nav.simulate).parameters["filter_sampling"].default == "dense"
