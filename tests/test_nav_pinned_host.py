"""CPU: the pinned float64 reference of the nav queries (oracle.callers_oracle, pin_float32) and the cases of tests/_nav_pinned_cases.py that
tests/test_gpu_nav_pinned.py holds the kernels to.  What is checked here are conditions on the REFERENCE and on the INPUTS: that pinning changes
nothing in float32, that the float64 run sits in the float32 run's cells, that the float32 oracle's distance from the reference (the yardstick of
the GPU test) is small on every ray of every case, and that the comparison needs the pinning at all."""
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")

import _nav_pinned_cases as C  # noqa: E402
from oracle import callers_oracle as CO  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built(oracle):
    return oracle


def test_pinned_mode_in_float32_is_the_plain_float32_oracle():
    """values bit for bit, gradients to 1e-6 relative per ray: run() on a batch with every special ray, and the point query with a rotation"""
    case = C.RUN_CASES["background"]
    plain, pinned = C.oracle_run(case, torch.float32, False), C.oracle_run(case, torch.float32, True)
    for k in ("image", "depth", "weights_sum", "weights", "mask"):
        assert np.array_equal(plain[k], pinned[k], equal_nan=True), k
    miss = C.case_rays(case)[2]
    hit = np.arange(plain["grad_o"].shape[0]) != miss
    for k in ("grad_o", "grad_d"):
        assert np.nanmax(C.row_error(pinned[k], plain[k], k)[hit]) <= 1e-6, k
    # the point query: the pinned rotated point against the same float32 values handed in as the points themselves
    x, _ = C.points(2.0)
    a = C.oracle_points("contrast", 2.0, C.ROT30, torch.float32, True, True)
    p = torch.from_numpy(CO.rotate_points_float32(x, C.ROT30))
    b = C.oracle_field("contrast", 2.0).density(p)
    assert torch.equal(torch.from_numpy(a["sigma"]), b["sigma"].detach()) and torch.equal(torch.from_numpy(a["geo"]), b["geo_feat"].detach())


def test_pinned_float64_sits_in_the_float32_cells():
    """floor(pos) at all 16 levels and the out-of-box test of the pinned float64 encoder are the float32 encoder's, the fractions are its fractions cast
    up, and d frac / d x is scale / (2 bound); the run's colour mask is the float32 run's on every case"""
    bound = 2.0
    x, names = C.points(bound)
    emb, offsets, pls, _, _ = C.field_arrays("fog", bound)
    tx = torch.from_numpy(x).double().requires_grad_(True)
    oob32, lv32 = CO.grid_cells(torch.from_numpy(x), torch.float32, 16, pls, bound=bound)
    oob64, lv64 = CO.grid_cells(tx, torch.float64, 16, pls, bound=bound, pin_float32=True)
    _, lvp = CO.grid_cells(torch.from_numpy(x).double(), torch.float64, 16, pls, bound=bound)
    assert torch.equal(oob32, oob64)
    left = 0
    for level in range(16):
        assert torch.equal(lv32[level][0], lv64[level][0]) and torch.equal(lv32[level][1].double(), lv64[level][1].detach()), level
        assert np.array_equal(lv32[level][0].numpy()[~oob32.numpy()[:, 0]], np.floor(C.grid_pos32(x, level, bound)).astype(np.int64)[~oob32.numpy()[:, 0]])
        (g,) = torch.autograd.grad(lv64[level][1].sum(), tx, retain_graph=True)
        assert torch.allclose(g, torch.full_like(g, float(C.level_scale(level, bound)) / (2 * bound)), rtol=1e-15, atol=0)
        left += int((lvp[level][0] != lv32[level][0]).any(dim=1).sum())
    assert left > 0                                                               # plain float64 does leave the float32 cells
    e32 = CO.grid_encode(torch.from_numpy(x), torch.from_numpy(emb), offsets, pls, bound=bound)
    tx = torch.from_numpy(x).double().requires_grad_(True)
    e64 = CO.grid_encode(tx, torch.from_numpy(emb).double(), offsets, pls, bound=bound, pin_float32=True)
    # same cells and fractions: the float64 interpolation of float32 fractions differs from the float32 one by rounding only (|table| <= 0.5)
    assert float((e64.detach() - e32.double()).abs().max()) < 4e-7
    outside = np.array([names[n] for n in C.OUTSIDE_NAMES])
    assert torch.all(e64.detach()[outside] == 0) and torch.all(e32[outside] == 0)
    (g64,) = torch.autograd.grad(e64[:, 31].sum(), tx)
    tp = torch.from_numpy(x).double().requires_grad_(True)
    (gp,) = torch.autograd.grad(CO.grid_encode(tp, torch.from_numpy(emb).double(), offsets, pls, bound=bound)[:, 31].sum(), tp)
    t32 = torch.from_numpy(x).requires_grad_(True)
    (g32,) = torch.autograd.grad(CO.grid_encode(t32, torch.from_numpy(emb), offsets, pls, bound=bound)[:, 31].sum(), t32)
    rel = lambda a, b: (a - b).norm(dim=1) / b.norm(dim=1).clamp(min=1e-30)  # noqa: E731
    assert float(rel(g32.double(), g64).max()) < 1e-4                            # the finest level's gradient agrees only with the cells pinned
    assert float(rel(gp, g64).max()) > 1e-2
    for name in C.RUN_CASES:
        r = C.run_reference(name)
        assert np.array_equal(r["ref"]["mask"], r["f32"]["mask"]), name


def test_special_points_are_what_their_names_say():
    for bound in (2.0, 1.0, 1.5):
        x, names = C.points(bound)
        f = np.float32
        x01 = ((x + f(bound)) * (f(1.0) / f(2 * bound))).astype(f)
        for n, row in names.items():
            if n.startswith(("face", "corner")):
                assert ((x01[row] == 0) | (x01[row] == 1)).sum() == (1 if n.startswith("face") else 3), (bound, n)
            if n.startswith("above"):
                a = "xyz".index(n[-1])
                assert x[row, a] > bound and x01[row, a] == 1.0, (bound, n)     # past the face as a number, ON it after the encoder's own rounding
            if n in C.OUTSIDE_NAMES:
                assert ((x01[row] < 0) | (x01[row] > 1)).any(), (bound, n)
            if n.startswith("node"):
                level = int(n[-1])
                pos = C.grid_pos32(x[row], level, bound)
                assert np.all(pos == np.floor(pos)), (bound, n)


@pytest.mark.parametrize("T", C.STEP_COUNTS + [100, 511, 512, 1000])
def test_linspace_rule(T):
    """nv_lin's restated rule is torch.linspace bit for bit, so the pinned reference evaluates the kernels' own samples"""
    assert np.array_equal(C.lin_rule(T).view(np.uint32), torch.linspace(0.0, 1.0, T, dtype=torch.float32).numpy().view(np.uint32))


def test_contrast_field_has_contrast():
    """over the 146 base rays at 100 steps: the colour mask keeps 5-60 % of the samples; >= 10 % of the rays end translucent, >= 10 % opaque"""
    o, d = C.base_rays()
    assert o.shape[0] == 146
    with torch.no_grad():
        out = CO.run(C.oracle_field("contrast", 2.0), torch.from_numpy(o), torch.from_numpy(d), 2.0, num_steps=100)
        fog = CO.run(C.oracle_field("fog", 2.0), torch.from_numpy(o), torch.from_numpy(d), 2.0, num_steps=100)
    w, ws = out["weights"].numpy(), out["weights_sum"].numpy()
    share = float((w > 1e-4).mean())
    print(f"contrast: kept {share:.3f}, weights_sum < 0.99 on {(ws < 0.99).mean():.3f}, > 0.999 on {(ws > 0.999).mean():.3f}; fog kept {(fog['weights'].numpy() > 1e-4).mean():.3f}")
    assert 0.05 <= share <= 0.6
    assert (ws < 0.99).mean() >= 0.10 and (ws > 0.999).mean() >= 0.10
    assert (fog["weights"].numpy() > 1e-4).all()                                  # what the first suite's field never leaves


@pytest.mark.parametrize("name", list(C.RUN_CASES))
def test_run_case_is_well_conditioned(name):
    """the float32 oracle against the pinned reference, per ray: gradients p90 <= 1e-4 and max <= 1e-3 relative, values <= 1e-6 absolute; at most 2 % of
    the rays (the miss apart) left out of the relative check"""
    r = C.run_reference(name)
    n_hit = int(r["hit"].sum())
    dropped = int((r["hit"] & ~r["judged"]).sum())
    line = [f"{name}: rays {n_hit} + miss, left out {dropped}"]
    for k in ("grad_o", "grad_d"):
        e = r["e32"][k][r["judged"]]
        line.append(f"{k} median {np.median(e):.2g} p90 {np.percentile(e, 90):.2g} max {e.max():.2g}")
    for k in ("image", "depth", "weights_sum"):
        line.append(f"{k} {np.nanmax(r['e32'][k][r['hit']]):.2g}")
    print("; ".join(line))
    assert dropped <= 0.02 * n_hit
    for k in ("grad_o", "grad_d"):
        e = r["e32"][k][r["judged"]]
        assert np.percentile(e, 90) <= 1e-4 and e.max() <= 1e-3, k
    for k in ("image", "depth", "weights_sum"):
        assert np.nanmax(r["e32"][k][r["hit"]]) <= 1e-6, k
    miss = r["miss"]
    assert np.isnan(r["ref"]["depth"][miss]) and r["ref"]["weights_sum"][miss] == 0
    if name == "contrast":                                                        # opaque and saturated samples, masked samples: the branches the fog never takes
        w = r["ref"]["weights"][r["hit"]]
        assert (w <= 1e-4).mean() > 0.3 and (w > 0.5).any()


@pytest.mark.parametrize("kind,bound,rot", [("fog", 2.0, "none"), ("fog", 2.0, "nav"), ("fog", 2.0, "rot30"), ("contrast", 2.0, "rot30"), ("fog", 1.0, "nav"),
                                            ("fog", 1.5, "rot30")])
def test_point_case_is_well_conditioned(kind, bound, rot):
    r = C.point_reference(kind, bound, rot)
    inside = np.linalg.norm(r["ref"]["grad_x"], axis=1) > 0
    e = r["e32"]["grad_x"][inside]
    print(f"{kind} bound {bound} {rot}: sigma {np.nanmax(r['e32']['sigma']):.2g}; gradient median {np.median(e):.2g} p90 {np.percentile(e, 90):.2g} max {e.max():.2g}")
    # sigma = exp(h0): its relative error is the absolute error of h0, a 64-term float32 dot product whose size the contrast gain multiplies:
    # 2^-24 per rounding, sqrt(64) roundings accumulated, times the largest |log sigma| of the case -- 1e-6 for a field of unit log-density
    log_sigma = float(np.abs(np.log(r["ref"]["sigma"])).max())
    assert np.percentile(e, 90) <= 1e-4 and e.max() <= 1e-3 and np.nanmax(r["e32"]["sigma"]) <= 1e-6 * max(1.0, log_sigma)
    assert inside.sum() > 0.5 * len(inside)


def test_plain_float64_cannot_judge_these_gradients():
    """without the pinning a float64 run leaves the float32 run's cells: some ray's gradient differs by more than 1e-2.  This is why the reference is pinned."""
    case = C.RUN_CASES["base"]
    plain = C.oracle_run(case, torch.float64, False)
    r = C.run_reference("base")
    worst = max(float(np.nanmax(C.row_error(plain[k], r["ref"][k], k)[r["judged"]])) for k in ("grad_o", "grad_d"))
    print(f"plain float64 against pinned float64: worst ray {worst:.3g}")
    assert worst > 1e-2
