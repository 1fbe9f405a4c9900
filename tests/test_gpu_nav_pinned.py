"""GPU: the fused nav queries (csrc/nav_field.hip: k_nav_run_fwd / _bwd, k_nav_density_vj / _fwd / _bwd) against the PINNED float64 reference of
oracle/callers_oracle.py, ray by ray and point by point.  Cases, references and the rule live in tests/_nav_pinned_cases.py; what makes them a fair
yardstick is checked on the CPU by tests/test_nav_pinned_host.py.

The rule: for every ray (point) i of a case, error_kernel[i] <= 16 * max(error_float32_oracle[i], p90(error_float32_oracle)), both errors against
the same pinned reference; gradients and sigma relative to the reference's own size per row, image / depth / weights_sum / geo absolute.  Each
check prints its largest error / yardstick (run with -s).  For image, depth and weights_sum of a run longer than one 256-sample chunk the
yardstick has a floor derived from the kernel's carried transmittance product (_nav_pinned_cases.carry_floor); the margin is 16 everywhere.

What the first run of this file found (MI355X), and what became of it:
  * k_nav_run_bwd took d alpha / d sigma = delta scale (1 - alpha) from the SAVED alpha.  1 - alpha has an absolute error of 2^-25, which is 3e-4 of an
    opaque sample's exp(-delta scale sigma) = 1e-4, and the ray's gradient hangs on that sample: contrast (257 steps) ray 92 sat 3.1e-4 from the
    reference, 39.9 yardsticks; chunk_256 ray 11 9.9e-5, 25 yardsticks; tiny_3 11 yardsticks.  The record now keeps exp(-delta scale sigma) itself
    (alpha is recomputed from it bit for bit): 5.7, 1.2 and 0.84 yardsticks.  The fog of tests/test_gpu_nav_native.py has no opaque sample.
  * weights_sum at 4,096 steps on the ray axis_z: 18.2 yardsticks, 7.8e-7 absolute -- the carried product's own rounding against a float32 oracle that
    sat 1e-9 from the reference on that ray; hence the floor (1.01 of it).  That ray has since left the long batch (_nav_pinned_cases.rays: the float32
    oracle's own image is too far from the reference on it at 4,096 steps); on the present eight rays the largest is 4.2e-7 against an oracle at 2e-9.
  * the miss ray's depth is 0 here and NaN (0 / 0) in the reference: left alone, as in tests/test_gpu_nav_native.py.

Largest error / yardstick per case, after the fix (the file takes 5 s on the GPU, all of it the CPU references: 26 tests, the slowest 1.0 s):
  case                 image  weights_sum  depth  grad_o  grad_d
  base                  1.45     2.06       1.83   5.31    2.15
  contrast              3.03     1.31       1.49   5.66    3.86
  chunk_255             2.06     2.39       5.79   0.86    0.76
  chunk_256             2.81     2.54       2.68   1.22    1.31
  tiny_1                1.41     1.54       0      1.87    1.79
  tiny_2                1.54     1.30       1.83   1.87    1.74
  tiny_3                1.00     1.68       1.55   0.84    0.95
  long_513              1.78     0.63       0.39   2.37    1.98
  long_4096             1.27     0.55       0.44   2.57    2.23
  background            1.43     1.01       2.41   1.37    1.30
  scale_2               1.79     2.04       2.74   2.22    2.65
  bound_1               2.96     3.08       2.93   1.40    1.30
  weights_sum_alone     1.52     1.74       3.29   3.34    2.74
  depth_alone           1.52     1.74       3.29   2.54    1.98
  points (largest over the batch sizes)         sigma   geo   gradient
  vj fog bound 2 none / nav / rot30             1.58     -     3.18
  vj contrast bound 2 rot30                     1.77     -     1.84
  vj fog bound 1 nav, bound 1.5 rot30           1.53     -     2.69
  one-lane fog bound 2 / contrast / fog 1.5     2.36    1.65   3.70
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

import _nav_pinned_cases as C  # noqa: E402


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_RIGS = {}


def rig(dev, kind, bound=2.0, density_scale=1.0, min_near=0.2):
    """(renderer, ngp.nav._NativeField) over the product field holding the case's numbers; built once per module"""
    from ngp import nav
    from ngp.render import NGPRenderer
    key = (kind, bound, density_scale, min_near)
    if key not in _RIGS:
        ren = NGPRenderer(C.product_field(kind, bound, dev), bound=bound, cuda_ray=False, density_scale=density_scale, min_near=min_near).to(dev).eval()
        for p in ren.parameters():
            p.requires_grad_(False)
        _RIGS[key] = (ren, nav._NativeField(ren))
    return _RIGS[key]


def case_rig(dev, case):
    return rig(dev, case["field"], case["bound"], case["density_scale"], case["min_near"])


def bg3(case):
    return tuple(float(v) for v in (case["bg"] if not np.isscalar(case["bg"]) else (case["bg"],) * 3))


def gpu_run(dev, case, o=None, d=None, weights=None):
    """the case through ngp.nav._nav_run (one launch forward, one backward) -> numpy dict like _nav_pinned_cases.oracle_run's"""
    from ngp import nav
    if o is None:
        o, d, _ = C.case_rays(case)
    G, Gd, Gw = weights if weights is not None else C.loss_weights(o.shape[0])
    _, native = case_rig(dev, case)
    ro, rd = t(o, dev).requires_grad_(True), t(d, dev).requires_grad_(True)
    image, depth, ws = nav._nav_run.apply(ro, rd, native, case["T"], bg3(case))
    loss = 0
    if "image" in case["terms"]:
        loss = loss + (image * t(G, dev)).sum()
    if "depth" in case["terms"]:
        loss = loss + (depth * t(Gd, dev)).sum()
    if "weights_sum" in case["terms"]:
        loss = loss + (ws * t(Gw, dev)).sum()
    loss.backward()
    return dict(image=image.detach().cpu().numpy(), depth=depth.detach().cpu().numpy(), weights_sum=ws.detach().cpu().numpy(),
                grad_o=ro.grad.cpu().numpy(), grad_d=rd.grad.cpu().numpy())


def check_run(name, got):
    r = C.run_reference(name)
    ref, miss = r["ref"], r["miss"]
    everyone = np.ones(len(r["hit"]), bool)
    worst = {}
    # absolute, every ray: the miss too (image = background, weights_sum = 0; its depth is 0 / 0 in the reference and left alone)
    for k in ("image", "weights_sum", "depth"):
        worst[k] = C.judge(name, got[k], ref[k], r["e32"][k], everyone, k, floor=C.carry_floor(r["case"]["T"]))
    assert np.isfinite(got["image"]).all() and np.isfinite(got["weights_sum"]).all() and np.isfinite(np.delete(got["depth"], miss)).all()
    for k in ("grad_o", "grad_d"):
        worst[k] = C.judge(name, got[k], ref[k], r["e32"][k], r["judged"], k)
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# the run kernels against the reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.RUN_CASES))
def test_run_against_the_pinned_reference(dev, name):
    """every case of the table: image, depth, weights_sum and both ray gradients, ray by ray"""
    check_run(name, gpu_run(dev, C.RUN_CASES[name]))


def test_near_far_of_the_special_rays(dev, oracle):
    """the rays the reference and the kernels march must be the same rays: near / far of the product's op are the oracle's bits, also for the ray
    along a face (0 * inf in the slab test) and the axis-parallel ones (1 / 0)"""
    import raymarching
    for bound, min_near in ((2.0, 0.2), (1.0, 0.05)):
        o, d, miss = C.rays(bound)
        aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
        n, f = raymarching.near_far_from_aabb(t(o, dev), t(d, dev), t(aabb, dev), min_near)
        nr, fr = oracle.near_far_from_aabb(o, d, aabb, min_near)
        assert np.array_equal(n.cpu().numpy().view(np.uint32), nr.view(np.uint32)) and np.array_equal(f.cpu().numpy().view(np.uint32), fr.view(np.uint32))
        assert nr[miss] == np.finfo(np.float32).max and (np.delete(nr, miss) < 10).all()


# ------------------------------------------------------------------------------------------------------------------------
# the C ABI directly: what the wrapper cannot pass
# ------------------------------------------------------------------------------------------------------------------------
class Raw:
    """ngp_nav_run_forward / _backward through ctypes on one renderer"""

    def __init__(self, dev, case):
        import ngp_hip as H
        self.H, self.L, self.dev, self.case = H, H.lib(), dev, case
        self.ren, self.native = case_rig(dev, case)
        self.aabb = (ctypes.c_float * 6)(*[float(v) for v in self.ren._aabb().tolist()])
        self.bg = (ctypes.c_float * 3)(*bg3(case))

    def forward(self, o, d, T=None, keep=True, bg=True):
        import raymarching
        H, L = self.H, self.L
        T = self.case["T"] if T is None else T
        o, d = t(o, self.dev), t(d, self.dev)
        N = o.shape[0]
        nears, fars = raymarching.near_far_from_aabb(o, d, self.ren._aabb(), self.ren.min_near) if N else (o[:, 0], o[:, 0])
        image, depth, ws = (torch.full((max(N, 1), 3), -7.0, device=self.dev), torch.full((max(N, 1),), -7.0, device=self.dev),
                            torch.full((max(N, 1),), -7.0, device=self.dev))
        saved = H.workspace(L.ngp_nav_run_saved_bytes(N, T), self.dev) if keep and 1 <= T <= 4096 else None
        st, prep = self.native.struct()
        with torch.cuda.device(self.dev):
            rc = L.ngp_nav_run_forward(ctypes.byref(st), H.ptr(prep), H.ptr(o), H.ptr(d), H.ptr(nears), H.ptr(fars), N, T, self.aabb,
                                       self.bg if bg else None, H.ptr(image), H.ptr(depth), H.ptr(ws), H.ptr(saved), saved.numel() if saved is not None else 0,
                                       H.stream())
        return rc, dict(o=o, d=d, nears=nears, fars=fars, T=T, N=N, image=image, depth=depth, weights_sum=ws, saved=saved)

    def backward(self, f, g_image, g_depth, g_ws):
        H, L = self.H, self.L
        go, gd = torch.full_like(f["o"], -7.0), torch.full_like(f["d"], -7.0)
        st, prep = self.native.struct()
        dv = lambda a: None if a is None else t(a, self.dev)                     # noqa: E731
        gi, gde, gw = dv(g_image), dv(g_depth), dv(g_ws)
        with torch.cuda.device(self.dev):
            rc = L.ngp_nav_run_backward(ctypes.byref(st), H.ptr(prep), H.ptr(f["o"]), H.ptr(f["d"]), H.ptr(f["nears"]), H.ptr(f["fars"]), f["N"], f["T"],
                                        self.aabb, self.bg, H.ptr(gi), H.ptr(gde), H.ptr(gw), H.ptr(f["saved"]), f["saved"].numel(), H.ptr(go), H.ptr(gd),
                                        H.stream())
        torch.cuda.synchronize()
        return rc, go, gd


def same(a, b):
    """bit for bit, NaNs in the same places"""
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_ray_does_not_depend_on_its_batch(dev):
    """bit for bit, forward and backward: a ray rendered alone equals the same ray at positions 0, middle and last of the full batch (the saved record's
    stride is N * T: 152 x 257 words apart against 257); the hit rays are unchanged by the miss among them"""
    case = C.RUN_CASES["contrast"]
    raw = Raw(dev, case)
    o, d, miss = C.case_rays(case)
    G, Gd, Gw = C.loss_weights(o.shape[0])
    N = o.shape[0]
    src = 40                                                         # an orbit ray
    for at in (0, N // 2 - 1, N - 1):
        ob, db = o.copy(), d.copy()
        ob[at], db[at] = o[src], d[src]
        rc, f = raw.forward(ob, db)
        assert rc == 0
        rc, go, gd = raw.backward(f, G, Gd, Gw)
        assert rc == 0
        rc, f1 = raw.forward(o[src:src + 1], d[src:src + 1])
        assert rc == 0
        rc, go1, gd1 = raw.backward(f1, G[at:at + 1], Gd[at:at + 1], Gw[at:at + 1])
        assert rc == 0
        for k in ("image", "depth", "weights_sum"):
            assert same(f[k][at:at + 1], f1[k]), (at, k)
        assert same(go[at:at + 1], go1) and same(gd[at:at + 1], gd1), at
        assert float(go1.abs().sum()) > 0 and torch.isfinite(go1).all()
    # the batch without its miss
    rc, f = raw.forward(o, d)
    rc2, go, gd = raw.backward(f, G, Gd, Gw)
    keep = np.arange(N) != miss
    rc3, fh = raw.forward(o[keep], d[keep])
    rc4, goh, gdh = raw.backward(fh, G[keep], Gd[keep], Gw[keep])
    assert rc == rc2 == rc3 == rc4 == 0
    kt = torch.from_numpy(keep).to(dev)
    for k in ("image", "depth", "weights_sum"):
        assert same(f[k][kt], fh[k]), k
    assert same(go[kt], goh) and same(gd[kt], gdh)
    bgc = torch.tensor(bg3(case), device=dev)
    assert torch.equal(f["image"][miss], bgc) and float(f["weights_sum"][miss]) == 0


def test_optional_arguments_of_the_run_abi(dev):
    """saved = NULL gives the forward outputs of saved given; NULL grad_depth / grad_weights_sum are zero tensors; a NULL background is (1, 1, 1);
    num_steps 0 and 4097 are refused with their message and write nothing; N = 0 is OK"""
    case = C.RUN_CASES["background"]
    raw = Raw(dev, case)
    o, d, _ = C.case_rays(case)
    N = o.shape[0]
    G, Gd, Gw = C.loss_weights(N)
    rc, f = raw.forward(o, d)
    rc2, f0 = raw.forward(o, d, keep=False)
    assert rc == rc2 == 0 and f0["saved"] is None
    for k in ("image", "depth", "weights_sum"):
        assert same(f[k], f0[k]), k
    zero = np.zeros(N, np.float32)
    _, go, gd = raw.backward(f, G, Gd, Gw)
    for gde, gw in ((None, Gw), (Gd, None), (None, None)):
        rc, a, b = raw.backward(f, G, gde, gw)
        rc2, a0, b0 = raw.backward(f, G, zero if gde is None else gde, zero if gw is None else gw)
        assert rc == rc2 == 0 and same(a, a0) and same(b, b0)
        assert not same(a, go)                                        # and the term that was dropped did matter
    white = Raw(dev, C.RUN_CASES["scale_2"])                          # a case whose background is 1
    rc, fw = white.forward(o, d)
    rc2, fn = white.forward(o, d, bg=False)
    assert rc == rc2 == 0 and same(fw["image"], fn["image"]) and not same(fw["image"], f["image"])
    for T in (0, 4097):
        rc, fr = raw.forward(o, d, T=T, keep=False)
        assert rc != 0 and "num_steps must be in [1, 4096]" in raw.L.ngp_last_error().decode()
        torch.cuda.synchronize()
        assert float(fr["image"].min()) == -7.0 and float(fr["weights_sum"].max()) == -7.0
    rc, fe = raw.forward(o[:0], d[:0])
    assert rc == 0 and float(fe["image"].min()) == -7.0


# ------------------------------------------------------------------------------------------------------------------------
# the point kernels
# ------------------------------------------------------------------------------------------------------------------------
def outside_rows(p, bound):
    f = np.float32
    x01 = ((np.asarray(p, f) + f(bound)) * (f(1.0) / f(2 * bound))).astype(f)
    return ((x01 < 0) | (x01 > 1)).any(axis=1)


def judge_points(label, got, r, M, keys):
    ref, e32 = r["ref"], r["e32"]
    inside = np.linalg.norm(ref["grad_x"], axis=1) > 0
    for k in keys:
        rows = inside[:M] if k == "grad_x" else np.ones(M, bool)
        whole = inside if k == "grad_x" else np.ones(len(inside), bool)
        C.judge(label, got[k], ref[k][:M], e32[k][:M], rows, k, p90=float(np.percentile(e32[k][whole], 90)))
    return inside


@pytest.mark.parametrize("kind,bound,rot", [("fog", 2.0, "none"), ("fog", 2.0, "nav"), ("fog", 2.0, "rot30"), ("contrast", 2.0, "rot30"), ("fog", 1.0, "nav"),
                                            ("fog", 1.5, "rot30")])
def test_value_and_jacobian_kernel(dev, kind, bound, rot):
    """k_nav_density_vj, point by point, at every batch size around its 64-point workgroup and the one-lane kernels' 256: sigma and d (sum w sigma) / d x;
    the gradient is exactly zero outside the box and non-zero on its faces and corners; the rotation not symmetric, so a transposed matrix on the way
    out shows"""
    from ngp import nav
    from oracle import callers_oracle as CO
    _, native = rig(dev, kind, bound)
    r = C.point_reference(kind, bound, rot)
    x, names = C.points(bound)
    w, _ = C.point_weights()
    m = C.ROTATIONS[rot]
    rot9 = None if m is None else tuple(float(v) for v in np.asarray(m, np.float32).reshape(-1))
    out = outside_rows(x if m is None else CO.rotate_points_float32(x, m), bound)
    assert out[[names[n] for n in C.OUTSIDE_NAMES if n.startswith("far")]].all()
    for M in C.POINT_SIZES:
        xg = t(x[:M], dev).requires_grad_(True)
        sigma = nav._nav_density_vj.apply(xg, native, rot9)
        (sigma * t(w[:M], dev)).sum().backward()
        got = dict(sigma=sigma.detach().cpu().numpy(), grad_x=xg.grad.cpu().numpy())
        inside = judge_points(f"{kind} bound {bound:g} {rot} M={M}", got, r, M, ("sigma", "grad_x"))
        assert np.array_equal(inside[:M], ~out[:M])                 # the reference and the float32 rule agree on who is outside
        assert np.all(got["grad_x"][out[:M]] == 0) and np.all(got["sigma"][out[:M]] == 1.0)
        assert np.all(np.abs(got["grad_x"][~out[:M]]).sum(axis=1) > 0)
    if m is None:
        on_box = [names[n] for n in names if n.startswith(("face", "corner", "above"))]
        assert not out[on_box].any() and out[[names[n] for n in C.OUTSIDE_NAMES]].all()


@pytest.mark.parametrize("kind,bound", [("fog", 2.0), ("contrast", 2.0), ("fog", 1.5)])
def test_one_lane_kernels_with_geo(dev, kind, bound):
    """k_nav_density_fwd's `geo` output and k_nav_density_bwd's `grad_geo` input (the wrappers pass NULL for both): sigma, geo_feat and the gradient of
    sum(w sigma) + sum(Gg geo_feat), point by point, on the rotated points; then the value-and-Jacobian kernel against them on the same rotated
    points (2e-6 / 2e-5, another summation order of the same sums)"""
    import ngp_hip as H
    from ngp import nav
    L = H.lib()
    _, native = rig(dev, kind, bound)
    r = C.point_reference(kind, bound, "rot30", with_geo=True, prerotated=True)
    p = r["x"]
    w, Gg = C.point_weights()
    st, prep = native.struct()

    def one_lane(M, with_geo):
        pg = t(p[:M], dev)
        sigma, geo, gx = torch.full((M,), -7.0, device=dev), torch.full((M, 15), -7.0, device=dev), torch.full((M, 3), -7.0, device=dev)
        gs, gg = t(w[:M], dev), t(Gg[:M], dev)
        with torch.cuda.device(dev):
            H.check(L.ngp_nav_density_forward(ctypes.byref(st), H.ptr(prep), H.ptr(pg), M, H.ptr(sigma), H.ptr(geo) if with_geo else None, H.stream()), "fwd")
            H.check(L.ngp_nav_density_backward(ctypes.byref(st), H.ptr(prep), H.ptr(pg), M, H.ptr(gs), H.ptr(gg) if with_geo else None, H.ptr(gx), H.stream()),
                    "bwd")
        torch.cuda.synchronize()
        return sigma, geo, gx

    for M in C.POINT_SIZES:
        sigma, geo, gx = one_lane(M, True)
        got = dict(sigma=sigma.cpu().numpy(), geo=geo.cpu().numpy(), grad_x=gx.cpu().numpy())
        judge_points(f"{kind} bound {bound:g} one-lane M={M}", got, r, M, ("sigma", "geo", "grad_x"))
        s0, g0, _ = one_lane(M, False)
        assert torch.equal(s0, sigma) and float(g0.min()) == -7.0     # a NULL geo changes nothing else and nothing is written
    # second line: the level-parallel kernel on the unrotated points against the one-lane kernels on the rotated ones.  Fog only: 2e-6 of sigma is
    # 2e-6 ABSOLUTE in log sigma, which the contrast field's gain of 120 scales out of float32's reach (its first line above is per point instead)
    if kind != "fog":
        return
    x, _ = C.points(bound)
    sigma, _, gp = one_lane(C.N_POINTS, False)
    xg = t(x, dev).requires_grad_(True)
    s_vj = nav._nav_density_vj.apply(xg, native, tuple(float(v) for v in C.ROT30.reshape(-1)))
    (s_vj * t(w, dev)).sum().backward()
    assert torch.allclose(s_vj, sigma, rtol=2e-6, atol=0)
    want = gp.double().cpu().numpy() @ C.ROT30.astype(np.float64).T   # d / d x = rot (d / d p)
    g = xg.grad.double().cpu().numpy()
    assert np.linalg.norm(g - want) / np.linalg.norm(want) < 2e-5
