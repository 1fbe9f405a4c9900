"""GPU: the resampled run (csrc/nav_field.hip: k_sample_pdf, k_nav_resample, k_nav_run_fwd<true> / _bwd<true>; csrc/nav_filter.hip: the _res entry points;
include/ngp_hip.h "Resampled run").

  * ngp_sample_pdf is bit-equal to the numpy restatement (tests/_resample_restated.py) on the reference-recorded vectors and on constructed weights;
  * ngp_nav_run_resample: the coarse weights against the pinned float64 oracle by _nav_pinned_cases.judge; z bit-equal to the restatement applied to the
    kernel's own coarse weights; the coarse depths inside z are the dense lattice's bits; z non-decreasing; the miss ray gets T copies of near;
  * ngp_nav_run_at_forward / _backward against a float64 reference evaluated at the same float32 depth list (tests/_run_at_cases.py), by the dense rule
    and margin (16 x max(own float32-oracle error, p90), carry_floor beyond one chunk);
  * render_fn_resampled end to end against callers_oracle.run(float64, upsample_steps) with its own depths; the difference from NGPRenderer.run on the
    GPU is printed beside it;
  * the filter's resampled route: K = 1 against K = 3, the Hessian against an update = 0 iteration, two runs, set_sampling round trips, simulate().

Each check prints its largest error / yardstick (run with -s).
Largest error / yardstick per case on an MI355X (the two files take 6 s, most of it the CPU references: 46 tests, the slowest 0.6 s).  The coarse weights
column is ngp_nav_run_resample's against the pinned float64 run at upsample_steps = 0; the others are the run over the kernel's own depth list:
  case (Nc + Nf)         coarse w  image  weights_sum  depth  grad_o  grad_d
  r3_1                     0.55    1.10     1.84       1.56    0.84    0.99
  r8_5 (fog)               1.57    1.69     2.34       1.62    0.86    0.56
  r64_64                   1.75    2.16     2.72       8.09    2.23    2.17
  r255_1                   1.76    1.41     2.46       3.86    2.50    2.60
  r256_256                 1.23    3.38     1.91       3.01    9.15    5.84
  r257_130 (fog)           0.71    0.80     0.88       0.96    3.93    2.84
  r128_128                 1.38    2.11     3.24       5.61    2.01    2.01
  r2048_2048 (8 rays)      0.88    2.10     2.84       1.42    1.11    1.02
  bound_1 (64 + 64)        2.09    3.23     2.97       3.77    1.76    1.90
  scale_2 (fog, 64 + 64)   1.10    0.86     1.67       1.81    1.75    1.48
  background (8 + 5)       1.44    1.14     2.09       2.35    1.66    1.69
  weights_sum_alone        1.40    1.47     2.00       2.66   15.27   14.47
  depth_alone              1.40    1.47     2.00       2.66    1.04    1.25
weights_sum_alone, row 14: the loss is flat where a ray saturates, and with 64 more samples at its surface this ray does (the float32 oracle itself is
2.7 % from the reference there); its gradient is the difference A T_i - S_i / keep_i of two numbers a million times its size.  Inside the margin, and
the largest figure of the file.
ngp_sample_pdf against the reference-recorded vectors: det 8.3e-6, rand 2.4e-6 (allowed 5e-5); bit-equal to the restatement everywhere.
End to end (render_fn_resampled against the float64 oracle with its own depths): 1.00 - 1.03 yardsticks at (64, 64) and (128, 128) -- the float32 oracle's
own error (up to 1e-2: one ulp of a coarse weight moves a new depth across a bin) is the yardstick and the kernel sits where it sits; the difference from
NGPRenderer.run on the same GPU is at most 7e-5 in image and depth.
"""
import ctypes
import functools
import importlib
import os

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

import _nav_cases as NC  # noqa: E402
import _nav_pinned_cases as C  # noqa: E402
import _resample_restated as RS  # noqa: E402
import _run_at_cases as RA  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits_of(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, F).view(np.uint32)


_RIGS = {}


def case_rig(dev, case):
    """(renderer, ngp.nav._NativeField) over the product field holding the case's numbers; built once per module.  cuda_ray=False: no occupancy grid"""
    from ngp import nav
    from ngp.render import NGPRenderer
    key = (case["field"], case["bound"], case["density_scale"], case["min_near"])
    if key not in _RIGS:
        ren = NGPRenderer(C.product_field(case["field"], case["bound"], dev), bound=case["bound"], cuda_ray=False, density_scale=case["density_scale"],
                          min_near=case["min_near"]).to(dev).eval()
        for p in ren.parameters():
            p.requires_grad_(False)
        _RIGS[key] = (ren, nav._NativeField(ren))
    return _RIGS[key]


def bg3(case):
    return tuple(float(v) for v in (case["bg"] if not np.isscalar(case["bg"]) else (case["bg"],) * 3))


class Ops:
    """the four ops through ctypes on one case's renderer"""

    def __init__(self, dev, case):
        import ngp_hip as H
        self.H, self.L, self.dev, self.case = H, H.lib(), dev, case
        self.ren, self.native = case_rig(dev, case)
        self.aabb = (ctypes.c_float * 6)(*[float(v) for v in self.ren._aabb().tolist()])
        self.bg = (ctypes.c_float * 3)(*bg3(case))

    def rays(self, o, d):
        import raymarching
        o, d = t(o, self.dev), t(d, self.dev)
        nears, fars = raymarching.near_far_from_aabb(o, d, self.ren._aabb(), self.ren.min_near)
        return dict(o=o, d=d, nears=nears, fars=fars, N=o.shape[0])

    def resample(self, r, Nc, Nf, weights=True):
        H, L = self.H, self.L
        z = torch.full((r["N"], Nc + Nf), float("nan"), device=self.dev)
        w = torch.full((r["N"], Nc), float("nan"), device=self.dev) if weights else None
        st, prep = self.native.struct()
        with torch.cuda.device(self.dev):
            rc = L.ngp_nav_run_resample(ctypes.byref(st), H.ptr(prep), H.ptr(r["o"]), H.ptr(r["d"]), H.ptr(r["nears"]), H.ptr(r["fars"]), r["N"], Nc, Nf,
                                        self.aabb, H.ptr(z), H.ptr(w), H.stream())
        assert rc == 0, L.ngp_last_error()
        return z, w

    def forward(self, r, z, Nc, keep=True):
        H, L = self.H, self.L
        N, T = z.shape
        image, depth, ws = torch.full((N, 3), -7.0, device=self.dev), torch.full((N,), -7.0, device=self.dev), torch.full((N,), -7.0, device=self.dev)
        saved = H.workspace(L.ngp_nav_run_saved_bytes(N, T), self.dev) if keep else None
        st, prep = self.native.struct()
        with torch.cuda.device(self.dev):
            rc = L.ngp_nav_run_at_forward(ctypes.byref(st), H.ptr(prep), H.ptr(r["o"]), H.ptr(r["d"]), H.ptr(r["nears"]), H.ptr(r["fars"]), N, T, self.aabb,
                                          self.bg, H.ptr(image), H.ptr(depth), H.ptr(ws), H.ptr(saved), saved.numel() if keep else 0, H.ptr(z), Nc,
                                          H.stream())
        assert rc == 0, L.ngp_last_error()
        return dict(image=image, depth=depth, weights_sum=ws, saved=saved)

    def backward(self, r, z, Nc, f, G, Gd, Gw):
        H, L = self.H, self.L
        N, T = z.shape
        go, gd = torch.full_like(r["o"], -7.0), torch.full_like(r["d"], -7.0)
        st, prep = self.native.struct()
        dv = lambda a: None if a is None else t(a, self.dev)                     # noqa: E731
        gi, gde, gw = dv(G), dv(Gd), dv(Gw)
        with torch.cuda.device(self.dev):
            rc = L.ngp_nav_run_at_backward(ctypes.byref(st), H.ptr(prep), H.ptr(r["o"]), H.ptr(r["d"]), H.ptr(r["nears"]), H.ptr(r["fars"]), N, T, self.aabb,
                                           self.bg, H.ptr(gi), H.ptr(gde), H.ptr(gw), H.ptr(f["saved"]), f["saved"].numel(), H.ptr(go), H.ptr(gd), H.ptr(z),
                                           Nc, H.stream())
        assert rc == 0, L.ngp_last_error()
        torch.cuda.synchronize()
        return go, gd


# ------------------------------------------------------------------------------------------------------------------------
# 1. ngp_sample_pdf against the restatement, bit for bit
# ------------------------------------------------------------------------------------------------------------------------
def gpu_sample_pdf(dev, bins, wts, n, u=None):
    import ngp_hip as H
    N, Tb = bins.shape
    out = torch.full((N, n), float("nan"), device=dev)
    b, w, uu = t(bins, dev), t(wts, dev), None if u is None else t(u, dev)
    with torch.cuda.device(dev):
        rc = H.lib().ngp_sample_pdf(H.ptr(b), H.ptr(w), N, Tb, H.ptr(uu), n, H.ptr(out), H.stream())
    assert rc == 0, H.lib().ngp_last_error()
    return out.cpu().numpy()


def test_sample_pdf_on_the_recorded_vectors(dev):
    g = np.load(os.path.join(ROOT, "tests", "golden", "callers_tier1.npz"))
    bins, wts, n = g["pdf_bins"], g["pdf_weights"], g["pdf_det"].shape[1]
    det = gpu_sample_pdf(dev, bins, wts, n)
    assert np.array_equal(bits_of(det), bits_of(RS.sample_pdf(bins, wts, n)))
    rand = gpu_sample_pdf(dev, bins, wts, n, g["pdf_u"])
    assert np.array_equal(bits_of(rand), bits_of(RS.sample_pdf(bins, wts, n, u=g["pdf_u"])))
    e_det, e_rand = float(np.max(np.abs(det - g["pdf_det"]))), float(np.max(np.abs(rand - g["pdf_rand"])))
    print(f"ngp_sample_pdf against the recorded sample_pdf: det {e_det:.3g}, rand {e_rand:.3g} (allowed 5e-5)")
    assert e_det < 5e-5 and e_rand < 5e-5


@functools.lru_cache(maxsize=None)
def constructed(Tb):
    """bins [5,Tb] and weights [5,Tb-1]: all zero, one spike, a spike in the first bin, a spike in the last bin, random"""
    rng = np.random.default_rng(100 + Tb)
    bins = np.sort(rng.uniform(0.2, 6.0, size=(5, Tb)).astype(F), axis=1)
    wts = np.zeros((5, Tb - 1), F)
    wts[1, (Tb - 1) // 2] = 1.0
    wts[2, 0] = 1.0
    wts[3, -1] = 1.0
    wts[4] = rng.uniform(0, 1, Tb - 1).astype(F)
    return bins, wts


@pytest.mark.parametrize("n", [1, 5, 64, 257])
def test_sample_pdf_on_constructed_weights(dev, n):
    """Tb = 2 is one bin; 256 / 257 / 258 weights straddle one weight per thread; 4096 is the largest row"""
    for Tb in (2, 3, 17, 257, 258, 259, 1000, 4096):
        bins, wts = constructed(Tb)
        got = gpu_sample_pdf(dev, bins, wts, n)
        ref = RS.sample_pdf(bins, wts, n)
        assert np.array_equal(bits_of(got), bits_of(ref)), (Tb, n, float(np.nanmax(np.abs(got - ref))))
        assert (np.diff(got, axis=1) >= 0).all() and (got >= bins[:, :1]).all() and (got <= bins[:, -1:]).all(), (Tb, n)
        u = np.random.default_rng(n).uniform(0, 1, size=(5, n)).astype(F)
        u[0, 0], u[1, 0] = 0.0, 1.0                                      # the ends of the cdf
        assert np.array_equal(bits_of(gpu_sample_pdf(dev, bins, wts, n, u)), bits_of(RS.sample_pdf(bins, wts, n, u=u))), (Tb, n, "u")


# ------------------------------------------------------------------------------------------------------------------------
# 2. ngp_nav_run_resample
# ------------------------------------------------------------------------------------------------------------------------
_GPU = {}


def gpu_resample(dev, name):
    """the case's rays through ngp_nav_run_resample once: dict(ops, rays, z, w (device), z_np, w_np, near, far)"""
    if name not in _GPU:
        case = RA.RES_CASES[name]
        ops = Ops(dev, case)
        o, d, miss = C.case_rays(case)
        r = ops.rays(o, d)
        z, w = ops.resample(r, case["T"], case["Nf"])
        torch.cuda.synchronize()
        _GPU[name] = dict(ops=ops, rays=r, z=z, w=w, z_np=z.cpu().numpy(), w_np=w.cpu().numpy(), near=r["nears"].cpu().numpy(), far=r["fars"].cpu().numpy(),
                          miss=miss)
    return _GPU[name]


@pytest.mark.parametrize("name", list(RA.RES_CASES))
def test_resample_against_the_restatement_and_the_pinned_weights(dev, oracle, name):
    case = RA.RES_CASES[name]
    Nc, Nf = case["T"], case["Nf"]
    g = gpu_resample(dev, name)
    o, d, miss = C.case_rays(case)
    n_ref, f_ref = RS.near_far(o, d, case["bound"], case["min_near"])
    assert np.array_equal(bits_of(g["near"]), bits_of(n_ref)) and np.array_equal(bits_of(g["far"]), bits_of(f_ref))
    # the coarse weights, absolutely, every ray
    cr = RA.coarse_reference(name)
    everyone = np.ones(o.shape[0], bool)
    C.judge(f"{name} coarse", g["w_np"], cr["ref"], cr["e32"], everyone, "weights", floor=C.carry_floor(Nc))
    # z: the restatement applied to the kernel's own float32 weights, bit for bit
    z_ref, zc, zn = RS.resample(g["near"], g["far"], g["w_np"], Nf)
    assert np.isfinite(g["z_np"]).all()
    assert np.array_equal(bits_of(g["z_np"]), bits_of(z_ref)), (name, int((bits_of(g["z_np"]) != bits_of(z_ref)).sum()))
    assert (np.diff(g["z_np"], axis=1) >= 0).all()
    # the Nc coarse depths inside z are the dense lattice's
    for r in range(o.shape[0]):
        rank = np.arange(Nc) + (zn[r][None, :] < zc[r][:, None]).sum(axis=1)
        assert np.array_equal(bits_of(g["z_np"][r, rank]), bits_of(zc[r])), (name, r)
    assert np.array_equal(bits_of(zc), bits_of(RS.coarse_z(n_ref, f_ref, Nc)))
    assert (zn >= zc[:, :1]).all() and (zn <= zc[:, -1:]).all()
    # the miss: T copies of near, zero weights
    assert np.array_equal(bits_of(g["z_np"][miss]), bits_of(np.full(Nc + Nf, n_ref[miss], F))) and (g["w_np"][miss] == 0).all()
    # the weights are optional and change nothing
    z2, _ = g["ops"].resample(g["rays"], Nc, Nf, weights=False)
    assert torch.equal(z2.view(torch.int32), g["z"].view(torch.int32))


def test_a_ray_alone_resamples_to_the_same_bits(dev):
    name = "r257_130"
    case = RA.RES_CASES[name]
    g = gpu_resample(dev, name)
    o, d, _ = C.case_rays(case)
    for at in (0, 5, o.shape[0] - 1):
        r1 = g["ops"].rays(o[at:at + 1], d[at:at + 1])
        z1, w1 = g["ops"].resample(r1, case["T"], case["Nf"])
        assert torch.equal(z1.view(torch.int32), g["z"][at:at + 1].view(torch.int32)) and torch.equal(w1.view(torch.int32), g["w"][at:at + 1].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------
# 3. the run over an explicit depth list
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RA.RES_CASES))
def test_run_at_against_the_float64_pass_at_the_same_depths(dev, oracle, name):
    case = RA.RES_CASES[name]
    Nc, T = case["T"], case["T"] + case["Nf"]
    g = gpu_resample(dev, name)
    ops, r, z = g["ops"], g["rays"], g["z"]
    N = r["N"]
    G, Gd, Gw = C.loss_weights(N)
    f = ops.forward(r, z, Nc)
    go, gd = ops.backward(r, z, Nc, f, G if "image" in case["terms"] else np.zeros_like(G), Gd if "depth" in case["terms"] else None,
                          Gw if "weights_sum" in case["terms"] else None)
    got = {k: f[k].cpu().numpy() for k in ("image", "depth", "weights_sum")}
    got["grad_o"], got["grad_d"] = go.cpu().numpy(), gd.cpu().numpy()
    ref = RA.at_reference(case, g["z_np"])
    miss = ref["miss"]
    everyone = np.ones(N, bool)
    worst = {}
    for k in ("image", "weights_sum", "depth"):
        worst[k] = C.judge(name, got[k], ref["ref"][k], ref["e32"][k], everyone, k, floor=C.carry_floor(T))
    assert np.isfinite(got["image"]).all() and np.isfinite(got["weights_sum"]).all() and np.isfinite(np.delete(got["depth"], miss)).all()
    for k in ("grad_o", "grad_d"):
        worst[k] = C.judge(name, got[k], ref["ref"][k], ref["e32"][k], ref["judged"], k)
    print(f"TABLE {name:20s} " + " ".join(f"{worst[k]:7.2f}" for k in ("image", "weights_sum", "depth", "grad_o", "grad_d")))
    # the miss: the background, zeros, zero gradients; nothing NaN
    assert np.array_equal(got["image"][miss], np.array(bg3(case), F)) and got["weights_sum"][miss] == 0 and got["depth"][miss] == 0
    assert not got["grad_o"][miss].any() and not got["grad_d"][miss].any()
    assert np.isfinite(got["grad_o"]).all() and np.isfinite(got["grad_d"]).all()
    # saved = NULL gives the same forward; a second run the same bits
    f2 = ops.forward(r, z, Nc, keep=False)
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(f2[k].view(torch.int32), f[k].view(torch.int32)), k


def test_run_at_over_the_dense_lattice_is_the_dense_run(dev):
    """the explicit-list instantiation given the lattice's own depths and dist_steps = T is ngp_nav_run_forward / _backward bit for bit"""
    from ngp import nav
    case = C.RUN_CASES["contrast"]
    ops = Ops(dev, case)
    o, d, _ = C.rays(case["bound"], 16)
    r = ops.rays(o, d)
    T = case["T"]
    z = t(RS.coarse_z(r["nears"].cpu().numpy(), r["fars"].cpu().numpy(), T), dev)
    G, Gd, Gw = C.loss_weights(16)
    f = ops.forward(r, z, T)
    go, gd = ops.backward(r, z, T, f, G, Gd, Gw)
    ro, rd = r["o"].clone().requires_grad_(True), r["d"].clone().requires_grad_(True)
    image, depth, ws = nav._nav_run.apply(ro, rd, ops.native, T, bg3(case))
    ((image * t(G, dev)).sum() + (depth * t(Gd, dev)).sum() + (ws * t(Gw, dev)).sum()).backward()
    for a, b in ((f["image"], image), (f["depth"], depth), (f["weights_sum"], ws), (go, ro.grad), (gd, rd.grad)):
        assert np.array_equal(bits_of(a), bits_of(b))


# ------------------------------------------------------------------------------------------------------------------------
# 4. end to end: render_fn_resampled against the float64 oracle with its own depths
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64), (128, 128)])
def test_render_fn_resampled_end_to_end(dev, oracle, shape):
    from ngp import nav
    from oracle import callers_oracle as CO
    Nc, Nf = shape
    case = C._run_case(field="contrast", T=Nc, count=16)
    ren, _ = case_rig(dev, case)
    q = nav.NativeNavQueries(ren, (20.0, 20.0, 8.0, 8.0), 16, 16, num_steps=Nc)
    o, d, miss = C.case_rays(case)
    ro, rd = t(o, dev)[None].requires_grad_(True), t(d, dev)[None].requires_grad_(True)
    out = q.render_fn_resampled(ro, rd, Nf)
    (out["image"].sum() + out["depth"].sum()).backward()
    assert bool(torch.isfinite(ro.grad).all()) and bool(torch.isfinite(rd.grad).all()) and float(ro.grad.abs().sum()) > 0
    img, ws_t = nav._nav_run_resampled.apply(t(o, dev), t(d, dev), q.native, Nc, Nf, (1.0, 1.0, 1.0))[::2]
    got = dict(image=out["image"][0].detach().cpu().numpy(), depth=out["depth"][0].detach().cpu().numpy(), weights_sum=ws_t.cpu().numpy())
    assert np.array_equal(bits_of(img), bits_of(got["image"]))          # no gradient asked: no record kept, the same forward
    res = {}
    for dtype in (torch.float64, torch.float32):
        with torch.no_grad():
            r = CO.run(C.oracle_field("contrast", case["bound"], dtype), torch.from_numpy(o).to(dtype), torch.from_numpy(d).to(dtype), case["bound"],
                       num_steps=Nc, upsample_steps=Nf, min_near=case["min_near"])
        res[dtype] = {k: r[k].numpy() for k in ("image", "depth", "weights_sum")}
    with torch.no_grad():
        chain = ren.run(t(o, dev)[None], t(d, dev)[None], num_steps=Nc, upsample_steps=Nf, bg_color=1)
    everyone = np.ones(o.shape[0], bool)
    for k in ("image", "depth", "weights_sum"):
        e32 = C.row_error(res[torch.float32][k], res[torch.float64][k], k)
        other = chain[k].reshape(-1, *got[k].shape[1:]).cpu().numpy() if k in chain else None
        if other is not None:
            with np.errstate(invalid="ignore"):
                print(f"end to end {shape} {k}: largest difference from NGPRenderer.run on the GPU {np.nanmax(np.abs(other - got[k])):.3g}")
        C.judge(f"end to end {shape}", got[k], res[torch.float64][k], e32, everyone, k, floor=C.carry_floor(Nc + Nf))
    with pytest.raises(ValueError):
        q.render_fn_resampled(ro, rd, 0)
    with pytest.raises(ValueError):
        nav.NativeNavQueries(ren, (20.0, 20.0, 8.0, 8.0), 16, 16, num_steps=Nc, upsample_steps=Nf)       # the constructor keeps refusing


# ------------------------------------------------------------------------------------------------------------------------
# 5. the filter's resampled route
# ------------------------------------------------------------------------------------------------------------------------
H = W = 20
LR = 1e-3
FB, FT, FU = 64, 64, 32


@pytest.fixture(scope="module")
def queries(dev):
    """tests/test_gpu_nav_filter.py's scene (NGPField + workload.nav_weights(0), 20 x 20 pixels, 64 steps) on a renderer WITHOUT an occupancy grid"""
    from ngp import nav
    from ngp import workload as Wl
    from ngp.field import NGPField
    from ngp.render import NGPRenderer
    g = NC.gold()
    model = Wl.make_model(0)
    sw, cw = Wl.nav_weights(0)
    field = NGPField(bound=Wl.BOUND).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(model["embeddings"]))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            layer.weight.copy_(torch.from_numpy(w))
    ren = NGPRenderer(field, bound=Wl.BOUND, cuda_ray=False).to(dev).eval()
    for p in ren.parameters():
        p.requires_grad_(False)
    assert tuple(int(v) for v in g["mf_HW"]) == (H, W) and int(g["mf_num_steps"]) == FT
    return nav.NativeNavQueries(ren, g["mf_intrinsics"], H, W, num_steps=FT)


def gold_t(dev):
    g = NC.gold()
    return {k: torch.from_numpy(g[f"mf_{k}"]).to(dev) for k in ("state", "start", "sig", "target")}


def make_filter(queries, B=FB, n_iter=3, **kw):
    from ngp import nav
    return nav.NativePoseFilter({"batch_size": B, "lrate": LR, "N_iter": n_iter, "sig0": torch.eye(12), "Q": torch.eye(12)}, queries, **kw)


def all_pixels():
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([rows.ravel(), cols.ravel()], -1)


def loop(filt, g, batches, update, dev):
    state = g["start"].clone() + 1e-6
    kw = dict(dtype=torch.float32, device=dev)
    losses, states, grads = torch.empty(3, **kw), torch.empty(3, 12, **kw), torch.empty(3, 12, **kw)
    filt.run_iterations(0, 3, filt.new_adam_state(), state, g["start"], g["sig"], g["target"], batches, update=bool(update), losses=losses, states=states,
                        grads=grads)
    return dict(final=state, losses=losses, states=states, grads=grads)


@pytest.fixture(scope="module")
def res_loop(queries, dev):
    """three iterations of the resampled loop at B = 64, 64 + 32 samples, update = 1 and update = 0, all records kept; shared and left unchanged"""
    g = gold_t(dev)
    filt = make_filter(queries, sampling="resampled", upsample_steps=FU)
    batches = filt.draw_batches(all_pixels(), 3, np.random.default_rng(7))
    return dict(filt=filt, batches=batches, runs={u: loop(filt, g, batches, u, dev) for u in (1, 0)}, **g)


def test_filter_loop_is_the_ops_in_order_and_two_runs_agree(queries, res_loop, dev):
    """iteration 0's loss is the mean squared error of render_fn_resampled at the filter's rays plus the Mahalanobis term (zero at the start state up to
    the 1e-6 shift); a second loop gives the same bits; the objective is not the dense one"""
    L, filt = res_loop, res_loop["filt"]
    for u in (1, 0):
        again = loop(filt, L, L["batches"], u, dev)
        for k in ("final", "losses", "states", "grads"):
            assert torch.equal(again[k], L["runs"][u][k]), (u, k)
    run = L["runs"][1]
    assert bool(torch.isfinite(run["losses"]).all()) and bool(torch.isfinite(run["grads"]).all())
    assert float((run["states"][1:] - run["states"][:-1]).abs().max()) > 0.5 * LR
    assert torch.equal(L["runs"][0]["states"][1], L["runs"][0]["states"][0])
    state = L["start"] + 1e-6
    rays = filt.rays(state, L["batches"][0])
    out = queries.render_fn_resampled(rays["rays_o"][None], rays["rays_d"][None], FU)
    b = L["batches"][0].long()
    mse = ((out["image"][0] - L["target"][b[:, 0], b[:, 1]]) ** 2).mean()
    cg = filt.cost_and_gradient(state, L["start"], L["sig"], L["target"], L["batches"][0])
    np.testing.assert_allclose(float(cg["rgb_loss"]), float(mse), rtol=1e-4)     # tests/test_gpu_nav_filter.py's bar for the loss
    assert torch.equal(cg["loss"], L["runs"][0]["losses"][0]) and torch.equal(cg["grad"], L["runs"][0]["grads"][0])
    dense = make_filter(queries).cost_and_gradient(state, L["start"], L["sig"], L["target"], L["batches"][0])
    assert not torch.equal(dense["loss"], cg["loss"])


def test_three_hypotheses_are_three_single_runs(queries, res_loop, dev):
    L, filt = res_loop, res_loop["filt"]
    K = 3
    offsets = torch.from_numpy(np.random.default_rng(5).uniform(-0.02, 0.02, (K, 12)).astype(np.float32)).to(dev)
    offsets[0] = 0
    kw = dict(dtype=torch.float32, device=dev)
    for update in (True, False):
        states = ((L["start"][None] + offsets) + 1e-6).contiguous()
        first = states.clone()
        losses, hist, grads = torch.empty(3, K, **kw), torch.empty(3, K, 12, **kw), torch.empty(3, K, 12, **kw)
        filt.run_iterations_multi(0, 3, filt.new_adam_state_multi(K), states, L["start"], L["sig"], L["target"], L["batches"], update=update, losses=losses,
                                  states_out=hist, grads=grads)
        for k in range(K):
            one = first[k].clone()
            l1, s1, g1 = torch.empty(3, **kw), torch.empty(3, 12, **kw), torch.empty(3, 12, **kw)
            filt.run_iterations(0, 3, filt.new_adam_state(), one, L["start"], L["sig"], L["target"], L["batches"], update=update, losses=l1, states=s1, grads=g1)
            assert torch.equal(one, states[k]) and torch.equal(l1, losses[:, k]) and torch.equal(s1, hist[:, k]) and torch.equal(g1, grads[:, k]), (update, k)
        assert not torch.equal(losses[:, 1], losses[:, 0])
    run = L["runs"][0]                                               # the zero offset is the single run of the fixture
    assert torch.equal(losses[:, 0], run["losses"]) and torch.equal(grads[:, 0], run["grads"])


def test_hessian_res_gradient_and_loss_are_an_update_zero_iteration(queries, res_loop):
    L, filt = res_loop, res_loop["filt"]
    state = L["start"] + 1e-6
    res = filt.hessian_and_gradient(state, L["start"], L["sig"], L["target"], L["batches"][0])
    run = L["runs"][0]
    assert torch.equal(res["grad"], run["grads"][0]) and torch.equal(res["loss"], run["losses"][0])
    Hs = res["hessian"]
    assert bool(torch.isfinite(Hs).all()) and float(Hs[6:9, 6:9].abs().max()) > 0


def test_set_sampling_round_trips_leave_dense_untouched(queries, dev):
    g = gold_t(dev)
    plain = make_filter(queries)
    batches = plain.draw_batches(all_pixels(), 3, np.random.default_rng(7))
    want = loop(plain, g, batches, 1, dev)
    filt = make_filter(queries)
    filt.set_sampling("resampled", upsample_steps=FU)
    mid = loop(filt, g, batches, 1, dev)
    filt.set_sampling("dense")
    got = loop(filt, g, batches, 1, dev)
    filt.set_sampling("resampled", upsample_steps=5)
    filt.set_sampling("dense")
    got2 = loop(filt, g, batches, 1, dev)
    for k in ("final", "losses", "states", "grads"):
        assert torch.equal(got[k], want[k]) and torch.equal(got2[k], want[k]), k
    assert not torch.equal(mid["losses"], want["losses"])
    for word in ("sparse", "occupied"):                              # "occupied" needs a grid this renderer does not hold
        with pytest.raises(ValueError):
            filt.set_sampling(word)
    assert filt.sampling == "dense"


def test_estimate_state_end_to_end(queries, dev):
    from ngp import nav
    gold = np.load(os.path.join(ROOT, "tests", "golden", "callers_estimator.npz"))
    dt, mass, grav = (float(v) for v in gold["generic_cfg"])
    agent = {"dt": dt, "mass": mass, "g": grav, "I": torch.from_numpy(gold["generic_I"])}
    g = gold_t(dev)
    Q = torch.diag(torch.from_numpy(np.random.default_rng(3).uniform(0.005, 0.02, 12).astype(np.float32)))
    cfg = {"batch_size": 16, "lrate": LR, "N_iter": 4, "sig0": g["sig"].cpu(), "Q": Q}
    action = torch.tensor([10.1, 0.01, -0.02, 0.015])
    filt = nav.NativePoseFilter(cfg, queries, g["start"].clone(), agent, sampling="resampled", upsample_steps=FU)
    xt = filt.estimate_state(g["target"], action, all_pixels(), rng=np.random.default_rng(50))
    assert xt.is_cuda and bool(torch.isfinite(xt).all()) and bool(torch.isfinite(filt.sig).all()) and tuple(filt.losses.shape) == (4,)
    np.linalg.cholesky(filt.sig.double().cpu().numpy())
    single = filt.losses.clone()
    filt = nav.NativePoseFilter(cfg, queries, g["start"].clone(), agent, sampling="resampled", upsample_steps=FU)
    offsets = torch.zeros(2, 12)
    offsets[1, :3] = 0.01
    xt = filt.estimate_state(g["target"], action, all_pixels(), rng=np.random.default_rng(50), offsets=offsets)
    assert bool(torch.isfinite(xt).all()) and torch.equal(filt.multi["losses"][:, 0], single)


# ------------------------------------------------------------------------------------------------------------------------
# 6. the closed loop passes the option through
# ------------------------------------------------------------------------------------------------------------------------
from test_gpu_agent import loop_cfgs, same_bits  # noqa: E402
from test_gpu_plan_astar import scene  # noqa: E402,F401


def test_simulate_runs_the_resampled_filter_to_the_end(queries, dev, scene, tmp_path):  # noqa: F811
    from ngp import nav
    run = lambda **kw: nav.simulate(*loop_cfgs(dev, scene), queries, generator=torch.Generator(device=dev).manual_seed(11),      # noqa: E731
                                    interest_regions=all_pixels(), seed=5, **kw)
    plain = run()
    res = run(filter_sampling="resampled", filter_upsample_steps=FU, basefolder=tmp_path / "run")
    steps = res["estimates"].shape[0]
    assert plain["filter"].sampling == "dense" and res["filter"].sampling == "resampled" and res["filter"].upsample_steps == FU
    assert steps >= 1 and res["filter"].iteration == steps and tuple(res["true_states"].shape) == (steps + 1, 12)
    assert bool(torch.isfinite(res["estimates"]).all()) and bool(torch.isfinite(res["true_states"]).all())
    assert not same_bits(res["estimates"], plain["estimates"])       # the sensor is the same, the filter's objective is another
    base = tmp_path / "run"
    found = sorted(str(p.relative_to(base)) for p in base.rglob("*") if p.is_file())
    assert "true_states.json" in found and all(f"estimator_data/step{n}.json" in found for n in range(steps))
    with pytest.raises(ValueError, match="upsample_steps"):
        run(filter_sampling="resampled")
