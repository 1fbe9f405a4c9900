"""GPU: the occupancy-masked run (csrc/nav_field.hip: k_nav_run_occ_fwd / _bwd) and the pose filter's occupied route (ngp_filter_iterations_occ,
ngp_filter_hessian_occ, NativePoseFilter(sampling="occupied")).  DESIGN.md 3.5 "Occupancy-masked pose filter".

The kernels are held to the masked pinned float64 reference of tests/_run_occ_cases.py, ray by ray, by the dense kernels' rule (_nav_pinned_cases.judge,
MARGIN = 16, left_out), with a carry floor worked out for the new kernel's 64-sample chunks and each ray's own occupied count; what makes that
reference a fair yardstick is checked on the CPU by tests/test_run_occ_host.py.  Each check prints its largest error / yardstick (run with -s).

First run (MI355X; 50 tests, 9 s, most of it the CPU references).  Largest error / yardstick over the nine cases, margin 16:
  bitfield                       image  weights_sum  depth  grad_o  grad_d
  all ones (masked reference)     3.17     3.22       2.32   5.68    3.87
  rand50                          2.78     3.17       2.29  12.11   13.42     (chunk_256 grad_o, contrast grad_d; contrast / long_513 with rays of 63, 64, 65)
  sparse                          3.40     2.84       2.13   2.38    2.37
  all ones (DENSE reference)      3.17     3.22       2.32   5.68    3.87
  filter, B = 64, T = 64: loss <= 9.2e-8 relative, gradient <= 2.9e-7 relative against autograd of the restatement (bars 1e-4, 2e-3)"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

import _nav_cases as NC  # noqa: E402
import _nav_pinned_cases as C  # noqa: E402
import _run_occ_cases as RO  # noqa: E402
from oracle import nav_oracle as NO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("tiny_1", "tiny_2", "tiny_3", "chunk_255", "chunk_256", "contrast", "long_513", "bound_1", "scale_2")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits_of(a):
    return a.detach().cpu().numpy().view(np.uint32)


_RIGS = {}


def rig(dev, case, bits):
    """(renderer with a 32^3 grid per cascade holding `bits`, ngp.nav._NativeField); one renderer per field / bound / scale, its bitfield rewritten"""
    from ngp import nav
    from ngp.render import NGPRenderer
    key = (case["field"], case["bound"], case["density_scale"], case["min_near"])
    if key not in _RIGS:
        ren = NGPRenderer(C.product_field(case["field"], case["bound"], dev), bound=case["bound"], cuda_ray=True, density_scale=case["density_scale"],
                          min_near=case["min_near"], grid_size=RO.H_GRID).to(dev).eval()
        for p in ren.parameters():
            p.requires_grad_(False)
        assert ren.cascade == RO.cascades(case["bound"])
        _RIGS[key] = (ren, nav._NativeField(ren))
    ren, native = _RIGS[key]
    ren.density_bitfield.copy_(t(np.array(bits), dev))               # a copy: the cached bitfields are read-only
    return ren, native


def bg3(case):
    return tuple(float(v) for v in (case["bg"] if not np.isscalar(case["bg"]) else (case["bg"],) * 3))


def gpu_run(dev, case, bits, rows=None, dense=False):
    """the case through ngp.nav._nav_run_occ (one launch forward, one backward) -> numpy dict like _run_occ_cases.masked_run's, plus counts.
    dense: through ngp.nav._nav_run on the same renderer instead (the counts stay as they were filled)"""
    from ngp import nav
    o, d, _ = C.case_rays(case)
    G, Gd, Gw = C.loss_weights(o.shape[0])
    if rows is not None:
        o, d, G, Gd, Gw = o[rows], d[rows], G[rows], Gd[rows], Gw[rows]
    _, native = rig(dev, case, bits)
    ro, rd = t(o, dev).requires_grad_(True), t(d, dev).requires_grad_(True)
    counts = torch.full((o.shape[0],), -7, dtype=torch.int32, device=dev)
    if dense:
        image, depth, ws = nav._nav_run.apply(ro, rd, native, case["T"], bg3(case))
    else:
        image, depth, ws = nav._nav_run_occ.apply(ro, rd, native, case["T"], bg3(case), counts)
    loss = 0
    if "image" in case["terms"]:
        loss = loss + (image * t(G, dev)).sum()
    if "depth" in case["terms"]:
        loss = loss + (depth * t(Gd, dev)).sum()
    if "weights_sum" in case["terms"]:
        loss = loss + (ws * t(Gw, dev)).sum()
    loss.backward()
    return dict(image=image.detach().cpu().numpy(), depth=depth.detach().cpu().numpy(), weights_sum=ws.detach().cpu().numpy(),
                grad_o=ro.grad.cpu().numpy(), grad_d=rd.grad.cpu().numpy(), counts=counts.cpu().numpy())


def check(label, got, r):
    """counts exactly; image, depth, weights_sum of every ray and both gradients of the judged rays against the reference; exact zeros where the
    reference's gradient is exactly zero"""
    assert np.array_equal(got["counts"], r["counts"]), (label, np.flatnonzero(got["counts"] != r["counts"])[:8], got["counts"][:8], r["counts"][:8])
    worst = {k: RO.judge_absolute(label, got, r, k) for k in ("image", "weights_sum", "depth")}
    assert np.isfinite(got["image"]).all() and np.isfinite(got["weights_sum"]).all() and np.isfinite(np.delete(got["depth"], r["miss"])).all()
    for k in ("grad_o", "grad_d"):
        worst[k] = C.judge(label, got[k], r["ref"][k], r["e32"][k], r["judged"], k)
        zero = r["zero"][k] & r["hit"]
        assert np.all(got[k][zero] == 0), (label, k, np.flatnonzero(zero & (np.abs(got[k]).sum(axis=1) > 0)))
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# 1, 2. counts and the five outputs against the masked pinned reference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", RO.BITFIELDS)
@pytest.mark.parametrize("name", CASES)
def test_run_against_the_masked_pinned_reference(dev, name, bf):
    r = RO.occ_reference(name, bf)
    got = gpu_run(dev, r["case"], r["bits"])
    if (name, bf) in RO.STRADDLE:                                    # rays of 63, 64 and 65 occupied samples: one chunk short, one full, two
        rows = RO.straddle_rays(name)
        for count in RO.STRADDLE_COUNTS:
            assert len(rows[count]) >= 1 and np.all(got["counts"][rows[count]] == count)
    worst = check(f"{name} {bf}", got, r)
    print(f"{name} {bf}: mean occupied {r['counts'].mean():.1f} of {r['case']['T']}; worst ratios " + " ".join(f"{k} {v:.2f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------------------
# 3. nothing occupied
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_1", "contrast", "long_513", "bound_1"])
def test_empty_grid_gives_the_background_and_exact_zeros(dev, name):
    case = dict(C.RUN_CASES[name], bg=C.BG)
    got = gpu_run(dev, case, RO.bitfield("zeros", case["bound"]))
    n = got["image"].shape[0]
    assert np.array_equal(got["image"].view(np.uint32), np.tile(np.asarray(C.BG, np.float32), (n, 1)).view(np.uint32))
    for k in ("depth", "weights_sum", "grad_o", "grad_d"):
        assert np.array_equal(got[k].view(np.uint32), np.zeros_like(got[k]).view(np.uint32)), k      # +0, every ray, the miss too
    assert np.all(got["counts"] == 0)


# ------------------------------------------------------------------------------------------------------------------------
# 4. everything occupied: the dense pinned reference, unchanged
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_full_grid_against_the_dense_pinned_reference(dev, name):
    d = C.run_reference(name)
    case = d["case"]
    n = len(d["hit"])
    zero = {k: np.zeros(n, bool) for k in ("grad_o", "grad_d")}
    r = dict(d, counts=np.full(n, case["T"], np.int64), zero=zero)
    got = gpu_run(dev, case, RO.bitfield("ones", case["bound"]))
    worst = check(f"{name} dense reference", got, r)
    print(f"{name} against run_reference: worst ratios " + " ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("T", [1, 3, 63, 64])
def test_full_grid_and_one_chunk_is_the_dense_run_bit_for_bit(dev, T):
    """Every cell occupied and T <= 64: the compacted list is the lattice and fits one chunk, so the one-wave kernels and the four-wave kernels run the
    one per-sample body (nv_run_sample_fwd / _bwd of csrc/nav_field.hip) on the same numbers.  In the dense kernels only wave 0 holds live samples; the
    other waves hand the team scans exact 1.0f factors and +0.0f terms, and a lane's sums start at +0, so no rounding and no sign of zero differs."""
    case = C._run_case(field="contrast", T=T, count=16)
    bits = RO.bitfield("ones", case["bound"])
    occ, dense = gpu_run(dev, case, bits), gpu_run(dev, case, bits, dense=True)
    assert np.all(occ["counts"] == T)
    for k in ("image", "depth", "weights_sum", "grad_o", "grad_d"):
        assert np.array_equal(occ[k].view(np.uint32), dense[k].view(np.uint32)), (k, np.flatnonzero((occ[k] != dense[k]).reshape(16, -1).any(axis=1)))
    assert T < 63 or (np.abs(occ["grad_d"]).sum() > 0 and occ["weights_sum"].max() > 0.5)      # the rays do hit something


# ------------------------------------------------------------------------------------------------------------------------
# 5. two runs, and a ray alone
# ------------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_ray_alone_give_the_same_bits(dev):
    name, bf = "contrast", "rand50"
    r = RO.occ_reference(name, bf)
    case, bits = r["case"], r["bits"]
    a, b = gpu_run(dev, case, bits), gpu_run(dev, case, bits)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    rows = RO.straddle_rays(name)
    n = len(r["hit"])
    picks = [int(rows[c][0]) for c in RO.STRADDLE_COUNTS] + [0, 40, n - 1, r["miss"]]
    for at in picks:                                                 # the record's stride is N T for the batch and T alone
        one = gpu_run(dev, case, bits, rows=np.array([at]))
        for k in a:
            assert np.array_equal(a[k][at:at + 1].view(np.uint32), one[k].view(np.uint32)), (at, k)
    some = np.array(sorted(set(picks[:5])))                          # and a sub-batch, in another order of blocks
    sub = gpu_run(dev, case, bits, rows=some[::-1].copy())
    for k in a:
        assert np.array_equal(a[k][some[::-1]].view(np.uint32), sub[k].view(np.uint32)), k
    assert a["counts"].max() > RO.CHUNK and np.abs(a["grad_o"][picks[2]]).sum() > 0


def test_no_gradient_asked_keeps_no_record_and_gives_the_same_forward(dev):
    from ngp import nav
    r = RO.occ_reference("chunk_255", "rand50")
    case = r["case"]
    got = gpu_run(dev, case, r["bits"])
    o, d, _ = C.case_rays(case)
    _, native = rig(dev, case, r["bits"])
    with torch.no_grad():
        image, depth, ws = nav._nav_run_occ.apply(t(o, dev), t(d, dev), native, case["T"], bg3(case))
    assert np.array_equal(bits_of(image), got["image"].view(np.uint32)) and np.array_equal(bits_of(ws), got["weights_sum"].view(np.uint32))
    assert np.array_equal(bits_of(depth), got["depth"].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------
# 6, 7. the filter's occupied route
# ------------------------------------------------------------------------------------------------------------------------
H = W = 20
LR = 1e-3
FB, FT = 64, 64


@pytest.fixture(scope="module")
def queries(dev):
    """tests/test_gpu_nav_filter.py's scene (NGPField + workload.nav_weights(0), 20 x 20 pixels, 64 steps) on a renderer that holds the workload's grid"""
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
    ren = NGPRenderer(field, bound=Wl.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
    ren.load_density_grid(Wl.density_grid())
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


def restated(queries, filt, state, start, sig, target, batch):
    """loss and gradient by torch autograd of the restated measurement function (oracle/nav_oracle.py) over render_fn_occupied, at the rays the filter
    renders (tests/test_gpu_nav_filter.py's `restated` says why the rays are pinned) -- the masked run itself is held to its reference above"""
    x = state.detach().clone().requires_grad_(True)
    native = filt.rays(state, all_pixels())

    def pinned_rays_fn(pose):
        rays = dict(queries.get_rays_fn(pose))
        for key in ("rays_o", "rays_d"):
            v, n = rays[key], native[key].reshape(rays[key].shape)
            assert float((n - v.detach()).abs().max()) <= 5e-7
            rays[key] = v + (n - v).detach()
        return rays

    def render_fn(o, d):
        image, depth, _ = queries.render_fn_occupied(o[0], d[0])
        return {"image": image[None], "depth": depth[None]}

    loss = NO.measurement_loss(x, start, sig, target, batch.long(), pinned_rays_fn, render_fn)
    loss.backward()
    return float(loss.detach()), x.grad.cpu().numpy()


def check_against_restated(queries, filt, loss, grad, state, start, sig, target, batch, tag):
    """tests/test_gpu_nav_filter.py's bars: loss 1e-4 relative, gradient 2e-3 relative in norm"""
    ref_loss, ref_grad = restated(queries, filt, state, start, sig, target, batch)
    loss, grad = float(loss), grad.cpu().numpy()
    print(f"{tag}: loss {loss:.8g} vs {ref_loss:.8g} (rel {abs(loss - ref_loss) / abs(ref_loss):.2e}); gradient rel {NC.rel(grad, ref_grad):.2e}")
    np.testing.assert_allclose(loss, ref_loss, rtol=1e-4)
    assert NC.rel(grad, ref_grad) < 2e-3, NC.rel(grad, ref_grad)


@pytest.fixture(scope="module")
def occ_loop(queries, dev):
    """three iterations of the occupied loop at B = 64, T = 64, update = 1 and update = 0, all records kept; shared and left unchanged"""
    g = gold_t(dev)
    filt = make_filter(queries, sampling="occupied")
    batches = filt.draw_batches(all_pixels(), 3, np.random.default_rng(7))
    out = {}
    for update in (1, 0):
        state = g["start"].clone() + 1e-6
        kw = dict(dtype=torch.float32, device=dev)
        losses, states, grads = torch.empty(3, **kw), torch.empty(3, 12, **kw), torch.empty(3, 12, **kw)
        filt.run_iterations(0, 3, filt.new_adam_state(), state, g["start"], g["sig"], g["target"], batches, update=bool(update), losses=losses,
                            states=states, grads=grads)
        out[update] = dict(final=state, losses=losses, states=states, grads=grads)
    return dict(filt=filt, batches=batches, runs=out, **g)


@pytest.mark.parametrize("update", [0, 1])
def test_filter_iterations_occ_against_autograd_of_the_restatement(queries, occ_loop, update):
    run, L = occ_loop["runs"][update], occ_loop
    assert torch.equal(run["states"][0], L["start"] + 1e-6)
    if update:
        assert float((run["states"][1:] - run["states"][:-1]).abs().max()) > 0.5 * LR and not torch.equal(run["final"], run["states"][2])
    else:
        assert torch.equal(run["states"][1], run["states"][0]) and torch.equal(run["final"], run["states"][0])
    for k in range(3):
        check_against_restated(queries, L["filt"], run["losses"][k], run["grads"][k], run["states"][k], L["start"], L["sig"], L["target"], L["batches"][k],
                               tag=f"update {update} iteration {k}")


def test_the_occupied_objective_is_not_the_dense_one(queries, occ_loop, dev):
    """the grid does mask samples of these rays: the two routes give different losses at the same state and batch"""
    L = occ_loop
    dense = make_filter(queries)
    res = dense.cost_and_gradient(L["start"] + 1e-6, L["start"], L["sig"], L["target"], L["batches"][0])
    assert dense.sampling == "dense" and not torch.equal(res["loss"], L["runs"][0]["losses"][0])
    counts = torch.empty(FB, dtype=torch.int32, device=dev)
    rays = L["filt"].rays(L["start"] + 1e-6, L["batches"][0])
    queries.render_fn_occupied(rays["rays_o"], rays["rays_d"], counts)
    assert 0 < float(counts.float().mean()) < FT


def test_three_hypotheses_are_three_single_runs(queries, occ_loop, dev):
    L, filt = occ_loop, occ_loop["filt"]
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


def test_hessian_occ_gradient_and_loss_are_an_update_zero_iteration(queries, occ_loop):
    L, filt = occ_loop, occ_loop["filt"]
    state = L["start"] + 1e-6
    res = filt.hessian_and_gradient(state, L["start"], L["sig"], L["target"], L["batches"][0])
    run = L["runs"][0]
    assert torch.equal(res["grad"], run["grads"][0]) and torch.equal(res["loss"], run["losses"][0])
    cg = filt.cost_and_gradient(state, L["start"], L["sig"], L["target"], L["batches"][0])
    assert torch.equal(cg["grad"], res["grad"]) and torch.equal(cg["loss"], res["loss"])
    Hs = res["hessian"]
    assert bool(torch.isfinite(Hs).all()) and float(Hs[6:9, 6:9].abs().max()) > 0
    dense = make_filter(queries).hessian_and_gradient(state, L["start"], L["sig"], L["target"], L["batches"][0])
    assert not torch.equal(dense["grad"], res["grad"])


def test_estimate_state_end_to_end_and_dense_is_unchanged(queries, dev):
    from ngp import nav
    gold = np.load(os.path.join(ROOT, "tests", "golden", "callers_estimator.npz"))
    dt, mass, grav = (float(v) for v in gold["generic_cfg"])
    agent = {"dt": dt, "mass": mass, "g": grav, "I": torch.from_numpy(gold["generic_I"])}
    g = gold_t(dev)
    Q = torch.diag(torch.from_numpy(np.random.default_rng(3).uniform(0.005, 0.02, 12).astype(np.float32)))
    cfg = {"batch_size": 16, "lrate": LR, "N_iter": 4, "sig0": g["sig"].cpu(), "Q": Q}
    action = torch.tensor([10.1, 0.01, -0.02, 0.015])
    out = {}
    for tag, kw in (("plain", {}), ("dense", {"sampling": "dense"}), ("occupied", {"sampling": "occupied"})):
        filt = nav.NativePoseFilter(cfg, queries, g["start"].clone(), agent, **kw)
        xt = filt.estimate_state(g["target"], action, all_pixels(), rng=np.random.default_rng(50))
        assert xt.is_cuda and bool(torch.isfinite(xt).all()) and bool(torch.isfinite(filt.sig).all()) and tuple(filt.losses.shape) == (4,)
        np.linalg.cholesky(filt.sig.double().cpu().numpy())
        out[tag] = (xt, filt.losses.clone(), filt.grads.clone(), filt.sig.clone())
    for a, b in zip(out["plain"], out["dense"]):                     # the default route's bits, with and without the argument
        assert torch.equal(a, b)
    assert not torch.equal(out["occupied"][1], out["plain"][1])
    # multi-start on the occupied route
    filt = nav.NativePoseFilter(cfg, queries, g["start"].clone(), agent, sampling="occupied")
    offsets = torch.zeros(2, 12)
    offsets[1, :3] = 0.01
    xt = filt.estimate_state(g["target"], action, all_pixels(), rng=np.random.default_rng(50), offsets=offsets)
    assert bool(torch.isfinite(xt).all()) and torch.equal(filt.multi["losses"][:, 0], out["occupied"][1])


def test_c_abi_counts_are_optional_and_outputs_fully_written(dev):
    """ngp_nav_run_occ_forward directly: counts = NULL and saved = NULL change nothing else"""
    import raymarching
    import ngp_hip as Hh
    r = RO.occ_reference("chunk_256", "sparse")
    case = r["case"]
    ren, native = rig(dev, case, r["bits"])
    from ngp import nav
    grid, _bits = nav.occupancy_grid(ren)
    o, d, _ = C.case_rays(case)
    o, d = t(o, dev), t(d, dev)
    N, T = o.shape[0], case["T"]
    nears, fars = raymarching.near_far_from_aabb(o, d, ren._aabb(), ren.min_near)
    aabb = (ctypes.c_float * 6)(*[float(v) for v in ren._aabb().tolist()])
    st, prep = native.struct()
    L = Hh.lib()
    outs = []
    for with_counts, keep in ((True, True), (False, False)):
        image, depth, ws = torch.full((N, 3), -7.0, device=dev), torch.full((N,), -7.0, device=dev), torch.full((N,), -7.0, device=dev)
        counts = torch.full((N,), -7, dtype=torch.int32, device=dev)
        saved = Hh.workspace(L.ngp_nav_run_occ_saved_bytes(N, T), dev) if keep else None
        with torch.cuda.device(dev):
            rc = L.ngp_nav_run_occ_forward(ctypes.byref(st), Hh.ptr(prep), ctypes.byref(grid), Hh.ptr(o), Hh.ptr(d), Hh.ptr(nears), Hh.ptr(fars), N, T, aabb,
                                           None, Hh.ptr(image), Hh.ptr(depth), Hh.ptr(ws), Hh.ptr(counts) if with_counts else None, Hh.ptr(saved),
                                           saved.numel() if keep else 0, Hh.stream())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((image, depth, ws, counts))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert np.array_equal(bits_of(a), bits_of(b))
    assert np.array_equal(outs[0][3].cpu().numpy(), r["counts"]) and bool((outs[1][3] == -7).all())


# ------------------------------------------------------------------------------------------------------------------------
# 8. the closed loop passes the option through
# ------------------------------------------------------------------------------------------------------------------------
from test_gpu_agent import loop_cfgs, same_bits  # noqa: E402
from test_gpu_plan_astar import scene  # noqa: E402,F401


def test_simulate_passes_filter_sampling_through(queries, dev, scene):  # noqa: F811
    """tests/test_gpu_agent.py's closed loop on the renderer that holds the grid: filter_sampling="dense" is the loop without the argument bit for bit,
    "occupied" runs every time step's filter on the occupied route and ends finite"""
    from ngp import nav
    run = lambda **kw: nav.simulate(*loop_cfgs(dev, scene), queries, generator=torch.Generator(device=dev).manual_seed(11),      # noqa: E731
                                    interest_regions=all_pixels(), seed=5, **kw)
    plain, dense, occ = run(), run(filter_sampling="dense"), run(filter_sampling="occupied")
    for key in ("true_states", "estimates", "actions", "noises"):
        assert same_bits(plain[key], dense[key]), key
    steps = plain["estimates"].shape[0]
    assert plain["filter"].sampling == dense["filter"].sampling == "dense" and occ["filter"].sampling == "occupied"
    assert occ["filter"].iteration == steps and bool(torch.isfinite(occ["estimates"]).all()) and bool(torch.isfinite(occ["true_states"]).all())
    assert same_bits(occ["noises"], plain["noises"]) and not torch.equal(occ["estimates"], plain["estimates"])
    with pytest.raises(ValueError, match="sampling must be"):
        run(filter_sampling="sparse")
