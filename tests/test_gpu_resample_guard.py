"""GPU: guard bytes around every buffer the resampled run's ops are handed (tests/_guard.py's helpers as they are): z, coarse_weights, the saved record,
the filter's workspace and depth list, and every output, under two fills.  The guards stay intact, every output element is written, and the results do not
depend on what the buffers held.  The new entry points add no size function: the record is ngp_nav_run_saved_bytes(N, T), the filter's workspace
ngp_filter_multi_workspace(K, B, T), and the depth list's shape is stated in the header.  Then a kept workspace: a smaller (B, Nc, Nf) after a larger one
on one NativePoseFilter gives a fresh object's bits."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

import _nav_pinned_cases as C  # noqa: E402
import _run_at_cases as RA  # noqa: E402
from _guard import check_guarded, check_written, guarded, guarded_tensor, same_bits  # noqa: E402,F401
from test_gpu_resample import FU, all_pixels, case_rig, bg3, gold_t, loop, make_filter, queries  # noqa: E402,F401

FILLS = (0xAB, 0xFF)                                                     # a pattern no op writes; every float a NaN


def run_ops(dev, case, fill):
    """the four ops through the C ABI with every buffer between guard bytes -> the outputs"""
    import raymarching
    import ngp_hip as H
    L = H.lib()
    ren, native = case_rig(dev, case)
    o, d, _ = C.case_rays(case)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    N, Nc, Nf = o.shape[0], case["T"], case["Nf"]
    T = Nc + Nf
    nears, fars = raymarching.near_far_from_aabb(o, d, ren._aabb(), ren.min_near)
    aabb = (ctypes.c_float * 6)(*[float(v) for v in ren._aabb().tolist()])
    bg = (ctypes.c_float * 3)(*bg3(case))
    f32 = torch.float32
    z, w = guarded_tensor((N, T), f32, dev, fill), guarded_tensor((N, Nc), f32, dev, fill)
    image, depth, ws = guarded_tensor((N, 3), f32, dev, fill), guarded_tensor(N, f32, dev, fill), guarded_tensor(N, f32, dev, fill)
    go, gd = guarded_tensor((N, 3), f32, dev, fill), guarded_tensor((N, 3), f32, dev, fill)
    saved = guarded_tensor(L.ngp_nav_run_saved_bytes(N, T), torch.uint8, dev, fill)
    G, Gd, Gw = (torch.from_numpy(a).to(dev) for a in C.loss_weights(N))
    st, prep = native.struct()
    rays = (H.ptr(o), H.ptr(d), H.ptr(nears), H.ptr(fars))
    with torch.cuda.device(dev):
        assert L.ngp_nav_run_resample(ctypes.byref(st), H.ptr(prep), *rays, N, Nc, Nf, aabb, H.ptr(z), H.ptr(w), H.stream()) == 0
        assert L.ngp_nav_run_at_forward(ctypes.byref(st), H.ptr(prep), *rays, N, T, aabb, bg, H.ptr(image), H.ptr(depth), H.ptr(ws), H.ptr(saved), saved.numel(),
                                        H.ptr(z), Nc, H.stream()) == 0
        assert L.ngp_nav_run_at_backward(ctypes.byref(st), H.ptr(prep), *rays, N, T, aabb, bg, H.ptr(G), H.ptr(Gd), H.ptr(Gw), H.ptr(saved), saved.numel(),
                                         H.ptr(go), H.ptr(gd), H.ptr(z), Nc, H.stream()) == 0
        # ngp_sample_pdf on the run's own rows: the kernel's z as bins, its weights between them
        out = guarded_tensor((N, Nf), f32, dev, fill)
        bins, between = z[:, :Nc].contiguous(), w[:, :Nc - 1].contiguous()
        assert L.ngp_sample_pdf(H.ptr(bins), H.ptr(between), N, Nc, None, Nf, H.ptr(out), H.stream()) == 0
    torch.cuda.synchronize()
    outs = dict(z=z, coarse_weights=w, image=image, depth=depth, weights_sum=ws, grad_o=go, grad_d=gd, sample_pdf=out)
    for name, ten in outs.items():
        check_written(ten, name)
    check_guarded(saved, "saved")
    return {k: v.clone() for k, v in outs.items()}


@pytest.mark.parametrize("name", ["r3_1", "r257_130", "r2048_2048"])
def test_the_four_ops_between_guard_bytes(dev, name):
    case = RA.RES_CASES[name]
    a, b = (run_ops(dev, case, fill) for fill in FILLS)
    for k in a:
        assert same_bits(a[k], b[k]), f"{name}: {k} depends on what the buffers held"


def test_filter_loop_between_guard_bytes(queries, guarded, dev):  # noqa: F811
    """the resampled loop (K = 1 and K = 3) and the Hessian: the workspace through ngp_hip.workspace's stand-in, the kept depth list swapped for a guarded one"""
    g = gold_t(dev)
    K, B, T = 3, 16, int(queries.num_steps) + FU
    zs = []

    def op():
        fill = FILLS[len(zs) % 2]
        filt = make_filter(queries, B=B, sampling="resampled", upsample_steps=FU)
        filt._z_res = guarded_tensor(K * B * T, torch.float32, dev, fill)
        zs.append(filt._z_res)
        batches = filt.draw_batches(all_pixels(), 3, np.random.default_rng(7))
        one = loop(filt, g, batches, 1, dev)
        states = (g["start"][None].repeat(K, 1) + 1e-6).contiguous()
        states[1, :3] += 0.01
        kw = dict(dtype=torch.float32, device=dev)
        losses, hist, grads = torch.empty(3, K, **kw), torch.empty(3, K, 12, **kw), torch.empty(3, K, 12, **kw)
        filt.run_iterations_multi(0, 3, filt.new_adam_state_multi(K), states, g["start"], g["sig"], g["target"], batches, losses=losses, states_out=hist, grads=grads)
        hess = filt.hessian_and_gradient(g["start"] + 1e-6, g["start"], g["sig"], g["target"], batches[0])
        assert filt._z_res is zs[-1]                                     # large enough for every call: kept, not regrown
        return [one["final"], one["losses"], one["grads"], states, losses, grads, hess["hessian"], hess["grad"]]

    guarded(op, at_least=1)
    for z in zs:
        check_written(z, "the filter's depth list")


def test_a_smaller_shape_after_a_larger_one_gives_a_fresh_filters_bits(queries, dev):  # noqa: F811
    """one NativePoseFilter keeps its workspace and depth list; (B, Nc, Nf) = (64, 64, 32) and then (16, 32, 8) on it -- Nc is the queries' num_steps, set on
    a queries object of this test's own -- equal a fresh filter's (16, 32, 8)"""
    from ngp import nav
    g = gold_t(dev)
    own = nav.NativeNavQueries(queries.renderer, queries.intrinsics, queries.H, queries.W, num_steps=64)

    drawn = {B: make_filter(own, B=B).draw_batches(all_pixels(), 3, np.random.default_rng(B)) for B in (64, 16)}

    def run(filt, B, Nc, Nf):
        own.num_steps = Nc
        filt.set_sampling("resampled", upsample_steps=Nf)
        batches = drawn[B]
        out = loop(filt, g, batches, 1, dev)
        hess = filt.hessian_and_gradient(g["start"] + 1e-6, g["start"], g["sig"], g["target"], batches[0])
        return [out["final"], out["losses"], out["states"], out["grads"], hess["hessian"], hess["grad"]]

    kept = make_filter(own, B=64)
    run(kept, 64, 64, 32)
    ws, z = kept._ws_res, kept._z_res
    got = run(kept, 16, 32, 8)
    assert kept._ws_res is ws and kept._z_res is z                      # the larger buffers were kept
    want = run(make_filter(own, B=16), 16, 32, 8)
    for k, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b), k
