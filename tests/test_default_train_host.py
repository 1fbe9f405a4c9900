"""CPU: the C ABI of the default float32 field's native training (include/ngp_hip.h, csrc/nav_train.hip) -- exported symbols, the two size
functions and every refusal, none of which touches a device; the conditions on the samples the GPU test uses; and NGPField's opt-in flag on CPU
tensors, where it must fall back."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
import ngp_hip  # noqa: E402

import _default_train_cases as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ngp_nav_field_train_saved_bytes", "ngp_nav_field_train_workspace", "ngp_nav_field_train_forward", "ngp_nav_field_train_backward")
EINVAL, EWORKSPACE = -1, -3
SAVED_PER_SAMPLE = 128                   # the 32 encoded features, float32


def test_train_symbols_are_declared_exported_and_callable():
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    for name in NEW:
        assert name in ngp_hip.EXPORTS and f"{name}(" in header
        getattr(ngp_hip.lib(), name)
    L = ngp_hip.lib().raw
    assert L.ngp_abi_version() == 1
    assert L.ngp_nav_field_train_saved_bytes(1) > 0 and L.ngp_nav_field_train_workspace(1) > 0
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"128 B(ytes)? per sample", design[design.index("3.12"):])


def test_size_functions():
    L = ngp_hip.lib()
    Ms = (0, 1, 2, 63, 64, 65, 255, 256, 257, 900, 4096, 65535, 65536, 65537, 1 << 20, 1800000, (1 << 32) - 1)
    for fn in (L.ngp_nav_field_train_saved_bytes, L.ngp_nav_field_train_workspace):
        sizes = [fn(M) for M in Ms]
        assert sizes[0] == 0 and sizes[1] > 0
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
        assert all(s % 256 == 0 for s in sizes), sizes
    for M in Ms[1:]:
        assert L.ngp_nav_field_train_saved_bytes(M) >= SAVED_PER_SAMPLE * M
    # the partial sums are bounded: a fixed number of workgroups, not one partial per 256 samples
    assert L.ngp_nav_field_train_workspace(1 << 20) == L.ngp_nav_field_train_workspace(1 << 24) <= 32 << 20


def _fake(n=16):
    return ctypes.c_void_p(n)                                             # never dereferenced: validation fails first


def _field(per_level_scale_log2=1.0, H=16, offsets=None):
    f = _fake()
    keep = (ctypes.c_int32 * 17)(*(offsets if offsets is not None else [8 * l for l in range(17)]))
    return ngp_hip.ngp_nav_field_t(f, ctypes.cast(keep, ctypes.c_void_p), f, f, f, f, f, 16, H, per_level_scale_log2, 1.0, 1.0), keep


def _good_field():
    """a field nav_fill accepts: every level hashed (8 rows each, side 17 and up)"""
    return _field()


def _forward(L, fld, M=100, prepared=True, x=True, d=True, sig=True, rgb=True, saved=True, saved_bytes=1 << 40):
    p = lambda on: _fake() if on else None                                # noqa: E731
    return L.ngp_nav_field_train_forward(ctypes.byref(fld) if fld is not None else None, p(prepared), p(x), p(d), M, p(sig), p(rgb), p(saved), saved_bytes, None)


def _backward(L, fld, M=100, prepared=True, saved=True, x=True, d=True, gs=True, gc=True, genc=True, gw=True, ws=True, ws_bytes=1 << 40):
    p = lambda on: _fake() if on else None                                # noqa: E731
    return L.ngp_nav_field_train_backward(ctypes.byref(fld) if fld is not None else None, p(prepared), p(saved), p(x), p(d), M, p(gs), p(gc), p(genc), p(gw),
                                          p(ws), ws_bytes, None)


def test_refusals_need_no_device():
    L = ngp_hip.lib().raw
    fld, keep = _good_field()
    assert _forward(L, None) == EINVAL and b"null field" in L.ngp_last_error()
    assert _forward(L, fld, prepared=False) == EINVAL and b"null field" in L.ngp_last_error()
    for hole in ("x", "d", "sig", "rgb"):
        assert _forward(L, fld, **{hole: False}) == EINVAL, hole
        assert b"null pointer" in L.ngp_last_error()
    need = L.ngp_nav_field_train_saved_bytes(100)
    assert _forward(L, fld, saved_bytes=need - 1) == EWORKSPACE and b"ngp_nav_field_train_saved_bytes" in L.ngp_last_error()
    assert _forward(L, fld, saved=False, saved_bytes=need) == EWORKSPACE
    assert _forward(L, fld, M=0, saved=False, saved_bytes=0) == 0                  # M = 0: nothing to do, nothing queued

    assert _backward(L, None) == EINVAL and b"null field" in L.ngp_last_error()
    assert _backward(L, fld, prepared=False) == EINVAL
    for hole in ("saved", "x", "d", "gs", "gc"):
        assert _backward(L, fld, **{hole: False}) == EINVAL, hole
        assert b"null pointer" in L.ngp_last_error()
    assert _backward(L, fld, genc=False, gw=False) == EINVAL and b"null pointer" in L.ngp_last_error()
    need = L.ngp_nav_field_train_workspace(100)
    assert _backward(L, fld, ws_bytes=need - 1) == EWORKSPACE and b"ngp_nav_field_train_workspace" in L.ngp_last_error()
    assert _backward(L, fld, ws=False, ws_bytes=need) == EWORKSPACE
    assert _backward(L, fld, M=0, ws=False, ws_bytes=0) == 0


def test_field_refusals_are_nav_field_prepares_word_for_word():
    L = ngp_hip.lib().raw
    rows = 1 << 24
    offsets = [0]
    for l in range(16):
        side = 16 * 2 ** l + 1
        offsets.append(offsets[-1] + min(rows, (side ** 3 + 7) // 8 * 8))
    cases = {"default field": _field(offsets=list(range(0, 17 * 8, 8))), "empty level": _field(offsets=[0] * 17),
             "wrapped 32-bit strides": _field(offsets=offsets)}        # per_level_scale 2 from 16, 2^24 rows: level 12's stride product wraps
    cases["default field"][0].L = 15
    for words, (fld, keep) in cases.items():
        assert L.ngp_nav_field_prepare(ctypes.byref(fld), _fake(), 1 << 30, None) == EINVAL
        want = L.ngp_last_error().split(b":", 1)[1]
        assert words.encode() in want
        for call in (_forward, _backward):
            assert call(L, fld) == EINVAL
            who, said = L.ngp_last_error().split(b":", 1)
            assert said == want and who.startswith(b"nav_field_train_"), (who, said)


def test_sample_conditions():
    x, d, names = T.candidates()
    assert x.shape == (1000, 3) and np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    for kind in T.FIELDS:
        out, worst = T.kink_report(kind)
        print(f"{kind}: {int(out.sum())} of {len(out)} candidates left out; special points left out: {[n for n, r in names.items() if out[r]]}")
        assert out.sum() <= 0.08 * len(out)
        for cat in T.CATEGORIES:
            members = [r for n, r in names.items() if n.startswith(cat)]
            assert members and any(not out[r] for r in members), f"{kind}: no point of category {cat} is left"
        keep = T.survivors(kind)
        assert len(keep) >= max(T.SIZES) and len(keep) == len(out) - out.sum()
        assert np.array_equal(T.batch_rows(kind, 64), keep[:64])
        big = T.batch_rows(kind, T.BIG)
        assert len(big) == T.BIG and np.array_equal(big[len(keep):2 * len(keep)], keep)
    assert T.BIG > 256 * 256                                               # more chunks than the backward has workgroups
    assert set((1, 63, 64, 65, 255, 256, 257, 900)) <= set(T.SIZES)


def test_reference_yardstick_is_never_zero():
    ref = T.reference("fog", 65)
    assert (ref["yard"]["weights"] > 0).all() and (ref["yard"]["levels"] > 0).all()
    assert ref["yard"]["weights"].max() < 1e-5 and ref["yard"]["levels"].max() < 1e-5
    assert np.isfinite(ref["e32"]["sigma"]).all() and ref["e32"]["sigma"].max() < 1e-5


def test_flag_defaults_to_off_and_falls_back_on_cpu_tensors():
    from ngp.field import NGPField
    assert NGPField(bound=1).fused_training is False
    torch.manual_seed(3)
    a, b = NGPField(bound=1, fused_training=True), NGPField(bound=1)
    assert a.fused_training is True
    b.load_state_dict(a.state_dict())
    x = torch.rand(257, 3) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(257, 3), dim=1)
    assert not a._fused_training_applies(x, d)
    # the encoders have no CPU path: with them in place both fields refuse CPU tensors, in the op chain's words
    for f in (a, b):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(x, d)
    # with CPU stand-ins for the two encoders (same numbers for both fields) the forward runs, and the flag changes nothing
    for f in (a, b):
        emb = f.encoder.embeddings
        f.encoder.forward = lambda p, bound=1, emb=emb: torch.sin(p @ torch.linspace(-3, 3, 96).reshape(3, 32)) * emb[:32, 0]
        f.encoder_dir.forward = lambda q: torch.cos(q @ torch.linspace(-2, 2, 48).reshape(3, 16))
    outs = []
    for f in (a, b):
        sigma, rgb = f(x, d)
        (sigma.sum() + (rgb * rgb).sum()).backward()
        outs.append((sigma, rgb, [p.grad for p in f.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for ga, gb in zip(outs[0][2], outs[1][2]):
        assert ga is not None and torch.equal(ga, gb)
