"""CPU: the host side of the default float32 field's frame (csrc/nav_frame.hip: ngp_nav_render_frame, ngp_nav_render_frame_camera) -- the symbols,
the workspace size, the refusals that come before anything reaches a device -- and the conditioning of the frames tests/test_gpu_default_frame.py
renders: the float32 reference must not be sensitive to its own rounding, or the GPU test's 2e-4 would be spent on the inputs.

Workspace: ngp_nav_render_frame_workspace(N) = 256 bytes for every N (a header of 64 words whose first word is the ray queue's head)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")

import _default_frame_cases as DC  # noqa: E402

WORKSPACE_BYTES = {1: 256, 64: 256, 65: 256, 640000: 256}


def test_symbols_and_workspace_size():
    import ngp_hip as H
    L = H.lib()
    for name in ("ngp_nav_render_frame_workspace", "ngp_nav_render_frame", "ngp_nav_render_frame_camera"):
        assert name in H.EXPORTS and hasattr(L.raw, name), name
    sizes = [int(L.ngp_nav_render_frame_workspace(n)) for n in sorted(WORKSPACE_BYTES)]
    assert sizes == [WORKSPACE_BYTES[n] for n in sorted(WORKSPACE_BYTES)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert L.ngp_abi_version() == 1


def test_refusals_need_no_device():
    """every pointer is a dummy: the entry points refuse before they dereference anything or ask the runtime for anything"""
    import ngp_hip as H
    L = H.lib()
    one = ctypes.c_void_p(16)
    offsets = (ctypes.c_int32 * 17)(*[i * 4096 for i in range(17)])
    nav = H.ngp_nav_field_t(16, ctypes.cast(offsets, ctypes.c_void_p), 16, 16, 16, 16, 16, 16, 16, 0.5, 2.0, 1.0)
    nv = ctypes.byref(nav)
    host = ctypes.cast((ctypes.c_float * 16)(-2, -2, -2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1), ctypes.c_void_p)     # aabb, bg, pose, intrinsics: read on the host
    need = int(L.ngp_nav_render_frame_workspace(64))

    def rays(image=one, hgrid=16, nbytes=need, field=nv):
        return L.ngp_nav_render_frame(field, one, one, one, 64, 8, host, 0.2, one, 1, hgrid, 0.0, 64, host, image, one, one, one, one, nbytes, None)

    def camera(image=one, hgrid=16, nbytes=need):
        return L.ngp_nav_render_frame_camera(nv, one, host, host, 8, 8, host, 0.2, one, 1, hgrid, 0.0, 64, host, image, one, one, one, one, nbytes, None)

    for call, op in ((rays, b"nav_render_frame:"), (camera, b"nav_render_frame_camera:")):
        assert call(nbytes=need - 1) == -3 and L.ngp_last_error().startswith(op) and b"workspace" in L.ngp_last_error()       # NGP_EWORKSPACE
        assert call(image=None) == -1 and L.ngp_last_error().startswith(op) and b"null" in L.ngp_last_error()                 # NGP_EINVAL
        assert call(hgrid=100) == -1 and L.ngp_last_error().startswith(op) and b"power of two" in L.ngp_last_error()
    # what nav_fill refuses: another architecture, and the grid of bound 256, whose level 8 the reference indexes with wrapped strides
    odd = H.ngp_nav_field_t(16, ctypes.cast(offsets, ctypes.c_void_p), 16, 16, 16, 16, 16, 8, 16, 0.5, 2.0, 1.0)
    assert rays(field=ctypes.byref(odd)) == -1 and b"default field" in L.ngp_last_error()
    from ngp import workload as W
    off256, pls = W.grid_offsets(256.0)
    wrapped = H.ngp_nav_field_t(16, ctypes.cast((ctypes.c_int32 * 17)(*[int(v) for v in off256]), ctypes.c_void_p), 16, 16, 16, 16, 16, 16, 16,
                                float(np.log2(pls)), 256.0, 1.0)
    assert rays(field=ctypes.byref(wrapped)) == -1 and b"wrapped" in L.ngp_last_error()


def test_a_grid_of_fewer_bits_than_a_byte_is_refused():
    """H = 1: C cells, a bitfield of C / 8 bytes -- none at all for the renderer's C < 8.  Refused unless C H^3 is a multiple of 8; H = 2 is 8 cells a
    cascade and passes this check for every C (the call below gets as far as the workspace check, which is the last one before the device)."""
    import ngp_hip as H
    L = H.lib()
    one = ctypes.c_void_p(16)
    offsets = (ctypes.c_int32 * 17)(*[i * 4096 for i in range(17)])
    nav = H.ngp_nav_field_t(16, ctypes.cast(offsets, ctypes.c_void_p), 16, 16, 16, 16, 16, 16, 16, 0.5, 2.0, 1.0)
    host = ctypes.cast((ctypes.c_float * 16)(-2, -2, -2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1), ctypes.c_void_p)
    need = int(L.ngp_nav_render_frame_workspace(64))

    def rays(cascades, hgrid, nbytes):
        return L.ngp_nav_render_frame(ctypes.byref(nav), one, one, one, 64, 8, host, 0.2, one, cascades, hgrid, 0.0, 64, host, one, one, one, one, one, nbytes, None)

    for cascades in (1, 2, 3, 7, 9):
        assert rays(cascades, 1, need) == -1 and b"whole number of bytes" in L.ngp_last_error(), cascades
        assert rays(cascades, 2, need - 1) == -3 and b"workspace" in L.ngp_last_error(), cascades
    assert rays(8, 1, need - 1) == -3 and rays(16, 1, need - 1) == -3          # H = 1 with whole bytes is a grid like any other


@pytest.mark.parametrize("name", DC.CONDITIONED + DC.CONDITIONED_INSIDE)
def test_gpu_cases_are_well_conditioned(oracle, name):
    """A condition on the inputs, not a measurement of a kernel: the reference in float32 and in float64 (same sample positions, the field and
    sigma * density_scale in the other precision) agree to 5e-5 in image and weights_sum, no ray consumes a different number of samples, and the
    depth maps are NaN for the same rays.  Largest difference seen: 2.4e-5 (weights_sum, sample_cap).  The frames from inside the scene
    (DC.CONDITIONED_INSIDE, rendered by tests/test_gpu_default_frame_inside.py) are held to the same bar; three of the poses see nothing on purpose,
    and their frames have no sample in either precision."""
    a = DC.reference32(name)
    b = DC.reference(name, oracle, dtype=torch.float64)
    d_image = float(np.max(np.abs(a["image"].astype(np.float64) - b["image"])))
    d_ws = float(np.max(np.abs(a["weights_sum"].astype(np.float64) - b["weights_sum"])))
    print(f"{name}: image {d_image:.3g} weights_sum {d_ws:.3g} samples {a['samples']}")
    if name in DC.INSIDE_NO_SAMPLES:
        assert a["samples"] == 0 and b["samples"] == 0
    else:
        assert a["samples"] > 1000
    assert d_image < 5e-5 and d_ws < 5e-5
    assert np.array_equal(a["consumed"], b["consumed"])
    assert np.array_equal(np.isnan(a["depth"]), np.isnan(b["depth"]))
