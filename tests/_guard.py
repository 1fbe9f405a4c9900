"""Guard bytes around what the native ops are handed: the shared pieces of tests/test_gpu_workspace_guard.py (every workspace), tests/test_gpu_workspace_reuse.py
(kept workspaces) and tests/test_gpu_output_guard.py (outputs, through the C ABI), and the table that says which case covers which size function.

A plain helper module, not a conftest: the test files import `guarded` (a fixture) and the functions by name."""
import pytest
import torch

GUARD = 256


class GuardedWorkspaces:
    """a stand-in for ngp_hip.workspace: the middle n bytes of a buffer of n + 512 filled with `fill` (offset 256, so the alignment the allocator gives is kept)"""

    def __init__(self, fill):
        self.fill, self.buffers = fill, []

    def __call__(self, nbytes, device):
        n = max(int(nbytes), 16)
        buf = torch.full((n + 2 * GUARD,), self.fill, dtype=torch.uint8, device=device)
        assert buf.data_ptr() % 256 == 0
        self.buffers.append(buf)
        return buf[GUARD:GUARD + n]

    def check(self, at_least):
        assert len(self.buffers) >= at_least, f"{len(self.buffers)} workspaces were allocated through ngp_hip.workspace, expected {at_least}"
        for k, buf in enumerate(self.buffers):
            assert bool((buf[:GUARD] == self.fill).all()), f"workspace {k} ({buf.numel() - 2 * GUARD} bytes): written in front of it"
            assert bool((buf[-GUARD:] == self.fill).all()), f"workspace {k} ({buf.numel() - 2 * GUARD} bytes): written behind it"


def same_bits(a, b):
    """bit for bit (NaNs included), shapes and types too"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


@pytest.fixture
def guarded(monkeypatch, dev):
    """guarded(op, at_least): runs op() under both fills, checks the guards of the (at least `at_least`) workspaces it allocated and that its
    outputs (a list of tensors) do not depend on the fill; returns the outputs"""
    import ngp_hip

    def run(op, at_least=1):
        outs = []
        for fill in (0xAB, 0x00):
            spaces = GuardedWorkspaces(fill)
            monkeypatch.setattr(ngp_hip, "workspace", spaces)
            result = [r.detach().clone() for r in op()]
            torch.cuda.synchronize()
            spaces.check(at_least)
            outs.append(result)
        assert len(outs[0]) == len(outs[1]) > 0
        for k, (a, b) in enumerate(zip(*outs)):
            assert a.shape == b.shape and a.dtype == b.dtype and a.numel() > 0, k
            assert same_bits(a, b), f"output {k} depends on what the workspace held"
        return outs[0]
    return run


def guarded_tensor(shape, dtype, dev, fill):
    """a contiguous tensor of `shape` in the middle of a byte buffer with GUARD bytes on each side, its data_ptr() 256-byte aligned and the back guard right
    behind its last element; every byte of the buffer (the tensor's too) is `fill`: 0xFF makes every float a NaN, 0xAB a pattern no op writes"""
    if isinstance(shape, int):
        shape = (shape,)
    count = 1
    for s in shape:
        count *= int(s)
    nbytes = count * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    t = buf[GUARD:GUARD + nbytes].view(dtype).view(*shape)
    assert t.is_contiguous() and t.data_ptr() % 256 == 0 and t.data_ptr() == buf.data_ptr() + GUARD
    t.guard_buffer, t.guard_fill = buf, fill
    return t


def check_guarded(t, name="tensor"):
    """both guards of a guarded_tensor still hold the fill"""
    buf, fill = t.guard_buffer, t.guard_fill
    assert bool((buf[:GUARD] == fill).all()), f"{name} {tuple(t.shape)}: written in front of it"
    assert bool((buf[-GUARD:] == fill).all()), f"{name} {tuple(t.shape)}: written behind it"


def unwritten(t):
    """how many elements of a guarded_tensor still hold the fill pattern in every byte"""
    size = t.element_size()
    return int((t.contiguous().view(-1).view(torch.uint8).view(-1, size) == t.guard_fill).all(dim=1).sum())


def check_written(t, name="tensor"):
    check_guarded(t, name)
    assert unwritten(t) == 0, f"{name} {tuple(t.shape)}: {unwritten(t)} elements were never written"


# ------------------------------------------------------------------------------------------------------------------------
# which case runs which size function's buffer between guard bytes (tests/test_workspace_table.py holds ngp_hip.EXPORTS to this table)
# ------------------------------------------------------------------------------------------------------------------------
WS, REUSE, OUT = "test_gpu_workspace_guard", "test_gpu_workspace_reuse", "test_gpu_output_guard"

COVERED = {
    "ngp_march_rays_train_workspace_full": f"{WS}::test_training_march",
    "ngp_march_rays_workspace": f"{WS}::test_inference_march",
    "ngp_compact_alive_workspace": f"{WS}::test_compact_alive",
    "ngp_density_grid_workspace": f"{WS}::test_update_extra_state",
    "ngp_grid_scatter_binned_workspace": f"{WS}::test_binned_scatter",
    "ngp_grid_scatter_binned_f32_workspace": f"{WS}::test_default_field_training_step",
    "ngp_mse_head_workspace": f"{WS}::test_mse_head_workspace",
    "ngp_ffmlp_backward_workspace": f"{WS}::test_ffmlp_autograd",
    "ngp_field_density_workspace": f"{WS}::test_density_sigma",
    "ngp_field_train_saved_bytes": f"{WS}::test_field_train_forward_and_backward",
    "ngp_field_train_workspace": f"{WS}::test_field_train_forward_and_backward",
    "ngp_render_frame_workspace": f"{WS}::test_half_frame_single_routes",
    "ngp_render_frames_workspace": f"{WS}::test_render_fused_cameras",
    "ngp_nav_field_workspace": f"{WS}::test_nav_run",
    "ngp_nav_field_train_saved_bytes": f"{WS}::test_default_field_training_step",
    "ngp_nav_field_train_workspace": f"{WS}::test_default_field_training_step",
    "ngp_nav_run_saved_bytes": f"{WS}::test_nav_run",
    "ngp_nav_run_occ_saved_bytes": f"{WS}::test_nav_run",
    "ngp_nav_render_frame_workspace": f"{WS}::test_default_frame",
    "ngp_marching_cubes_workspace": f"{WS}::test_marching_cubes",
    "ngp_plan_workspace": f"{WS}::test_plan_epochs",
    "ngp_plan_multi_workspace": f"{WS}::test_plan_epochs_multi",
    "ngp_filter_workspace": f"{WS}::test_pose_filter_loop",
    "ngp_filter_occ_workspace": f"{WS}::test_pose_filter_loop",
    "ngp_filter_multi_workspace": f"{WS}::test_pose_filter_multi",
    "ngp_features_workspace": f"{WS}::test_feature_front",
}

EXEMPT = {
    "ngp_march_rays_train_workspace": "the wrapper draws this size only when the `_full` one exceeds 256 MiB, beyond any quick case; it is the front part of the "
                                      "`_full` layout, which test_training_march runs between guard bytes",
}
