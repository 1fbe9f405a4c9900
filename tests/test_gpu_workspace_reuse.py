"""GPU: an object that keeps its workspace gives, on a smaller shape after a larger one, what a freshly built object gives.

NativePoseFilter (_ws, _ws_occ, _ws_multi, _feat_ws), NativePlanner (_ws) and NGPRenderer (_grid_ws) allocate a workspace once and lay the next call's
shape over whatever the last call left there.  Each case runs the larger shape, then the smaller one on the SAME object, and compares every output of the
smaller run, with torch.equal on the bits, with a new object's; it also shows that the buffer was kept (same data_ptr() before and after) and is larger
than the smaller shape needs, without which the comparison would prove nothing.  The scene, the sizes and the order of writes and reads inside the ops
are tests/test_gpu_workspace_guard.py's."""
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

from _guard import same_bits  # noqa: E402
from test_gpu_workspace_guard import feature_image, filter_queries, filter_setting, make_filter, nav_renderer, scene  # noqa: E402,F401

N_ITER, T = 2, 8


def assert_same(got, want, tag):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b), f"{tag}: output {k} differs from a fresh object's"


def loop_outputs(filt, s):
    final = filt.estimate_relative_pose(s["target"], s["start"], s["sig"], s["batches"])
    return [final.clone(), filt.losses.clone(), filt.states.clone(), filt.grads.clone()]


@pytest.mark.parametrize("sampling", ["dense", "occupied"])
def test_pose_filter_loop_after_a_larger_batch(dev, nav_renderer, sampling):
    """B = 65 then B = 16: the 16-ray layout (every piece a quarter as long) lands on the 65-ray run's rays, records, gradients and partials"""
    import ngp_hip
    big, small = filter_setting(dev, 65, N_ITER, 65), filter_setting(dev, 16, N_ITER, 16)
    kept = "_ws_occ" if sampling == "occupied" else "_ws"
    size = ngp_hip.lib().ngp_filter_occ_workspace if sampling == "occupied" else ngp_hip.lib().ngp_filter_workspace
    need = size(1, 16, T) if sampling == "occupied" else size(16, T)
    filt = make_filter(filter_queries(nav_renderer), 65, N_ITER, sampling=sampling)
    first = loop_outputs(filt, big)
    ws = getattr(filt, kept)
    ptr, numel = ws.data_ptr(), ws.numel()
    got = loop_outputs(filt, small)
    assert getattr(filt, kept).data_ptr() == ptr and getattr(filt, kept).numel() == numel > need > 0
    want = loop_outputs(make_filter(filter_queries(nav_renderer), 16, N_ITER, sampling=sampling), small)
    assert_same(got, want, f"{sampling} B = 16 after B = 65")
    assert float(got[3].abs().max()) > 0 and not same_bits(first[1], got[1])


def multi_outputs(filt, s, offsets):
    best = filt.estimate_relative_pose_multi(s["target"], s["start"], s["sig"], s["batches"], offsets)
    m = filt.multi
    return [best.clone()] + [m[k].clone() for k in ("states", "final_losses", "index", "losses", "states_hist", "grads")]


def test_multi_start_after_more_hypotheses(dev, nav_renderer):
    """K = 3 then K = 2 at B = 33: hypothesis 1's slices of the K = 2 layout begin inside what were hypothesis 0's and 1's of the K = 3 run"""
    import ngp_hip
    s = filter_setting(dev, 33, N_ITER, 33)
    offsets = torch.zeros(3, 12)
    offsets[1, :3], offsets[2, 6:9] = torch.tensor([0.05, -0.04, 0.03]), torch.tensor([0.04, 0.0, -0.03])
    filt = make_filter(filter_queries(nav_renderer), 33, N_ITER)
    multi_outputs(filt, s, offsets)
    ptr, numel = filt._ws_multi.data_ptr(), filt._ws_multi.numel()
    got = multi_outputs(filt, s, offsets[[2, 1]])
    assert filt._ws_multi.data_ptr() == ptr and filt._ws_multi.numel() == numel > ngp_hip.lib().ngp_filter_multi_workspace(2, 33, T) > 0
    want = multi_outputs(make_filter(filter_queries(nav_renderer), 33, N_ITER), s, offsets[[2, 1]])
    assert_same(got, want, "K = 2 after K = 3")
    assert float(got[6].abs().max()) > 0


def test_feature_front_around_a_filter_run(dev, nav_renderer):
    """detect / interest_regions, a filter run (its buffers are allocated in between), then detect / interest_regions on another image: the pyramid,
    the dilated mask, the counts and the bitmap of the first image are still in the detector's workspace"""
    import ngp_hip
    s = filter_setting(dev, 65, N_ITER, 65)
    filt = make_filter(filter_queries(nav_renderer), 65, N_ITER)
    mask0, regions0 = filt.detect(feature_image(dev, 0)).clone(), filt.interest_regions(feature_image(dev, 0)).clone()
    ptr, numel = filt._feat_ws.data_ptr(), filt._feat_ws.numel()
    loop_outputs(filt, s)
    got = [filt.detect(feature_image(dev, 1)).clone(), filt.interest_regions(feature_image(dev, 1)).clone()]
    assert filt._feat_ws.data_ptr() == ptr and filt._feat_ws.numel() == numel >= ngp_hip.lib().ngp_features_workspace(16, 16) > 0
    fresh = make_filter(filter_queries(nav_renderer), 65, N_ITER)
    want = [fresh.detect(feature_image(dev, 1)).clone(), fresh.interest_regions(feature_image(dev, 1)).clone()]
    assert_same(got, want, "second image")
    assert 0 < got[1].shape[0] < regions0.shape[0] and int(mask0.sum()) > int(got[0].sum()) > 0       # fewer keypoints than the image before: stale ones would show


PLAN_CFG = {"T_final": 2., "steps": 4, "lr": 0.001, "epochs_init": 1, "epochs_update": 1, "fade_out_epoch": 0, "fade_out_sharpness": 10, "mass": 1.,
            "I": torch.eye(3), "g": 10., "body": np.array([[-0.05, 0.05], [-0.05, 0.05], [-0.02, 0.02]]), "nbins": [3, 1, 1]}


def make_planner(nav_renderer):
    from ngp import nav
    from oracle import nav_oracle as NO
    queries = nav.NativeNavQueries(nav_renderer, (20.0, 20.0, 4.0, 4.0), 8, 8, num_steps=8)
    return nav.NativePlanner(NO.state18([0.39, -0.67, 0.2]), NO.state18([-0.4, 0.55, 0.16]), PLAN_CFG, queries)


def plan_multi(plan, offsets, dev):
    K = offsets.shape[0]
    states, accel = (plan.states[None] + offsets).contiguous(), plan.initial_accel[None].repeat(K, 1).contiguous()
    adam, losses, per_state = plan.new_adam_state_multi(K), torch.empty(1, K, device=dev), torch.empty(K, 2, plan.S, device=dev)
    plan.run_epochs_multi(states, accel, 0, 1, adam, losses=losses, per_state=per_state)
    return [states, accel, adam, losses, per_state]


def plan_single(plan, dev):
    adam, losses, per_state = plan.new_adam_state(), torch.empty(1, device=dev), torch.empty(2, plan.S, device=dev)
    plan.run_epochs(0, 1, adam, losses=losses, per_state=per_state)
    return [plan.states.clone(), plan.initial_accel.clone(), adam, losses, per_state]


def test_planner_after_more_hypotheses(dev, nav_renderer):
    """run_epochs_multi K = 3, then K = 2, then plain run_epochs, on one planner (R = 2, three body points): points, sigma and jac of 15 K points each"""
    import ngp_hip
    plan = make_planner(nav_renderer)
    offsets = plan.draw_offsets(3, 0.05, generator=torch.Generator().manual_seed(1))
    plan_multi(plan, offsets, dev)
    ptr, numel = plan._ws.data_ptr(), plan._ws.numel()
    got = plan_multi(plan, offsets[[0, 2]], dev) + plan_single(plan, dev)
    L = ngp_hip.lib()
    assert plan._ws.data_ptr() == ptr and plan._ws.numel() == numel > L.ngp_plan_multi_workspace(2, 2, 3) > L.ngp_plan_workspace(2, 3) > 0
    fresh = make_planner(nav_renderer)
    want = plan_multi(fresh, offsets[[0, 2]], dev) + plan_single(fresh, dev)
    assert_same(got, want, "K = 2 and the single run after K = 3")
    assert float(got[2].abs().max()) > 0 and float(got[7].abs().max()) > 0


def test_density_grid_full_sweep_after_a_partial_one(dev, scene):
    """one renderer (two cascades of 8^3): a full sweep, a partial sweep (the occupied-cell lists, n_occ and thresh are written), then the grid cleared,
    the iteration reset and a full sweep again: equal to a fresh renderer's first sweep.  The grid workspace has one size per grid, so the kept buffer is
    as large as, not larger than, what the sweep needs"""
    import ngp_hip
    from ngp.render import NGPRenderer
    W, field = scene

    def build():
        ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0, grid_size=8).to(dev).train()
        assert ren.cascade == 2
        return ren

    def sweep(ren):
        with torch.autocast("cuda", dtype=torch.float16):
            ren.update_extra_state()
        return [ren.density_grid.clone(), ren.density_bitfield.clone(), ren._mean_dev.clone()]
    ren = build()
    first = sweep(ren)
    ptr, numel = ren._grid_ws.data_ptr(), ren._grid_ws.numel()
    ren.iter_density = 16
    partial = sweep(ren)
    assert not same_bits(first[0], partial[0])
    ren.density_grid.zero_()
    ren.iter_density = 0
    got = sweep(ren)
    assert ren._grid_ws.data_ptr() == ptr and ren._grid_ws.numel() == numel >= ngp_hip.lib().ngp_density_grid_workspace(2, 8) > 0
    want = sweep(build())
    assert_same(got, want, "full sweep after a partial one")
    assert_same(got, first, "the first sweep")
    assert float(got[0].max()) > 0
