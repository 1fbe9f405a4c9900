"""GPU: the native agent, its sensor and the closed navigation loop (csrc/nav_agent.hip; ngp.nav.NativeAgent, ngp.nav.simulate), in
tests/test_gpu_nav_filter.py's setting (the callers_nav.npz field, 20 x 20 pixels, 64 steps) with tests/test_gpu_plan_astar.py's planner.

  * ngp_agent_step evaluates the reference's formulas in float64 from float32 inputs and rounds once, so it is held to the EXECUTED reference's float64
    Agent.step (tests/golden/agent.npz) at test_gpu_filter_step.py's bar: 2 float32 ulps of the largest entry of each 3-block.
  * ngp_agent_rays is the filter's own ray kernel over every pixel: bit for bit.
  * ngp_agent_sensor is integer-exact: bit for bit against its numpy restatement (tests/_agent_cases.py, held to the reference's expressions on the CPU).
  * the loop is a composition: bit for bit the same sequence made by hand from the public methods."""
import ctypes
import importlib
import json
import time

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

import _agent_cases as AC  # noqa: E402
from test_gpu_filter_step import step_filter, ulps2  # noqa: E402
from test_gpu_nav_filter import H, W, all_pixels, case_state, queries  # noqa: E402,F401
from test_gpu_plan_astar import K, SIDE, centre, cfg as plan_cfg, scene, state as plan_state  # noqa: E402,F401

NAMES = AC.names()
NOISE_STD = [2e-2, 2e-2, 2e-2, 1e-2, 1e-2, 1e-2, 2e-2, 2e-2, 2e-2, 1e-2, 1e-2, 1e-2]           # simulate.py:264


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b)


def dyn_of(name):
    import ngp_hip
    g = AC.gold()
    d = ngp_hip.ngp_filter_dyn_t()
    d.dt, d.mass, d.g = (float(v) for v in g[f"{name}_cfg"])
    d.I[:] = [float(v) for v in g[f"{name}_I"].reshape(-1)]
    return d


def agent_step(d, state, action, noise, poses=True):
    import ngp_hip
    dev = state.device
    nxt = torch.full((12,), float("nan"), device=dev)
    blender = torch.full((4, 4), float("nan"), device=dev) if poses else None
    body = torch.full((4, 4), float("nan"), device=dev) if poses else None
    ngp_hip.check(ngp_hip.lib().ngp_agent_step(ctypes.byref(d), ngp_hip.ptr(state), ngp_hip.ptr(action), ngp_hip.ptr(noise), ngp_hip.ptr(nxt),
                                               ngp_hip.ptr(blender), ngp_hip.ptr(body), ngp_hip.stream()), "agent_step")
    return nxt, blender, body


def agent_cfg_of(x0=None):
    return {"x0": x0, "dt": 0.1, "mass": 1.0, "g": 10.0, "I": torch.eye(3)}


# ------------------------------------------------------------------------------------------------------------------------
# 1. ngp_agent_step
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_step_against_the_executed_float64_agent(queries, dev, name):
    g = AC.gold()
    d = dyn_of(name)
    state, action, noise = (torch.from_numpy(g[f"{name}_{k}"]).to(dev) for k in ("state", "action", "noise"))
    nxt, blender, body = agent_step(d, state, action, noise)
    got = {"new_state": nxt.cpu().numpy().astype(np.float64), "blender_pose": blender.cpu().numpy().astype(np.float64),
           "true_pose": body.cpu().numpy().astype(np.float64)}
    pose_blocks = [(i, slice(0, 3)) for i in range(3)] + [(slice(0, 3), 3)]
    for key, blocks in (("new_state", [(slice(i, i + 3),) for i in range(0, 12, 3)]), ("blender_pose", pose_blocks), ("true_pose", pose_blocks)):
        ref, f32 = g[f"{name}_{key}_f64"], g[f"{name}_{key}_f32"].astype(np.float64)
        assert ref.dtype == np.float64
        for blk in blocks:
            bar = ulps2(ref[blk])
            err, own = np.abs(got[key][blk] - ref[blk]).max(), np.abs(f32[blk] - ref[blk]).max()
            unit = bar / 2 if bar else 1.0
            print(f"{name} {key}{blk}: kernel {err / unit:.3f} ulp, the reference's float32 run {own / unit:.3f} ulp (of the block's largest)")
            assert err <= bar, (name, key, blk, err, bar)
        if key != "new_state":
            assert got[key][3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert np.array_equal(got["blender_pose"][:3, 3], got["new_state"][:3]) and np.array_equal(got["true_pose"][:3, 3], got["new_state"][:3])
    # noise = NULL: a zero noise vector's result, and the filter's own propagation, bit for bit
    quiet, blender0, body0 = agent_step(d, state, action, None)
    zero, blender1, body1 = agent_step(d, state, action, torch.zeros(12, device=dev))
    assert same_bits(quiet, zero) and same_bits(blender0, blender1) and same_bits(body0, body1)
    filt = step_filter(queries, name)
    assert torch.equal(quiet, filt.propagate(state, action)["state"])
    # the poses are optional and change nothing
    alone, _, _ = agent_step(d, state, action, noise, poses=False)
    assert same_bits(alone, nxt)
    # twice
    again = agent_step(d, state, action, noise)
    assert all(same_bits(a, b) for a, b in zip(again, (nxt, blender, body)))


# ------------------------------------------------------------------------------------------------------------------------
# 2. ngp_agent_rays
# ------------------------------------------------------------------------------------------------------------------------
def pixels_of(h, w):
    rows, cols = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([rows.ravel(), cols.ravel()], -1)


@pytest.mark.parametrize("shape", [(20, 20), (12, 20), (7, 9), (33, 35)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rays_are_the_filters_own_bit_for_bit(queries, dev, shape):
    """square; rectangular (a swapped row and column shows); 63 pixels (a lane with fewer than four); 1,155 (a second workgroup, an odd tail)"""
    import ngp_hip
    from ngp import nav
    h, w = shape
    q = queries if shape == (H, W) else nav.NativeNavQueries(queries.renderer, queries.intrinsics, h, w, num_steps=64)
    filt = nav.NativePoseFilter({"batch_size": 16, "lrate": 1e-3, "N_iter": 1, "sig0": torch.eye(12), "Q": torch.eye(12)}, q)
    agent = nav.NativeAgent(agent_cfg_of(torch.zeros(12)), q)
    for name in ("golden", "zero_rotation", "near_pi", "inside_looking_out"):
        state = torch.from_numpy(case_state(name)[0]).to(dev)
        want = filt.rays(state, pixels_of(h, w))
        rays_o, rays_d = agent.rays(state)
        assert tuple(rays_o.shape) == (h * w, 3) and same_bits(rays_o, want["rays_o"]) and same_bits(rays_d, want["rays_d"]), (shape, name)
        # outputs that are not 16-byte aligned take the element-by-element kernel: the same bits, nothing written outside
        buf_o, buf_d = (torch.full((3 * h * w + 2,), float("nan"), device=dev) for _ in range(2))
        ngp_hip.check(ngp_hip.lib().ngp_agent_rays(ctypes.byref(agent._view), ngp_hip.ptr(state), ngp_hip.ptr(buf_o[1:]), ngp_hip.ptr(buf_d[1:]),
                                                   ngp_hip.stream()), "agent_rays")
        assert buf_o[1:].data_ptr() % 16 == 4
        for buf, ref in ((buf_o, rays_o), (buf_d, rays_d)):
            assert same_bits(buf[1:-1].view(-1, 3), ref) and bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[-1]))


# ------------------------------------------------------------------------------------------------------------------------
# 3. ngp_agent_sensor
# ------------------------------------------------------------------------------------------------------------------------
def sensor(image, N, png, target):
    import ngp_hip
    ngp_hip.check(ngp_hip.lib().ngp_agent_sensor(ngp_hip.ptr(image), ngp_hip.ptr(png), ngp_hip.ptr(target), N, ngp_hip.stream()), "agent_sensor")


@pytest.mark.parametrize("N", [1, 63, 64, 65, 20 * 20 * 3 + 1])
def test_sensor_is_its_restatement_bit_for_bit(dev, N):
    x = AC.sensor_input(N)
    want_png, want_target = AC.sensor_restated(x)
    for shift in (0, 1):                                                               # 0: the 16-byte stores; 1: pointers that are not aligned for them
        image = torch.zeros(3 * N + 8, device=dev)
        image[shift:shift + 3 * N] = torch.from_numpy(x.reshape(-1)).to(dev)
        png = torch.full((3 * N + 8,), 77, dtype=torch.uint8, device=dev)
        target = torch.full((3 * N + 8,), float("nan"), device=dev)
        sensor(image[shift:], N, png[shift:], target[shift:])
        assert image[shift:].data_ptr() % 16 == 4 * shift
        got_png, got_target = png[shift:shift + 3 * N].cpu().numpy().reshape(N, 3), target[shift:shift + 3 * N].cpu().numpy().reshape(N, 3)
        assert np.array_equal(got_png, want_png), (N, shift)
        assert np.array_equal(got_target.view(np.uint32), want_target.view(np.uint32)), (N, shift)
        # nothing outside the 3 N elements is written
        assert bool((png[:shift] == 77).all()) and bool((png[shift + 3 * N:] == 77).all())
        assert bool(torch.isnan(target[:shift]).all()) and bool(torch.isnan(target[shift + 3 * N:]).all())


# ------------------------------------------------------------------------------------------------------------------------
# 4. the agent: consistency with the filter, the frame route, no synchronisation
# ------------------------------------------------------------------------------------------------------------------------
ACTION = [10.1, 0.01, -0.02, 0.015]


def start12(dev):
    return torch.from_numpy(case_state("golden")[0]).to(dev)


def test_the_observation_is_the_filters_prediction_up_to_the_8_bit_round_trip(queries, dev):
    """sensor=None, no noise: at the true state the filter predicts the observation before quantisation (the same rays, the same run kernel); truncation
    moves a channel by less than 1/255, the clamp and the float32 quotient by at most 2^-22 more, the Mahalanobis term is exactly 0: the loss (a mean of
    squares) is below (1/255 + 2^-22)^2."""
    from ngp import nav
    agent = nav.NativeAgent(agent_cfg_of(start12(dev)), queries)
    true_pose, true_state, img = agent.step(torch.tensor(ACTION))
    assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == (H, W, 3)
    assert agent.target.dtype == torch.float32 and tuple(agent.target.shape) == (H, W, 3) and tuple(true_pose.shape) == (4, 4)
    assert agent.iter == 1 and tuple(agent.states_history.shape) == (2, 12) and agent.states_history.is_cuda
    assert same_bits(agent.states_history[1], true_state) and same_bits(agent.x, true_state)
    filt = step_filter(queries, "generic", B=H * W)
    res = filt.cost_and_gradient(true_state, true_state, torch.eye(12), agent.target, all_pixels())
    loss, bound = float(res["loss"]), (1 / 255 + 2.0 ** -22) ** 2
    print(f"loss at the true state {loss:.4e}, bound {bound:.4e}; distinct levels in the observation {len(torch.unique(img))}")
    assert float(res["loss"] - res["rgb_loss"]) == 0.0
    assert 0 < loss < bound
    assert len(torch.unique(img)) > 8                                                  # the field is seen, not a blank wall
    assert same_bits(agent.target, (img.double() / 255.0).float())
    # the same step by the filter's propagation; state2image observes a state as it is
    assert torch.equal(true_state, filt.propagate(start12(dev), torch.tensor(ACTION))["state"])
    pose, state, img2 = agent.state2image(true_state.clone())
    assert torch.equal(img2, img) and torch.equal(state, true_state) and tuple(agent.states_history.shape) == (3, 12)
    assert float((pose - agent_step(dyn_of("generic"), start12(dev), torch.tensor(ACTION, device=dev), None)[1]).abs().max()) < 1e-6


def frame_sensor(queries, dev):
    from ngp import workload as Wl
    from ngp.render import NGPRenderer
    ren = NGPRenderer(queries.renderer.field, bound=Wl.BOUND, cuda_ray=True).to(dev).eval()
    ren.density_bitfield.fill_(255)
    return ren


def test_frame_route_is_the_sensor_of_render_fused_over_the_agents_rays(queries, dev):
    from ngp import nav
    from ngp.render import NGPRenderer
    from ngp import workload as Wl
    ren = frame_sensor(queries, dev)
    agent = nav.NativeAgent(agent_cfg_of(start12(dev)), queries, sensor=ren)
    noise = torch.from_numpy(AC.gold()["generic_noise"]).to(dev)
    _, true_state, img = agent.step(torch.tensor(ACTION), noise)
    rays_o, rays_d = agent.rays(true_state)
    image = ren.render_fused(rays_o, rays_d, image_width=W, bg_color=1)["image"]
    png, target = AC.sensor_restated(image.cpu().numpy())
    assert np.array_equal(img.cpu().numpy(), png.reshape(H, W, 3))
    assert np.array_equal(agent.target.cpu().numpy().view(np.uint32), target.reshape(H, W, 3).view(np.uint32))
    own_png, own_target = agent.sense(image)
    assert torch.equal(own_png, img) and same_bits(own_target, agent.target)
    assert len(torch.unique(img)) > 8
    # an unbuilt bitfield and a foreign renderer without a grid are refused, not rendered some other way
    with pytest.raises(ValueError, match="bitfield is empty"):
        nav.NativeAgent(agent_cfg_of(start12(dev)), queries, sensor=NGPRenderer(queries.renderer.field, bound=Wl.BOUND, cuda_ray=True).to(dev).eval())
    with pytest.raises(ValueError, match="cuda_ray=False"):
        nav.NativeAgent(agent_cfg_of(start12(dev)), queries, sensor=NGPRenderer(queries.renderer.field, bound=Wl.BOUND, cuda_ray=False).to(dev).eval())
    nav.NativeAgent(agent_cfg_of(start12(dev)), queries, sensor=queries.renderer)           # the queries' own renderer is sensor=None


def state_at(pose):
    """the state whose sensor camera is `pose` (camera-to-world, +z forward): the inverse of ngp_filter_pose.h's chain P = cycle (rot_x(pi/2) R)
    diag(1, -1, -1), T = cycle position, with R = exp of the state's rotation vector.  Velocities are zero."""
    P, T = np.asarray(pose, np.float64)[:3, :3], np.asarray(pose, np.float64)[:3, 3]
    flip = np.diag([1.0, -1.0, -1.0])
    Rb = np.stack([P[2] @ flip, P[0] @ flip, P[1] @ flip])                  # P[i] = Rb[(i + 1) % 3] diag(1, -1, -1)
    R = np.stack([Rb[0], Rb[2], -Rb[1]])                                    # Rb = rot_x(pi / 2) R: rows R0, -R2, R1
    assert abs(np.linalg.det(R) - 1.0) < 1e-6
    angle = float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
    if np.sin(angle) > 1e-6:
        axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2.0 * np.sin(angle))
    else:                                                                   # a half turn: R = 2 a a^T - I
        k = int(np.argmax(np.diag(R)))
        axis = (R[k] + np.eye(3)[k]) / np.sqrt(2.0 * (R[k, k] + 1.0))
    state = np.zeros(12, np.float32)
    state[[1, 2, 0]] = T                                                    # T[i] = state[(i + 1) % 3]
    state[6:9] = angle * axis
    return state


@pytest.mark.parametrize("name", ["centre", "in_solid"])
def test_the_sensor_sees_the_scene_from_inside_it(queries, oracle, dev, name):
    """The navigation loop's sensor renders from the vehicle's own pose, among the obstacles.  A sensor over the ring scene (field A of
    tests/_default_frame_cases.py), the vehicle at the scene's centre and inside a pillar (tests/_frame_poses.py): the observation is bit for bit the
    sensor's 8-bit round trip of render_fused over ngp_agent_rays' rays, and that frame is within test_gpu_default_frame.check's bars of the CPU
    oracle's march along the same rays."""
    import _default_frame_cases as DC
    import _frame_poses as FP
    from ngp import nav
    from ngp import workload as Wl
    from oracle import render_oracle as R
    from test_gpu_default_frame import check, renderer
    ren = renderer(dev, oracle, DC._case("A", 2.0, None))
    agent = nav.NativeAgent(agent_cfg_of(start12(dev)), queries, sensor=ren)
    _, state, img = agent.state2image(torch.from_numpy(state_at(FP.pose(name))))
    rays_o, rays_d = agent.rays(state)
    o, d = rays_o.cpu().numpy(), rays_d.cpu().numpy()
    want_o, want_d = Wl.get_rays(FP.pose(name), [float(v) for v in queries.intrinsics], H, W)
    assert np.array_equal(o, want_o) and float(np.max(np.abs(d - want_d))) < 1e-5, "the sensor's camera is not where the pose puts it"
    out = ren.render_fused(rays_o, rays_d, image_width=W, bg_color=1)
    assert torch.equal(agent.render(rays_o, rays_d), out["image"])
    png, target = AC.sensor_restated(out["image"].cpu().numpy())
    assert np.array_equal(img.cpu().numpy(), png.reshape(H, W, 3))
    assert np.array_equal(agent.target.cpu().numpy().view(np.uint32), target.reshape(H, W, 3).view(np.uint32))
    assert len(torch.unique(img)) > 8
    ref = R.render_single_march(DC.field_fn(DC.oracle_field("A", 2.0)), o, d, FP.scene(2.0)[0], 2.0, 2)
    assert ref["samples"] > 1000 and 0 < int((ref["consumed"] > 0).sum())
    stats = check(out, ref, DC._case("A", 2.0, (o, d), image_width=W), oracle, f"sensor from {name}")
    assert int(stats[1]) == 0


@pytest.mark.parametrize("route", ["render_fn", "frame"])
def test_step_returns_before_the_device_has_run_it(queries, dev, route):
    """a step queued behind a long-running kernel returns while that kernel is still running: it waits for nothing on the device"""
    from ngp import nav
    agent = nav.NativeAgent(agent_cfg_of(start12(dev)), queries, sensor=frame_sensor(queries, dev) if route == "frame" else None)
    action, noise = torch.tensor(ACTION, device=dev), torch.from_numpy(AC.gold()["generic_noise"]).to(dev)
    for _ in range(2):
        agent.step(action, noise)                                                      # lazy initialisation and the allocator's first blocks, out of the way
    torch.cuda.synchronize()
    busy, begin = torch.cuda.Event(), time.perf_counter()
    torch.cuda._sleep(100_000_000)
    busy.record()
    _, state, img = agent.step(action, noise)
    returned_early, host_ms = not busy.query(), 1e3 * (time.perf_counter() - begin)
    busy.synchronize()
    print(f"{route}: step returned after {host_ms:.2f} ms on the host; the kernel before it ran {1e3 * (time.perf_counter() - begin):.1f} ms")
    assert returned_early
    torch.cuda.synchronize()
    assert agent.iter == 3 and bool(torch.isfinite(state).all()) and tuple(img.shape) == (H, W, 3)


# ------------------------------------------------------------------------------------------------------------------------
# 5. the closed loop
# ------------------------------------------------------------------------------------------------------------------------
def loop_cfgs(dev, scene):
    """test_gpu_plan_astar.py's planner and scene: the 8^3 lattice at a threshold that leaves about 70 % of this field free, between two free cells a path apart"""
    planner_cfg = plan_cfg(start_state=plan_state(centre(scene["start"])), end_state=plan_state(centre(scene["goal"])),
                           a_star=dict(side=SIDE, kernel_size=K, threshold=scene["t"]))
    assert planner_cfg["epochs_init"] == 3 and planner_cfg["epochs_update"] == 2
    agent_cfg = {"dt": planner_cfg["T_final"] / planner_cfg["steps"], "mass": 1.0, "g": 10.0, "I": torch.eye(3)}
    filter_cfg = {"batch_size": 16, "lrate": 1e-3, "N_iter": 4, "sig0": 0.1 * torch.eye(12), "Q": 0.01 * torch.eye(12)}
    extra_cfg = {"mpc_noise_mean": torch.zeros(12, device=dev), "mpc_noise_std": torch.tensor(NOISE_STD, device=dev)}
    return planner_cfg, agent_cfg, filter_cfg, extra_cfg


def loop_by_hand(queries, dev, scene, seed, gen_seed):
    """simulate() spelled out with the public methods"""
    from ngp import nav
    planner_cfg, agent_cfg, filter_cfg, extra_cfg = loop_cfgs(dev, scene)
    gen = torch.Generator(device=dev).manual_seed(gen_seed)
    plan = nav.NativePlanner(planner_cfg["start_state"], planner_cfg["end_state"], planner_cfg, queries)
    plan.a_star_init(side=SIDE, kernel_size=K, threshold=scene["t"], generator=torch.Generator().manual_seed(seed))
    plan.learn_init()
    s18 = planner_cfg["start_state"]
    x0 = torch.cat([s18[:6], nav._rot_matrix_to_vec(s18[6:15].reshape(3, 3)), s18[15:]]).to(dev)
    agent = nav.NativeAgent(dict(agent_cfg, x0=x0), queries)
    filt = nav.NativePoseFilter(filter_cfg, queries, x0, agent_cfg)
    rng = np.random.default_rng(seed)
    steps = int(plan.get_actions().shape[0])
    estimates, actions, noises, branches = [], [], [], []
    for it in range(steps):
        if it < steps - 5:
            action = plan.get_next_action().clone()
        else:
            action = plan.get_actions()[it - steps + 5, :]
        noise = torch.normal(extra_cfg["mpc_noise_mean"], extra_cfg["mpc_noise_std"], generator=gen)
        agent.step(action, noise=noise)
        est = filt.estimate_state(agent.target, action, all_pixels(), rng=rng)
        estimates.append(est), actions.append(action), noises.append(noise), branches.append(it < steps - 5)
        if it < steps - 5:
            plan.update_state(torch.cat([est[:6], nav._vec_to_rot_matrix(est[6:9]).reshape(-1), est[9:]]))
            plan.learn_update(it)
    return dict(true_states=agent.states_history, estimates=torch.stack(estimates), actions=torch.stack(actions), noises=torch.stack(noises),
                branches=branches, steps=steps)


def test_closed_loop_is_its_parts_in_order(queries, dev, scene, tmp_path):
    from ngp import nav
    begin = time.perf_counter()
    hand = loop_by_hand(queries, dev, scene, seed=5, gen_seed=11)
    steps = hand["steps"]
    assert steps >= 7 and hand["branches"][:steps - 5] == [True] * (steps - 5) and hand["branches"][steps - 5:] == [False] * 5     # both branches are taken
    runs = []
    for folder in (None, tmp_path / "run"):
        out = nav.simulate(*loop_cfgs(dev, scene), queries, basefolder=folder, generator=torch.Generator(device=dev).manual_seed(11), interest_regions=all_pixels(),
                           seed=5)
        runs.append(out)
        assert tuple(out["true_states"].shape) == (steps + 1, 12) and tuple(out["estimates"].shape) == (steps, 12)
        assert tuple(out["actions"].shape) == (steps, 4) and tuple(out["noises"].shape) == (steps, 12)
        for key in ("true_states", "estimates", "actions", "noises"):
            assert out[key].is_cuda and out[key].dtype == torch.float32 and same_bits(out[key], hand[key]), key
        assert isinstance(out["planner"], nav.NativePlanner) and isinstance(out["agent"], nav.NativeAgent) and isinstance(out["filter"], nav.NativePoseFilter)
        assert out["agent"].iter == steps and out["filter"].iteration == steps and out["planner"].R == 2
    print(f"{steps} MPC steps; three loops in {time.perf_counter() - begin:.2f} s")
    assert bool(torch.isfinite(runs[0]["true_states"]).all()) and bool(torch.isfinite(runs[0]["estimates"]).all())
    assert float(runs[0]["noises"].abs().max()) > 0 and not torch.equal(runs[0]["true_states"][1:, :3], runs[0]["estimates"][:, :3])
    # the reference's file layout, exactly
    base = tmp_path / "run"
    found = sorted(str(p.relative_to(base)) for p in base.rglob("*") if p.is_file())
    replanned = range(steps - 5)
    want = sorted(["true_states.json", "init_poses/0.json", "init_costs/0.json"] + [f"estimator_data/step{n}.json" for n in range(steps)]
                  + [f"replan_poses/0_time{n}.json" for n in replanned] + [f"replan_costs/0_time{n}.json" for n in replanned])
    assert found == want
    assert sorted(p.name for p in base.iterdir() if p.is_dir()) == sorted(nav.SIMULATE_FOLDERS)
    rows = json.load(open(base / "true_states.json"))["true_states"]
    assert len(rows) == steps + 1 and all(len(r) == 12 for r in rows)
    assert np.array_equal(np.array(rows, np.float32), runs[1]["true_states"].cpu().numpy())
    step0 = json.load(open(base / "estimator_data" / "step0.json"))
    assert sorted(step0) == ["action", "covariance", "grad_states", "loss", "state_estimate"] and len(step0["loss"]) == 4
    # without a folder nothing is written
    assert sorted(p.name for p in tmp_path.iterdir()) == ["run"]



def test_loop_finds_its_own_regions_by_default(queries, dev, scene):
    """interest_regions=None: every time step's regions come from the observation itself (features="native") and the draws from `seed`, so the run repeats bit
    for bit; another seed draws other batches.  (At 20 x 20 pixels the detector may find no keypoint in this field; every step then takes the reference's
    "feature detection failed" path, which the loop must survive just as well, and the seeds cannot differ.)"""
    from ngp import nav
    outs = [nav.simulate(*loop_cfgs(dev, scene), queries, generator=torch.Generator(device=dev).manual_seed(11), seed=s) for s in (5, 5, 6)]
    steps = outs[0]["estimates"].shape[0]
    for key in ("true_states", "estimates", "actions", "noises"):
        assert same_bits(outs[0][key], outs[1][key]), key
    assert outs[0]["filter"].iteration == steps and bool(torch.isfinite(outs[0]["estimates"]).all())
    found = int(outs[0]["filter"].interest_regions(outs[0]["agent"].target).shape[0])
    print(f"{steps} MPC steps; interest pixels in the last observation: {found}")
    if found:
        assert same_bits(outs[0]["noises"], outs[2]["noises"]) and not torch.equal(outs[0]["estimates"], outs[2]["estimates"])
