"""GPU: the native planner (ngp.nav.NativePlanner over csrc/nav_plan.hip) against the reference's own Planner numbers (tests/golden/callers_nav.npz)
and against torch autograd of the restated planner (oracle/nav_oracle.py) + torch.optim.Adam(capturable=True) over the same native density query.

Tolerances: test_gpu_nav_golden.py's (cost 1e-4 relative, gradient 2e-3 relative in norm); kinematics 1e-5; Adam trajectories 1e-4 relative."""
import importlib
import json
import pathlib
import types

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

import _nav_cases as NC  # noqa: E402
from oracle import nav_oracle as NO  # noqa: E402

BODY = [[-0.05, 0.05], [-0.05, 0.05], [-0.02, 0.02]]
SIM_START, SIM_END = [0.39, -0.67, 0.2], [-0.4, 0.55, 0.16]           # simulate.py:236-237


@pytest.fixture(scope="module")
def queries(dev):
    """test_gpu_nav_golden.py's field: NGPField + workload.nav_weights(0), float32"""
    from ngp import nav
    from ngp import workload as W
    from ngp.field import NGPField
    from ngp.render import NGPRenderer
    g = NC.gold()
    model = W.make_model(0)
    sw, cw = W.nav_weights(0)
    field = NGPField(bound=W.BOUND).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(model["embeddings"]))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            layer.weight.copy_(torch.from_numpy(w))
    ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=False).to(dev).eval()
    H, Wd = (int(v) for v in g["mf_HW"])
    return nav.NativeNavQueries(ren, g["mf_intrinsics"], H, Wd, num_steps=int(g["mf_num_steps"]))


def sim_cfg(steps=20, fade_out_epoch=0, **kw):
    cfg = {"T_final": 2., "steps": steps, "lr": 0.001, "epochs_init": 2500, "epochs_update": 250, "fade_out_epoch": fade_out_epoch,
           "fade_out_sharpness": 10, "mass": 1., "I": torch.eye(3), "g": 10., "body": np.array(BODY), "nbins": [10, 10, 5]}
    cfg.update(kw)
    return cfg


def stand_in(dev, cfg, start, end, states, accel, body):
    """an object with the attributes of the reference Planner that NativePlanner reads and writes"""
    return types.SimpleNamespace(cfg=cfg, start_state=start.to(dev), end_state=end.to(dev), states=states.to(dev).requires_grad_(True),
                                 initial_accel=accel.to(dev).requires_grad_(True), robot_body=body.to(dev), epoch=0, dt=cfg["T_final"] / cfg["steps"])


def planner(queries, dev, cfg, start, end, states, accel, body=None):
    from ngp import nav
    if body is None:
        body = NO.robot_body(cfg["body"], cfg["nbins"])
    return nav.NativePlanner.from_planner(stand_in(dev, cfg, start, end, states, accel, body), queries)


def restated(queries, plan, epoch):
    """autograd of the restatement at the planner's current parameters, over the same native density query"""
    st = plan.states.detach().clone().requires_grad_(True)
    ia = plan.initial_accel.detach().clone().requires_grad_(True)
    res = NO.planner_costs(st, ia, plan.start_state, plan.end_state, plan.cfg, plan.robot_body, queries.density_fn, epoch=epoch)
    res["total"].backward()
    return res, st.grad, ia.grad


def check_against_restated(queries, plan, epoch):
    nat = plan.cost_and_gradient(epoch)
    res, gs, ga = restated(queries, plan, epoch)
    np.testing.assert_allclose(float(nat["total"]), float(res["total"].detach()), rtol=1e-4)
    np.testing.assert_allclose(nat["per_state"].cpu().numpy(), res["per_state"].detach().cpu().numpy(), rtol=1e-4)
    np.testing.assert_allclose(nat["collision"].cpu().numpy(), res["collision"].detach().cpu().numpy(), rtol=1e-4, atol=1e-6)
    g_nat = torch.cat([nat["grad_initial_accel"], nat["grad_states"].reshape(-1)]).cpu().numpy()
    g_ref = torch.cat([ga, gs.reshape(-1)]).cpu().numpy()
    assert NC.rel(g_nat, g_ref) < 2e-3, NC.rel(g_nat, g_ref)
    return nat, res


# ------------------------------------------------------------------------------------------------------------------------
# 1. the reference's own numbers
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["pl", "plf"])
def test_cost_and_gradient_against_executed_planner(queries, dev, tag):
    g = NC.gold()
    t = lambda k: torch.from_numpy(g[f"{tag}_{k}"])                                    # noqa: E731
    cfg = dict(NC.planner_cfg(g, tag), lr=0.001, epochs_init=1, epochs_update=1, body=np.array(BODY), nbins=g[f"{tag}_nbins"])
    plan = planner(queries, dev, cfg, t("start"), t("end"), t("states"), t("initial_accel"), t("robot_body"))
    res = plan.cost_and_gradient(int(g[f"{tag}_epoch"]))
    np.testing.assert_allclose(float(res["total"]), float(g[f"{tag}_total"]), rtol=1e-4)
    np.testing.assert_allclose(res["per_state"].cpu().numpy(), g[f"{tag}_per_state"], rtol=1e-4)
    np.testing.assert_allclose(res["collision"].cpu().numpy(), g[f"{tag}_collision"], rtol=1e-4, atol=1e-6)
    assert NC.rel(res["grad_states"].cpu().numpy(), g[f"{tag}_grad_states"]) < 2e-3
    assert NC.rel(res["grad_initial_accel"].cpu().numpy(), g[f"{tag}_grad_initial_accel"]) < 2e-3
    np.testing.assert_allclose(plan.body_to_world().cpu().numpy(), g[f"{tag}_points"], rtol=0, atol=1e-6)
    if tag == "pl":
        np.testing.assert_allclose(plan.get_actions().cpu().numpy(), g["pl_actions"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(plan.get_full_states().cpu().numpy(), g["pl_full_states"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(plan.get_next_action().cpu().numpy(), g["pl_actions"][0], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------------
# 2. autograd of the restatement over the same density, many parameter sets
# ------------------------------------------------------------------------------------------------------------------------
def zigzag(steps, seed):
    """like a smoothed A* path (nav/quad_plot.py:65-118): grid-aligned steps with a lateral zig-zag through the occupied middle of the scene,
    N(0, 0.001) noise, the 3-point smoothing"""
    gen = torch.Generator().manual_seed(seed)
    n = steps - 2
    s = torch.linspace(0, 1, n)[:, None]
    a, b = torch.tensor(SIM_START), torch.tensor(SIM_END)
    path = (1 - s) * a + s * b
    path[:, 0] += 0.1 * torch.tensor([(-1.0) ** k for k in range(n)])
    path = torch.round(path * 10) / 10
    states = torch.cat([path, torch.zeros(n, 1)], dim=-1) + 0.001 * torch.randn(n, 4, generator=gen)
    prev = torch.cat([states[:1], states[:-1]]); nxt = torch.cat([states[1:], states[-1:]])
    return (prev + nxt + states) / 3


# Perturbations are N(0, 0.01) at dt = 0.1 and scaled with dt^2 at R = 60 (dt = 0.032): there 0.01 would swing consecutive thrust axes by up to
# ~pi, where the log map's 1 / sin(angle) makes every float32 rounding of the trace visible in 1e12-sized torque costs -- on both sides.
CASES = {  # name: (steps, fade_out_epoch, epoch, kind, seed)
    "line": (20, 0, 0, "line", 0),
    "line_fade": (20, 100, 10, "line", 0),
    "pert_a": (20, 0, 0, "pert", 1),
    "pert_b_fade": (20, 50, 7, "pert", 2),
    "zigzag": (20, 0, 0, "zigzag", 3),
    "zigzag_fade": (20, 40, 30, "zigzag", 4),
    "R2": (4, 0, 0, "pert", 5),
    "R3": (5, 10, 2, "pert", 6),
    "R60": (62, 0, 0, "pert", 7),
    "R60_line": (62, 0, 0, "line", 0),
}


def case_states(kind, steps, seed, start, end):
    line = NO.planner_initial_states(start, end, steps)
    if kind == "line":
        return line
    if kind == "zigzag":
        return zigzag(steps, seed)
    gen = torch.Generator().manual_seed(seed)
    amp = 0.01 * min(1.0, (20 / steps) ** 2)
    return line + amp * torch.randn(line.shape, generator=gen)


@pytest.mark.parametrize("name", list(CASES))
def test_cost_and_gradient_against_autograd_of_the_restatement(queries, dev, name):
    steps, fade, epoch, kind, seed = CASES[name]
    start, end = NO.state18(SIM_START), NO.state18(SIM_END)
    cfg = sim_cfg(steps, fade)
    plan = planner(queries, dev, cfg, start, end, case_states(kind, steps, seed, start, end), torch.tensor([10.3, 9.7]))
    assert plan.R == steps - 2
    nat, res = check_against_restated(queries, plan, epoch)
    if kind == "zigzag":
        assert float(res["collision"].detach().sum()) > 1.0                              # the collision term is in play
    if kind == "line":
        # consecutive rotations near identity: the linearised acos branch
        pos, vel, acc, rot, *_ = NO.planner_kinematics(plan.states, plan.initial_accel, plan.start_state, plan.end_state, cfg)
        x = (torch.diagonal(rot[1:] @ rot[:-1].swapdims(-1, -2), dim1=-2, dim2=-1).sum(-1) - 1) / 2
        assert bool((x.abs() > 1 - 1e-7).any())


# ------------------------------------------------------------------------------------------------------------------------
# 3. Adam
# ------------------------------------------------------------------------------------------------------------------------
ADAM_CASE = dict(steps=12, z=3.0, amp=0.05)


def adam_start(dev, queries):
    """a seeded perturbation whose gradient components (those the cost depends on at all: not states[0:2, :3]) are all >= 1e-3 of its norm"""
    st, en = NO.state18([SIM_START[0], SIM_START[1], SIM_START[2] + ADAM_CASE["z"]]), NO.state18([SIM_END[0], SIM_END[1], SIM_END[2] + ADAM_CASE["z"]])
    cfg = sim_cfg(ADAM_CASE["steps"])
    line = NO.planner_initial_states(st, en, ADAM_CASE["steps"])
    gen = torch.Generator().manual_seed(ADAM_SEED)
    plan = planner(queries, dev, cfg, st, en, line + ADAM_CASE["amp"] * torch.randn(line.shape, generator=gen), torch.tensor([10.3, 9.7]))
    return plan


ADAM_SEED = 8


def torch_adam_epochs(queries, plan, n, first_epoch=0):
    """n epochs of Planner.learn_* on the restatement: a new torch.optim.Adam(capturable=True) per call"""
    st = plan.states.detach().clone().requires_grad_(True)
    ia = plan.initial_accel.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([ia, st], lr=plan.cfg["lr"], capturable=True)
    losses = []
    for it in range(n):
        opt.zero_grad()
        loss = NO.planner_costs(st, ia, plan.start_state, plan.end_state, plan.cfg, plan.robot_body, queries.density_fn, epoch=first_epoch + it)["total"]
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return st.detach(), ia.detach(), torch.stack(losses)


def test_adam_epochs_against_torch_adam(queries, dev):
    plan = adam_start(dev, queries)
    _, gs, ga = restated(queries, plan, 0)
    used = torch.ones_like(gs, dtype=torch.bool)
    used[:2, :3] = False
    g = torch.cat([ga, gs[used]])
    assert float((g.abs() / g.norm()).min()) >= 1e-3                             # no component's sign is noise
    ref_s, ref_a, ref_l = torch_adam_epochs(queries, plan, 20)
    adam = plan.new_adam_state()
    losses = torch.empty(20, device=dev)
    plan.run_epochs(0, 20, adam, losses=losses)
    np.testing.assert_allclose(losses.cpu().numpy(), ref_l.cpu().numpy(), rtol=1e-4)
    assert NC.rel(plan.states.cpu().numpy(), ref_s.cpu().numpy()) < 1e-4
    assert NC.rel(plan.initial_accel.cpu().numpy(), ref_a.cpu().numpy()) < 1e-4
    assert float(adam[-1]) == 20.0
    # learn_update restarts the moments: 5 more epochs from fresh moments on both sides
    ref_s2, ref_a2, ref_l2 = torch_adam_epochs(queries, plan, 5)
    plan.cfg["epochs_update"] = 5
    plan.epochs_update = 5
    plan.learn_update(0)
    np.testing.assert_allclose(plan.losses.cpu().numpy(), ref_l2.cpu().numpy(), rtol=1e-4)
    assert NC.rel(plan.states.cpu().numpy(), ref_s2.cpu().numpy()) < 1e-4
    # ... which continuing the old moments would not give
    cont = plan.new_adam_state()
    assert not torch.equal(cont, adam)


# ------------------------------------------------------------------------------------------------------------------------
# 4. along a long run, 5. reproducible
# ------------------------------------------------------------------------------------------------------------------------
def test_gradient_along_a_long_run(queries, dev):
    start, end = NO.state18(SIM_START), NO.state18(SIM_END)
    cfg = sim_cfg()
    plan = planner(queries, dev, cfg, start, end, NO.planner_initial_states(start, end, 20), torch.tensor([10., 10.]))
    adam = plan.new_adam_state()
    losses = torch.empty(2500, device=dev)
    for k in range(10):
        plan.run_epochs(250 * k, 250, adam, losses=losses[250 * k:])
        check_against_restated(queries, plan, 250 * (k + 1))
    assert bool(torch.isfinite(losses).all()) and float(losses[-1]) < float(losses[0])


def test_two_runs_are_bit_identical(queries, dev):
    start, end = NO.state18(SIM_START), NO.state18(SIM_END)
    out = []
    for _ in range(2):
        plan = planner(queries, dev, sim_cfg(), start, end, zigzag(20, 3), torch.tensor([10.3, 9.7]))
        adam = plan.new_adam_state()
        losses = torch.empty(100, device=dev)
        plan.run_epochs(0, 100, adam, losses=losses)
        out.append((plan.states.cpu(), plan.initial_accel.cpu(), losses.cpu(), adam.cpu()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------------
# 6. semantics
# ------------------------------------------------------------------------------------------------------------------------
def test_update_state_matches_the_restatement(queries, dev):
    start, end = NO.state18(SIM_START), NO.state18(SIM_END)
    cfg = sim_cfg()
    plan = planner(queries, dev, cfg, start, end, case_states("pert", 20, 1, start, end), torch.tensor([10.3, 9.7]))
    *_, actions = NO.planner_kinematics(plan.states, plan.initial_accel, plan.start_state, plan.end_state, cfg)
    old = plan.states.clone()
    measured = NO.state18([0.38, -0.6, 0.21], rotvec=(0.01, 0.0, 0.02)).to(dev)
    plan.update_state(measured)
    assert plan.R == 17 and torch.equal(plan.states, old[1:])
    np.testing.assert_allclose(plan.initial_accel.cpu().numpy(), actions[1:3, 0].cpu().numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(plan.start_state, measured)
    check_against_restated(queries, plan, 0)
    *_, a2 = NO.planner_kinematics(plan.states, plan.initial_accel, plan.start_state, plan.end_state, cfg)
    np.testing.assert_allclose(plan.get_actions().cpu().numpy(), a2.cpu().numpy(), rtol=1e-5, atol=1e-4)


def test_from_planner_store_into_round_trip(queries, dev):
    from ngp import nav
    start, end = NO.state18(SIM_START), NO.state18(SIM_END)
    cfg = sim_cfg(epochs_init=30)
    ref = stand_in(dev, cfg, start, end, case_states("pert", 20, 2, start, end), torch.tensor([10.3, 9.7]), NO.robot_body(BODY, [10, 10, 5]))
    plan = nav.NativePlanner.from_planner(ref, queries)
    assert torch.equal(plan.states, ref.states.detach()) and torch.equal(plan.robot_body, ref.robot_body)
    plan.learn_init()
    assert plan.losses.shape == (30,) and plan.losses.is_cuda
    plan.store_into(ref)
    assert ref.states.is_leaf and ref.states.requires_grad and ref.initial_accel.is_leaf and ref.initial_accel.requires_grad
    assert torch.equal(ref.states.detach(), plan.states) and torch.equal(ref.initial_accel.detach(), plan.initial_accel)
    again = nav.NativePlanner.from_planner(ref, queries)
    assert torch.equal(again.states, plan.states)
    # a fresh planner builds the reference's straight line and body cloud
    fresh = nav.NativePlanner(start, end, cfg, queries)
    np.testing.assert_allclose(fresh.states.cpu().numpy(), NO.planner_initial_states(start, end, 20).numpy(), atol=1e-6)
    assert torch.equal(fresh.robot_body.cpu(), NO.robot_body(BODY, [10, 10, 5]))
    assert fresh.initial_accel.tolist() == [10., 10.]


def test_non_native_queries_raise(queries):
    from ngp import nav
    chain = nav.NavQueries(queries.renderer, queries.intrinsics, queries.H, queries.W)
    with pytest.raises(ValueError, match="NativeNavQueries"):
        nav.NativePlanner(NO.state18(SIM_START), NO.state18(SIM_END), sim_cfg(), chain)


def test_saves_write_the_reference_keys(queries, dev, tmp_path):
    start, end = NO.state18(SIM_START), NO.state18(SIM_END)
    cfg = sim_cfg(epochs_init=60, epochs_update=51)
    plan = planner(queries, dev, cfg, start, end, NO.planner_initial_states(start, end, 20), torch.tensor([10., 10.]))
    plan.basefolder = pathlib.Path(tmp_path)
    for d in ("init_poses", "init_costs", "replan_poses", "replan_costs"):
        (tmp_path / d).mkdir()
    plan.learn_init()
    assert sorted(p.name for p in (tmp_path / "init_poses").iterdir()) == ["0.json", "1.json"]
    poses = json.load(open(tmp_path / "init_poses" / "1.json"))
    assert list(poses) == ["poses"] and np.array(poses["poses"]).shape == (plan.S, 4, 4)
    costs = json.load(open(tmp_path / "init_costs" / "1.json"))
    assert list(costs) == ["colision_loss", "pos", "actions", "total_cost"]
    assert np.array(costs["actions"]).shape == (plan.S, 4) and len(costs["total_cost"]) == plan.S
    plan.learn_update(3)
    assert sorted(p.name for p in (tmp_path / "replan_costs").iterdir()) == ["0_time3.json", "1_time3.json"]
    # the chunks (1 + 50 + 9 epochs) are the same epochs as one call
    other = planner(queries, dev, cfg, start, end, NO.planner_initial_states(start, end, 20), torch.tensor([10., 10.]))
    other.learn_init()
    plan2 = planner(queries, dev, cfg, start, end, NO.planner_initial_states(start, end, 20), torch.tensor([10., 10.]))
    plan2.basefolder = pathlib.Path(tmp_path)
    plan2.learn_init()
    assert torch.equal(other.states, plan2.states) and torch.equal(other.losses, plan2.losses)
