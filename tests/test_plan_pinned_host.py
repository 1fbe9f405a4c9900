"""CPU: what makes tests/_plan_pinned_cases.py a fair yardstick for the native planner (tests/test_gpu_plan_pinned.py holds csrc/nav_plan.hip to it on
the GPU).  A synthetic analytic density (a few Gaussians along the path) stands in for the field.

  * PinnedDensity, fed a density's own float64 value and Jacobian, reproduces plain float64 autograd of that density;
  * every case is well conditioned: no consecutive rotation near the linearised-acos branch, every thrust above 1, and the float32 restatement within
    4e-6 of its kind's largest reference component per parameter (measured: at most 1.7e-6) and 4e-6 relative per state cost;
  * every case's P, S and B take the kernel path the table claims for it, and no judged kind is empty."""
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")

import _plan_pinned_cases as PC  # noqa: E402


def test_positions_are_those_of_the_float32_planner_tests():
    import test_gpu_nav_plan as NP
    assert PC.SIM_START == NP.SIM_START and PC.SIM_END == NP.SIM_END and PC.BODY == NP.BODY


@pytest.mark.parametrize("name", ["full18", "R3", "B1"])
def test_pinned_density_reproduces_float64_autograd(name):
    inp = PC.inputs(name)
    plain = PC.restated(inp, PC.synthetic_density, torch.float64)
    sigma, jac = PC.value_and_jac(PC.synthetic_density, torch.from_numpy(plain["points"]))
    assert sigma.dtype == torch.float64 and float(sigma.max()) > 0.1
    pin = PC.restated(inp, PC.pinned(sigma, jac), torch.float64)
    assert pin["total"] == plain["total"] and np.array_equal(pin["per_state"], plain["per_state"])
    scale = np.abs(plain["grad"]).max()
    kind, _ = PC.param_layout(inp["R"])
    for k in range(3):
        sel = kind == k
        if sel.any():
            assert np.abs(pin["grad"][sel] - plain["grad"][sel]).max() <= 1e-12 * np.abs(plain["grad"][sel]).max()
    assert np.abs(pin["grad"] - plain["grad"]).max() <= 1e-12 * scale
    # ... and it is the Jacobian it is given, not the points, that it differentiates: the gradient is linear in that Jacobian, the value is not touched
    none, twice = (PC.restated(inp, PC.pinned(sigma, f * jac), torch.float64) for f in (0, 2))
    assert none["total"] == plain["total"] and twice["total"] == plain["total"]
    part = plain["grad"] - none["grad"]                                                # the gradient through the field alone
    assert np.abs(part).max() > 1e-6 * scale
    assert np.abs((twice["grad"] - plain["grad"]) - part).max() <= 1e-12 * scale       # the differences of whole gradients round at their own size


def test_pinned_density_casts_to_the_points_dtype():
    pts = torch.zeros(4, 5, 3, dtype=torch.float64, requires_grad=True)
    sigma32 = torch.arange(20, dtype=torch.float32).reshape(4, 5) / 3
    jac32 = torch.arange(60, dtype=torch.float32).reshape(4, 5, 3) / 7
    out = PC.PinnedDensity.apply(pts, sigma32, jac32)
    assert out.dtype == torch.float64 and torch.equal(out, sigma32.double())
    w = torch.arange(20, dtype=torch.float64).reshape(4, 5) + 1
    (g,) = torch.autograd.grad((out * w).sum(), [pts])
    assert torch.equal(g, w[..., None] * jac32.double())


@pytest.mark.parametrize("name", list(PC.CASES))
def test_case_is_well_conditioned(name):
    inp = PC.inputs(name)
    both = PC.synthetic_reference(name)
    ref, f32 = both["ref"], both["f32"]
    # consecutive rotations: rows 1 .. S-2 involve a rotation the parameters move.  Row 0's pair is fixed by the start state: with a resting start (the
    # stock cases) it is the identity exactly, omega_0 is 0 in every precision and nothing differentiable passes through it
    x = (np.trace(ref["rot"][1:] @ ref["rot"][:-1].swapaxes(-1, -2), axis1=-2, axis2=-1) - 1) / 2
    assert (np.abs(x[1:]) <= 1 - 1e-5).all(), np.abs(x[1:]).max()
    if not abs(x[0]) <= 1 - 1e-5:
        assert PC.CASES[name]["stock"] and (ref["full"][0, 15:] == 0).all() and (f32["full"][0, 15:] == 0).all()
    # ... nor near a half turn, the log map's other pole: omega = ang / (2 sin ang) v / dt, and one ulp of the trace (2^-24 of x) moves it by
    # kappa 2^-24 of itself, kappa = |1 / ang - cot ang| / sin ang (1 / 3 at ang = 0, 2.3 at x = -0.75, 26 at x = -0.98).  The torque cost carries omega
    # to the fourth power, so that one rounding alone must stay within the 4e-6 the whole float32 restatement is held to below: kappa <= 16.7
    ang = np.arccos(x[1:])
    kappa = np.abs(1 / ang - np.cos(ang) / np.sin(ang)) / np.sin(ang)
    assert 4 * kappa.max() * 2.0 ** -24 <= 4e-6, (kappa.max(), x[1:].min())
    assert (ref["actions"][:, 0] / PC.f32(inp["cfg"]["mass"]) > 1.0).all()
    kind, _ = PC.param_layout(inp["R"])
    worst = 0.0
    for k in range(3):
        sel = kind == k
        if sel.any():
            worst = max(worst, np.abs(f32["grad"][sel] - ref["grad"][sel]).max() / np.abs(ref["grad"][sel]).max())
    ps = (np.abs(f32["per_state"] - ref["per_state"]) / np.abs(ref["per_state"])).max()
    print(f"{name}: float32 restatement per parameter {worst:.3g} of its kind's largest component, per_state {ps:.3g} relative; "
          f"x {x[1:].min():.4f} .. {x[1:].max():.6f}, kappa {kappa.max():.3g}")
    assert worst <= 4e-6 and ps <= 4e-6
    assert float(ref["collision"].sum()) > 1.0                                          # the synthetic density is in play too


def test_cases_take_the_paths_the_table_claims():
    shape = {n: (PC.inputs(n)["P"], PC.inputs(n)["S"], PC.inputs(n)["B"]) for n in PC.CASES}
    assert [shape[n][0] for n in ("R126", "R127", "R128")] == [506, 510, 514]           # either side of k_plan_cost_step's 512 lanes
    assert shape["R255"] == (1022, 258, 500) and 18 * 258 > 1024                        # k_plan_kinematics' 1,024 lanes take a second trip
    assert 18 * shape["R128"][1] > 1024 and 18 * shape["stock18"][1] < 1024
    assert [shape[n][2] for n in ("B1", "B63", "B64", "B65")] == [1, 63, 64, 65]        # the wave's lanes: one, all but one, all, one on a second trip
    assert shape["R126"][2] == 65 and shape["stock18"][2] == 500 and 500 % 64 != 0
    assert shape["full18_fade"][1] % 2 == 1 and shape["R3"][1] % 2 == 0                 # the fade mask's linspace mirrors about S / 2
    for n, c in PC.CASES.items():
        assert (c["epoch"] < c["fade"]) == (c["fade"] > 0)                              # a fade case is inside its fade
        inp = PC.inputs(n)
        assert inp["body"].shape == (c["B"], 3) and inp["states"].shape == (c["R"], 4)
        lo, hi = torch.tensor(PC.BODY)[:, 0], torch.tensor(PC.BODY)[:, 1]
        assert bool(((inp["body"] >= lo) & (inp["body"] <= hi)).all())
    full = PC.inputs("full18")
    assert not torch.equal(full["cfg"]["I"], full["cfg"]["I"].T) and full["cfg"]["mass"] != 1 and full["cfg"]["g"] != 10
    assert float(full["start"][15:].norm()) > 0 and float(full["end"][3:6].norm()) > 0 and float(full["end"][15:].norm()) > 0
    for n in ("stock18", "stock60"):
        s = PC.inputs(n)
        assert torch.equal(s["cfg"]["I"], torch.eye(3)) and s["cfg"]["mass"] == 1 and s["cfg"]["g"] == 10 and s["cfg"]["T_final"] == 2
        assert float(s["start"][3:6].norm()) == 0 and float(s["start"][15:].norm()) == 0 and float(s["end"][3:6].norm()) == 0
    for n in PC.CASES:
        if n not in ("stock18", "stock60", "R2", "R3"):                                 # R2, R3: T_final = 2, see _plan_pinned_cases.CASES
            i = PC.inputs(n)
            assert PC.f32(i["cfg"]["T_final"] / i["cfg"]["steps"]) == PC.f32(0.1)


def test_no_judged_kind_is_empty():
    for n in PC.CASES:
        kind, row = PC.param_layout(PC.inputs(n)["R"])
        R = PC.inputs(n)["R"]
        assert (kind == 0).sum() == 2 and (kind == 2).sum() == R and (kind == -1).sum() == 6
        assert (kind == 1).sum() == 3 * (R - 2)
        assert ((kind == 1).sum() > 0) == (R > 2)                                       # positions at R = 2: none, all of states[:, :3] is unused
        assert row.max() == R - 1


def test_yardstick_takes_the_row_window_and_the_percentile():
    e = np.zeros(20)
    e[7] = 1.0
    y = PC.yardstick(e, np.arange(20))
    assert (y[5:10] == 1.0).all() and (y[:5] == 0).all() and (y[10:] == 0).all()
    e = np.full(20, 0.25)
    e[0] = 0.0
    assert (PC.yardstick(e, np.arange(20)) == 0.25).all()
    assert (PC.yardstick(np.zeros(3), np.arange(3), floor=0.5) == 0.5).all()
    with pytest.raises(AssertionError, match="yardsticks"):
        PC.judge("t", "q", np.full(4, 17.0), np.zeros(4), np.ones(4), np.arange(4))
    assert PC.judge("t", "q", np.full(4, 16.0), np.zeros(4), np.ones(4), np.arange(4)) == 16.0
