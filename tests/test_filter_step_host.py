"""CPU: the pose filter's native time step (include/ngp_hip.h: ngp_filter_propagate, ngp_filter_hessian; csrc/nav_filter.hip) -- exported symbols, the
host struct and every refusal, none of which touches a device; ngp.nav.drone_dynamics against the EXECUTED reference (tests/golden/
callers_estimator.npz, written by tests/golden/make_estimator_golden.py); and the host side of NativePoseFilter.estimate_state / save_data."""
import ctypes
import importlib
import json
import os
import re
import types

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
import ngp_hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ngp_filter_propagate", "ngp_filter_hessian")
EINVAL, EWORKSPACE = -1, -3
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "callers_estimator.npz"))
NAMES = [str(n) for n in GOLD["names"]]


def test_step_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    assert "ngp_filter_dyn_t" in header
    for name in NEW:
        assert name in ngp_hip.EXPORTS and f"{name}(" in header
        getattr(ngp_hip.lib(), name)


def test_dyn_struct_matches_the_header_field_for_field():
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ngp_filter_dyn_t;", header).group(1)
    declared = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("float ")
            declared += [re.sub(r"\[\d+\]", "", n.strip()) for n in decl[len("float "):].split(",")]
    assert declared == [n for n, _ in ngp_hip.ngp_filter_dyn_t._fields_] == ["dt", "mass", "g", "I"]
    assert ctypes.sizeof(ngp_hip.ngp_filter_dyn_t) == 4 * (3 + 9)


# ------------------------------------------------------------------------------------------------------------------------
# refusals: fake pointers, no device
# ------------------------------------------------------------------------------------------------------------------------
def _fake(n=16):
    return ctypes.c_void_p(n)                                                     # never dereferenced: validation fails first


def _dyn(dt=0.1, mass=1.0, g=10.0, I=(1, 0, 0, 0, 1, 0, 0, 0, 1)):
    d = ngp_hip.ngp_filter_dyn_t()
    d.dt, d.mass, d.g = dt, mass, g
    d.I[:] = [float(v) for v in I]
    return d


def _propagate(L, d, state=True, action=True, sig=True, Q=True, nxt=True, A=True, sig_prop=True):
    f = _fake()
    p = lambda on: f if on else None                                               # noqa: E731
    return L.ngp_filter_propagate(ctypes.byref(d) if d is not None else None, p(state), p(action), p(sig), p(Q), p(nxt), p(A), p(sig_prop), None)


def test_filter_propagate_refusals_need_no_device():
    L = ngp_hip.lib().raw
    assert _propagate(L, None) == EINVAL and b"null cfg" in L.ngp_last_error()
    for missing in ("state", "action", "nxt"):
        assert _propagate(L, _dyn(), **{missing: False}) == EINVAL, missing
        assert b"null state" in L.ngp_last_error()
    for missing in ("sig", "Q"):
        assert _propagate(L, _dyn(), **{missing: False}) == EINVAL, missing
        assert b"sig_prop needs sig and Q" in L.ngp_last_error()
    inf, nan = float("inf"), float("nan")
    for bad in (dict(dt=0.0), dict(dt=-0.1), dict(dt=inf), dict(dt=nan), dict(mass=0.0), dict(mass=-1.0), dict(mass=inf), dict(mass=nan)):
        assert _propagate(L, _dyn(**bad)) == EINVAL, bad
        assert b"finite and > 0" in L.ngp_last_error()
    for I in ((0,) * 9, (1, 2, 3, 2, 4, 6, 0, 0, 1), (nan, 0, 0, 0, 1, 0, 0, 0, 1), (inf, 0, 0, 0, 1, 0, 0, 0, 1), (0, 0, 0, 0, 1, 0, 0, 0, 1)):
        assert _propagate(L, _dyn(I=I)) == EINVAL, I
        assert b"singular" in L.ngp_last_error()


def _cfg(B=16, num_steps=64):
    c = ngp_hip.ngp_filter_cfg_t()
    c.H, c.W, c.num_steps, c.B = 20, 20, num_steps, B
    c.intrinsics[:] = [27.8, 27.8, 10.0, 10.0]
    c.aabb[:] = [-1, -1, -1, 1, 1, 1]
    c.min_near = 0.2
    c.bg[:] = [1, 1, 1]
    c.sig_inv[:] = [1.0 if k % 13 == 0 else 0.0 for k in range(144)]
    c.lr, c.beta1, c.beta2, c.eps = 1e-3, 0.9, 0.999, 1e-8
    return c


def _hessian(L, c, field=None, state=True, target=True, batch=True, hessian=True, ws=True, ws_bytes=1 << 40):
    f = _fake()
    field = ngp_hip.ngp_nav_field_t() if field is None else field
    p = lambda on: f if on else None                                               # noqa: E731
    return L.ngp_filter_hessian(ctypes.byref(field), f, ctypes.byref(c) if c is not None else None, p(state), p(target), p(batch), p(hessian),
                                None, None, None, p(ws), ws_bytes, None)


def test_filter_hessian_refusals_need_no_device():
    L = ngp_hip.lib().raw
    assert _hessian(L, None) == EINVAL and b"null cfg" in L.ngp_last_error()
    assert _hessian(L, _cfg(B=0)) == EINVAL and b"B = 0" in L.ngp_last_error()
    assert _hessian(L, _cfg(B=(1 << 20) + 1)) == EINVAL
    for T in (0, 4097, 1 << 20):
        assert _hessian(L, _cfg(num_steps=T)) == EINVAL, T
        assert b"num_steps" in L.ngp_last_error()
    for missing in ("state", "target", "batch", "hessian"):
        assert _hessian(L, _cfg(), **{missing: False}) == EINVAL, missing
        assert b"null state" in L.ngp_last_error()
    need = L.ngp_filter_workspace(16, 64)
    assert _hessian(L, _cfg(), ws_bytes=need - 1) == EWORKSPACE
    assert _hessian(L, _cfg(), ws=False, ws_bytes=need) == EWORKSPACE
    # a large enough workspace: the field is judged next, before anything is queued
    assert _hessian(L, _cfg(), ws_bytes=need) == EINVAL and b"null field" in L.ngp_last_error()
    f = _fake()
    keep = (ctypes.c_int32 * 17)(*([0] * 17))
    fld = ngp_hip.ngp_nav_field_t(f, ctypes.cast(keep, ctypes.c_void_p), f, f, f, f, f, 16, 16, 1.0, 1.0, 1.0)
    assert _hessian(L, _cfg(), field=fld, ws_bytes=need) == EINVAL and b"empty level" in L.ngp_last_error()


# ------------------------------------------------------------------------------------------------------------------------
# ngp.nav.drone_dynamics against the executed reference
# ------------------------------------------------------------------------------------------------------------------------
def _restated(name, dtype):
    from ngp import nav
    dt, mass, g = (float(v) for v in GOLD[f"{name}_cfg"])
    x = torch.from_numpy(GOLD[f"{name}_state"]).to(dtype)
    a = torch.from_numpy(GOLD[f"{name}_action"]).to(dtype)
    I = torch.from_numpy(GOLD[f"{name}_I"]).to(dtype)
    fn = lambda s: nav.drone_dynamics(s, a, dt, mass, g, I)                        # noqa: E731
    nxt = fn(x)
    assert nxt.dtype == dtype and tuple(nxt.shape) == (12,)
    return nxt.detach().numpy(), torch.autograd.functional.jacobian(fn, x).numpy()


def test_fixture_cases_are_what_their_names_say_and_float64_is_a_fair_yardstick():
    assert NAMES == ["generic", "omega_zero", "hover_at_zero", "filter_start", "small_angle", "large_angle", "full_inertia"]
    s = {n: GOLD[f"{n}_state"] for n in NAMES}
    assert np.all(s["omega_zero"][9:] == 0) and np.all(GOLD["omega_zero_A_f64"][6:9, 9:12] == 0)          # theta == 0: no derivative through omega
    assert np.all(s["hover_at_zero"][6:] == 0) and GOLD["hover_at_zero_action"][0] == GOLD["hover_at_zero_cfg"][1] * GOLD["hover_at_zero_cfg"][2]
    assert np.all(s["filter_start"][6:] == np.float32(1e-6))
    assert abs(np.linalg.norm(s["small_angle"][6:9]) - 2e-2) < 2e-3 and abs(np.linalg.norm(s["large_angle"][6:9]) - 2.4) < 0.05
    I = GOLD["full_inertia_I"]
    assert np.array_equal(I, I.T) and np.abs(I - np.diag(np.diag(I))).max() > 0.01
    np.testing.assert_allclose(GOLD["full_inertia_cfg"], [0.05, 1.7, 9.81], rtol=1e-7)
    sig, Q = GOLD["sig"], GOLD["Q"]
    assert np.abs(sig - sig.T).max() > 1e-3 and np.linalg.cond(sig.astype(np.float64)) < 100 and np.array_equal(Q, np.diag(np.diag(Q)))
    for n in NAMES:
        angle = float(np.linalg.norm(GOLD[f"{n}_next_f64"][6:9]))
        assert angle <= np.pi - 0.2, (n, angle)                                    # the log map's 1 / sin
        x = _next_trace_term(n)
        assert abs(abs(x) - (1 - 1e-7)) > 1e-9, (n, x)                             # not at acos_safe's branch point


def _rot64(r):
    r = np.asarray(r, np.float64)
    a = np.linalg.norm(r)
    k = r / (1e-10 + a)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def _next_trace_term(name):
    """(trace(next_R) - 1) / 2 of drone_dynamics, in float64 numpy"""
    st = GOLD[f"{name}_state"].astype(np.float64)
    R = _rot64(st[6:9])
    step = st[9:] * float(GOLD[f"{name}_cfg"][0])
    th = np.linalg.norm(step)
    if th == 0:
        E = np.eye(3)
    else:
        n = step / th
        K = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]])
        E = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    return (np.trace(R @ E) - 1) / 2


@pytest.mark.parametrize("name", NAMES)
def test_drone_dynamics_float64_equals_the_executed_reference(name):
    nxt, A = _restated(name, torch.float64)
    for got, ref in ((nxt, GOLD[f"{name}_next_f64"]), (A, GOLD[f"{name}_A_f64"])):
        assert ref.dtype == np.float64
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(name, "relative distance from the executed float64", err)
        assert err <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_drone_dynamics_float32_equals_the_executed_reference_within_its_own_rounding(name):
    nxt, A = _restated(name, torch.float32)
    for tag, got in (("next", nxt), ("A", A)):
        f32, f64 = GOLD[f"{name}_{tag}_f32"], GOLD[f"{name}_{tag}_f64"]
        assert f32.dtype == np.float32
        own = np.abs(f32.astype(np.float64) - f64).max()                           # the reference's float32 against its float64
        err = np.abs(got.astype(np.float64) - f32.astype(np.float64)).max()
        print(name, tag, "distance from the executed float32", err, "that one's distance from float64", own)
        assert err <= own


def test_sig_prop_of_the_fixture_is_estimate_states_formula():
    for n in NAMES:
        A = GOLD[f"{n}_A_f64"]
        ref = A @ GOLD["sig"].astype(np.float64) @ A.T + GOLD["Q"].astype(np.float64)
        np.testing.assert_allclose(GOLD[f"{n}_sig_prop_f64"], ref, rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------------------------------
# NativePoseFilter's host side
# ------------------------------------------------------------------------------------------------------------------------
AGENT = {"dt": 0.1, "mass": 1.0, "g": 10.0, "I": torch.eye(3)}


def _host_filter(agent_cfg=AGENT):
    """a NativePoseFilter around a stand-in for the queries, on the CPU; `propagate` is the torch route (nav.drone_dynamics and its autograd Jacobian)"""
    from ngp import nav
    filt = nav.NativePoseFilter.__new__(nav.NativePoseFilter)
    filt.queries = types.SimpleNamespace(H=20, W=20)
    filt.device = torch.device("cpu")
    filt.batch_size, filt.iter = 16, 4
    filt.agent_cfg = agent_cfg
    filt.sig, filt.Q = torch.from_numpy(GOLD["sig"]), torch.from_numpy(GOLD["Q"])
    filt.xt = torch.from_numpy(GOLD["generic_state"])
    filt.losses = filt.states = filt.grads = filt.target = filt.batch = None
    filt.action = filt.covariance_estimate = filt.state_estimate = None
    filt.iteration = 0
    calls = []

    def propagate(state, action, sig=None, Q=None):
        calls.append("propagate")
        fn = lambda s: nav.drone_dynamics(s, action, AGENT["dt"], AGENT["mass"], AGENT["g"], AGENT["I"])       # noqa: E731
        A = torch.autograd.functional.jacobian(fn, state)
        return dict(state=fn(state).detach(), A=A, sig_prop=(A @ sig) @ A.T + Q)

    def never(*a, **k):
        raise AssertionError("the failure path runs neither the loop nor the Hessian")

    filt.propagate, filt.estimate_relative_pose, filt.measurement_hessian = propagate, never, never
    return filt, calls


@pytest.mark.parametrize("regions", [None, np.zeros((0, 2), np.int64), np.zeros((0,), np.int64)])
def test_estimate_state_without_interest_points_returns_the_propagated_state_and_keeps_sig(regions, tmp_path):
    from ngp import nav
    filt, calls = _host_filter()
    sig0, x0 = filt.sig.clone(), filt.xt.clone()
    action = torch.from_numpy(GOLD["generic_action"])
    xt = filt.estimate_state(torch.zeros(20, 20, 3), action, regions)
    assert calls == ["propagate"]
    assert torch.equal(xt, nav.drone_dynamics(x0, action, AGENT["dt"], AGENT["mass"], AGENT["g"], AGENT["I"])) and torch.equal(filt.xt, xt)
    assert torch.equal(torch.as_tensor(filt.sig), sig0)                           # the previous posterior, not sig_prop
    assert filt.losses == [] and filt.states == []
    assert filt.iteration == 1 and filt.action == action.tolist() and filt.state_estimate == xt.tolist() and filt.covariance_estimate == sig0.tolist()
    path = tmp_path / "step0.json"
    filt.save_data(path)
    data = json.load(open(path))
    assert list(data) == ["loss", "covariance", "state_estimate", "grad_states", "action"]
    assert data["loss"] == [] and data["grad_states"] == [] and data["covariance"] == sig0.tolist() and data["state_estimate"] == xt.tolist()
    assert data["action"] == action.tolist()


def test_save_data_writes_the_histories_of_a_loop():
    import tempfile
    filt, _ = _host_filter()
    filt.losses, filt.states = torch.tensor([0.5, 0.25]), torch.arange(24.).reshape(2, 12)
    filt.covariance_estimate, filt.state_estimate, filt.action = torch.eye(12).tolist(), list(range(12)), [1.0, 0.0, 0.0, 0.0]
    with tempfile.TemporaryDirectory() as d:
        filt.save_data(os.path.join(d, "s.json"))
        data = json.load(open(os.path.join(d, "s.json")))
    assert data["loss"] == [0.5, 0.25] and data["grad_states"] == torch.arange(24.).reshape(2, 12).tolist() and data["action"] == [1.0, 0.0, 0.0, 0.0]


def test_propagate_without_agent_cfg_raises():
    from ngp import nav
    filt = nav.NativePoseFilter.__new__(nav.NativePoseFilter)
    filt.device, filt.agent_cfg = torch.device("cpu"), None
    with pytest.raises(ValueError, match="agent_cfg"):
        filt.propagate(torch.zeros(12), torch.zeros(4))
    with pytest.raises(ValueError, match="agent_cfg"):
        filt.propagate(torch.zeros(12), torch.zeros(4), torch.eye(12), torch.eye(12))


def test_constructor_takes_agent_cfg_last_and_defaults_to_none():
    import inspect
    from ngp import nav
    params = list(inspect.signature(nav.NativePoseFilter.__init__).parameters.values())
    assert [p.name for p in params] == ["self", "filter_cfg", "queries", "start_state", "agent_cfg"] and params[3].default is None and params[4].default is None
    sig = inspect.signature(nav.NativePoseFilter.measurement_hessian)
    assert list(sig.parameters) == ["self", "state", "start_state", "sig", "native"] and sig.parameters["native"].default is False
