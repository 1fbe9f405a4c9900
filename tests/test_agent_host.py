"""CPU: the agent's three entry points (include/ngp_hip.h: ngp_agent_step, ngp_agent_rays, ngp_agent_sensor; csrc/nav_agent.hip) -- declared, bound and built;
their refusals, none of which touches a device; the numpy restatement of the sensor contract against the reference's literal expressions; the loop's action
rule; and the golden file of Agent.step (tests/golden/agent.npz) against ngp.nav's torch restatement of the dynamics."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
import ngp_hip  # noqa: E402

import _agent_cases as AC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ngp_agent_step", "ngp_agent_rays", "ngp_agent_sensor")
EINVAL = -1


def test_header_ctypes_table_and_makefile_agree():
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    makefile = open(os.path.join(ROOT, "nerf-navigation_amd", "csrc", "Makefile")).read()
    source = open(os.path.join(ROOT, "nerf-navigation_amd", "csrc", "nav_agent.hip")).read()
    srcs = re.search(r"^SRCS = (.*)$", makefile, re.M).group(1).split()
    assert "nav_agent.hip" in srcs
    assert "ngp_filter_pose.h" in makefile                                         # the shared pose chain is a dependency of every object
    for name in NEW:
        assert name in ngp_hip.EXPORTS and f'extern "C" int {name}(' in source
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        res, args = ngp_hip._SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, params)
        for p, a in zip(params, args):
            assert (a is ctypes.c_uint32) == p.startswith("uint32_t "), (name, p)
            assert (a is ctypes.c_void_p) == ("*" in p), (name, p)
        assert params[-1] == "void* stream"
        getattr(ngp_hip.lib(), name)


def test_the_pose_chain_has_one_copy():
    """nf_pose and ngp_camera_ray are defined once and used by both the filter's and the agent's ray kernels"""
    csrc = os.path.join(ROOT, "nerf-navigation_amd", "csrc")
    read = lambda f: open(os.path.join(csrc, f)).read()                            # noqa: E731
    definitions = [f for f in os.listdir(csrc) if re.search(r"void nf_pose\(", read(f))]
    assert definitions == ["ngp_filter_pose.h"]
    for f in ("nav_filter.hip", "nav_agent.hip"):
        text = read(f)
        assert '#include "ngp_filter_pose.h"' in text and "nf_pose(" in text and "ngp_camera_ray(" in text
    assert "nfs_drone_dynamics(" in read("nav_agent.hip") and "void nfs_drone_dynamics" not in read("nav_agent.hip")


def _fake(n=16):
    return ctypes.c_void_p(n)                                                      # never dereferenced: validation fails first


def _dyn(dt=0.1, mass=1.0, g=10.0, I=(1, 0, 0, 0, 1, 0, 0, 0, 1)):
    d = ngp_hip.ngp_filter_dyn_t()
    d.dt, d.mass, d.g = dt, mass, g
    d.I[:] = [float(v) for v in I]
    return d


def test_refusals_touch_no_device():
    L = ngp_hip.lib()
    err = lambda: L.ngp_last_error().decode()                                      # noqa: E731
    f = _fake()
    assert L.ngp_agent_step(None, f, f, None, f, f, f, None) == EINVAL and "null cfg" in err()
    for state, action, nxt in ((None, f, f), (f, None, f), (f, f, None)):
        assert L.ngp_agent_step(ctypes.byref(_dyn()), state, action, None, nxt, f, f, None) == EINVAL and "null state" in err()
    assert L.ngp_agent_step(ctypes.byref(_dyn(dt=0.0)), f, f, None, f, f, f, None) == EINVAL and "dt" in err()
    assert L.ngp_agent_step(ctypes.byref(_dyn(mass=float("nan"))), f, f, None, f, f, f, None) == EINVAL and "mass" in err()
    assert L.ngp_agent_step(ctypes.byref(_dyn(I=(1, 0, 0, 0, 1, 0, 1, 1, 0))), f, f, None, f, f, f, None) == EINVAL and "singular" in err()
    c = ngp_hip.ngp_filter_cfg_t()
    c.H, c.W = 20, 20
    assert L.ngp_agent_rays(None, f, f, f, None) == EINVAL and "null cfg" in err()
    for state, o, d in ((None, f, f), (f, None, f), (f, f, None)):
        assert L.ngp_agent_rays(ctypes.byref(c), state, o, d, None) == EINVAL and "null pointer" in err()
    for H, W in ((0, 20), (20, 0), (65536, 65536)):
        c.H, c.W = H, W
        assert L.ngp_agent_rays(ctypes.byref(c), f, f, f, None) == EINVAL and "image size" in err()
    for image, png, target in ((None, f, f), (f, None, f), (f, f, None)):
        assert L.ngp_agent_sensor(image, png, target, 4, None) == EINVAL and "null image" in err()
    assert L.ngp_agent_sensor(f, f, f, 0, None) == 0                                # nothing to do, nothing launched


def test_sensor_restatement_is_the_reference_on_the_unit_interval():
    """nav/agent_helpers.py:205 and nav/estimator_helpers.py:192 as written, on every test value inside [0, 1] and on a dense sweep of it"""
    v = AC.sensor_values()
    v = v[(v >= 0) & (v <= 1)]
    sweep = np.linspace(0, 1, 200001).astype(np.float32)
    rng = np.random.default_rng(5)
    for img in (v, sweep, rng.random(100000, dtype=np.float32)):
        png, target = AC.sensor_restated(img)
        u8 = (np.array(img) * 255.).astype(np.uint8)                               # agent_helpers.py:205
        back = (np.array(u8) / 255.).astype(np.float32)                            # estimator_helpers.py:192
        assert png.dtype == np.uint8 and target.dtype == np.float32
        assert np.array_equal(png, u8) and np.array_equal(target.view(np.uint32), back.view(np.uint32))
    png, target = AC.sensor_restated(AC.sensor_values())
    assert set(png.tolist()) == set(range(256))                                    # the input reaches every level ...
    k = (np.arange(256) / 255.0).astype(np.float32)
    at, below = AC.sensor_restated(k)[0], AC.sensor_restated(np.nextafter(k, np.float32(-1)))[0]
    assert np.array_equal(at, np.arange(256))                                      # ... an 8-bit image passes through unchanged (the float32 product is exact) ...
    assert int((below[1:] == np.arange(255)).sum()) > 0                            # ... and one float32 below a level truncates to the level under it
    outside = np.array([-3.0, -1e-7, 1.0 + 1e-6, 255.0], np.float32)
    assert AC.sensor_restated(outside)[0].tolist() == [0, 0, 255, 255]              # the clamp: this project's addition


def test_sensor_input_shapes():
    for N in (1, 63, 64, 65, 20 * 20 * 3 + 1):
        x = AC.sensor_input(N)
        assert x.shape == (N, 3) and x.dtype == np.float32
    full = AC.sensor_input(20 * 20 * 3 + 1).reshape(-1)
    assert set(AC.sensor_values().view(np.uint32).tolist()) <= set(full.view(np.uint32).tolist())


def test_action_rule_for_eight_steps():
    """simulate.py:73-76 for steps = 8: three replanned steps take the planner's next action, the last five walk the last plan's first five rows"""
    from ngp import nav
    by_hand = [None, None, None, 0, 1, 2, 3, 4]
    assert [nav.mpc_action_row(it, 8) for it in range(8)] == by_hand
    assert [nav.mpc_action_row(it, 5) for it in range(5)] == [0, 1, 2, 3, 4]        # the shortest plan (2 states): never replanned


@pytest.mark.parametrize("name", AC.names())
def test_golden_step_is_dynamics_plus_noise_and_two_rotations(name):
    """the executed float64 Agent.step against ngp.nav.drone_dynamics (held to the executed dynamics by test_filter_step_host.py) + noise, and the poses
    against rot_x(+-pi/2) with the reference's float32 cosine"""
    from ngp import nav
    g = AC.gold()
    dt, mass, grav = (float(v) for v in g[f"{name}_cfg"])
    state, action, noise = (torch.from_numpy(g[f"{name}_{k}"]).double() for k in ("state", "action", "noise"))
    want = nav.drone_dynamics(state, action, dt, mass, grav, torch.from_numpy(g[f"{name}_I"]).double()) + noise
    new = g[f"{name}_new_state_f64"]
    assert new.dtype == np.float64 and np.abs(new - want.numpy()).max() < 1e-13
    c90 = float(np.cos(np.float32(np.pi / 2), dtype=np.float32))
    assert c90 == float(np.float32(-4.37113883e-08))
    R = nav._vec_to_rot_matrix(torch.from_numpy(new[6:9])).numpy()
    blender = np.eye(4)
    blender[:3, :3] = np.array([[1, 0, 0], [0, c90, -1], [0, 1, c90]]) @ R
    blender[:3, 3] = new[:3]
    body = blender.copy()
    body[:3, :3] = np.array([[1, 0, 0], [0, c90, 1], [0, -1, c90]]) @ blender[:3, :3]
    assert np.abs(g[f"{name}_blender_pose_f64"] - blender).max() < 1e-13 and np.abs(g[f"{name}_true_pose_f64"] - body).max() < 1e-13
    assert np.abs(g[f"{name}_new_state_f32"] - new).max() < 1e-6 and np.abs(g[f"{name}_true_pose_f32"] - body).max() < 1e-6
