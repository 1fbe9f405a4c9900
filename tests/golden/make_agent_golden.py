"""Golden vectors for the agent's step, produced by EXECUTING THE REFERENCE'S OWN PYTHON on the CPU.

Build container only: needs a checkout of the reference, named by the environment variable NGP_REFERENCE; run as
`NGP_REFERENCE=... python -B tests/golden/make_agent_golden.py` from the repository root.  Writes data only: tests/golden/agent.npz.

What executes:
  * imported from the reference and run: nav/agent_helpers.py -- Agent.__init__ (:35-63) and Agent.step (:65-99) with drone_dynamics under it -- and
    nav/math_utils.py (rot_x, vec_to_rot_matrix, rot_matrix_to_vec);
  * `get_img` is replaced ON THE AGENT INSTANCE by a function of this file that returns a zero image, so step() never writes a pose file and never starts
    a subprocess; everything else of step() runs as written;
  * the seven named cases of callers_estimator.npz (make_estimator_golden.cases), each with a fixed seeded noise vector (simulate.py's mpc_noise_std,
    :264), once under torch.set_default_dtype(torch.float64) with float64 inputs (`*_f64`: the yardstick) and once as the reference runs it, in float32
    (`*_f32`: its own rounding).  The inputs are float32 values in both runs;
  * one thing has to be widened for the float64 run: the reference's rot_x returns a float32 matrix whatever the default dtype (nav/math_utils.py:17-20),
    and float32 @ float64 raises.  Under float64 the module's name `rot_x` is bound to a wrapper that calls the reference's own rot_x with the float32
    angle the reference gives it and widens the result, so the matrix holds the reference's float32 cosine (-4.37e-8) in both runs;
  * the third-party modules agent_helpers imports and this path never uses (cv2, imageio) are EMPTY placeholder modules in sys.modules;
  * nothing is written into the reference tree (python -B / sys.dont_write_bytecode).

Stored per case: state, action, noise (float32), cfg (dt, mass, g), I, and per dtype new_state [12], blender_pose [4,4] (agent.data['pose']) and
true_pose [4,4] (what step returns).
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NGP_REFERENCE", "")
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_estimator_golden import NAMES, cases  # noqa: E402

NOISE_STD = np.array([2e-2, 2e-2, 2e-2, 1e-2, 1e-2, 1e-2, 2e-2, 2e-2, 2e-2, 1e-2, 1e-2, 1e-2])          # simulate.py:264


def noise_of(index):
    return np.random.default_rng(7000 + index).normal(0.0, NOISE_STD).astype(np.float32)


def blank_image(data):
    return np.zeros((1, 1, 3), np.uint8)


def run(AH, dtype, state, action, noise, dt, mass, g, I):
    reference_rot_x = AH.rot_x
    torch.set_default_dtype(dtype)
    if dtype == torch.float64:
        AH.rot_x = lambda phi: reference_rot_x(phi.float()).to(dtype)
    try:
        camera = {"path": "", "half_res": False, "white_bg": False, "res_x": 1, "res_y": 1, "trans": False, "mode": "RGB"}
        agent = AH.Agent({"x0": torch.from_numpy(state).to(dtype), "dt": dt, "g": g, "mass": mass, "I": torch.from_numpy(I).to(dtype)}, camera,
                         {"blend_path": "", "script_path": ""})
        agent.get_img = blank_image
        true_pose, new_state, img = agent.step(torch.from_numpy(action).to(dtype), noise=torch.from_numpy(noise).to(dtype))
        blender = np.array(agent.data["pose"], dtype=np.float64 if dtype == torch.float64 else np.float32)
        want = np.float64 if dtype == torch.float64 else np.float32
        assert true_pose.dtype == want and new_state.dtype == want and agent.iter == 1 and len(agent.states_history) == 2
        assert np.array_equal(np.array(agent.states_history[1], dtype=want), new_state)
        return new_state, blender, true_pose
    finally:
        AH.rot_x = reference_rot_x
        torch.set_default_dtype(torch.float32)


def main():
    if not os.path.isdir(os.path.join(REF, "nav")):
        raise SystemExit("set NGP_REFERENCE to a checkout of the reference")
    for name in ("cv2", "imageio"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    import nav.agent_helpers as AH
    assert AH.__file__.startswith(os.path.abspath(REF))
    torch.set_num_threads(1)
    data = {"names": np.array(NAMES)}
    for index, (name, (state, action, dt, mass, g, I)) in enumerate(cases().items()):
        noise = noise_of(index)
        data.update({f"{name}_state": state, f"{name}_action": action, f"{name}_noise": noise, f"{name}_cfg": np.array([dt, mass, g], np.float64),
                     f"{name}_I": I})
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            new_state, blender, true_pose = run(AH, dtype, state, action, noise, dt, mass, g, I)
            data.update({f"{name}_new_state_{tag}": new_state, f"{name}_blender_pose_{tag}": blender, f"{name}_true_pose_{tag}": true_pose})
        d = np.abs(data[f"{name}_new_state_f32"] - data[f"{name}_new_state_f64"]).max()
        p = np.abs(data[f"{name}_blender_pose_f32"] - data[f"{name}_blender_pose_f64"]).max()
        print(f"{name}: |new_state f32 - f64| max {d:.2e}, |blender pose f32 - f64| max {p:.2e}, cos in rot_x {data[f'{name}_blender_pose_f64'][1, 1]:.3e}")
    path = os.path.join(HERE, "agent.npz")
    np.savez_compressed(path, **data)
    print(f"agent: {len(data)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
