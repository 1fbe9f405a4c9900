"""Golden vectors for the pose filter's time step, produced by EXECUTING THE REFERENCE'S OWN PYTHON on the CPU.

Build container only: needs a checkout of the reference, named by the environment variable NGP_REFERENCE; run as
`NGP_REFERENCE=... python -B tests/golden/make_estimator_golden.py` from the repository root.  Writes data only: tests/golden/callers_estimator.npz.

What executes:
  * imported from the reference and run: nav/agent_helpers.py (Agent.__init__ :35-63 for dt, g, mass, I and invI = torch.inverse(I);
    Agent.drone_dynamics :124-171) and nav/math_utils.py under it (vec_to_rot_matrix, rot_matrix_to_vec with acos_safe, skew_matrix_torch);
  * torch.autograd.functional.jacobian of drone_dynamics at the state, and `A @ sig @ A.T + Q`, as Estimator.estimate_state does
    (nav/estimator_helpers.py:355-369);
  * the third-party modules agent_helpers imports and this path never uses (cv2, imageio) are EMPTY placeholder modules in sys.modules;
  * every case runs twice: under torch.set_default_dtype(torch.float64) with float64 inputs (the `*_f64` arrays: the yardstick), and as the
    reference runs it, in float32 (the `*_f32` arrays: they document the reference's own rounding).  The inputs are float32 values in both runs.
  * nothing is written into the reference tree (python -B / sys.dont_write_bytecode).
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("NGP_REFERENCE", "")

import numpy as np  # noqa: E402
import torch  # noqa: E402

NAMES = ("generic", "omega_zero", "hover_at_zero", "filter_start", "small_angle", "large_angle", "full_inertia")


def cases():
    """name -> (state [12], action [4], dt, mass, g, I [3,3]) as float32 arrays / python floats that hold float32 values.  simulate.py's agent: mass 1, g 10, I = eye, dt = 2 / 20."""
    eye = np.eye(3, dtype=np.float32)
    pos, vel = [0.93, -1.11, 0.44], [0.1, -0.03, 0.02]
    sim = (0.1, 1.0, 10.0, eye)
    full = np.array([[0.9, 0.1, -0.05], [0.1, 1.3, 0.2], [-0.05, 0.2, 0.7]], np.float32)
    out = {
        "generic": (pos + vel + [0.3, -0.2, 0.5] + [0.4, -0.3, 0.2], [9.4, 0.05, -0.02, 0.03]) + sim,
        "omega_zero": (pos + vel + [0.3, -0.2, 0.5] + [0.0, 0.0, 0.0], [9.4, 0.05, -0.02, 0.03]) + sim,
        "hover_at_zero": ([0.0, 0.0, 0.5] + [0.0] * 3 + [0.0] * 3 + [0.0] * 3, [10.0, 0.0, 0.0, 0.0]) + sim,
        "filter_start": (pos + vel + [1e-6] * 3 + [1e-6] * 3, [10.2, 0.01, 0.02, -0.01]) + sim,
        "small_angle": (pos + vel + [0.012, -0.008, 0.014] + [0.05, 0.02, -0.04], [9.9, 0.02, 0.0, -0.03]) + sim,
        "large_angle": (pos + vel + [1.3, -1.2, 1.6] + [0.2, 0.1, -0.3], [11.0, -0.04, 0.03, 0.02]) + sim,
        "full_inertia": (pos + vel + [0.3, -0.2, 0.5] + [0.4, -0.3, 0.2], [15.0, 0.05, -0.02, 0.03], 0.05, 1.7, 9.81, full),
    }
    assert tuple(out) == NAMES
    f32 = lambda v: float(np.float32(v))                                                          # noqa: E731  what ngp_filter_dyn_t carries
    return {k: (np.array(s, np.float32), np.array(a, np.float32), f32(dt), f32(m), f32(g), I) for k, (s, a, dt, m, g, I) in out.items()}


def covariances():
    """sig: a seeded, well-conditioned, non-symmetric perturbation of an SPD matrix; Q: diagonal.  float32."""
    rng = np.random.default_rng(2024)
    X = rng.standard_normal((12, 12))
    sig = 0.1 * (np.eye(12) + 0.05 * X @ X.T) + np.triu(rng.uniform(-0.004, 0.004, (12, 12)), 1)
    Q = np.diag(rng.uniform(0.005, 0.02, 12))
    return sig.astype(np.float32), Q.astype(np.float32)


def run(AH, dtype, state, action, dt, mass, g, I, sig, Q):
    torch.set_default_dtype(dtype)
    try:
        camera = {"path": "", "half_res": False, "white_bg": False, "res_x": 1, "res_y": 1, "trans": False, "mode": "RGB"}
        x0 = torch.from_numpy(state).to(dtype)
        agent = AH.Agent({"x0": x0, "dt": dt, "g": g, "mass": mass, "I": torch.from_numpy(I).to(dtype)}, camera, {"blend_path": "", "script_path": ""})
        act = torch.from_numpy(action).to(dtype)
        nxt = agent.drone_dynamics(x0, act)                                                       # estimate_state:355
        A = torch.autograd.functional.jacobian(lambda x: agent.drone_dynamics(x, act), x0)        # :362's call, at the state handed in
        sig_t, Q_t = torch.from_numpy(sig).to(dtype), torch.from_numpy(Q).to(dtype)
        sig_prop = A @ sig_t @ A.T + Q_t                                                          # :369
        assert nxt.dtype == dtype and A.dtype == dtype and sig_prop.dtype == dtype
        return nxt.detach().numpy(), A.numpy(), sig_prop.numpy()
    finally:
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
    sig, Q = covariances()
    data = {"names": np.array(NAMES), "sig": sig, "Q": Q}
    for name, (state, action, dt, mass, g, I) in cases().items():
        data.update({f"{name}_state": state, f"{name}_action": action, f"{name}_cfg": np.array([dt, mass, g], np.float64), f"{name}_I": I})
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            nxt, A, sp = run(AH, dtype, state, action, dt, mass, g, I, sig, Q)
            data.update({f"{name}_next_{tag}": nxt, f"{name}_A_{tag}": A, f"{name}_sig_prop_{tag}": sp})
        d = np.abs(data[f"{name}_A_f32"] - data[f"{name}_A_f64"]).max()
        print(f"{name}: next rotation {data[f'{name}_next_f64'][6:9]}, |A f32 - A f64| max {d:.2e}")
    path = os.path.join(HERE, "callers_estimator.npz")
    np.savez_compressed(path, **data)
    print(f"callers_estimator: {len(data)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
