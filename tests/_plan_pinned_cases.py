"""What tests/test_plan_pinned_host.py (CPU) and tests/test_gpu_plan_pinned.py (GPU) share: the trajectories the native planner (csrc/nav_plan.hip,
ngp.nav.NativePlanner) is held to, the pinned float64 reference of each, and the comparison rule.

Reference: oracle.nav_oracle.planner_costs in float64 over PinnedDensity -- the field enters as the float32 value and Jacobian the cost kernel itself
consumed, so the reference gradient is the exact derivative of the kernel's own cost model and only the planner's arithmetic is compared.  The scalars
the kernel receives as float32 (dt, mass, g) enter the float64 run as those float32 numbers.  Yardstick: the same call in float32 under plain torch
autograd over the same pinned function; its distance from the reference is e32, and the kernel may be MARGIN (16) times as far:

    |kernel[p] - ref[p]| <= 16 * max(e32 over the entries of p's kind in trajectory rows r-2 .. r+2, p90 of e32 over the kind)

Kinds of gradient entries: initial_accel, position (states[2:, :3]), heading (states[:, 3]); states[0:2, :3] do not enter the cost (nav/quad_plot.py:148)
and must come out exactly 0.  per_state, collision, total and the kinematics follow the same rule per trajectory row.  The row window is there because
the float32 error is local to the rows where the torque terms are large; one entry's own e32 can be small by luck.
Everything here is computed once per process and shared: do not write to what these functions return."""
import functools
import math

import numpy as np
import torch

from _nav_pinned_cases import MARGIN
from oracle import nav_oracle as NO

SIM_START, SIM_END = [0.39, -0.67, 0.2], [-0.4, 0.55, 0.16]           # tests/test_gpu_nav_plan.py's, simulate.py:236-237
BODY = [[-0.05, 0.05], [-0.05, 0.05], [-0.02, 0.02]]
NBINS = [10, 10, 5]
ACCEL = (10.3, 9.7)
WINDOW = 2                                                            # rows either side whose e32 a row's yardstick may take

STOCK = dict(J=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], mass=1.0, g=10.0,
             start=dict(rotvec=(0.0, 0.0, 0.0), vel=(0.0, 0.0, 0.0), rate=(0.0, 0.0, 0.0)),
             end=dict(rotvec=(0.0, 0.0, 0.0), vel=(0.0, 0.0, 0.0), rate=(0.0, 0.0, 0.0)))
# J is deliberately not symmetric (the reference computes I @ alpha for any matrix): J^T in the torque adjoint is then not J
FULL = dict(J=[[1.0, 0.3, -0.2], [0.1, 2.0, 0.4], [0.25, -0.15, 0.5]], mass=1.7, g=9.81,
            start=dict(rotvec=(0.02, -0.03, 0.4), vel=(0.1, -0.05, 0.02), rate=(0.3, -0.2, 0.5)),
            end=dict(rotvec=(-0.03, 0.01, -0.6), vel=(-0.08, 0.04, 0.01), rate=(-0.1, 0.25, 0.2)))


def _case(R, B=500, stock=False, fade=0, epoch=0, seed=0, T_final=None, amp=0.01):
    return dict(R=R, B=B, stock=stock, fade=fade, epoch=epoch, seed=seed, T_final=T_final, amp=amp)


# T_final None: steps / 10, i.e. dt = 0.1.  B = 500: the 10 x 10 x 5 body lattice; any other B: seeded uniform points in the body box.
# k_plan_cost_step runs 512 lanes over P = 4 R + 2 parameters (R126 .. R128: P = 506, 510, 514); k_plan_kinematics 1,024 over 18 S outputs.
CASES = {
    "stock18": _case(18, stock=True, T_final=2.0, seed=11),
    "full18": _case(18, seed=12),
    "full18_fade": _case(18, fade=50, epoch=7, seed=13),                                  # S = 21, odd
    # R2 and R3 run at T_final = 2 (dt = 0.5 and 0.4) as tests/test_gpu_nav_plan.py's do.  At dt = 0.1 they would cross the 1.45 m in 0.4 and 0.5 s with
    # accelerations of 130 to 190 m/s^2: the float32 restatement of R2 is then 1e-5 to 4e-5 of scale from float64 on initial_accel whatever the seed
    # (the conditioning bar is 4e-6), and R3 turns by 169 degrees between rows 2 and 3 (x = -0.98), where one ulp of the trace moves omega by 1.6e-6
    # of itself (tests/test_plan_pinned_host.py bounds that amplification; the kernel sat 2e-6 from the reference there, the float32 restatement 2e-7
    # by the luck of its roundings, and the position gradient 19.1 yardsticks out).
    "R2": _case(2, seed=14, T_final=2.0),
    "R3": _case(3, fade=10, epoch=2, seed=15, T_final=2.0),                               # S = 6, even
    "R126": _case(126, B=65, seed=16),
    "R127": _case(127, B=65, seed=17),
    "R128": _case(128, B=65, seed=18),
    "R255": _case(255, fade=40, epoch=30, seed=19),                                       # the maximum: S = 258, all 66 KB of LDS rows
    "B1": _case(18, B=1, seed=20),
    "B63": _case(18, B=63, seed=21),
    "B64": _case(18, B=64, seed=22),
    "B65": _case(18, B=65, seed=23),
    # dt = 0.032: the perturbation scales with dt^2 as in tests/test_gpu_nav_plan.py (there 0.01 would swing consecutive thrust axes by up to ~pi)
    "stock60": _case(60, stock=True, T_final=2.0, seed=1, amp=0.01 * (20.0 / 60.0) ** 2),
}
COLLISION_IN_PLAY = ("stock18", "full18", "R255", "B64")               # the GPU test asserts a reference collision sum > 1.0 on these


def _state(pos, rotvec, vel, rate):
    s = NO.state18(pos, rotvec=rotvec)
    s[3:6] = torch.tensor(vel)
    s[15:18] = torch.tensor(rate)
    return s


@functools.lru_cache(maxsize=None)
def inputs(name, seed=None):
    """dict(cfg, start, end, states [R,4], accel [2], body [B,3], epoch, R, S, B, P): float32 CPU tensors of a case (`seed`: another perturbation)"""
    c = CASES[name]
    kind = STOCK if c["stock"] else FULL
    steps = c["R"] + 2
    T_final = c["T_final"] if c["T_final"] is not None else steps / 10
    cfg = {"T_final": T_final, "steps": steps, "lr": 0.001, "epochs_init": 1, "epochs_update": 1, "fade_out_epoch": c["fade"], "fade_out_sharpness": 10,
           "mass": kind["mass"], "I": torch.tensor(kind["J"]), "g": kind["g"], "body": np.array(BODY), "nbins": NBINS}
    start = _state(SIM_START, **kind["start"])
    end = _state(SIM_END, **kind["end"])
    gen = torch.Generator().manual_seed(c["seed"] if seed is None else seed)
    line = NO.planner_initial_states(start, end, steps)
    states = line + c["amp"] * torch.randn(line.shape, generator=gen)
    if c["B"] == 500:
        body = NO.robot_body(BODY, NBINS)
    else:
        box = torch.tensor(BODY)
        body = box[:, 0] + (box[:, 1] - box[:, 0]) * torch.rand(c["B"], 3, generator=torch.Generator().manual_seed(100 + c["B"]))
    R = c["R"]
    return dict(name=name, cfg=cfg, start=start, end=end, states=states.contiguous(), accel=torch.tensor(ACCEL), body=body.contiguous(), epoch=c["epoch"],
                R=R, S=R + 3, B=int(body.shape[0]), P=4 * R + 2)


def f32(v):
    """the float32 nearest a Python number, as a Python float"""
    return float(np.float32(v))


def cfg_as(cfg, dtype):
    """the cfg the restatement runs on in `dtype`.  float64: J as the float64 copy of the float32 matrix, and dt, mass, g as the float32 numbers the
    kernel is handed (ngp_plan_cfg_t holds them as float), so that the reference differs from the kernel by arithmetic alone"""
    out = dict(cfg)
    out["I"] = cfg["I"].to(dtype)
    if dtype == torch.float64:
        out["mass"], out["g"] = f32(cfg["mass"]), f32(cfg["g"])
        out["T_final"] = f32(cfg["T_final"] / cfg["steps"]) * cfg["steps"]
    return out


class PinnedDensity(torch.autograd.Function):
    """The reference's view of the field: (points, sigma32, jac32) -> sigma32 in the points' dtype; backward grad[..., None] * jac32 likewise.
    Value and Jacobian are the numbers given, whatever the points are."""

    @staticmethod
    def forward(ctx, points, sigma32, jac32):
        ctx.save_for_backward(jac32)
        return sigma32.to(points.dtype).reshape(points.shape[:-1]).clone()

    @staticmethod
    def backward(ctx, grad):
        (jac32,) = ctx.saved_tensors
        return grad[..., None] * jac32.to(grad.dtype).reshape(*grad.shape, 3), None, None


def pinned(sigma32, jac32):
    return lambda points: PinnedDensity.apply(points, sigma32, jac32)


def restated(inp, density_fn, dtype):
    """oracle.nav_oracle.planner_costs of a case in `dtype` under torch autograd -> float64 numpy dict(total, per_state [S], collision [S], grad [P] =
    (initial_accel, states row-major), full [S,18] (get_full_states' layout), actions [S,4], points [S,B,3], rot [S,3,3])"""
    cfg = cfg_as(inp["cfg"], dtype)
    st = inp["states"].to(dtype).clone().requires_grad_(True)
    ia = inp["accel"].to(dtype).clone().requires_grad_(True)
    start, end, body = inp["start"].to(dtype), inp["end"].to(dtype), inp["body"].to(dtype)
    res = NO.planner_costs(st, ia, start, end, cfg, body, density_fn, epoch=inp["epoch"])
    ga, gs = torch.autograd.grad(res["total"], [ia, st])
    with torch.no_grad():
        pos, vel, acc, rot, omega, alpha, actions = NO.planner_kinematics(st, ia, start, end, cfg)
    n = lambda t: t.detach().double().numpy()                                          # noqa: E731
    return dict(total=float(res["total"].detach()), per_state=n(res["per_state"]), collision=n(res["collision"]), grad=n(torch.cat([ga, gs.reshape(-1)])),
                full=n(torch.cat([pos, vel, rot.reshape(-1, 9), omega], dim=-1)), actions=n(actions), points=n(res["points"]), rot=n(rot))


def reference(inp, sigma32, jac32):
    """dict(ref = the pinned float64 run, f32 = the float32 run over the same pinned function).  sigma32 [S,B], jac32 [S,B,3]: float32 CPU tensors"""
    fn = pinned(sigma32, jac32)
    return dict(ref=restated(inp, fn, torch.float64), f32=restated(inp, fn, torch.float32))


# ------------------------------------------------------------------------------------------------------------------------
# a synthetic density for the CPU tests
# ------------------------------------------------------------------------------------------------------------------------
def synthetic_density(points):
    """a few Gaussians along the path, in the points' dtype: sigma up to ~2 where the body passes, as the field's is"""
    t = torch.tensor([0.15, 0.4, 0.55, 0.8], dtype=points.dtype)[:, None]
    a, b = torch.tensor(SIM_START, dtype=points.dtype), torch.tensor(SIM_END, dtype=points.dtype)
    centres = (1 - t) * a + t * b + torch.tensor([[0.03, 0.0, 0.02], [-0.02, 0.04, 0.0], [0.0, -0.03, -0.02], [0.02, 0.02, 0.01]], dtype=points.dtype)
    amps = torch.tensor([1.5, 0.8, 2.0, 1.1], dtype=points.dtype)
    d2 = ((points[..., None, :] - centres) ** 2).sum(-1)
    return (amps * torch.exp(-d2 / (2 * 0.12 ** 2))).sum(-1)


def value_and_jac(fn, points):
    p = points.detach().clone().requires_grad_(True)
    s = fn(p)
    (j,) = torch.autograd.grad(s.sum(), [p])
    return s.detach(), j


@functools.lru_cache(maxsize=None)
def synthetic_reference(name):
    """reference() of a case with the synthetic density's float32 value and Jacobian at the float32 run's own points standing in for the field"""
    inp = inputs(name)
    with torch.no_grad():
        pts = NO.planner_costs(inp["states"], inp["accel"], inp["start"], inp["end"], inp["cfg"], inp["body"], synthetic_density, epoch=inp["epoch"])["points"]
    sigma32, jac32 = value_and_jac(synthetic_density, pts)
    return reference(inp, sigma32, jac32)


# ------------------------------------------------------------------------------------------------------------------------
# the comparison rule
# ------------------------------------------------------------------------------------------------------------------------
KINDS = ("initial_accel", "position", "heading")


def param_layout(R):
    """(kind [P]: index into KINDS or -1 for states[0:2, :3], row [P]: the states row of the entry, 0 for initial_accel)"""
    P = 4 * R + 2
    kind, row = np.empty(P, int), np.zeros(P, int)
    kind[:2] = 0
    q = np.arange(P - 2)
    row[2:] = q // 4
    kind[2:] = np.where(q % 4 == 3, 2, np.where(q // 4 < 2, -1, 1))
    return kind, row


def yardstick(e32, rows, floor=0.0):
    """[n]: max(e32 over the entries within WINDOW rows, p90 of e32, floor)"""
    e32, rows = np.asarray(e32, np.float64), np.asarray(rows)
    near = np.abs(rows[:, None] - rows[None, :]) <= WINDOW
    local = np.where(near, e32[None, :], 0.0).max(axis=1)
    return np.maximum(local, max(float(np.percentile(e32, 90)), floor))


RATIOS = {}                                                            # (case, quantity) -> largest error / yardstick seen; filled by judge()


def judge(case, quantity, got, ref, ref32, rows, scale=None, floor=0.0):
    """The rule over one kind or one per-row quantity.  got, ref, ref32 [n] or [n, k] (Euclidean norm over k); `scale` [n]: errors are divided by it
    (a relative quantity).  Prints and returns the largest error / yardstick; raises AssertionError naming the worst entry."""
    got, ref, ref32 = (np.asarray(a, np.float64).reshape(len(rows), -1) for a in (got, ref, ref32))
    ek, e32 = np.linalg.norm(got - ref, axis=1), np.linalg.norm(ref32 - ref, axis=1)
    if scale is not None:
        ek, e32 = ek / scale, e32 / scale
    assert np.isfinite(ek).all(), f"{case} {quantity}: not finite at {np.flatnonzero(~np.isfinite(ek))[:8].tolist()}"
    y = yardstick(e32, rows, floor)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(ek > 0, ek / y, 0.0)
    worst = int(np.argmax(ratio))
    RATIOS[(case, quantity)] = max(RATIOS.get((case, quantity), 0.0), float(ratio[worst]))
    print(f"{case} {quantity}: max error / yardstick {ratio[worst]:.3g} (entry {worst}, row {int(rows[worst])}: error {ek[worst]:.3g}, "
          f"float32 restatement {e32[worst]:.3g}, yardstick {y[worst]:.3g})")
    assert ratio[worst] <= MARGIN, f"{case} {quantity}: entry {worst} (row {int(rows[worst])}) is {ratio[worst]:.3g} yardsticks from the pinned reference"
    return float(ratio[worst])


def judge_gradient(case, R, got, ref, ref32):
    """the rule per kind of gradient entry; states[0:2, :3] must be exactly 0.0.  -> {kind: largest ratio}"""
    kind, row = param_layout(R)
    got = np.asarray(got, np.float64)
    unused = kind == -1
    assert (got[unused] == 0.0).all() and (ref[unused] == 0.0).all(), f"{case}: a gradient reaches states[0:2, :3]"
    out = {}
    for k, label in enumerate(KINDS):
        sel = kind == k
        if sel.any():
            out[label] = judge(case, "grad " + label, got[sel], ref[sel], ref32[sel], row[sel])
    return out


def total_floor(ref, ref32, S):
    """A floor under the yardstick of `total`, which is ONE number: its own e32 can be small by luck, and there is no neighbour or percentile to lean on.
    total = (1 / S) sum_i per_state_i, so an implementation whose per-state errors are e_i, independent in sign, is sqrt(sum e_i^2) / S from the reference
    before it rounds anything in the sum itself.  With e_i the float32 restatement's own per-state errors this is the distance at which float32
    arithmetic places the mean; relative to the reference total like the error it is compared with.
    The sum itself: k_plan_cost_step adds the S per-state costs in one running float32 sum (torch.mean sums pairwise).  The terms are positive, so every
    partial sum is at most the total, and each of the S - 1 additions rounds by at most 2^-25 of it; independent in sign that is 2^-25 sqrt(S - 1) of the
    total -- 1.3e-7 at S = 21, 4.8e-7 at S = 258 (found on the GPU: R255's total 2.6e-7 from the reference, the float32 restatement 1.4e-9).  The two
    parts add in quadrature."""
    e = np.asarray(ref32["per_state"]) - np.asarray(ref["per_state"])
    rows = math.sqrt(float((e ** 2).sum())) / S / abs(ref["total"])
    return math.hypot(rows, 2.0 ** -25 * math.sqrt(S - 1))


def judge_costs(case, got_total, got_per_state, got_collision, ref, ref32):
    """per_state and collision per row, relative to the reference (rows whose reference is 0 must be 0), and the total"""
    S = len(ref["per_state"])
    rows = np.arange(S)
    out = {"per_state": judge(case, "per_state", got_per_state, ref["per_state"], ref32["per_state"], rows, scale=np.abs(ref["per_state"]))}
    live = ref["collision"] != 0
    assert (np.asarray(got_collision)[~live] == 0).all(), f"{case}: collision where the reference has none"
    if live.any():
        out["collision"] = judge(case, "collision", np.asarray(got_collision)[live], ref["collision"][live], ref32["collision"][live], rows[live],
                                 scale=np.abs(ref["collision"][live]))
    out["total"] = judge(case, "total", [got_total], [ref["total"]], [ref32["total"]], np.zeros(1, int), scale=np.array([abs(ref["total"])]),
                         floor=total_floor(ref, ref32, S))
    return out


def judge_kinematics(case, full, actions, points, ref, ref32):
    """get_full_states, get_actions, body_to_world per trajectory row, absolute"""
    rows = np.arange(ref["full"].shape[0])
    return {"full_states": judge(case, "full_states", full, ref["full"], ref32["full"], rows),
            "actions": judge(case, "actions", actions, ref["actions"], ref32["actions"], rows),
            "points": judge(case, "points", points, ref["points"], ref32["points"], rows)}
