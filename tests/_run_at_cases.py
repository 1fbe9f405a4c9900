"""What the GPU tests of the resampled run (tests/test_gpu_resample.py, tests/test_gpu_resample_guard.py) share: the cases, and the float64 reference of
NeRFRenderer.run's final pass (nerf/renderer.py:206-241) evaluated at a GIVEN float32 depth list -- oracle.callers_oracle.run refuses pin_float32 with
upsample_steps > 0, so the pass is written here from its pieces (CO._weights, CO._pinned, the pinned oracle field of _nav_pinned_cases).

Fields, rays, loss weights, the rule (judge, MARGIN, left_out, carry_floor) are _nav_pinned_cases'.  Everything is computed once per process and shared:
do not write to what these functions return."""
import functools

import numpy as np
import torch

import _nav_pinned_cases as C

F = np.float32


def _case(Nc, Nf, field="contrast", count=16, **kw):
    case = C._run_case(field=field, T=Nc, count=count, **kw)           # T = Nc: the coarse pass is the dense case of that many steps
    case["Nf"] = Nf
    return case


# the shapes (Nc, Nf) the issue names, both fields, bounds 2 and 1, density_scale 2, the two single-term losses; at most 16 rays each
RES_CASES = {
    "r3_1": _case(3, 1),
    "r8_5": _case(8, 5, field="fog"),
    "r64_64": _case(64, 64),
    "r255_1": _case(255, 1),
    "r256_256": _case(256, 256),
    "r257_130": _case(257, 130, field="fog"),
    "r128_128": _case(128, 128),
    "r2048_2048": _case(2048, 2048, count=8, long=True),
    "bound_1": _case(64, 64, bound=1.0, min_near=0.05),
    "scale_2": _case(64, 64, field="fog", density_scale=2.0),
    "background": _case(8, 5, bg=C.BG),
    "weights_sum_alone": _case(64, 64, terms=("weights_sum",), translucent=True),
    "depth_alone": _case(64, 64, terms=("depth",), translucent=True),
}


def run_at(case, z32, dtype, pin):
    """the final pass over the float32 depth list z32 [N,T] -> dict like _nav_pinned_cases.oracle_run's.  pin: near, far, sample_dist and the unclipped
    positions take the float32 run's values with this dtype's gradient path (callers_oracle.run's pin_float32, restated for a given list)"""
    from oracle import callers_oracle as CO
    from oracle import ngp_oracle as O
    o, d, _ = C.case_rays(case)
    N, T = z32.shape
    Nc, bound = case["T"], case["bound"]
    G, Gd, Gw = C.loss_weights(N)
    field = C.oracle_field(case["field"], bound, dtype, pin_float32=pin)
    to, td = torch.from_numpy(o).to(dtype).requires_grad_(True), torch.from_numpy(d).to(dtype).requires_grad_(True)
    aabb = torch.tensor([-bound] * 3 + [bound] * 3, dtype=dtype)
    n, f = O.near_far_from_aabb(o, d, aabb.numpy().astype(F), case["min_near"])
    n32, f32 = torch.from_numpy(n).unsqueeze(-1), torch.from_numpy(f).unsqueeze(-1)
    nears, fars = n32.to(dtype), f32.to(dtype)
    z_32 = torch.from_numpy(np.ascontiguousarray(z32))
    z_vals = z_32.to(dtype)                                            # a constant: no gradient through the depths (:173, :184)
    sample_dist = ((f32 - n32) / Nc).to(dtype) if pin else (fars - nears) / Nc       # :153 with num_steps = Nc, not T
    xyzs = to.unsqueeze(-2) + td.unsqueeze(-2) * z_vals.unsqueeze(-1)
    if pin:
        xyzs32 = to.detach().to(torch.float32).unsqueeze(-2) + td.detach().to(torch.float32).unsqueeze(-2) * z_32.unsqueeze(-1)
        xyzs = CO._pinned(xyzs32, xyzs)
    xyzs = torch.min(torch.max(xyzs, aabb[:3]), aabb[3:])
    dens = {k: v.view(N, T, -1) for k, v in field.density(xyzs.reshape(-1, 3)).items()}
    weights, _ = CO._weights(z_vals, sample_dist, dens["sigma"].squeeze(-1), case["density_scale"])
    dirs = td.view(-1, 1, 3).expand_as(xyzs)
    flat = {k: v.reshape(-1, v.shape[-1]) for k, v in dens.items()}
    mask = weights > 1e-4
    rgbs = field.color(xyzs.reshape(-1, 3), dirs.reshape(-1, 3), mask=mask.reshape(-1), **flat).view(N, T, 3)
    weights_sum = weights.sum(dim=-1)
    ori_z = ((z_vals - nears) / (fars - nears)).clamp(0, 1)
    depth = torch.sum(weights * ori_z, dim=-1)
    bg = case["bg"] if isinstance(case["bg"], (int, float)) else torch.as_tensor(np.asarray(case["bg"], F)).to(dtype)
    image = torch.sum(weights.unsqueeze(-1) * rgbs, dim=-2) + (1 - weights_sum).unsqueeze(-1) * bg
    loss = 0
    if "image" in case["terms"]:
        loss = loss + (image * torch.from_numpy(G).to(dtype)).sum()
    if "depth" in case["terms"]:
        loss = loss + (depth * torch.from_numpy(Gd).to(dtype)).sum()
    if "weights_sum" in case["terms"]:
        loss = loss + (weights_sum * torch.from_numpy(Gw).to(dtype)).sum()
    go, gd = torch.autograd.grad(loss, [to, td])
    res = dict(image=image, depth=depth, weights_sum=weights_sum, weights=weights, mask=mask)
    res = {k: v.detach().numpy() for k, v in res.items()}
    res["grad_o"], res["grad_d"] = go.numpy(), gd.numpy()
    return res


def at_reference(case, z32):
    """dict(ref = the pinned float64 pass at z32, f32 = the float32 pass at z32, miss, hit, judged, e32)"""
    _, _, miss = C.case_rays(case)
    ref, f32 = run_at(case, z32, torch.float64, True), run_at(case, z32, torch.float32, False)
    hit = np.ones(ref["grad_o"].shape[0], bool)
    hit[miss] = False
    judged = hit & ~C.left_out(ref, miss)
    e32 = {k: C.row_error(f32[k], ref[k], k) for k in ("image", "depth", "weights_sum", "grad_o", "grad_d")}
    return dict(case=case, ref=ref, f32=f32, miss=miss, hit=hit, judged=judged, e32=e32)


@functools.lru_cache(maxsize=None)
def coarse_reference(name):
    """the coarse pass's weights [N,Nc]: the pinned float64 run at upsample_steps = 0 and the float32 oracle's error against it, per ray"""
    case = RES_CASES[name]
    ref, f32 = C.oracle_run(case, torch.float64, True), C.oracle_run(case, torch.float32, False)
    return dict(ref=ref["weights"], e32=C.row_error(f32["weights"], ref["weights"], "weights"))
