"""GPU: the default float32 field trained with `NGPField(reproducible=True)`: the fused backward's table gradient comes from the float32 binned
scatter (ngp_grid_scatter_binned_f32, integer adds) instead of float atomics.  Held to the pinned float64 reference by the rule of
tests/_default_train_cases.py, unchanged, and to what the atomic route cannot promise: the same bits on every run, the table gradient included."""
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

import _default_train_cases as T  # noqa: E402


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def fields(dev):
    """{kind: NGPField(reproducible=True) on the GPU holding the pinned cases' numbers}"""
    from ngp.field import NGPField
    out = {}
    for kind in T.FIELDS:
        field = NGPField(bound=T.BOUND, reproducible=True).to(dev)
        field.load_state_dict(T.product_field(kind, T.BOUND, dev).state_dict())
        out[kind] = field
    return out


def weights_of(field):
    return [l.weight for l in list(field.sigma_net) + list(field.color_net)]


def run(field, ref, seed, dev, fused):
    """forward and backward of one batch -> (sigma, rgb numpy, [five weight gradients numpy], table gradient on the GPU)"""
    field.fused_training = fused
    for p in field.parameters():
        p.grad = None
    s = ref["seeds"][seed]
    sigma, rgb = field(t(ref["x"], dev), t(ref["d"], dev))
    assert (sigma.grad_fn is not None) and (type(sigma.grad_fn).__name__.startswith("_field_train_f32") == fused)
    ((sigma * t(s["gs"], dev)).sum() + (rgb * t(s["gc"], dev)).sum()).backward()
    field.fused_training = False
    return (sigma.detach().cpu().numpy(), rgb.detach().cpu().numpy(), [w.grad.detach().cpu().numpy() for w in weights_of(field)],
            field.encoder.embeddings.grad)


@pytest.mark.parametrize("kind", T.FIELDS)
@pytest.mark.parametrize("M", (1, 257, 900, T.BIG))
def test_reproducible_route_against_the_pinned_reference(fields, dev, kind, M):
    """Worst table ratio measured on an MI355X: DESIGN.md 3.12."""
    import ngp_hip
    ref = T.reference(kind, M)
    worst = 0.0
    ngp_hip.TIMERS = {}
    try:
        for seed in T.SEEDS:
            label = f"reproducible {kind} M={M}"
            _, _, gw, gt = run(fields[kind], ref, seed, dev, True)
            T.judge_weights(label, gw, ref, seed)
            worst = max(worst, T.judge_table(label, gt, ref, seed))
        assert len(ngp_hip.TIMERS.get("grid_scatter_binned_f32", [])) == len(T.SEEDS) and "grid_encode_backward" not in ngp_hip.TIMERS
    finally:
        ngp_hip.TIMERS = None
    print(f"WORST reproducible {kind} M={M}: table {worst:.3g}")


@pytest.mark.parametrize("M", [257, T.BIG])
def test_two_fused_runs_give_the_same_bits_table_included(fields, dev, M):
    ref = T.reference("contrast", M)
    a = run(fields["contrast"], ref, 0, dev, True)
    table_a = a[3].clone()
    b = run(fields["contrast"], ref, 0, dev, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for ga, gb in zip(a[2], b[2]):
        assert np.array_equal(ga, gb)
    assert float(table_a.abs().max()) > 0 and torch.equal(table_a.view(torch.int32), b[3].view(torch.int32))


def test_op_chain_takes_the_binned_route_when_switched_on(fields, dev):
    import ngp_hip
    from gridencoder import grid as G
    ref = T.reference("fog", 900)
    field = fields["fog"]
    assert G.BINNED_SCATTER_F32 is False                                    # off by default
    G.BINNED_SCATTER_F32, ngp_hip.TIMERS = True, {}
    try:
        for seed in T.SEEDS:
            _, _, _, gt = run(field, ref, seed, dev, False)
            T.judge_table("op chain, binned f32, fog M=900", gt, ref, seed)
        assert len(ngp_hip.TIMERS.get("grid_scatter_binned_f32", [])) == len(T.SEEDS) and "grid_encode_backward" not in ngp_hip.TIMERS
    finally:
        G.BINNED_SCATTER_F32, ngp_hip.TIMERS = False, None
    ngp_hip.TIMERS = {}
    try:                                                                     # ... and the atomic route with the switch off
        run(field, ref, 0, dev, False)
        assert "grid_scatter_binned_f32" not in ngp_hip.TIMERS and len(ngp_hip.TIMERS.get("grid_encode_backward", [])) == 1
    finally:
        ngp_hip.TIMERS = None


@pytest.fixture(scope="module")
def scene(dev):
    from ngp import workload as W
    o, d = W.get_rays(W.orbit_pose(1), W.intrinsics(64, 64), 64, 64)
    return dict(W=W, grid=W.density_grid(), o=o, d=d)


def make(scene, dev, fused, reproducible, seed=7):
    from ngp.field import NGPField
    from ngp.render import NGPRenderer
    W = scene["W"]
    torch.manual_seed(seed)
    field = NGPField(bound=W.BOUND, fused_training=fused, reproducible=reproducible).to(dev)
    ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev)
    ren.load_density_grid(scene["grid"])
    return ren


def train(scene, dev, fused, reproducible, steps):
    """the recipe of tests/test_gpu_default_train.py's twelve-step test -> (losses, {name: parameter after the last step})"""
    o, d = t(scene["o"], dev)[None], t(scene["d"], dev)[None]
    target = torch.full((1, 4096, 3), 0.25, device=dev)
    ren = make(scene, dev, fused, reproducible).train()
    opt = torch.optim.Adam(ren.field.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    losses = []
    for it in range(steps):
        opt.zero_grad(set_to_none=True)
        torch.manual_seed(100 + it)                                          # the march's perturbation
        out = ren.run_cuda(o, d, dt_gamma=0, bg_color=1, perturb=True, force_all_rays=False, max_steps=1024)
        loss = torch.nn.functional.mse_loss(out["image"], target)
        loss.backward()
        opt.step()
        ren.field.mark_updated()
        losses.append(float(loss))
    return losses, {n: p.detach().clone() for n, p in ren.field.named_parameters()}


def test_two_trainers_from_one_seed_end_on_the_same_bits(scene, dev):
    """twelve steps, twice: every parameter bit-identical after the last step; the first step's loss is the op chain's (a forward-only quantity,
    float32 against float32 from the same seed: 1e-5 relative, as in tests/test_gpu_default_train.py)"""
    la, pa = train(scene, dev, True, True, 12)
    lb, pb = train(scene, dev, True, True, 12)
    chain, _ = train(scene, dev, False, False, 1)
    print(f"first loss: op chain {chain[0]:.9g}, fused reproducible {la[0]:.9g}; last loss {la[-1]:.9g}")
    assert la[-1] < 0.7 * la[0], la
    differing = [n for n in pa if not torch.equal(pa[n].view(torch.int32), pb[n].view(torch.int32))]
    assert not differing, differing
    assert la == lb
    assert abs(la[0] - chain[0]) <= 1e-5 * abs(chain[0])
