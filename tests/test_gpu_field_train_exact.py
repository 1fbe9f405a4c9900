"""GPU: the field's fused training step (ngp/field.py `_field_train`; csrc/field_train.hip) against the oracle's composition of the same step, with ==.

The inputs (tests/_field_cases.py) make every float32 sum the kernels form exact in any order; tests/test_field_train_inputs_host.py proves that per
case from the oracle alone.  So there is no tolerance here: sigma, rgb, the table gradient and both weight gradients are compared entry by entry.  The
step goes through the module under autocast, the product route: forward (one launch, or two passes from 65,536 samples), the list of live samples,
both backward launches, the fixed-order finish and the listed binned table scatter."""
import numpy as np
import pytest
import torch

from _field_cases import BOUND, CASE, PARAMS, SMALL_BATCHES

pytestmark = pytest.mark.gpu

_fields = {}


@pytest.fixture(scope="module")
def sh_oracle():
    from oracle import sh_oracle
    return sh_oracle


def _field(dev, oracle, name):
    if name not in _fields:
        from ngp.field import NGPFieldFF
        field = NGPFieldFF(bound=BOUND).to(dev)
        assert field.encoder.per_level_scale == 2.0 and field._fused_shape_ok()
        _fields[name] = field.load_arrays(PARAMS[name].model(oracle)).train()
    return _fields[name]


def _step(dev, oracle, B):
    """one training step of the module on the case's inputs: (sigma, rgb, table gradient, density-net and colour-net weight gradients)"""
    from gridencoder import grid as G
    field = _field(dev, oracle, B["P"].name)
    assert G.BINNED_SCATTER and G.offsets_max_rows(field.encoder.offsets) <= (1 << 19)      # the listed binned scatter, not the atomic one
    for p in field.parameters():
        p.grad = None
    x, d, gs, gc = (torch.from_numpy(B[k]).to(dev) for k in ("x", "d", "gs", "gc"))
    with torch.autocast("cuda", dtype=torch.float16):
        assert field._fused_training_applies(x, d)
        sig, rgb = field(x, d)
    torch.autograd.backward([sig, rgb], [gs, gc])                       # the incoming gradients as they are: no loss in between to round them
    torch.cuda.synchronize()
    return (sig.detach().cpu().numpy(), rgb.detach().float().cpu().numpy(), field.encoder.embeddings.grad, field.sigma_net.weights.grad.cpu().numpy(),
            field.color_net.weights.grad.cpu().numpy())


def _same(name, got, ref):
    bad = np.flatnonzero(got.ravel() != ref.ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {ref.size} entries differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} != {ref.ravel()[bad[0]]!r}"


def _check(B, got):
    F, R = B["F"], B["R"]
    sig, rgb, g_table, g_ws, g_wc = got
    assert sig.dtype == np.float32 and sig.shape == F["sigma"].shape and rgb.shape == F["rgb"].shape
    _same("sigma", sig, F["sigma"])                                      # ngp_expf and the oracle's expf are the same operations
    keep = ~F["margin"]                                                  # (within 2^-20 of a half rounding boundary the float32 sigmoid may round either way)
    _same("rgb", rgb[keep], F["rgb"][keep])
    assert g_table.dtype == torch.float32 and tuple(g_table.shape) == R["table_shape"]
    rows = torch.from_numpy(R["table_rows"]).to(g_table.device)
    _same("table gradient", g_table[rows].cpu().numpy(), R["table_values"].astype(np.float32))
    assert int(torch.count_nonzero(g_table)) == int(np.count_nonzero(R["table_values"])), "table gradient: rows written that no live sample touches"
    _same("density-net weight gradient", g_ws, R["gws"])
    _same("colour-net weight gradient", g_wc, R["gwc"])


@pytest.mark.parametrize("M", SMALL_BATCHES)
def test_all_live_small_batches(dev, oracle, sh_oracle, M):
    """tile, pair, wave and workgroup edges; the last pair's slots past the end of the list"""
    B = CASE[f"M{M}-all"].build(oracle, sh_oracle)
    _check(B, _step(dev, oracle, B))


@pytest.mark.parametrize("cid", ["M5000-sparse", "M40000-sparse-ends"])
def test_sparse_live_list_and_the_same_step_over_every_sample(dev, oracle, sh_oracle, cid):
    """about 220 live samples between dead runs of every length and alignment (40,000 samples: the workgroup count is capped at 256); a sample whose only
    gradient is one colour channel, one outside the box, one that is live by the sign bit of a -0.0 alone.  Then with the compaction switched off: the
    same kernels over every sample give the same bits (these sums are exact; on general data they differ by half ulps)."""
    import ngp_hip
    B = CASE[cid].build(oracle, sh_oracle)
    _check(B, _step(dev, oracle, B))
    previous = ngp_hip.lib().ngp_field_train_set_live_only(0)
    try:
        every = _step(dev, oracle, B)
    finally:
        ngp_hip.lib().ngp_field_train_set_live_only(previous)
    _check(B, every)


def test_two_pass_forward_and_the_one_launch_forward_above_its_threshold(dev, oracle, sh_oracle):
    """70,001 samples: the forward encodes level by level (k_ft_encode_levels) and runs the networks in a second pass; sigma and rgb of all 70,001 samples
    and the gradients of the 220 live ones.  Then the single launch on the same batch."""
    import ngp_hip
    B = CASE["M70001-sparse"].build(oracle, sh_oracle)
    L = ngp_hip.lib()
    previous = L.ngp_field_train_set_two_pass(1)
    try:
        _check(B, _step(dev, oracle, B))
        L.ngp_field_train_set_two_pass(0)
        _check(B, _step(dev, oracle, B))
    finally:
        L.ngp_field_train_set_two_pass(previous)


def test_every_wave_iterates_its_pair_loop(dev, oracle, sh_oracle):
    """110,000 samples, nine in ten live: 3,100 pairs for 1,024 waves, so every wave takes three or four and the prefetch of the next pair and of the list
    entries of the one after runs; the per-workgroup rows of all 256 workgroups go through the finish"""
    B = CASE["M110000-dense-large"].build(oracle, sh_oracle)
    _check(B, _step(dev, oracle, B))


def test_density_logits_beyond_the_clamp(dev, oracle, sh_oracle):
    """trunc_exp's backward is g * exp(min(h0, 15)): on this field some density logits reach 22, and the incoming gradients are sized for the clamped value"""
    B = CASE["M200-all-clamp"].build(oracle, sh_oracle)
    _check(B, _step(dev, oracle, B))
