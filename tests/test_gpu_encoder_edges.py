"""GPU: the fused field's cell / fraction arithmetic (csrc/ngp_field.h rf_gather_pair: cell = truncating conversion of p, fraction = v_fract_f32(p),
p = x * scale + 0.5) on the positions where a floor and a truncation, or a subtraction and a fract, could part: p a whole number, one float below and one above.

The fused field on explicit points (`NGPFieldFF.forward_fused`: ngp_field_forward, one launch, the non-INRANGE instance of rf_encode) against the op-by-op field
on the same GPU: `k_grid_forward` (gridencoder.hip, which keeps floorf and pos - floor as the reference writes them) + SH + FFMLP.

What is compared, and how:
  sigma   == on bits.  The two routes gather the same corners and run the same density net, so their 16 logits are the same halves (tests/test_gpu_pipeline.py
          test_field_per_op_vs_fused); the op chain then calls torch.exp where the kernel calls ngp_expf (<= 2 ulp apart), so the reference sigma is the oracle's
          expf -- the same operations as ngp_expf (tests/test_gpu_field_train_exact.py) -- of the op chain's logit.
  rgb     the colour net of the fused kernel takes {SH, h} in a permuted k order, i.e. another binary32 summation order inside the MFMA, so the two routes' rgb are
          NOT the same bits on any build (test_field_per_op_vs_fused: 2e-3); the bar here is that test's, 2e-3, and the share of bit-equal values is printed.
          The 15 geometry features the colour net reads are the density net's other outputs, which the sigma comparison's gathers produce.

Points, per table: for every level l and axis, the world positions whose p = x * scale_l + 0.5 is k in {1, 2, res_l / 2, res_l} (res_l lies outside the box: those
take the out-of-range branch), each with its two neighbours on either side (the other two coordinates random); {-bound, 0, bound}^3; points one float and 1e-6
outside each face; 4,096 random points.  Tables: the bench's hand-set one and random halves on the default 16-level grid, and random halves on a grid whose hashed
levels have sizes that are not powers of two (the generic class), as tests/test_gpu_fused_tables.py builds it."""
import numpy as np
import pytest
import torch

from test_gpu_fused_tables import _field, _model, _tables

pytestmark = pytest.mark.gpu
F32 = np.float32


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _edge_points(bound, scales, rng):
    """(points [M,3] float32, number of them whose p is a whole number on the edge axis, as binary32 evaluates (x + bound) * (1 / (2 bound)) * scale + 0.5)"""
    b = F32(bound)
    inv = F32(1) / (F32(2) * b)
    pts, whole = [], 0
    for scale in scales:
        res = int(np.ceil(scale)) + 1
        for axis in range(3):
            for k in (1, 2, res // 2, res):
                w0 = F32(F32((k - 0.5) / float(scale)) * F32(2) * b - b)
                near = [w0]                                           # the nearest float whose p IS the whole number, within 64 floats either way
                for direction in (-np.inf, np.inf):
                    w = w0
                    for _ in range(64):
                        w = np.nextafter(w, F32(direction))
                        near.append(w)
                near = np.array(near, F32)
                hit = (((near + b) * inv) * F32(scale) + F32(0.5)) == F32(k)
                if hit.any():
                    near = near[hit]
                    w0 = near[np.argmin(np.abs(near - w0))]
                cand = [w0]
                for direction in (-np.inf, np.inf):
                    w = w0
                    for _ in range(2):
                        w = np.nextafter(w, F32(direction))
                        cand.append(w)
                for w in cand:
                    p = F32(F32(F32(w + b) * inv) * F32(scale)) + F32(0.5)
                    whole += int(p == np.floor(p))
                    x = rng.uniform(-bound, bound, size=3).astype(F32)
                    x[axis] = w
                    pts.append(x)
    corners = np.array([[i, j, k] for i in (-b, 0, b) for j in (-b, 0, b) for k in (-b, 0, b)], F32)
    outside = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for w in (np.nextafter(b, F32(np.inf)), F32(b * F32(1 + 1e-6))):
                x = rng.uniform(-bound, bound, size=3).astype(F32)
                x[axis] = F32(sign) * w
                outside.append(x)
    rand = rng.uniform(-bound, bound, size=(4096, 3)).astype(F32)
    return np.concatenate([np.array(pts, F32), corners, np.array(outside, F32), rand]), whole


CASES = ("default_bench_table", "default_random_halves", "odd_sizes_random_halves", "odd_sizes_wide_halves")


@pytest.mark.parametrize("case", CASES)
def test_fused_field_equals_the_op_chain_on_cell_edges(oracle, dev, case):
    from ngp import workload as W
    if case.startswith("default"):
        offsets, pls = W.grid_offsets(W.BOUND)
        model = W.make_model(0) if case == "default_bench_table" else _model(W, offsets, pls, seed=3)
        log2 = 19
    else:
        offsets, pls, log2 = _tables(W)["odd_sizes"]
        model = _model(W, offsets, pls, seed=4)
        if case == "odd_sizes_wide_halves":                          # halves over many binades, both signs: products that round at every position
            rng_t = np.random.default_rng(5)
            emb = rng_t.uniform(-1, 1, size=model["embeddings"].shape) * np.exp2(rng_t.integers(-12, 0, size=model["embeddings"].shape))
            model = dict(model, embeddings=emb.astype(np.float16).astype(F32))
    field = _field(dev, W, model, log2).eval()
    enc = field.encoder
    S = F32(np.log2(enc.per_level_scale))
    scales = [F32(np.exp2(F32(l) * S) * F32(enc.base_resolution) - F32(1)) for l in range(enc.num_levels)]      # gridencoder.cu:108
    rng = np.random.default_rng(11)
    x, whole = _edge_points(W.BOUND, scales, rng)
    assert whole >= 16 * 3 * 4, f"only {whole} of the edge points have a whole-number p"      # on average one of the five neighbours per (level, axis, k)
    d = rng.normal(size=x.shape).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xt, dt = t(x, dev), t(d, dev)
    sig, rgb = field.forward_fused(xt, dt)
    field.fused_inference = False
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            h = field.sigma_net(enc(xt, bound=field.bound))                 # k_grid_forward + FFMLP: the 16 logits as halves
            _, rgb_op = field(xt, dt)
    finally:
        field.fused_inference = True
    assert h.dtype == torch.float16 and rgb_op.dtype == torch.float16
    sig_ref = oracle.expf(h[:, 0].float().cpu().numpy())
    sig, rgb, rgb_op = sig.cpu().numpy(), rgb.cpu().numpy(), rgb_op.float().cpu().numpy()
    outside = (np.abs(x) > F32(W.BOUND)).any(axis=1)
    bad = np.flatnonzero(sig.view(np.uint32) != sig_ref.view(np.uint32))
    e_rgb = float(np.max(np.abs(rgb - rgb_op)))
    print(f"{case}: {x.shape[0]} points, {whole} with a whole-number p, {int(outside.sum())} outside the box; sigma differs at {bad.size}; "
          f"rgb max |diff| {e_rgb:.2e}, bit-equal {float((rgb == rgb_op).mean()):.4f}")
    assert int(outside.sum()) >= 12 + 16 * 3                          # the face points and every level's k = res_l
    assert bad.size == 0, (case, bad[:8].tolist(), x[bad[:8]].tolist(), sig[bad[:8]].tolist(), sig_ref[bad[:8]].tolist())
    assert e_rgb < 2e-3, (case, e_rgb)
