"""GPU: every instantiation of the grid encoder's gradient kernels (csrc/gridencoder.hip) against the CPU oracle.

Table gradient (k_grid_backward: D in 2..5 x C in 1, 2, 4, 8 x float / half, 28 variants; k_gs_bin / k_gs_accumulate for D = 3, C = 2 half):
  * on run-structured lattice inputs every sum is exact whatever the order of the atomics (tests/_grid_cases.py; the conditions are proved on the oracle
    by tests/test_grid_gradient_inputs_host.py), so the comparison is ==: a contribution that is dropped, doubled, sent to another row or channel or
    taken from another lane changes an entry by at least one quantum;
  * on random values, where products and sums do round, with a bound derived per row from the oracle's own sums.
Input gradient (k_grid_input_backward from a saved dy_dx, k_grid_input_backward_recompute without): same bits as the oracle.
GridEncoder with autograd in the shape of the background model's 2-D grid, and the default 3-D grid under autocast (the binned route)."""
import ctypes

import numpy as np
import pytest
import torch

from _grid_cases import BASE, SCATTER_CASES, SMALL_BATCHES, lattice_gradients, lattice_walks, small_batch_cases
from test_gpu_encoders import CASES, make_points, same_bits, t

pytestmark = pytest.mark.gpu


def table_gradient(dev, grad, x, offsets, D, C, L, S, base, gid, align):
    """ngp_grid_encode_backward without the input gradient, into a zero-filled table of the gradient's dtype; returns the table on the device"""
    import ngp_hip as H
    tdt = torch.float16 if grad.dtype == np.float16 else torch.float32
    out = torch.zeros(int(offsets[-1]), C, dtype=tdt, device=dev)
    dummy = torch.empty(1, dtype=tdt, device=dev)
    H.check(H.lib().ngp_grid_encode_backward(H.ptr(t(grad, dev)), H.ptr(t(x, dev)), H.ptr(out), H.ptr(t(offsets, dev)), H.ptr(out), x.shape[0], D, C, L,
                                             float(S), base, 0, H.ptr(dummy), H.ptr(dummy), gid, int(align), H.dtype_code(tdt), H.stream()))
    return out


def bits(a):
    return a.view(torch.int16 if a.dtype == torch.float16 else torch.int32)


def assert_equal_everywhere(got, ref, what):
    """== after widening (-0.0 equals +0.0: the suppression of all-zero runs may leave +0 where a sum of cancelling terms would be -0)"""
    g = got.detach().cpu().numpy().astype(np.float64)
    assert g.shape == ref.shape, f"{what}: {g.shape} vs {ref.shape}"
    bad = np.argwhere(g != ref)
    assert len(bad) == 0, f"{what}: {len(bad)}/{g.size} entries differ, first (row, channel) {bad[:4].tolist()}: got {g[g != ref][:4]} want {ref[g != ref][:4]}"


_SCATTER_PARAMS = [(c, c.B) for c in SCATTER_CASES] + [(c, b) for c in small_batch_cases() for b in SMALL_BATCHES]


@pytest.mark.parametrize("case,B", _SCATTER_PARAMS, ids=[f"{c.id}-B{b}" for c, b in _SCATTER_PARAMS])
def test_table_gradient_equals_the_oracle_on_exact_data(oracle, dev, case, B):
    """k_grid_backward<T, D, C>: every entry of the table gradient equals the oracle's float64 sum, and a second launch gives the same bits in spite of the
    atomics.  The main batch of every case, and for four variants the batches 1, 63, 64, 65 and 257 (prefixes of the main batch, so their sums of |terms|
    are no larger and the exactness condition carries over)."""
    c = case
    x, grad = c.inputs(B)
    offsets = c.offsets(oracle)
    ref = c.reference(oracle, x, grad)
    got = table_gradient(dev, grad, x, offsets, c.D, c.C, c.L, 1.0, BASE, c.gid, c.align)
    again = table_gradient(dev, grad, x, offsets, c.D, c.C, c.L, 1.0, BASE, c.gid, c.align)
    assert_equal_everywhere(got, ref, f"{c.id} B={B}")
    assert torch.equal(bits(got), bits(again))
    assert np.count_nonzero(ref) > (50 if B == c.B else 0)


@pytest.mark.parametrize("route", ["binned_f32", "binned_f16", "listed"])
def test_binned_scatter_equals_the_oracle_on_exact_data(oracle, dev, route):
    """k_gs_bin / k_gs_accumulate on the D = 3, C = 2 half case: run sums in float32, rounded to half, summed in 64-bit fixed point in units of 2^-24 --
    all exact on this data.  `listed`: every second sample, its gradient rows moved to the front (a subset of the case's terms: the condition carries over)."""
    from gridencoder import grid as G
    c = next(k for k in SCATTER_CASES if k.D == 3 and k.C == 2 and k.half)
    x, grad = c.inputs()
    offsets = c.offsets(oracle)
    to = t(offsets, dev)
    if route == "listed":
        order = np.arange(0, c.B, 2, dtype=np.int32)
        count = len(order)
        moved = np.zeros_like(grad)
        moved[:, :count] = grad[:, order]
        moved[:, count:] = np.nan                                          # rows from `count` on are not read
        lst, cnt = t(np.concatenate([order, np.zeros(c.B - count, np.int32)]), dev), torch.tensor([count], dtype=torch.int32, device=dev)
        listed = (ctypes.c_void_p(lst.data_ptr()), ctypes.c_void_p(cnt.data_ptr()))
        got = G.table_gradient_binned(t(moved, dev), t(x, dev), to, c.B, c.L, 1.0, BASE, c.gid, c.align, listed=listed)
        ref = c.reference(oracle, np.ascontiguousarray(x[order]), np.ascontiguousarray(grad[:, order]))
    else:
        out_dtype = torch.float32 if route == "binned_f32" else torch.float16
        got = G.table_gradient_binned(t(grad, dev), t(x, dev), to, c.B, c.L, 1.0, BASE, c.gid, c.align, out_dtype=out_dtype, out_scale=1.0)
        assert got.dtype == out_dtype
        ref = c.reference(oracle, x, grad)
    assert np.count_nonzero(ref) > 50
    assert_equal_everywhere(got, ref, route)


# ---------------------------------------------------------------------------------------------------------------------
# random values: products and sums round; the bound comes from the oracle's own per-row sums
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SCATTER_CASES, ids=lambda c: c.id)
def test_table_gradient_on_random_values_within_a_bound_derived_per_row(oracle, dev, case):
    """48 random points (not on the lattice) in a few same-cell runs, normal gradients, every variant with the grid kind of its exact case.
    Bound per entry: |got - ref| <= (n_row + 2) * u * A_row, with n_row the number of samples that contribute to the entry, A_row the entry's sum of
    |terms| (both from the oracle, one call per sample) and u = 2^-24 for float, 2^-11 for half.  Derivation:
      * the kernel's terms are the oracle's terms: w * g in float32, for half tables rounded to half ((__half)(w * g));
      * the entry is reached by at most n_row additions; each errs by at most u times a partial sum, and a partial sum is at most A_row;
      * where a lane carries a whole sample (C <= 2) a run of samples is summed in float32 first and the half path rounds that sum to half once: the +2
        covers the float32 run sums (and, in the half path, that the run's terms enter unrounded, at most u * A_row in all) and the single rounding.
    A run of one sample adds exactly the oracle's term, and the variants that do not aggregate (C = 4, 8) add every term on its own: an entry that
    one sample reaches, through one of its corners, must EQUAL the oracle's."""
    c = case
    rng = np.random.default_rng(1000 + 10 * c.D + c.C)
    lengths = (1, 2, 5, 8, 12, 20)
    B = sum(lengths)
    cell = 1.0 / (BASE * 2 ** (c.L - 1))
    x = np.concatenate([rng.uniform(0.05, 0.95, size=(1, c.D)) + rng.uniform(0, 0.5 * cell, size=(n, c.D)) for n in lengths]).astype(np.float32)
    grad = rng.normal(size=(c.L, B, c.C)).astype(c.dtype)
    offsets = c.offsets(oracle)
    ref = c.reference(oracle, x, grad)
    n_row = np.zeros(ref.shape, np.int64)
    A_row = np.zeros(ref.shape, np.float64)
    folded = np.zeros(ref.shape, bool)          # entries that one sample reaches through two of its corners (a tiled level wraps, a hashed one collides)
    for i in range(B):
        part = c.reference(oracle, x[i:i + 1], np.abs(grad[:, i:i + 1]))
        n_row += part != 0
        A_row += part
        for level in range(c.L):
            rows = slice(int(offsets[level]), int(offsets[level + 1]))
            if np.count_nonzero(part[rows].sum(axis=1)) < 2 ** c.D:
                folded[rows] |= part[rows] != 0
    assert np.allclose(A_row, c.reference(oracle, x, np.abs(grad)), rtol=1e-12, atol=0)
    got = table_gradient(dev, grad, x, offsets, c.D, c.C, c.L, 1.0, BASE, c.gid, c.align).cpu().numpy().astype(np.float64)
    u = 2.0 ** -11 if c.half else 2.0 ** -24
    err, bound = np.abs(got - ref), (n_row + 2) * u * A_row
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{c.id}: largest error / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}, entries reached {np.count_nonzero(n_row)}, by one sample {np.count_nonzero(n_row == 1)}")
    assert np.all(err <= bound), f"{c.id}: entry {worst}: |{got[worst]} - {ref[worst]}| = {err[worst]} > {bound[worst]} (n_row {n_row[worst]}, A_row {A_row[worst]})"
    assert np.all(got[n_row == 0] == 0) and n_row.max() >= 8
    if c.C >= 4:
        alone = (n_row == 1) & ~folded                                              # one sample AND one of its corners: a single addition to zero
        assert alone.sum() >= 16 and np.array_equal(got[alone], ref[alone])


# ---------------------------------------------------------------------------------------------------------------------
# the two input-gradient kernels
# ---------------------------------------------------------------------------------------------------------------------
def face_points(B, D, seed):
    """make_points (uniform, the closed ends, out-of-range rows) followed by a block of lattice points: 0, 1/2 and 1 lie exactly on cell faces of every
    level, where the one-sided derivative matters"""
    return np.concatenate([make_points(B - 500, D, seed), lattice_walks(500, D, 3, seed + 1)])


def input_gradient_reference(oracle, D, C, L, base, log2T, res, gid, align, dtype, seed):
    offsets, pls = oracle.grid_offsets(D, L, C, 2, base, log2T, res, align)
    rng = np.random.default_rng(seed)
    emb = rng.uniform(-1, 1, size=(offsets[-1], C)).astype(dtype)
    x = face_points(3001, D, seed + 1)
    _, jac = oracle.grid_encode_forward(x, emb, offsets, pls, base, True, gid, align)
    grad = rng.normal(size=(L, x.shape[0], C)).astype(dtype)
    _, gi_ref = oracle.grid_encode_backward(grad, x, emb, offsets, pls, base, jac, gid, align)
    assert not gi_ref[2].any() and not gi_ref[3].any() and np.count_nonzero(gi_ref) > 2000 * D       # out-of-range rows are zero, the rest is not
    return offsets, pls, emb, x, jac, grad, gi_ref


# the nine forward cases in float, and in half where C is even (the library refuses a half table with odd C, as the reference never runs one: grid.py:38)
_JACOBIAN = [(case, dtype) for dtype in (np.float32, np.float16) for case in CASES if not (dtype == np.float16 and case[1] % 2)]


@pytest.mark.parametrize("case,dtype", _JACOBIAN,
                         ids=[f"D{c[0]}C{c[1]}L{c[2]}{c[6]}{'ac' if c[7] else ''}-{'f32' if dt == np.float32 else 'f16'}" for c, dt in _JACOBIAN])
def test_input_gradient_from_saved_jacobian_bit_exact(oracle, dev, case, dtype):
    """k_grid_input_backward<T, D, C> (ngp_grid_encode_backward with calc_grad_inputs = 1) for the nine forward cases: the oracle's bits"""
    import ngp_hip as H
    D, C, L, base, log2T, res, gridtype, align = case
    gid = 0 if gridtype == "hash" else 1
    offsets, pls, emb, x, jac, grad, gi_ref = input_gradient_reference(oracle, D, C, L, base, log2T, res, gid, align, dtype, 11)
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    gi = torch.full((x.shape[0], D), float("nan"), dtype=tdt, device=dev)
    H.check(H.lib().ngp_grid_encode_backward(H.ptr(t(grad, dev)), H.ptr(t(x, dev)), H.ptr(t(emb, dev)), H.ptr(t(offsets, dev)), None, x.shape[0], D, C, L,
                                             float(np.log2(pls)), base, 1, H.ptr(t(jac, dev)), H.ptr(gi), gid, int(align), H.dtype_code(tdt), H.stream()))
    same_bits(gi, gi_ref, "grad_inputs")


_KINDS = (("hash", False), ("tiled", False), ("hash", True), ("tiled", True))
_RECOMPUTE = [(D, C, dtype) + _KINDS[(i + j + k) % 4] for k, dtype in enumerate((np.float32, np.float16)) for i, D in enumerate((2, 3))
              for j, C in enumerate((1, 2, 4, 8))]


@pytest.mark.parametrize("D,C,dtype,gridtype,align", _RECOMPUTE,
                         ids=[f"D{D}C{C}{'f32' if dt == np.float32 else 'f16'}-{g}{'-ac' if a else ''}" for D, C, dt, g, a in _RECOMPUTE])
def test_input_gradient_recomputed_bit_exact(oracle, dev, D, C, dtype, gridtype, align):
    """k_grid_input_backward_recompute<T, D, C> (ngp_grid_encode_backward_inputs), all sixteen instantiations: the oracle's bits, i.e. those of the
    reference's two-kernel route (dy_dx in the forward, grad * dy_dx in the backward)"""
    import ngp_hip as H
    gid = 0 if gridtype == "hash" else 1
    L, base = 4, 8
    offsets, pls, emb, x, _, grad, gi_ref = input_gradient_reference(oracle, D, C, L, base, 12, 64, gid, align, dtype, 13)
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    gi = torch.full((x.shape[0], D), float("nan"), dtype=tdt, device=dev)
    H.check(H.lib().ngp_grid_encode_backward_inputs(H.ptr(t(grad, dev)), H.ptr(t(x, dev)), H.ptr(t(emb, dev)), H.ptr(t(offsets, dev)), x.shape[0], D, C, L,
                                                    float(np.log2(pls)), base, H.ptr(gi), gid, int(align), H.dtype_code(tdt), H.stream()))
    same_bits(gi, gi_ref, "grad_inputs")


def test_the_kinds_of_the_recompute_cases_cover_every_combination():
    assert len(_RECOMPUTE) == 16 and {(g, a) for _, _, _, g, a in _RECOMPUTE} == set(_KINDS)
    for D in (2, 3):
        assert {(g, a) for d, _, _, g, a in _RECOMPUTE if d == D} == set(_KINDS)


@pytest.mark.parametrize("D", [4, 5])
@pytest.mark.parametrize("tdt", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_input_gradient_recompute_refuses_four_and_five_dimensions(dev, D, tdt):
    import ngp_hip as H
    B, C, L = 64, 2, 2
    z = torch.zeros(4096, dtype=tdt, device=dev)
    x = torch.rand(B, D, device=dev)
    offsets = torch.tensor([0, 512, 1024], dtype=torch.int32, device=dev)
    gi = torch.full((B, D), 7.0, dtype=tdt, device=dev)
    rc = H.lib().ngp_grid_encode_backward_inputs(H.ptr(z), H.ptr(x), H.ptr(z), H.ptr(offsets), B, D, C, L, 1.0, 4, H.ptr(gi), 0, 0, H.dtype_code(tdt), H.stream())
    assert rc == -1 and b"D must be 2 or 3" in H.lib().ngp_last_error()            # NGP_EINVAL
    torch.cuda.synchronize()
    assert bool((gi == 7.0).all())                                                  # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# through the module, with autograd
# ---------------------------------------------------------------------------------------------------------------------
def module_inputs(D, L, C, autocast, B):
    """lattice points in [0,1]^D and a gradient [L, B, C] of integers times a power of two; under autocast coarser (m = 2) and sparser, so that the half
    sums stay exact"""
    m, gmax, unit, keep = (2, 1, 1.0, 0.3 if D == 3 else 0.5) if autocast else (5, 2, 0.25, 1.0)
    x01, zero = lattice_walks(B, D, m, 40 + D, marks=True)
    g = lattice_gradients(L, B, C, zero, 50 + D, gmax, unit, keep)
    return x01, g, 2.0 ** -(m * D) * unit


def module_forward_backward(oracle, dev, enc, autocast, recompute, B, amplitude=0.5):
    import gridencoder.grid as G
    D, L, C, base = enc.input_dim, enc.num_levels, enc.level_dim, enc.base_resolution
    assert enc.per_level_scale == 2
    with torch.no_grad():
        enc.embeddings.copy_(torch.from_numpy(np.random.default_rng(0).uniform(-amplitude, amplitude, size=tuple(enc.embeddings.shape)).astype(np.float32)))
    enc.embeddings.grad = None
    offsets = enc.offsets.cpu().numpy()
    x01, g_lbc, q = module_inputs(D, L, C, autocast, B)
    bound = 1.0
    xw = (x01 * np.float32(2 * bound) - np.float32(bound)).astype(np.float32)          # exact, and so is the module's (x + bound) / (2 bound)
    assert np.array_equal((xw + np.float32(bound)) / np.float32(2 * bound), x01)
    np_dt = np.float16 if autocast else np.float32
    emb = enc.embeddings.detach().cpu().numpy().astype(np_dt)
    out_ref, jac_ref = oracle.grid_encode_forward(x01, emb, offsets, 2.0, base, True, enc.gridtype_id, enc.align_corners)
    ge_ref, gi_ref = oracle.grid_encode_backward(g_lbc.astype(np_dt), x01, emb, offsets, 2.0, base, jac_ref, enc.gridtype_id, enc.align_corners)
    A = oracle.grid_encode_backward(np.abs(g_lbc).astype(np_dt), x01, emb, offsets, 2.0, base, None, enc.gridtype_id, enc.align_corners)[0].max()
    p = 11 if autocast else 24
    print(f"D={D} autocast={autocast}: A / q needs {np.log2(A / q):.1f} bits of {p - 1} allowed")
    assert A / q <= 2 ** (p - 1) and np.count_nonzero(ge_ref) > 50                      # the table gradient is exact: shown on the oracle

    xt = t(xw, dev).requires_grad_(True)
    keep = G.RECOMPUTE_INPUT_GRAD, G.RECOMPUTE_MIN_POINTS
    G.RECOMPUTE_INPUT_GRAD, G.RECOMPUTE_MIN_POINTS = True, (B if recompute else B + 1)  # one side of the threshold or the other
    try:
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
            y = enc(xt, bound=bound)
        g = np.ascontiguousarray(g_lbc.transpose(1, 0, 2).reshape(B, L * C))
        y.backward(t(g, dev).to(y.dtype))
    finally:
        G.RECOMPUTE_INPUT_GRAD, G.RECOMPUTE_MIN_POINTS = keep
    assert y.dtype == (torch.float16 if autocast else torch.float32)
    same_bits(y, np.ascontiguousarray(out_ref.transpose(1, 0, 2).reshape(B, L * C)), "GridEncoder output")
    # the chain factor 1 / (2 bound) = 1/2 is exact in float32
    assert xt.grad.dtype == torch.float32
    assert np.isfinite(gi_ref.astype(np.float32)).all() and np.count_nonzero(gi_ref) > B
    assert np.array_equal(xt.grad.cpu().numpy(), gi_ref.astype(np.float32) * np.float32(0.5))
    assert enc.embeddings.grad.dtype == torch.float32
    assert_equal_everywhere(enc.embeddings.grad, ge_ref, "embeddings.grad")


@pytest.mark.parametrize("recompute", [False, True], ids=["saved_jacobian", "recompute"])
@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "autocast"])
def test_background_grid_module_forward_backward_exact(oracle, dev, autocast, recompute):
    """the shape of NGPField's encoder_bg (2-D, 4 levels of 2 features from resolution 16, which trains through k_grid_backward<T, 2, 2>), per_level_scale
    made exactly 2: output, input gradient and embeddings.grad against the oracle, on each side of RECOMPUTE_MIN_POINTS"""
    from gridencoder import GridEncoder
    enc = GridEncoder(input_dim=2, num_levels=4, level_dim=2, base_resolution=16, log2_hashmap_size=19, per_level_scale=2).to(dev)
    module_forward_backward(oracle, dev, enc, autocast, recompute, 301 if autocast else 1501)


def test_default_grid_module_under_autocast_takes_the_binned_scatter_exact(oracle, dev):
    """GridEncoder() under autocast: the table gradient comes from the binned scatter inside _grid_encode.backward, float32 straight into .grad"""
    import gridencoder.grid as G
    from gridencoder import GridEncoder
    assert G.BINNED_SCATTER
    # (table entries up to 2^-7: dy_dx grows with the level scale, up to 2^19 here, and the input gradient is a half under autocast -- finite this way)
    module_forward_backward(oracle, dev, GridEncoder().to(dev), True, True, 301, amplitude=2.0 ** -7)
