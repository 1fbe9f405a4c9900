"""GPU: the float32 binned table-gradient scatter (csrc/gridencoder.hip "Binned scatter of FLOAT32 gradients": integer adds under a block exponent per
row and feature, no float atomics) against the CPU oracle's float64 scatter (oracle/ngp_oracle.c o_grid_encode_backward), and its reproducibility.

The bound, per row and feature, derived and not measured:   |got - ref| <= (d + 2 + extra passes) * 2^-24 * A + n_r * 2^(-K-1) * A
  A    the oracle's scatter of |grad|: weights are non-negative, so that is the sum of |entry| over the row's contributions.
  ref  the oracle's float32 branch rounds every product w * g to binary32 before its float64 add (ngp_oracle.c: `rnd(is_half, w * gval)`, a float
       argument), and computes w with the kernel's own binary32 operations: the products are the kernel's, bit for bit, and the product's rounding
       adds nothing to the bound.
  d    = 6: the bin stage merges a run of consecutive samples in one cell with k_gs_bin's segmented DPP scan: four steps inside a row of 16 lanes
       (row_shr 1, 2, 4, 8), one from the row below (row_bcast 15), one from the lower half of the wave (row_bcast 31).  Every step is one binary32
       add (fma(o, 1, v)), so a contribution reaches its run's total through at most 6 adds, each of relative error 2^-24 on a partial sum that is at
       most the run's sum of |entry|: 6 * 2^-24 * A over a row's runs.
  2    the output rounding and the pass add.  A single pass uses one of the two; the other covers the second-order terms of the six adds.
  n_r  the number of contributions to the row (counted here from the corner rows of every sample: at least the number of entries after merging);
       each entry is rounded to a multiple of 2^(E - K) with E <= log2(largest |entry|) <= log2 A: half a unit, 2^(-K-1) * A, per entry.  K = 36.
A row no contribution reaches must be exactly +0."""
import functools
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

K = 36                       # GSF_K of csrc/gridencoder.hip
D_CHAIN = 6                  # the longest chain of binary32 adds in the bin stage (docstring above)
PASS_SAMPLES = 1 << 22       # GSF_PASS_SAMPLES
NGP_EWORKSPACE = -3
BIG_TABLE = (16, 19, 4096)   # levels, log2 of the rows of a hashed level, finest resolution
SMALL_TABLE = (16, 12, 64)
P1, P2 = 2654435761, 805459861


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ray_points(n_rays, per_ray, seed):
    """march-ordered points as in tests/test_gpu_grid_scatter.py: runs of consecutive samples along rays, some points outside [0,1]"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(0.05, 0.95, (n_rays, 1, 3))
    d = rng.normal(size=(n_rays, 1, 3)); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    s = (np.arange(per_ray)[None, :, None] * 0.0017)
    x = (o + d * s).reshape(-1, 3).astype(np.float32)
    x[::97] = rng.uniform(-0.2, 1.2, (len(x[::97]), 3)).astype(np.float32)
    return x


def mixed_gradient(L, B, seed):
    """normal times 10^u, u uniform in [-6, 6] per sample: a row's contributions mix magnitudes"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-6, 6, size=(1, B, 1))
    return (rng.normal(size=(L, B, 2)) * 10.0 ** u).astype(np.float32)


def contribution_counts(oracle, x, offsets, pls, L):
    """per table row, how many (sample, corner) pairs land on it: get_grid_index of the reference (gridencoder.cu:54-72) in numpy"""
    scale, reso = oracle.grid_level_table(L, np.float32(np.log2(pls)), 16)
    inside = ((x >= 0) & (x <= 1)).all(axis=1)
    counts = np.zeros(int(offsets[-1]), np.int64)
    for level in range(L):
        T = int(offsets[level + 1] - offsets[level])
        pos = x[inside] * np.float32(scale[level]) + np.float32(0.5)
        pg = np.floor(pos).astype(np.uint32)
        side = np.uint32(int(reso[level]) + 1)
        for idx in range(8):
            pl = [pg[:, d] + np.uint32((idx >> d) & 1) for d in range(3)]
            index, stride, d = np.zeros(len(pg), np.uint32), np.uint32(1), 0
            while d < 3 and int(stride) <= T:
                index = index + pl[d] * stride
                stride = np.uint32((int(stride) * int(side)) & 0xFFFFFFFF)
                d += 1
            if int(stride) > T:
                index = pl[0] ^ (pl[1] * np.uint32(P1)) ^ (pl[2] * np.uint32(P2))
            counts[int(offsets[level]):int(offsets[level + 1])] += np.bincount((index % np.uint32(T)).astype(np.int64), minlength=T)
    return counts


@functools.lru_cache(maxsize=None)
def case(oracle, B, table, seed=3):
    """dict(x, grad, offsets, pls, L, ref float64 [rows, 2], A, n): computed once, shared, never written to"""
    L, log2T, res = table
    offsets, pls = oracle.grid_offsets(3, L, 2, 2, 16, log2T, res, False)
    x = ray_points(max(B // 50, 1) + 1, 50, seed)[:B]
    grad = mixed_gradient(L, B, seed + 1)
    emb = np.zeros((int(offsets[-1]), 2), np.float32)
    ref, _ = oracle.grid_encode_backward(grad, x, emb, offsets, pls, 16)
    A, _ = oracle.grid_encode_backward(np.abs(grad), x, emb, offsets, pls, 16)
    n = contribution_counts(oracle, x, offsets, pls, L)
    assert np.all(n[(A > 0).any(axis=1)] > 0)                     # the count's index function is the oracle's: every touched row is counted
    return dict(x=x, grad=grad, offsets=offsets, pls=pls, L=L, ref=ref, A=A, n=n)


def bound(A, n, extra_passes=0):
    return (D_CHAIN + 2 + extra_passes) * 2.0 ** -24 * A + n * 2.0 ** (-K - 1) * A


def scatter(c, dev, B=None, grad=None, x=None):
    from gridencoder import grid as G
    x, grad = c["x"] if x is None else x, c["grad"] if grad is None else grad
    B = x.shape[0] if B is None else B
    return G.table_gradient_binned_f32(t(grad, dev), t(x, dev), t(c["offsets"], dev), B, c["L"], np.log2(c["pls"]), 16, 0, False)


def raw_call(c, dev, out, ws, ws_bytes):
    """the entry point itself, on a caller's output buffer and workspace -> its return code"""
    import ngp_hip
    B = c["x"].shape[0]
    rows = int(np.max(np.diff(c["offsets"])))
    return ngp_hip.lib().ngp_grid_scatter_binned_f32(ngp_hip.ptr(t(c["grad"], dev)), ngp_hip.ptr(t(c["x"], dev)), ngp_hip.ptr(t(c["offsets"], dev)),
                                                     ngp_hip.ptr(out), B, c["L"], float(np.log2(c["pls"])), 16, rows, 0, 0, 1.0, ngp_hip.ptr(ws), ws_bytes,
                                                     ngp_hip.stream())


def worst_ratio(got, c, extra_passes=0):
    tol = bound(c["A"], c["n"][:, None], extra_passes)
    err = np.abs(got.astype(np.float64) - c["ref"])
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))))


@pytest.mark.parametrize("B,table", [(1, BIG_TABLE), (1023, BIG_TABLE), (1024, BIG_TABLE), (1025, BIG_TABLE), (5000, BIG_TABLE), (70001, BIG_TABLE),
                                     (70001, SMALL_TABLE)], ids=["1", "1023", "1024", "1025", "5000", "70001", "70001_small_table"])
def test_against_the_oracle(oracle, dev, B, table):
    """see the module docstring for the bound; the atomic kernel's worst ratio to the same bound is printed for the record, not asserted"""
    import ngp_hip
    c = case(oracle, B, table)
    out = scatter(c, dev)
    assert out.dtype == torch.float32 and tuple(out.shape) == c["ref"].shape
    got = out.cpu().numpy()
    untouched = c["A"] == 0
    assert not got[untouched].any() and not np.signbit(got[untouched]).any()
    ratio = worst_ratio(got, c)
    old = torch.zeros_like(out)
    dummy = torch.empty(1, dtype=torch.float32, device=dev)
    ngp_hip.check(ngp_hip.lib().ngp_grid_encode_backward(ngp_hip.ptr(t(c["grad"], dev)), ngp_hip.ptr(t(c["x"], dev)), ngp_hip.ptr(old), ngp_hip.ptr(t(c["offsets"], dev)),
                                                         ngp_hip.ptr(old), B, 3, 2, c["L"], float(np.log2(c["pls"])), 16, 0, ngp_hip.ptr(dummy), ngp_hip.ptr(dummy),
                                                         0, 0, ngp_hip.F32, ngp_hip.stream()))
    print(f"B={B} table 2^{table[1]}: binned f32 worst ratio to the bound {ratio:.3g}, atomic kernel {worst_ratio(old.cpu().numpy(), c):.3g}, "
          f"largest row count {int(c['n'].max())}")
    assert ratio <= 1.0


def test_two_calls_give_the_same_bits(oracle, dev):
    c = case(oracle, 70001, BIG_TABLE)
    a, b = scatter(c, dev), scatter(c, dev)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_regions_may_move(oracle, dev):
    """4,096 samples as one batch == the same samples behind 1,024 samples whose gradient is all +0: the zero samples shift every region and the
    ticket timing and contribute nothing (a wave holds 64 consecutive samples and 1,024 is a multiple of 64: no run crosses the boundary).  A sum
    that depended on region order would show here; the integer sum does not."""
    c = case(oracle, 5000, BIG_TABLE)
    x, grad = c["x"][:4096], np.ascontiguousarray(c["grad"][:, :4096])
    rng = np.random.default_rng(9)
    x2 = np.concatenate([rng.uniform(0, 1, (1024, 3)).astype(np.float32), x])
    grad2 = np.concatenate([np.zeros((c["L"], 1024, 2), np.float32), grad], axis=1)
    a, b = scatter(c, dev, x=x, grad=grad), scatter(c, dev, x=x2, grad=grad2)
    assert float(a.abs().max()) > 0 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_whole_table_written_and_empty_batch(oracle, dev):
    import ngp_hip
    c = case(oracle, 5000, BIG_TABLE)
    out = torch.full(c["ref"].shape, float("nan"), dtype=torch.float32, device=dev)
    nbytes = ngp_hip.lib().ngp_grid_scatter_binned_f32_workspace(5000, c["L"])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert raw_call(c, dev, out, ws, nbytes) == 0
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    untouched = c["A"] == 0
    assert not got[untouched].any() and not np.signbit(got[untouched]).any()
    assert worst_ratio(got, c) <= 1.0
    z = scatter(c, dev, B=0, x=np.zeros((0, 3), np.float32), grad=np.zeros((c["L"], 0, 2), np.float32))
    assert z.shape[0] == int(c["offsets"][-1]) and not z.any() and not torch.signbit(z).any()


def test_non_finite_contribution_stays_in_its_level(oracle, dev):
    c = case(oracle, 5000, BIG_TABLE)
    assert ((c["x"][17] >= 0) & (c["x"][17] <= 1)).all()
    clean = scatter(c, dev)
    grad = c["grad"].copy()
    grad[3, 17, 0] = np.inf
    got = scatter(c, dev, grad=grad)
    lo, hi = int(c["offsets"][3]), int(c["offsets"][4])
    assert not bool(torch.isfinite(got[lo:hi]).all())
    rest = torch.ones(got.shape[0], dtype=torch.bool, device=dev)
    rest[lo:hi] = False
    assert bool(torch.isfinite(got[rest]).all()) and torch.equal(got[rest].view(torch.int32), clean[rest].view(torch.int32))


def test_multi_pass(oracle, dev):
    """just beyond one pass (2^22 samples), on the small table, as tests/test_gpu_grid_scatter.py::test_binned_scatter_multi_pass_and_empty: the second
    pass adds into the output in float32, one more rounding (the pass count joins the leading factor); n_r = 8 B bounds every row's count.
    The gradient is a positive constant, so the reference is its own A."""
    from gridencoder import grid as G
    L = 4
    offsets, pls = oracle.grid_offsets(3, L, 2, 2, 16, 12, 64, False)
    B = PASS_SAMPLES + 12345
    x = ray_points(B // 64 + 1, 64, 5)[:B]
    grad = np.full((L, B, 2), 0.001, np.float32)
    out = G.table_gradient_binned_f32(t(grad, dev), t(x, dev), t(offsets, dev), B, L, np.log2(pls), 16, 0, False)
    ref, _ = oracle.grid_encode_backward(grad, x, np.zeros((int(offsets[-1]), 2), np.float32), offsets, pls, 16)
    tol = bound(ref, 8 * B, extra_passes=2)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print(f"two passes: worst ratio to the bound {float(np.max(err[tol > 0] / tol[tol > 0])):.3g}")
    assert np.all(err <= tol) and float(ref.max()) > 0


def test_workspace_is_checked_and_respected(oracle, dev):
    """one byte short: NGP_EWORKSPACE and nothing queued (the output keeps its NaN); an exact-size workspace between two 256-byte guards
    (tests/test_gpu_workspace_guard.py's pattern): the guards are intact after the call, and the result does not depend on what the workspace held"""
    import ngp_hip
    GUARD = 256
    c = case(oracle, 1025, BIG_TABLE)
    nbytes = ngp_hip.lib().ngp_grid_scatter_binned_f32_workspace(1025, c["L"])
    outs = []
    for fill in (0xAB, 0x00):
        buf = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 256 == 0
        ws = buf[GUARD:GUARD + nbytes]
        out = torch.full(c["ref"].shape, float("nan"), dtype=torch.float32, device=dev)
        assert raw_call(c, dev, out, ws, nbytes - 1) == NGP_EWORKSPACE
        assert b"workspace" in ngp_hip.lib().ngp_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool((buf == fill).all())
        assert raw_call(c, dev, out, ws, nbytes) == 0
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)) and worst_ratio(outs[0].cpu().numpy(), c) <= 1.0
