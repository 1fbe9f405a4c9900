"""What tests/test_default_train_host.py (CPU) and tests/test_gpu_default_train.py (GPU) share: the samples, loss weights and batches the native
training of the default float32 field (csrc/nav_train.hip, ngp.field._field_train_f32) is held to, the pinned float64 reference of every batch with
gradients down to all six parameters, and the comparison rule.

Reference: _nav_pinned_cases.oracle_field(kind, 2.0, float64, pin_float32=True).  Loss = sum gs sigma + sum gc rgb, gs and gc uniform in +-1.
Yardstick: the float32 oracle's own distance from that reference (per sample for sigma and rgb; per matrix and per grid level, as a relative
Frobenius norm and the largest over the three seeds, for the gradients); the code under test may be MARGIN times as far.
Everything here is computed once per process and shared: do not write to what these functions return."""
import functools

import numpy as np
import torch

import _nav_pinned_cases as C
from _nav_pinned_cases import MARGIN, field_arrays, oracle_field, points, product_field, row_error  # noqa: F401

BOUND = 2.0
FIELDS = ("fog", "contrast")
SEEDS = (0, 1, 2)
# the issue's sizes, and one either side of every boundary of the kernels: 64-lane waves (64, 128, 192), the two sample halves a chunk's
# weight-gradient products are split into (128), 256-sample chunks (256, 512)
SIZES = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 900)
# more chunks than the backward has workgroups (256): two workgroups walk a second chunk and keep summing in their registers; the last chunk holds
# one sample.  The survivors, repeated in order.
BIG = 256 * 256 + 257
WEIGHT_NAMES = ("sigma_net.0", "sigma_net.1", "color_net.0", "color_net.1", "color_net.2")
WEIGHT_SHAPES = ((64, 32), (16, 64), (64, 31), (64, 64), (3, 64))
KINK_MARGIN = 1e-4             # times sum |w| |a|: 25 times the worst-case float32 bound of a 64-term dot product (64 * 2^-24)
CATEGORIES = ("face", "corner", "above", "below", "centre", "node", "far")


@functools.lru_cache(maxsize=None)
def candidates():
    """(x [1000,3], d [1000,3] unit, names): _nav_pinned_cases.points(2.0) in order, directions from default_rng(5)"""
    x, names = points(BOUND)
    d = np.random.default_rng(5).standard_normal((x.shape[0], 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return x, np.ascontiguousarray(d), names


def loss_weights(seed, n):
    """(gs [n], gc [n,3]) float32, uniform in +-1"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, size=n).astype(np.float32), rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def kink_report(kind):
    """(left_out bool [1000], smallest |h| / sum |w| |a| per candidate): a candidate is left out of every batch when some hidden pre-activation h of
    the float64 reference has |h| < KINK_MARGIN * sum |w| |a| over its terms -- the float32 sign of that h, and with it the ReLU's derivative, is
    not determined by the arithmetic, and a gradient comparison on such a sample says nothing"""
    from oracle import callers_oracle as CO
    x, d, _ = candidates()
    emb, offsets, pls, sw, cw = field_arrays(kind, BOUND)
    dt = torch.float64
    with torch.no_grad():
        tx, td = torch.from_numpy(x).to(dt), torch.from_numpy(d).to(dt)
        enc = CO.grid_encode(tx, torch.from_numpy(emb).to(dt), [int(v) for v in offsets], pls, bound=BOUND, pin_float32=True)
        W0, W1, V0, V1 = (torch.from_numpy(w).to(dt) for w in (sw[0], sw[1], cw[0], cw[1]))
        worst = torch.full((x.shape[0],), float("inf"), dtype=dt)

        def layer(a, W):
            nonlocal worst
            h, size = a @ W.T, a.abs() @ W.abs().T
            ratio = torch.where(size > 0, h.abs() / size, torch.full_like(h, float("inf")))      # an all-zero input (outside the box): h is exactly 0 on both sides
            worst = torch.minimum(worst, ratio.min(dim=1).values)
            return torch.relu(h)
        out = layer(enc, W0) @ W1.T
        layer(layer(torch.cat([CO.sh_encode(td), out[:, 1:]], dim=-1), V0), V1)
    return (worst < KINK_MARGIN).numpy(), worst.numpy()


@functools.lru_cache(maxsize=None)
def survivors(kind):
    """rows of candidates() that enter the batches, in order"""
    return np.flatnonzero(~kink_report(kind)[0])


def batch_rows(kind, M):
    keep = survivors(kind)
    return keep[np.arange(M) % len(keep)] if M > len(keep) else keep[:M]


class _CompactTable:
    """Stands in for the [6.3 M, 2] table inside callers_oracle.grid_encode, which reads `.dtype`, `.shape[1]` and `table[rows]` and nothing else.
    A first pass records the rows that are read; from then on `table[rows]` gathers from a leaf that holds those rows only, so a backward pass costs
    what the batch costs and not 128 dense 100 MB tensors.  Same values, same arithmetic; the gradient of every other row is zero."""

    def __init__(self, full, dtype):
        self.full = torch.from_numpy(full).to(dtype)
        self.dtype, self.shape = dtype, tuple(self.full.shape)
        self._seen, self.rows, self.small = [], None, None

    def __getitem__(self, rows):
        rows = torch.as_tensor(rows, dtype=torch.int64)
        if self.small is None:
            self._seen.append(rows.reshape(-1).clone())
            return self.full[rows]
        at = torch.searchsorted(self.rows, rows)
        assert bool((self.rows[at] == rows).all())
        return self.small[at]

    def freeze(self):
        self.rows = torch.unique(torch.cat(self._seen))
        self.small = self.full[self.rows].clone().requires_grad_(True)
        self._seen = []


def _graph(kind, dtype, rows):
    """the oracle's forward over candidates()[rows] -> (sigma, rgb with their graph, [table rows' leaf, five weights], table rows)"""
    x, d, _ = candidates()
    f = oracle_field(kind, BOUND, dtype, pin_float32=True)                # pin_float32 changes nothing unless dtype is float64
    table = _CompactTable(field_arrays(kind, BOUND)[0], dtype)
    f.embeddings = table
    tx, td = torch.from_numpy(x[rows]).to(dtype), torch.from_numpy(d[rows]).to(dtype)
    with torch.no_grad():
        f(tx, td)
    table.freeze()
    sigma, rgb = f(tx, td)
    return sigma, rgb, [table.small] + f.sigma_weights + f.color_weights, table.rows.numpy()


def _gradients(sigma, rgb, params, use, gs, gc):
    """d (sum gs sigma + sum gc rgb over the samples `use`) / d params, float64 numpy"""
    dt = sigma.dtype
    loss = (sigma[use] * torch.from_numpy(gs).to(dt)).sum() + (rgb[use] * torch.from_numpy(gc).to(dt)).sum()
    return [g.detach().numpy().astype(np.float64) for g in torch.autograd.grad(loss, params, retain_graph=True)]


def _level_norms(table_rows, values):
    """per grid level, the Frobenius norm of a table gradient given on `table_rows`"""
    offsets = field_arrays("fog", BOUND)[1]
    level = np.searchsorted(np.asarray(offsets[1:], np.int64), table_rows, side="right")
    return np.sqrt(np.bincount(level, weights=(values ** 2).sum(axis=1), minlength=16)[:16])


def _rel(err, size):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(size > 0, err / size, 0.0)


@functools.lru_cache(maxsize=None)
def _small_graphs(kind):
    rows = survivors(kind)
    return {dt: _graph(kind, dt, rows) for dt in (torch.float64, torch.float32)}


@functools.lru_cache(maxsize=None)
def reference(kind, M):
    """dict(rows = candidate index of every sample, x, d, sigma, rgb = the reference's, e32 = {sigma, rgb: per-sample error of the float32 oracle},
    table_rows, seeds = {seed: dict(gs, gc, weights = five float64 matrices, table = float64 [len(table_rows), 2], level_size [16])},
    yard = dict(weights [5], levels [16]): the float32 oracle's largest relative Frobenius error over the seeds)"""
    x, d, _ = candidates()
    rows = batch_rows(kind, M)
    if M <= len(survivors(kind)):
        graphs, use = _small_graphs(kind), np.arange(M)
    else:
        graphs, use = {dt: _graph(kind, dt, rows) for dt in (torch.float64, torch.float32)}, np.arange(M)
    s64, r64, p64, t64 = graphs[torch.float64]
    s32, r32, p32, t32 = graphs[torch.float32]
    assert np.array_equal(t64, t32)                                      # pinned: both runs read the same cells
    res = dict(rows=rows, x=np.ascontiguousarray(x[rows]), d=np.ascontiguousarray(d[rows]), table_rows=t64,
               sigma=s64.detach().numpy()[use], rgb=r64.detach().numpy()[use], seeds={})
    res["e32"] = {"sigma": row_error(s32.detach().numpy()[use], res["sigma"], "sigma"), "rgb": row_error(r32.detach().numpy()[use], res["rgb"], "rgb")}
    yard_w, yard_l = np.zeros(5), np.zeros(16)
    for seed in SEEDS:
        gs, gc = loss_weights(seed, M)
        g64, g32 = _gradients(s64, r64, p64, use, gs, gc), _gradients(s32, r32, p32, use, gs, gc)
        yard_w = np.maximum(yard_w, [float(_rel(np.linalg.norm(a - b), np.linalg.norm(b))) for a, b in zip(g32[1:], g64[1:])])
        size = _level_norms(t64, g64[0])
        yard_l = np.maximum(yard_l, _rel(_level_norms(t64, g32[0] - g64[0]), size))
        res["seeds"][seed] = dict(gs=gs, gc=gc, weights=g64[1:], table=g64[0], level_size=size)
    res["yard"] = dict(weights=yard_w, levels=yard_l)
    return res


def judge_values(label, got_sigma, got_rgb, ref):
    """sigma (relative) and rgb (absolute) per sample by _nav_pinned_cases.judge; returns the two worst ratios"""
    every = np.ones(len(ref["rows"]), bool)
    return (C.judge(label, got_sigma, ref["sigma"], ref["e32"]["sigma"], every, "sigma"),
            C.judge(label, got_rgb, ref["rgb"], ref["e32"]["rgb"], every, "rgb"))


def judge_weights(label, got, ref, seed):
    """the five weight gradients: relative Frobenius error <= MARGIN * the float32 oracle's largest over the seeds; returns the worst ratio"""
    worst = 0.0
    for k, name in enumerate(WEIGHT_NAMES):
        want = ref["seeds"][seed]["weights"][k]
        g = np.asarray(got[k], np.float64)
        assert g.shape == want.shape and np.isfinite(g).all(), f"{label} {name}"
        err, y = float(np.linalg.norm(g - want) / np.linalg.norm(want)), float(ref["yard"]["weights"][k])
        assert y > 0
        print(f"{label} seed {seed} d {name}: error {err:.3g}, float32 oracle {y:.3g}, ratio {err / y:.3g}")
        assert err <= MARGIN * y, f"{label} seed {seed}: d {name} is {err / y:.3g} yardsticks from the pinned reference (margin {MARGIN:g})"
        worst = max(worst, err / y)
    return worst


def judge_table(label, got_table, ref, seed):
    """got_table: the dense [rows, 2] table gradient (a torch tensor on any device).  Per level, relative Frobenius error against the reference (zero
    outside `table_rows`) <= MARGIN * the float32 oracle's largest over the seeds; returns the worst ratio"""
    offsets = [int(v) for v in field_arrays("fog", BOUND)[1]]
    s = ref["seeds"][seed]
    want = torch.zeros(got_table.shape, dtype=torch.float64, device=got_table.device)
    want[torch.from_numpy(ref["table_rows"]).to(got_table.device)] = torch.from_numpy(s["table"]).to(got_table.device)
    diff = (got_table.to(torch.float64) - want) ** 2
    assert bool(torch.isfinite(diff).all()), label
    err = np.sqrt(np.array([float(diff[offsets[l]:offsets[l + 1]].sum()) for l in range(16)]))
    worst = 0.0
    for l in range(16):
        if s["level_size"][l] == 0:
            assert err[l] == 0, f"{label} seed {seed}: level {l} has a gradient where the reference has none"
            continue
        e, y = err[l] / s["level_size"][l], float(ref["yard"]["levels"][l])
        assert y > 0
        worst = max(worst, e / y)
        assert e <= MARGIN * y, f"{label} seed {seed}: table level {l} is {e / y:.3g} yardsticks from the pinned reference (error {e:.3g}, float32 oracle {y:.3g})"
    print(f"{label} seed {seed} d table: worst level ratio {worst:.3g}")
    return worst
