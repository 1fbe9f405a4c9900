"""Run-structured lattice inputs for the grid encoder's gradient kernels, and the table of scatter cases built on them.

Why a lattice: k_grid_backward adds with atomics, so the order of its sums is arbitrary and a comparison with the float64 oracle normally needs a
tolerance.  Not on these inputs.  With per_level_scale = 2 every level scale H * 2^l - 1 is an integer; a point x = k / 2^m gives a position
x * scale + 0.5 that is exact in float32, a fractional part that is a multiple of 2^-m and corner weights that are multiples of 2^-(m*D); a gradient
that is a small integer times a power of two makes every term w * g a multiple of ONE quantum q = 2^-(m*D) * gradient unit.  If the largest sum of
|terms| over the rows, A, satisfies A / q <= 2^(p-1) (p = 24 for float, 11 for half: one bit of margin), every partial sum in any order is a multiple
of q below 2^p * q, i.e. exactly representable: the float32 run sums, the rounding of a run's sum to half, every atomic add and the result are exact,
and the kernel must EQUAL the oracle.  tests/test_grid_gradient_inputs_host.py proves the condition for every case from the oracle alone (no GPU);
tests/test_gpu_grid_gradients.py then compares with ==.

What the sequence of points looks like matters as much: k_grid_backward merges runs of consecutive samples that share a cell (heads / start / tail,
a segmented shuffle scan, suppression of all-zero runs, and in the half path an exchange between even and odd lanes), so the samples come in runs."""
import numpy as np

RUN_LENGTHS = (1, 1, 2, 3, 5, 17, 63, 64, 65, 70)
BASE = 4                                    # base resolution of every scatter case: a walk is one long run at level 0 and many short ones further up


def lattice_walks(B, D, m, seed, marks=False):
    """float32 [B, D] points on k / 2^m (k = 0..2^m; out-of-range samples one lattice unit outside).  Sample i is lane i & 63 of the aggregating
    scatter.  In this order:
      0..3     neighbour pairs with exactly one member out of range: (valid, below 0 in axis 0), (above 1 in axis 1, valid)        -- item (e)
      4..12    a run of 9 whose middle sample is out of range in two axes (-2^-m and 1 + 2^-m): it must split the run              -- item (c)
      13..19   a run of 7 whose middle sample has an all-zero gradient: it must NOT split the run                                  -- item (d)
      20..24   a whole run of zero gradients                                                                                        -- item (d)
      25..94   a run of 70 across the wave boundary at 64 (and through B = 63, 64, 65)                                             -- item (a)
      95..194  a walk: every sample one lattice unit from its predecessor along a random axis                                      -- item (b)
      195..259 a run of 65 across the workgroup boundary at 256 (and through B = 257)
      260..262 a run at the point of sample 0: its rows receive contributions from two different runs
      then     runs with lengths from RUN_LENGTHS and walks of 20..90 samples, at random, until B is reached.
    A shorter B is a prefix of a longer one.  With marks=True also returns the indices whose gradient must be zero."""
    assert D >= 2 and m >= 1
    rng = np.random.default_rng(seed)
    n = 1 << m
    unit = np.float32(1.0 / n)
    pts, zero = [], []

    def fresh(avoid=None):
        while True:
            k = rng.integers(0, n + 1, size=D)
            if avoid is None or np.any(k != avoid):
                return k

    def run(k, length):
        pts.extend([k.copy()] * length)

    p0 = fresh()
    below = p0.copy(); below[0] = -1
    above = p0.copy(); above[1] = n + 1
    pts.extend([p0, below, above, p0])
    p1 = fresh(p0)
    run(p1, 9)
    both = p1.copy(); both[0] = -1; both[1] = n + 1
    pts[8] = both
    p2 = fresh(p1)
    run(p2, 7)
    zero.append(16)
    p3 = fresh(p2)
    run(p3, 5)
    zero.extend(range(20, 25))
    p4 = fresh(p3)
    run(p4, 70)

    def walk(k, length):
        k = k.copy()
        for _ in range(length):
            a = rng.integers(0, D)
            step = rng.choice((-1, 1))
            if not 0 <= k[a] + step <= n:
                step = -step
            k[a] += step
            pts.append(k.copy())
        return k

    last = walk(p4, 100)
    p5 = fresh(last)
    run(p5, 65)
    run(p0, 3)
    last = p0
    while len(pts) < B:
        if rng.random() < 0.35:
            last = walk(last, int(rng.integers(20, 91)))
        else:
            last = fresh(last)
            run(last, int(rng.choice(RUN_LENGTHS)))
    x = (np.asarray(pts[:B], dtype=np.int64).astype(np.float32) * unit).astype(np.float32)
    if marks:
        return x, np.asarray([i for i in zero if i < B], dtype=np.int64)
    return x


def lattice_gradients(L, B, C, zero_rows, seed, gmax, unit, keep=1.0):
    """float32 [L, B, C] (level-major, as the kernels take it): integers in [-gmax, gmax] times `unit` (a power of two); zero for the samples in
    `zero_rows`, for every 13th sample (samples behind a saturated ray carry exact zeros) and for a random 1 - keep of the entries."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-gmax, gmax + 1, size=(L, B, C)).astype(np.float32)
    if keep < 1.0:
        g *= rng.random(size=g.shape) < keep
    g[:, 12::13] = 0
    g[:, zero_rows] = 0
    return (g * np.float32(unit) + np.float32(0.0)).astype(np.float32)      # (+ 0.0: no negative zeros from the masks)


def level_cells(x, level, align_corners, base=BASE):
    """(valid [B], cell [B, D]) of the points at one level for per_level_scale = 2: the integer part of x * scale + 0.5 (exact on the lattice)"""
    scale = np.float32(base * 2.0 ** level - 1.0)
    pos = x * scale + np.float32(0.0 if align_corners else 0.5)
    valid = np.all((x >= 0) & (x <= 1), axis=1)
    return valid, np.floor(pos).astype(np.int64)


def run_ids(x, level, align_corners, base=BASE):
    """(valid, run id per sample): maximal sequences of consecutive in-range samples in the same cell of that level; -1 for out-of-range samples"""
    valid, cell = level_cells(x, level, align_corners, base)
    head = np.ones(len(x), bool)
    head[1:] = ~(valid[1:] & valid[:-1] & np.all(cell[1:] == cell[:-1], axis=1))
    ids = np.cumsum(head) - 1
    ids[~valid] = -1
    return valid, ids


class ScatterCase:
    """one instantiation of k_grid_backward with its inputs; everything derived from (D, C, half) and the tuning columns of SCATTER_CASES"""

    def __init__(self, D, C, half, gridtype, align, L, log2T, m, B, gmax, keep):
        self.D, self.C, self.half, self.gridtype, self.align, self.L, self.log2T = D, C, half, gridtype, align, L, log2T
        self.m, self.B, self.gmax, self.keep = m, B, gmax, keep
        self.unit = 1.0 if half else 0.25                  # gradient unit: halves stay normal numbers (q = 2^-(m*D) >= 2^-10)
        self.q = 2.0 ** -(m * D) * self.unit
        self.p = 11 if half else 24
        self.dtype = np.float16 if half else np.float32
        self.gid = 0 if gridtype == "hash" else 1
        self.id = f"D{D}C{C}{'f16' if half else 'f32'}-{gridtype}{'-ac' if align else ''}"

    def inputs(self, B=None):
        """(x [B, D] float32, grad [L, B, C] in the table dtype); B < self.B is a prefix of the main case"""
        x, zero = lattice_walks(self.B, self.D, self.m, 100 * self.D + self.C, marks=True)
        g = lattice_gradients(self.L, self.B, self.C, zero, 7 * self.D + self.C, self.gmax, self.unit, self.keep).astype(self.dtype)
        B = self.B if B is None else B
        return np.ascontiguousarray(x[:B]), np.ascontiguousarray(g[:, :B])

    def offsets(self, oracle):
        offsets, pls = oracle.grid_offsets(self.D, self.L, self.C, 2.0, BASE, self.log2T, None, self.align)
        assert pls == 2.0
        return offsets

    def reference(self, oracle, x, grad):
        """the float64 table gradient of the oracle"""
        offsets = self.offsets(oracle)
        emb = np.zeros((int(offsets[-1]), self.C), self.dtype)
        return oracle.grid_encode_backward(grad, x, emb, offsets, 2.0, BASE, None, self.gid, self.align)[0]


_COMBOS = (("hash", False), ("tiled", False), ("hash", True), ("tiled", True))
_DS, _CS = (2, 3, 4, 5), (1, 2, 4, 8)
_LEVELS = {2: 6, 3: 5, 4: 3, 5: 2}          # levels per D: level 0 is dense, the upper ones are hashed (collisions) at log2T = 9..12
_M_FLOAT = {2: 6, 3: 4, 4: 3, 5: 2}
_KEEP_HALF = {2: 0.5, 3: 0.3, 4: 0.5, 5: 0.5}   # share of the half gradients that is not zero: tuned until A / q fits 10 bits (host test)
_M_HALF = {2: 2, 3: 2, 4: 1, 5: 1}         # m * D <= 10 leaves a half quantum; at m = 1 a lattice point is a cell of its own at every level


def _scatter_cases():
    cases = []
    for half in (False, True):
        for i, D in enumerate(_DS):
            for j, C in enumerate(_CS):
                if half and C == 1:
                    continue                                # refused by the library: the reference never runs a half table with odd C
                gridtype, align = _COMBOS[(i + j + (2 if half else 0)) % 4]
                log2T = 9 + (i + 2 * j) % 4
                if half:
                    cases.append(ScatterCase(D, C, True, gridtype, align, _LEVELS[D], log2T, _M_HALF[D], 301, 1, _KEEP_HALF[D]))
                else:
                    cases.append(ScatterCase(D, C, False, gridtype, align, _LEVELS[D], log2T, _M_FLOAT[D], 1501 - 100 * i, 2, 1.0))
    return cases


SCATTER_CASES = _scatter_cases()
SMALL_BATCHES = (1, 63, 64, 65, 257)        # additionally, for the variants named in small_batch_cases(): prefixes of the main inputs


def small_batch_cases():
    return [c for c in SCATTER_CASES if (c.D == 3 and c.C == 2) or (c.D == 3 and c.C == 1 and not c.half) or (c.D == 3 and c.C == 4 and c.half)]
