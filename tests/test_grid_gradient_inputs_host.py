"""CPU: the inputs of tests/test_gpu_grid_gradients.py meet the conditions under which the table gradient is EXACT, shown from the oracle alone.

The GPU test compares k_grid_backward with the float64 oracle by ==.  That is only a fair demand if no sum can round (tests/_grid_cases.py), and it is
only a sharp one if the data has the structure the kernel's run aggregation acts on.  Both are checked here, on the reference, for every case of the
table, so that the GPU test cannot hide a failure behind its inputs."""
import numpy as np
import pytest

from _grid_cases import BASE, SCATTER_CASES, SMALL_BATCHES, lattice_walks, level_cells, run_ids, small_batch_cases


def test_the_case_table_covers_every_variant_and_every_grid_kind():
    keys = {(c.D, c.C, c.half) for c in SCATTER_CASES}
    assert len(SCATTER_CASES) == len(keys) == 28                               # 4 x 4 float + 4 x 3 half (half with C = 1 is refused)
    assert keys == {(D, C, h) for h in (False, True) for D in (2, 3, 4, 5) for C in (1, 2, 4, 8) if not (h and C == 1)}
    assert {(c.gridtype, c.align) for c in SCATTER_CASES} == {("hash", False), ("hash", True), ("tiled", False), ("tiled", True)}
    for D in (2, 3, 4, 5):
        assert any(c.D == D and c.gridtype == "tiled" for c in SCATTER_CASES) and any(c.D == D and c.align for c in SCATTER_CASES)
    for C in (1, 2, 4, 8):
        assert any(c.C == C and c.gridtype == "tiled" for c in SCATTER_CASES) and any(c.C == C and c.align for c in SCATTER_CASES)
    for c in SCATTER_CASES:
        assert 300 <= c.B <= 1501 and c.B % 256 and 9 <= c.log2T <= 12 and 2 <= c.L <= 6
        # x * scale + 0.5 is exact in float32: bits of the finest level's scale + m <= 24; the D factors of a weight multiply exactly: m * D <= 24
        assert int(BASE * 2 ** (c.L - 1) - 1).bit_length() + c.m <= 24 and c.m * c.D <= 24
    assert len(small_batch_cases()) == 4 and all(b < min(c.B for c in SCATTER_CASES) for b in SMALL_BATCHES)


def test_lattice_walks_has_the_pieces_it_promises():
    D, m = 3, 4
    x = lattice_walks(1200, D, m, 1)
    assert x.dtype == np.float32 and x.shape == (1200, D)
    assert np.array_equal(x * 2 ** m, np.round(x * 2 ** m))                     # on the lattice
    assert np.array_equal(x[:300], lattice_walks(300, D, m, 1))                 # a shorter batch is a prefix
    inside = np.all((x >= 0) & (x <= 1), axis=1)
    u = 2.0 ** -m
    assert list(inside[:4]) == [True, False, False, True] and x[1, 0] == -u and x[2, 1] == 1 + u        # one inactive partner, odd and even position
    assert not inside[8] and x[8, 0] == -u and x[8, 1] == 1 + u and inside[4:8].all() and inside[9:13].all()
    assert np.all(x[4:8] == x[4]) and np.all(x[9:13] == x[4])                   # ... in the middle of a run
    assert np.all(x[25:95] == x[25]) and np.all(x[195:260] == x[195]) and np.all(x[260:263] == x[0])
    step = np.abs(x[95:195] - x[94:194]) * 2 ** m
    assert np.all(step.sum(axis=1) == 1)                                        # the walk: one lattice unit along one axis per sample
    assert inside.sum() >= 1200 - 8


@pytest.mark.parametrize("case", SCATTER_CASES, ids=lambda c: c.id)
def test_scatter_case_is_exact_and_run_structured(oracle, case):
    c = case
    x, grad = c.inputs()
    assert np.array_equal(grad.astype(np.float64) / c.unit, np.round(grad.astype(np.float64) / c.unit))
    ref = c.reference(oracle, x, grad)
    A = c.reference(oracle, x, np.abs(grad)).max()                              # the weights are non-negative: the largest sum of |terms| of any entry
    bits = float(np.log2(A / c.q))
    print(f"{c.id}: m={c.m} B={c.B} L={c.L} log2T={c.log2T} q=2^{int(np.log2(c.q))} A={A:.4g} bits needed {bits:.1f} of {c.p - 1} allowed")
    assert A / c.q <= 2 ** (c.p - 1)
    assert np.array_equal(ref / c.q, np.round(ref / c.q))                       # every oracle sum is a multiple of the quantum
    assert np.count_nonzero(np.abs(ref).sum(axis=1)) >= 50

    offsets = c.offsets(oracle)
    collisions, n_runs = False, []
    for level in range(c.L):
        valid, ids = run_ids(x, level, c.align)
        n_runs.append(int(ids.max()) + 1)
        stride = BASE * 2 ** level + (0 if c.align else 1)
        collisions |= stride ** c.D > int(offsets[level + 1] - offsets[level])  # more cells than rows: the level is hashed, or tiled over itself
    assert collisions
    valid, ids = run_ids(x, 0, c.align)
    assert np.bincount(ids[valid]).max() > 64                                   # some run is longer than a wave
    assert n_runs[-1] > n_runs[0] if c.m > 1 else n_runs[-1] == n_runs[0]       # finer levels have runs of their own (at m = 1 a point is a cell)

    # at least one row receives contributions from two different runs: runs of level 0 that are not neighbours but lie in the same cell, both with a
    # non-zero gradient; the oracle, fed one run at a time, says whether they meet in a row
    _, cell = level_cells(x, 0, c.align)
    live = np.abs(grad[0]).sum(axis=1) > 0
    first_run_of_cell, meets = {}, 0
    for r in range(n_runs[0]):
        members = ids == r
        if not (members & live).any():
            continue
        key = tuple(cell[np.flatnonzero(members)[0]])
        if key not in first_run_of_cell:
            first_run_of_cell[key] = r
            continue
        parts = [c.reference(oracle, x, np.abs(grad) * (ids == s)[None, :, None])[offsets[0]:offsets[1]] for s in (first_run_of_cell[key], r)]
        meets += bool(((parts[0] != 0) & (parts[1] != 0)).any())
        if meets >= 3:
            break
    assert meets >= 1
