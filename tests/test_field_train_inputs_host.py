"""CPU: the inputs of tests/test_gpu_field_train_exact.py meet the conditions under which the fused training step is EXACT, shown from the oracle alone.

The GPU test compares csrc/field_train.hip with the oracle's composition of the same step by ==.  That is only a fair demand if no float32 sum of the
kernel can round (tests/_field_cases.py), and only a sharp one if the data reaches every block: both are checked here for every case of the table."""
import numpy as np
import pytest

import _field_cases as FC
from _field_cases import CASE, CASES, SMALL_BATCHES

BUDGET = 23.0                                # bits of a float32 significand, less one of margin (as tests/_grid_cases.py)


@pytest.fixture(scope="module")
def sh_oracle():
    from oracle import sh_oracle
    return sh_oracle


def test_the_case_table_holds_what_the_kernel_branches_on():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    assert SMALL_BATCHES == (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)      # tile (16), pair (32), wave (64), workgroup (128) edges
    assert all(f"M{M}-all" in CASE for M in SMALL_BATCHES)
    # sparse lists below and above the 32,768 samples at which the backward's workgroup count caps at 256; the two-pass forward's 65,536
    assert CASE["M5000-sparse"].M < 32768 < CASE["M40000-sparse-ends"].M < 65536 < CASE["M70001-sparse"].M
    assert CASE["M110000-dense-large"].n_colour == 200 and CASE["M200-all-clamp"].params == "clamp"


def test_the_field_has_scale_two_and_dense_and_hashed_levels(oracle):
    a = FC.PARAMS["small"].arrays(oracle)
    sizes = np.diff(a["offsets"])
    scale, reso = oracle.grid_level_table(FC.L, np.float32(1.0), FC.H)
    assert np.array_equal(scale, 16.0 * 2.0 ** np.arange(16) - 1.0)               # integers: a lattice point's position is exact
    assert list(sizes[:3]) == [4920, 35944, 274632] and np.all(sizes[3:] == 1 << 19)   # three dense levels, thirteen hashed; the binned scatter's limit
    # levels 12 and 13 (sides 65,537 and 131,073) are the ones whose 32-bit stride product wraps below the level's size: the reference does not hash
    # them, it indexes them with the wrapped strides modulo the size (gridencoder.cu:54-72), and the fused encoders must do the same
    indexed = []
    for level in range(FC.L):
        stride, side = 1, int(reso[level]) + 1
        for _ in range(3):
            if stride <= sizes[level]:
                stride = (stride * side) & 0xFFFFFFFF
        indexed.append(stride <= sizes[level])
    assert indexed == [True] * 3 + [False] * 9 + [True] * 2 + [False] * 2
    for P in FC.PARAMS.values():
        a = P.arrays(oracle)
        assert np.array_equal(a["emb"], np.round(a["emb"])) and float(np.abs(a["emb"]).max()) == P.tmax
        for w in a["sw"] + a["cw"]:
            assert set(np.unique(np.abs(w[w != 0])).tolist()) <= {0.5, 1.0, 0.5 * P.logit_gain}


def test_axis_directions_encode_to_halves_a_float_evaluation_cannot_miss(sh_oracle):
    sh = sh_oracle.sh_encode(FC.AXES.astype(np.float64), 4)
    nz = np.abs(sh) > 2.0 ** -26                                                    # (anything smaller is a zero of the polynomial: rounds to +-0)
    assert np.all((np.abs(sh[nz]) > 0.28) & (np.abs(sh[nz]) < 0.75)) and not FC.near_half_boundary(sh[nz]).any()
    assert FC.quantum_exp(sh.astype(np.float16)) >= -12


def _hidden_layers(oracle, B):
    """(name, exact pre-activations, kept activations, gradient arriving at the activations before the ReLU mask) of the five hidden layers"""
    a, F, R = B["P"].arrays(oracle), B["F"], B["R"]
    sw, cw = a["sw"], a["cw"]
    pre = FC.pre_activations
    return [("density h1", pre(sw[0], F["feats"]), F["fbs"][0], pre(sw[1].T, R["bbs"][0])),
            ("density h2", pre(sw[1], F["fbs"][0]), F["fbs"][1], pre(sw[2].T, R["gdo"])),
            ("colour c1", pre(cw[0], F["cin"]), F["fbc"][0], pre(cw[1].T, R["bbc"][1])),
            ("colour c2", pre(cw[1], F["fbc"][0]), F["fbc"][1], pre(cw[2].T, R["bbc"][0])),
            ("colour c3", pre(cw[2], F["fbc"][1]), F["fbc"][2], pre(cw[3].T, R["gout"]))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_is_exact_and_reaches_every_block(oracle, sh_oracle, case):
    B = case.build(oracle, sh_oracle)
    a, F, R, M = B["P"].arrays(oracle), B["F"], B["R"], case.M
    listed, gs, gc, ku = B["listed"], B["gs"], B["gc"], B["ku"]
    n_live = int(listed.sum())

    # ---- the quantum-and-budget condition, block by block ----
    bits = FC.block_bits(oracle, B)
    print(f"{case.id}: {n_live} live of {M}; bits needed of 24: " + ", ".join(f"{k} {v:.1f}" for k, v in bits.items()))
    for name, v in bits.items():
        assert v <= BUDGET, (name, v)
    # every half operand is a normal number or zero, and nothing overflowed
    for name in ("feats", "h", "fbs", "cin", "ho", "fbc"):
        v = np.abs(np.asarray(F[name], np.float32))
        assert np.isfinite(v).all() and (v[v > 0] >= 2.0 ** -14).all(), name
    for name in ("gout", "bbc", "ggeo", "gdo", "bbs", "genc"):
        v = np.abs(np.asarray(R[name], np.float32))
        assert np.isfinite(v).all() and (v[v > 0] >= 2.0 ** -14).all(), name
    assert np.isfinite(R["gwc"]).all() and np.isfinite(R["gws"]).all()          # (results, not operands: rounded to half once, subnormals included)
    # the input gradients of both nets are halves already: the rounding the op graph applies there changes nothing
    assert np.array_equal(R["ggeo"].astype(np.float32), R["gic"][:, 16:31])
    assert np.array_equal(R["gis"].astype(np.float16).astype(np.float32), R["gis"])
    # table: each term half(w * g), w >= 1/8, is exact (a normal half), and the float32 the scatter writes holds the sum
    assert FC.quantum_exp(R["genc"]) - 3 >= -14
    assert np.array_equal(R["table_values"].astype(np.float32).astype(np.float64), R["table_values"])

    # ---- no run of two samples in one cell, in the batch or in the list ----
    x = B["x"]
    assert np.array_equal(x, FC.world_points(B["k"])) and np.array_equal(F["xn"] * 2, np.round(F["xn"] * 2))
    assert np.any(x[1:] != x[:-1], axis=1).all()
    xl = x[listed]
    assert np.any(xl[1:] != xl[:-1], axis=1).all()

    # ---- the tailored gradients do what they were chosen for ----
    coloured = int(np.any(B["wanted"], axis=1).sum())
    print(f"{case.id}: colour gradients on {coloured} samples, {B['given_up']} channels given up; rgb margin set {int(F['margin'].sum())} of {3 * M}")
    assert B["given_up"] <= 0.01 * 3 * coloured                              # the sigmoid-margin cap
    assert not (F["margin"] & (gc != 0)).any()
    g_logit = FC.colour_logit_gradient(F["rgb"], gc).astype(np.float32)
    assert np.isin(np.abs(g_logit), [0.0, 0.25, 0.5, 0.75]).all() and np.array_equal(g_logit != 0, gc != 0)
    h0 = F["h"][:, 0].astype(np.float32)
    e = oracle.expf(np.minimum(h0, np.float32(15.0))).astype(np.float64)
    want = ku != 0
    assert float(np.max(np.abs(gs[want].astype(np.float64) * e[want] / ku[want] - 1.0), initial=0.0)) < 2.0 ** -13
    assert np.array_equal(FC.density_logit_gradient(oracle, h0, gs).astype(np.float64), ku)
    assert np.array_equal(listed, (gs.view(np.uint32) != 0) | np.any(gc.view(np.uint32) != 0, axis=1)) and np.array_equal(listed, B["live"])

    # ---- floors: no block is vacuous ----
    gwc, gws = R["gwc"], R["gws"]
    blocks = {"colour in": gwc[FC.C_IN:FC.C_HID1], "colour hid1": gwc[FC.C_HID1:FC.C_HID2], "colour hid2": gwc[FC.C_HID2:FC.C_OUT],
              "colour out (3 live rows)": gwc[FC.C_OUT:FC.C_OUT + 3 * 64], "density in": gws[FC.S_IN:FC.S_HID], "density hid": gws[FC.S_HID:FC.S_OUT],
              "density out": gws[FC.S_OUT:]}
    share = {k: float(np.mean(v != 0)) for k, v in blocks.items()}
    enc_share = float(np.mean(R["genc"][:, listed] != 0))
    print(f"{case.id}: non-zero share of the weight gradients: " + ", ".join(f"{k} {v:.2f}" for k, v in share.items()) + f"; of grad_enc {enc_share:.2f}")
    floor = 0.25 if n_live > 1 else 0.05          # (one sample's outer products of sparse ReLU activations cannot fill a quarter of a 64 x 64 block)
    for k, v in share.items():
        assert v >= floor, (k, v)
    assert not gwc[FC.C_OUT + 3 * 64:].any()      # the padded rows of the colour output layer get no gradient
    assert enc_share >= 0.10
    for name, pre, act, arriving in _hidden_layers(oracle, B):
        pre, act, arriving = pre[listed], act[listed].astype(np.float32), arriving[listed]
        assert np.array_equal(np.maximum(pre, 0).astype(np.float16).astype(np.float32), act), name
        assert (act > 0).any() and (pre < 0).any() and (pre == 0).any(), name
        assert ((act > 0) & (arriving != 0)).any() and ((act == 0) & (arriving != 0)).any(), name      # the mask passes some gradients and stops others
    levels = np.searchsorted(a["offsets"], R["table_rows"], side="right") - 1
    assert (levels < 3).any() and (levels >= 3).any()

    # ---- what each case is there for ----
    if case.layout == "all":
        assert n_live == M
    if case.layout.startswith("sparse"):
        assert 150 <= n_live <= 250 and bool(listed[0]) != bool(listed[-1]) and bool(listed[0]) == (case.layout == "sparse-ends")
        edges = np.flatnonzero(np.diff(np.concatenate([[0], (~listed).astype(np.int8), [0]])))
        starts, lengths = edges[::2], edges[1::2] - edges[::2]
        # dead runs of many lengths, starting and ending at every position of a 16-sample tile and most of a 32-sample pair
        assert len(set(lengths.tolist())) >= 40 and lengths.min() <= 4 and lengths.max() >= 100
        for at in (starts, starts + lengths):
            assert len(set((at % 16).tolist())) == 16 and len(set((at % 32).tolist())) >= 24
        one, negz = B["special"]["one_channel"], B["special"]["negative_zero"]
        assert gs[one] == 0 and np.count_nonzero(gc[one]) == 1
        assert gs.view(np.uint32)[negz] == 0x80000000 and not gc[negz].any() and listed[negz]
    if M > 4:
        out = listed & np.any((F["xn"] < 0) | (F["xn"] > 1), axis=1)
        assert out.any() and not F["feats"][out].any() and np.abs(R["gdo"][out]).sum() > 0 and not R["table_values"].size == 0
    if case.layout == "dense":
        assert n_live > 3 * 32 * 1024                                       # 256 workgroups of 4 waves: every wave takes three pairs or more
        assert (~listed).sum() > 1000
    if case.params == "clamp":
        live_h0 = h0[listed & want]
        assert (live_h0 > 15).sum() >= 5 and (live_h0 <= 15).sum() >= 5 and float(live_h0.max()) < 80
        # the gradients tell exp(min(h0, 15)) from exp(h0)
        assert not np.array_equal((gs * oracle.expf(h0)).astype(np.float16), (gs * oracle.expf(np.minimum(h0, np.float32(15)))).astype(np.float16))
