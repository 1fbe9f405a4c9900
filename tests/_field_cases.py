"""Exact inputs for the field's fused training step (csrc/field_train.hip), the oracle's composition of the same step, and the table of cases.

Why the data looks the way it does (the method of tests/_grid_cases.py, carried through two networks): if every term of a sum is a multiple of one
quantum q (a power of two) and the sum of the terms' magnitudes stays below 2^24 q, every partial sum in every order is a float32 -- the matrix-core
accumulators, the four-wave sum through LDS, the per-workgroup rows and k_field_train_wgrad_finish all form exact values, whatever their order.  Rounding
an exact value to half is one correctly rounded operation, the same in the kernel and in an oracle that sums in double and rounds once, and a multiple of
q rounded to half is still a multiple of q: the condition carries from layer to layer.  tests/test_field_train_inputs_host.py proves it for every block
of every case from the oracle alone; tests/test_gpu_field_train_exact.py then compares with ==.

  field      NGPFieldFF(bound=256): per_level_scale is exactly 2, every level scale 16 * 2^l - 1 an integer, the normalisation a power of two
             (levels 12 and 13 of this grid are the ones the reference indexes with wrapped 32-bit strides instead of hashing them)
  points     the lattice k / 2 of the unit cube (k = 0, 1, 2): corner weights are 0 or powers of two down to 1/8, and a lattice point is a cell of its
             own at every level; a few points one unit outside the box (zero features, live gradients); no two neighbours -- in the batch or in the
             list of live samples -- are the same point, so the binned scatter meets no run of more than one sample (it rounds a run's sum to half)
  table      small integers; weights: a few +-1 / +-0.5 per row; directions: the six axes (their SH values as halves are multiples of 2^-12)
  gradients  chosen from the oracle's own forward so that the two output-gradient formulas of the kernel return one- or two-bit numbers:
             d loss / d sigma = float32(k u / exp(min(h0, 15))), whose product with exp(min(h0, 15)) rounds to k u in half, and d loss / d rgb = a half
             gh for which half((gh * (1 - s)) * s) is 0.25, 0.5 or 0.75 (s = half(sigmoid(logit)); found by search over the normal halves)."""
import numpy as np

BOUND = 256                                  # desired_resolution 2048 * 256 = 16 * 2^15: per_level_scale == 2.0
L, C, H = 16, 2, 16
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
MARGIN = 2.0 ** -20                          # relative distance from a half rounding boundary below which a float32 evaluation may land on the other side
S_IN, S_HID, S_OUT = 0, 64 * 32, 64 * 32 + 64 * 64                                   # FFMLP's flat layout: [hidden, in] | [hidden, hidden] ... | [16, hidden]
C_IN, C_HID1, C_HID2, C_OUT = 0, 64 * 32, 64 * 32 + 64 * 64, 64 * 32 + 2 * 64 * 64
N_SIGMA, N_COLOR = 7168, 11264


# ---- quanta and budgets ------------------------------------------------------------------------------------------------------------------------------
def quantum_exp(a):
    """e such that every entry of a is a multiple of 2^e (the largest such e); None for an all-zero array"""
    a = np.abs(np.asarray(a, np.float64)).ravel()
    a = a[a > 0]
    if a.size == 0:
        return None
    mant, e = np.frexp(a)
    mi = (mant * 2.0 ** 53).astype(np.int64)
    return int((e - 53 + np.log2((mi & -mi).astype(np.float64)).astype(np.int64)).min())


def bits_over_samples(G, A):
    """bits that sum_s G[s, o] A[s, i] needs to be exact in any order: log2(largest sum of |terms| / quantum of a term)"""
    G, A = np.asarray(G, np.float64), np.asarray(A, np.float64)
    qg, qa = quantum_exp(G), quantum_exp(A)
    if qg is None or qa is None:
        return 0.0
    return float(np.log2((np.abs(G).T @ np.abs(A)).max())) - qg - qa


def bits_per_sample(W, X):
    """the same for the per-sample sums sum_k X[s, k] W[o, k] of a layer"""
    W, X = np.asarray(W, np.float64), np.asarray(X, np.float64)
    qw, qx = quantum_exp(W), quantum_exp(X)
    if qw is None or qx is None:
        return 0.0
    return float(np.log2((np.abs(X) @ np.abs(W).T).max())) - qw - qx


def near_half_boundary(v):
    """True where the float64 value lies within MARGIN (relative) of the midpoint of two neighbouring halves"""
    v = np.asarray(v, np.float64)
    h = v.astype(np.float16)
    lo, hi = np.nextafter(h, np.float16(-np.inf)), np.nextafter(h, np.float16(np.inf))
    b0, b1 = (h.astype(np.float64) + lo.astype(np.float64)) / 2, (h.astype(np.float64) + hi.astype(np.float64)) / 2
    return np.minimum(np.abs(v - b0), np.abs(v - b1)) < MARGIN * np.abs(v)


# ---- the field ---------------------------------------------------------------------------------------------------------------------------------------
def _sparse_rows(rng, shape, nnz, scale):
    w = np.zeros(shape, np.float16)
    for r in range(shape[0]):
        idx = rng.choice(shape[1], size=nnz, replace=False)
        w[r, idx] = rng.choice([-1.0, 1.0], size=nnz) * scale
    return w


class FieldParams:
    """table and weights of one exact field.  tmax: table entries are integers in [-tmax, tmax]; nnz: non-zero weights per row (+-1 in the input
    layers, +-0.5 elsewhere); logit_gain: factor on the density net's output row 0 (the clamp case pushes some density logits past 15 with it)"""

    def __init__(self, name, tmax, nnz, nnz_colour=4, nnz_colour_out=16, logit_gain=1.0, seed=0):
        self.name, self.tmax, self.nnz, self.logit_gain, self.seed = name, tmax, nnz, logit_gain, seed
        self.nnz_colour, self.nnz_colour_out = nnz_colour, nnz_colour_out
        self._arrays = None

    def arrays(self, oracle):
        if self._arrays is None:
            rng = np.random.default_rng(1000 + self.seed)
            offsets, pls = oracle.grid_offsets(3, L, C, 2.0, H, 19, 2048 * BOUND, False)
            assert pls == 2.0
            emb = rng.integers(-self.tmax, self.tmax + 1, size=(int(offsets[-1]), C)).astype(np.float16)
            sw = [_sparse_rows(rng, (64, 32), self.nnz, 1.0), _sparse_rows(rng, (64, 64), self.nnz, 0.5), _sparse_rows(rng, (16, 64), self.nnz, 0.5)]
            sw[2][0] *= np.float16(self.logit_gain)
            # (rows 3..15 of the colour net's padded output layer are live weights too: their outputs are unused and their gradients must come out zero)
            n = self.nnz_colour
            cw = [_sparse_rows(rng, (64, 32), n, 1.0), _sparse_rows(rng, (64, 64), n, 0.5), _sparse_rows(rng, (64, 64), n, 0.5),
                  _sparse_rows(rng, (16, 64), self.nnz_colour_out, 0.5)]
            cw[0][:, 31] = 0                                        # (column 31 of the colour input is the zero padding)
            self._arrays = dict(offsets=offsets, emb=emb, sw=sw, cw=cw, ws=np.concatenate([w.ravel() for w in sw]),
                                wc=np.concatenate([w.ravel() for w in cw]))
            assert self._arrays["ws"].size == N_SIGMA and self._arrays["wc"].size == N_COLOR
        return self._arrays

    def model(self, oracle):
        """the arrays NGPFieldFF.load_arrays takes"""
        a = self.arrays(oracle)
        return {"embeddings": a["emb"].astype(np.float32), "sigma_weights": a["ws"].astype(np.float32), "color_weights": a["wc"].astype(np.float32)}


PARAMS = {"small": FieldParams("small", tmax=2, nnz=4), "large": FieldParams("large", tmax=1, nnz=3, seed=1),
          "clamp": FieldParams("clamp", tmax=2, nnz=4, logit_gain=8.0)}


# ---- samples -----------------------------------------------------------------------------------------------------------------------------------------
def live_layout(M, kind, seed):
    """bool [M]: which samples get a gradient.  'all'; 'sparse' / 'sparse-ends' (about 200 live: single ones and blocks of 2..33, between dead runs of
    every length and alignment; first sample dead and last live / first live and last dead); 'dense' (nine in ten, dead runs of 1..40)"""
    if kind == "all":
        return np.ones(M, bool)
    rng = np.random.default_rng(seed)
    live = np.zeros(M, bool)
    if kind == "dense":
        i = 0
        while i < M:
            run = int(rng.integers(1, 400))
            live[i:i + run] = True
            i += run + int(rng.integers(1, 41))
        return live
    blocks = [1] * 100 + [2, 3, 5, 15, 16, 17, 31, 33]                 # 222 live samples
    rng.shuffle(blocks)
    room = M - sum(blocks) - 2
    assert room > 4 * len(blocks)
    cuts = np.sort(rng.choice(room, size=len(blocks), replace=False))
    gaps = np.diff(np.concatenate([[0], cuts])) + 1                    # dead runs of >= 1 in front of every block
    i = 0
    for gap, b in zip(gaps, blocks):
        i += int(gap)
        live[i:i + b] = True
        i += b
    if kind == "sparse":
        live[0], live[M - 1] = False, True
    else:
        live[0], live[M - 1] = True, False
    return live


def lattice_samples(M, listed, n_outside, seed):
    """(k int [M, 3], directions float32 [M, 3]).  k / 2 is the normalised position: 0..2 inside the box, -1 or 3 one unit outside in one axis (the first
    n_outside entries of `listed` that come round).  No sample sits on the point of its predecessor in the batch, and no sample of `listed` (the samples
    that will be in the live list) on the point of its predecessor in that list."""
    rng = np.random.default_rng(seed)
    draw = rng.integers(0, 27, size=M)
    k = np.zeros((M, 3), np.int64)
    outside = set(np.flatnonzero(listed)[3::7][:n_outside].tolist())
    prev = prev_listed = -1
    for i in range(M):
        c = int(draw[i])
        while c == prev or (listed[i] and c == prev_listed):
            c = (c + 1) % 27
        k[i] = (c % 3, (c // 3) % 3, c // 9)
        if i in outside:
            k[i, i % 3] = -1 if (i // 3) % 2 else 3                  # (still not its neighbours' point: c differs from theirs)
        prev = c
        if listed[i]:
            prev_listed = c
    return k, AXES[rng.integers(0, 6, size=M)]


def world_points(k):
    """float32 [M, 3] world coordinates of the lattice points: (k / 2 * 2 - 1) * BOUND, exact"""
    return ((k - 1) * BOUND).astype(np.float32)


# ---- the oracle's composition of the step (nerf/network_ff.py:51-77 and its autograd backward) -----------------------------------------------------------
def reference_forward(oracle, sh_oracle, P, x, d):
    a = P.arrays(oracle)
    # GridEncoder.forward: normalise to the unit cube (exact: 2 * BOUND is a power of two), encode with the half table, level-major -> [M, 32]
    xn = ((x + np.float32(BOUND)) / np.float32(2 * BOUND)).astype(np.float32)
    enc, _ = oracle.grid_encode_forward(xn, a["emb"], a["offsets"], 2.0, H)
    feats = np.ascontiguousarray(enc.transpose(1, 0, 2).reshape(len(x), L * C))
    # density net: FFMLP(32 -> 64 -> 64 -> 16), num_layers = 2 in its API; output 0 is the density logit, 1..15 the geometry features
    h, fbs = oracle.ffmlp_forward(feats, a["ws"], 32, 16, 64, 2, save=True)
    sigma = oracle.expf(h[:, 0].astype(np.float32))                   # trunc_exp: exp of the half logit in float32
    # colour net input: cat(SH16 rounded to half, geo15, one zero column); FFMLP(32 -> 64 -> 64 -> 64 -> 16 padded), num_layers = 3
    sh64 = sh_oracle.sh_encode(d.astype(np.float64), 4)
    cin = np.concatenate([sh64.astype(np.float16), h[:, 1:16], np.zeros((len(x), 1), np.float16)], axis=1)
    ho, fbc = oracle.ffmlp_forward(cin, a["wc"], 32, 16, 64, 3, save=True)
    # torch.sigmoid on the half logits: evaluated in float, rounded to half
    s64 = 1.0 / (1.0 + np.exp(-ho[:, :3].astype(np.float64)))
    rgb = s64.astype(np.float16).astype(np.float32)
    return dict(xn=xn, feats=feats, h=h, fbs=fbs, sigma=sigma, sh64=sh64, cin=cin, ho=ho, fbc=fbc, rgb=rgb, margin=near_half_boundary(s64))


def colour_logit_gradient(rgb, gc):
    """torch.sigmoid's backward on halves, float opmath: half(float32(float32(half(gc) * (1 - s)) * s)) -- numpy's float32 operations are these"""
    gh = np.asarray(gc, np.float32).astype(np.float16).astype(np.float32)
    s = np.asarray(rgb, np.float32)
    return ((gh * (np.float32(1.0) - s)) * s).astype(np.float16)


def density_logit_gradient(oracle, h0, gs):
    """trunc_exp's backward: half(float32(gs * exp(min(h0, 15)))), the exp in float32"""
    e = oracle.expf(np.minimum(np.asarray(h0, np.float32), np.float32(15.0)))
    return (np.asarray(gs, np.float32) * e).astype(np.float16)


def reference_backward(oracle, P, F, gs, gc):
    a = P.arrays(oracle)
    M = len(gs)
    # colour net: the gradient of its 3 logits (padded to 16 columns), back through the layers; weight gradients summed in double
    gout = np.zeros((M, 16), np.float16)
    gout[:, :3] = colour_logit_gradient(F["rgb"], gc)
    gwc, gic, bbc = oracle.ffmlp_backward(gout, F["cin"], a["wc"], F["fbc"], 32, 16, 64, 3, True)
    # its input gradient, columns 16..30, is the geometry features' gradient (a half tensor in the op graph); the density logit's comes from trunc_exp
    ggeo = gic[:, 16:31].astype(np.float16)
    gdo = np.concatenate([density_logit_gradient(oracle, F["h"][:, 0], gs)[:, None], ggeo], axis=1)
    gws, gis, bbs = oracle.ffmlp_backward(gdo, F["feats"], a["ws"], F["fbs"], 32, 16, 64, 2, True)
    # the encoded features' gradient as halves, level-major, into the table
    genc = np.ascontiguousarray(gis.astype(np.float16).reshape(M, L, C).transpose(1, 0, 2))
    table, _ = oracle.grid_encode_backward(genc, F["xn"], a["emb"], a["offsets"], 2.0, H)
    rows = np.flatnonzero(np.any(table != 0, axis=1))
    # weight gradients: one float32 sum rounded to half once, returned as float32 (k_field_train_wgrad_finish)
    return dict(gout=gout, gic=gic, bbc=bbc, ggeo=ggeo, gdo=gdo, gis=gis, bbs=bbs, genc=genc, gwc_sum=gwc, gws_sum=gws,
                gwc=gwc.astype(np.float16).astype(np.float32), gws=gws.astype(np.float16).astype(np.float32),
                table_rows=rows, table_values=table[rows], table_shape=table.shape)


# ---- gradients tailored to the forward ---------------------------------------------------------------------------------------------------------------
_NORMAL_HALVES = np.arange(0x0400, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
_TARGETS = np.array([0.25, 0.5, 0.75], np.float16)


def tailored_colour_gradients(F, wanted, rng):
    """float32 [M, 3]: +-gh where `wanted`, gh a normal half whose modelled logit gradient is 0.25, 0.5 or 0.75; 0 where the sigmoid is within MARGIN of
    a half rounding boundary (the kernel's float32 sigmoid may round the other way there) or no such half exists.  Returns (gc, channels given up)."""
    gc = np.zeros(F["rgb"].shape, np.float32)
    cache, given_up = {}, 0
    for i, ch in zip(*np.nonzero(wanted)):
        s = F["rgb"][i, ch]
        if s not in cache:
            g = ((_NORMAL_HALVES * (np.float32(1.0) - s)) * s).astype(np.float16)
            cache[s] = _NORMAL_HALVES[np.isin(g, _TARGETS)]
        if F["margin"][i, ch] or len(cache[s]) == 0:
            given_up += 1
            continue
        gc[i, ch] = rng.choice(cache[s]) * rng.choice([-1.0, 1.0])
    return gc, given_up


def tailored_density_gradients(oracle, F, ku):
    """float32 [M]: ku / exp(min(h0, 15)) for the wanted values ku of the density logit's gradient (one- or two-bit numbers, 0 for none)"""
    e = oracle.expf(np.minimum(F["h"][:, 0].astype(np.float32), np.float32(15.0))).astype(np.float64)
    return (np.asarray(ku, np.float64) / e).astype(np.float32)


class FieldCase:
    """one batch: M samples, a layout of live samples, which of them get colour gradients, and the field it runs on"""

    def __init__(self, M, layout="all", params="small", n_colour=None, specials=False, ku_max=3, seed=None):
        self.M, self.layout, self.params, self.n_colour, self.specials, self.ku_max = M, layout, params, n_colour, specials, ku_max
        self.seed = M if seed is None else seed
        self.id = f"M{M}-{layout}" + ("" if params == "small" else f"-{params}")
        self._built = None

    def build(self, oracle, sh_oracle):
        """inputs, the oracle's forward and backward; computed once per process"""
        if self._built is not None:
            return self._built
        M, P = self.M, PARAMS[self.params]
        rng = np.random.default_rng(7 * self.seed + 1)
        live = live_layout(M, self.layout, self.seed)
        k, d = lattice_samples(M, live, n_outside=3 if M >= 16 else (1 if M > 4 else 0), seed=self.seed)
        x = world_points(k)
        F = reference_forward(oracle, sh_oracle, P, x, d)
        idx = np.flatnonzero(live)
        # colour gradients on (about) n_colour live samples, two channels in three; density gradients k * 0.25 on four live samples in five
        coloured = idx if self.n_colour is None or self.n_colour >= len(idx) else np.sort(rng.choice(idx, size=self.n_colour, replace=False))
        wanted = np.zeros((M, 3), bool)
        wanted[coloured] = rng.random((len(coloured), 3)) < 0.67
        ku = np.zeros(M)
        ku[idx] = rng.choice([v for v in range(-self.ku_max, self.ku_max + 1) if v], size=len(idx)) * 0.25 * (rng.random(len(idx)) < 0.8)
        special = {}
        if self.specials:
            # a live sample whose only gradient is one colour channel; a sample whose density gradient is -0.0 and nothing else: live by its bits
            one, negz = int(idx[len(idx) // 3]), int(idx[2 * len(idx) // 3])
            ku[one], wanted[one] = 0.0, (False, True, False)
            ku[negz], wanted[negz] = 0.0, False
            special = {"one_channel": one, "negative_zero": negz}
        gc, given_up = tailored_colour_gradients(F, wanted, rng)
        if self.specials and gc[special["one_channel"], 1] == 0:       # (its channel was given up: any other will do)
            w = np.zeros((M, 3), bool)
            w[special["one_channel"], int(np.flatnonzero(~F["margin"][special["one_channel"]])[0])] = True
            gc += tailored_colour_gradients(F, w, rng)[0]
        # every live sample gets SOME gradient (the points were arranged for this list of live samples): a density gradient where nothing else came out
        bare = live & ~np.any(gc != 0, axis=1) & (ku == 0)
        if self.specials:
            bare[special["negative_zero"]] = False
        ku[bare] = 0.25
        gs = tailored_density_gradients(oracle, F, ku)
        if self.specials:
            gs[special["negative_zero"]] = np.float32(-0.0)
        # a sample is in the kernel's live list when any of its four incoming gradients has a bit set
        listed = (gs.view(np.uint32) != 0) | np.any(gc.view(np.uint32) != 0, axis=1)
        assert np.array_equal(listed, live)
        R = reference_backward(oracle, P, F, gs, gc)
        self._built = dict(case=self, P=P, k=k, x=x, d=d, gs=gs, gc=gc, ku=ku, wanted=wanted, given_up=given_up, live=live, listed=listed,
                           special=special, F=F, R=R)
        return self._built


SMALL_BATCHES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
CASES = ([FieldCase(M, seed={33: 1033}.get(M)) for M in SMALL_BATCHES]       # (seed: no wanted colour channel of M = 33 in the sigmoid's margin set)
         + [FieldCase(5000, "sparse", specials=True), FieldCase(40000, "sparse-ends", specials=True),
            FieldCase(70001, "sparse", specials=True, seed=3),
            FieldCase(110000, "dense", params="large", n_colour=200, ku_max=1),
            FieldCase(200, "all", params="clamp", seed=11)])
CASE = {c.id: c for c in CASES}


# ---- what the host test asserts, as figures ------------------------------------------------------------------------------------------------------------
def block_bits(oracle, B):
    """{block: bits its sums need out of 24}: the seven weight gradients (sums over samples), the forward layers and the backward chain (sums per
    sample) and the table gradient (sums per row)"""
    a, F, R = B["P"].arrays(oracle), B["F"], B["R"]
    sw, cw = a["sw"], a["cw"]
    bits = {
        "wgrad colour out": bits_over_samples(R["gout"], F["fbc"][2]), "wgrad colour hid2": bits_over_samples(R["bbc"][0], F["fbc"][1]),
        "wgrad colour hid1": bits_over_samples(R["bbc"][1], F["fbc"][0]), "wgrad colour in": bits_over_samples(R["bbc"][2], F["cin"]),
        "wgrad density out": bits_over_samples(R["gdo"], F["fbs"][1]), "wgrad density hid": bits_over_samples(R["bbs"][0], F["fbs"][0]),
        "wgrad density in": bits_over_samples(R["bbs"][1], F["feats"]),
        "forward density in": bits_per_sample(sw[0], F["feats"]), "forward density hid": bits_per_sample(sw[1], F["fbs"][0]),
        "forward density out": bits_per_sample(sw[2], F["fbs"][1]), "forward colour in": bits_per_sample(cw[0], F["cin"]),
        "forward colour hid1": bits_per_sample(cw[1], F["fbc"][0]), "forward colour hid2": bits_per_sample(cw[2], F["fbc"][1]),
        "forward colour out": bits_per_sample(cw[3], F["fbc"][2]),
        "backward colour out": bits_per_sample(cw[3].T, R["gout"]), "backward colour hid2": bits_per_sample(cw[2].T, R["bbc"][0]),
        "backward colour hid1": bits_per_sample(cw[1].T, R["bbc"][1]), "backward colour in": bits_per_sample(cw[0].T, R["bbc"][2]),
        "backward density out": bits_per_sample(sw[2].T, R["gdo"]), "backward density hid": bits_per_sample(sw[1].T, R["bbs"][0]),
        "backward density in": bits_per_sample(sw[0].T, R["bbs"][1]),
    }
    # table: every term is half(w * g) with w in {1/8, 1/4, 1/2, 1}; the weights are non-negative, so the oracle on |g| gives the sums of |terms|
    qe = quantum_exp(R["genc"])
    if qe is None:
        bits["table"] = 0.0
    else:
        A, _ = oracle.grid_encode_backward(np.abs(R["genc"]), F["xn"], a["emb"], a["offsets"], 2.0, H)
        bits["table"] = float(np.log2(A.max())) - (qe - 3)
    return bits


def pre_activations(W, X):
    """float64 X W^T: the exact pre-activations of a layer on these inputs"""
    return np.asarray(X, np.float64) @ np.asarray(W, np.float64).T
