"""What tests/test_run_occ_host.py (CPU) and tests/test_gpu_run_occ.py (GPU) share: the occupancy-masked run (csrc/nav_field.hip: k_nav_run_occ_fwd / _bwd,
DESIGN.md 3.5 "Occupancy-masked pose filter") -- the numpy statement of a sample's occupancy bit, the bitfields, the masked reference and its yardstick.

The contract: NeRFRenderer.run (upsample_steps = 0, perturb = False) with ONE change -- the sigma of every lattice sample whose occupancy bit is clear is
zero.  The reference is oracle.callers_oracle.run over a field whose density() multiplies sigma by that mask (MaskedField); the pinned float64 run
(pin_float32) is the reference, the float32 run its yardstick, and _nav_pinned_cases.judge / MARGIN / left_out judge as they judge the dense kernels.
Everything here is computed once per process and shared: do not write to what these functions return."""
import functools
import math

import numpy as np
import torch

import _nav_pinned_cases as C

H_GRID = 32                                    # the test grids: 32^3 cells per cascade
F = np.float32


def cascades(bound):
    return 1 + math.ceil(math.log2(bound))     # nerf/renderer.py:73


# ------------------------------------------------------------------------------------------------------------------------
# the bit of a position (include/ngp_hip.h: ngp_nav_run_occ_forward; csrc/ngp_march.h: ngp_point::at with the step's cascade left out)
# ------------------------------------------------------------------------------------------------------------------------
def cell_bits(x, bound, cascade, H):
    """x [...,3] float32 (clipped sample positions) -> (bit index int64 [...], level, cell [...,3]); every operation rounds to float32 in the order
    written: level = clamp(frexp exponent of max |x|, 0, C - 1); mip_bound = min(2^level, bound); r = 1 / mip_bound;
    n = (int)clamp(((x * r + 1) * 0.5) * H, 0, H - 1); bit = level * H^3 + morton3(n)."""
    from ngp import workload as W
    x = np.asarray(x, F)
    _, e = np.frexp(np.abs(x).max(axis=-1))                             # frexp(0) = (0, 0)
    level = np.clip(e, 0, cascade - 1).astype(np.int64)
    mip_bound = np.minimum(np.ldexp(F(1), level).astype(F), F(bound))
    r = (F(1) / mip_bound).astype(F)
    u = ((x * r[..., None]).astype(F) + F(1)).astype(F)
    c = ((u * F(0.5)).astype(F) * F(H)).astype(F)
    n = np.clip(c, F(0), F(H - 1)).astype(np.int64)                     # truncation of a non-negative float
    mort = W.morton3(n[..., 0].astype(np.uint32), n[..., 1].astype(np.uint32), n[..., 2].astype(np.uint32)).astype(np.int64)
    return level * H ** 3 + mort, level, n


def occupied(x, bitfield, bound, cascade, H):
    """bool [...]: the occupancy bit of each position"""
    bit, _, _ = cell_bits(x, bound, cascade, H)
    return ((bitfield[bit >> 3] >> (bit & 7).astype(np.uint8)) & 1).astype(bool)


# ------------------------------------------------------------------------------------------------------------------------
# bitfields
# ------------------------------------------------------------------------------------------------------------------------
BITFIELDS = ("ones", "rand50", "sparse")


@functools.lru_cache(maxsize=None)
def bitfield(name, bound, H=H_GRID):
    """uint8 [C * H^3 / 8]: "ones"; "zeros"; "rand50" = default_rng(7) bytes; "sparse" = the AND of four such arrays, seeds 8..11 (about 6 % set)"""
    n = cascades(bound) * H ** 3 // 8
    if name == "ones":
        return np.full(n, 255, np.uint8)
    if name == "zeros":
        return np.zeros(n, np.uint8)
    if name == "rand50":
        return np.random.default_rng(7).integers(0, 256, size=n, dtype=np.uint8)
    if name == "sparse":
        out = np.full(n, 255, np.uint8)
        for seed in (8, 9, 10, 11):
            out &= np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)
        return out
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------------
# the kernel's sample positions, restated (csrc/nav_field.hip: nv_sample_at) -> the per-ray counts without the oracle
# ------------------------------------------------------------------------------------------------------------------------
def sample_positions(o, d, bound, T, min_near):
    """[N,T,3] float32: clip(o + d * (near + (far - near) * lin_rule(T))), one rounding per operation"""
    from oracle import ngp_oracle as O
    aabb = np.array([-bound] * 3 + [bound] * 3, F)
    n, f = O.near_far_from_aabb(o, d, aabb, min_near)
    span = (f - n).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        z = (n[:, None] + (span[:, None] * C.lin_rule(T)[None, :]).astype(F)).astype(F)
        x = (o[:, None, :] + (d[:, None, :] * z[..., None]).astype(F)).astype(F)
    return np.minimum(np.maximum(x, F(-bound)), F(bound))


def case_mask(case, bits):
    """bool [N,T]: which lattice samples of the case's rays are occupied, by the restatement alone"""
    o, d, _ = C.case_rays(case)
    x = sample_positions(o, d, case["bound"], case["T"], case["min_near"])
    return occupied(x, bits, case["bound"], cascades(case["bound"]), H_GRID)


# ------------------------------------------------------------------------------------------------------------------------
# the masked reference
# ------------------------------------------------------------------------------------------------------------------------
class MaskedField:
    """callers_oracle.DefaultField whose density(x) multiplies sigma by the occupancy mask of x, computed in numpy in float32 from the positions (a
    constant: nothing flows through it).  Everything else is the wrapped field's.  `mask`: the mask of the last density() call, flat."""

    def __init__(self, field, bits, cascade, H):
        self.field, self.bits, self.cascade, self.H = field, bits, cascade, H
        self.mask = None

    def density(self, x):
        out = self.field.density(x)
        self.mask = occupied(x.detach().to(torch.float32).numpy(), self.bits, self.field.bound, self.cascade, self.H)
        out = dict(out)
        out["sigma"] = out["sigma"] * torch.from_numpy(self.mask).to(out["sigma"].dtype)
        return out

    def color(self, *args, **kwargs):
        return self.field.color(*args, **kwargs)


def masked_run(case, bits, dtype, pin):
    """_nav_pinned_cases.oracle_run over the masked field -> its dict plus mask [N,T] (as that run saw it)"""
    from oracle import callers_oracle as CO
    o, d, _ = C.case_rays(case)
    G, Gd, Gw = C.loss_weights(o.shape[0])
    field = MaskedField(C.oracle_field(case["field"], case["bound"], dtype, pin_float32=pin), bits, cascades(case["bound"]), H_GRID)
    to, td = torch.from_numpy(o).to(dtype).requires_grad_(True), torch.from_numpy(d).to(dtype).requires_grad_(True)
    out = CO.run(field, to, td, case["bound"], num_steps=case["T"], upsample_steps=0, bg_color=case["bg"], min_near=case["min_near"],
                 density_scale=case["density_scale"], pin_float32=pin)
    loss = 0
    if "image" in case["terms"]:
        loss = loss + (out["image"] * torch.from_numpy(G).to(dtype)).sum()
    if "depth" in case["terms"]:
        loss = loss + (out["depth"] * torch.from_numpy(Gd).to(dtype)).sum()
    if "weights_sum" in case["terms"]:
        loss = loss + (out["weights_sum"] * torch.from_numpy(Gw).to(dtype)).sum()
    go, gd = torch.autograd.grad(loss, [to, td])
    res = {k: out[k].detach().numpy() for k in ("image", "depth", "weights_sum", "weights", "mask")}
    res["grad_o"], res["grad_d"] = go.numpy(), gd.numpy()
    res["occupied"] = field.mask.reshape(o.shape[0], case["T"])
    return res


def case_bits(name, bf):
    """the bitfield a (case, bitfield name) pair uses: `bitfield(bf, bound)`, except where the straddle cases adjust it (STRADDLE)"""
    case = C.RUN_CASES[name]
    if (name, bf) in STRADDLE:
        return straddle_bits(name)
    return bitfield(bf, case["bound"])


@functools.lru_cache(maxsize=None)
def occ_reference(name, bf):
    """dict(case, ref = the pinned float64 masked run, f32 = the float32 masked run, miss, hit, zero = {grad: rows whose reference gradient is exactly
    zero}, left = left_out's rows, judged, e32, counts [N] = occupied samples per ray)"""
    case = C.RUN_CASES[name]
    bits = case_bits(name, bf)
    _, _, miss = C.case_rays(case)
    ref, f32 = masked_run(case, bits, torch.float64, True), masked_run(case, bits, torch.float32, False)
    n = ref["grad_o"].shape[0]
    hit = np.ones(n, bool)
    hit[miss] = False
    left = C.left_out(ref, miss)
    zero = {k: np.linalg.norm(ref[k].astype(np.float64), axis=1) == 0 for k in ("grad_o", "grad_d")}
    e32 = {k: C.row_error(f32[k], ref[k], k) for k in ("image", "depth", "weights_sum", "grad_o", "grad_d")}
    return dict(case=case, bits=bits, ref=ref, f32=f32, miss=miss, hit=hit, zero=zero, left=left, judged=hit & ~left, e32=e32,
                counts=ref["occupied"].sum(axis=1).astype(np.int64))


# ------------------------------------------------------------------------------------------------------------------------
# the carry floor of the one-wave-per-ray kernel
# ------------------------------------------------------------------------------------------------------------------------
CHUNK = 64                                     # NO_W of csrc/nav_field.hip: the compacted list is walked 64 samples at a time


def carry_floor(count):
    """_nav_pinned_cases.carry_floor's argument for k_nav_run_occ_fwd.  The oracle's transmittance is a sequential cumprod whose roundings all but
    cancel in the three sums; the kernel multiplies a scan's partial products: per chunk of CHUNK = 64 listed samples, `carry *= total` is one rounding
    on top of the six behind `total` (the six shuffle steps of the wave's inclusive product; there are no wave totals to combine, the ray is one
    wave), and that error is common to every later sample.  A masked sample is not in the list and its factor is exactly 1, so what counts is the
    ray's OCCUPIED count: behind chunk c stand 7 (c - 1) roundings of at most 2^-24, independent in sign: 2^-24 sqrt(7 (chunks - 1)), chunks =
    ceil(count / 64).  Zero for a ray of at most 64 occupied samples."""
    chunks = (int(count) + CHUNK - 1) // CHUNK
    return 2.0 ** -24 * math.sqrt(7.0 * max(chunks - 1, 0))


def judge_absolute(label, got, r, key):
    """image / depth / weights_sum of every ray, by _nav_pinned_cases.judge: the p90 over all rays, the floor of each ray's own occupied count (the rays
    are judged in groups of equal chunk count)"""
    n = len(r["hit"])
    everyone = np.ones(n, bool)
    e32 = r["e32"][key]
    finite = np.isfinite(C.row_error(r["ref"][key], r["ref"][key], key))
    p90 = float(np.percentile(e32[finite], 90)) if finite.any() else 0.0
    chunks = (r["counts"] + CHUNK - 1) // CHUNK
    worst = 0.0
    for c in np.unique(chunks):
        rows = everyone & (chunks == c)
        worst = max(worst, C.judge(f"{label} [{int(c)} chunks]", got[key], r["ref"][key], e32, rows, key, p90=p90, floor=carry_floor(int(c) * CHUNK)))
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# counts that straddle the chunk width
# ------------------------------------------------------------------------------------------------------------------------
STRADDLE = {("contrast", "rand50"), ("long_513", "rand50")}         # (case, bitfield) pairs whose bitfield is adjusted: T > 64 is needed for 65 samples
STRADDLE_COUNTS = (CHUNK - 1, CHUNK, CHUNK + 1)


@functools.lru_cache(maxsize=None)
def straddle_bits(name):
    """rand50 for the case, then the cells of three rays adjusted so that their occupied counts are 63, 64 and 65: walking a ray's lattice samples in
    order, a sample's bit is set while the ray is short of its target and cleared from then on.  The three rays are taken apart from each other (no
    lattice sample of one lies in a cell a sample of another uses, checked), so one ray's edits leave the others' counts alone; the result is checked."""
    case = C.RUN_CASES[name]
    bound, cascade = case["bound"], cascades(case["bound"])
    bits = bitfield("rand50", bound).copy()
    o, d, miss = C.case_rays(case)
    x = sample_positions(o, d, bound, case["T"], case["min_near"])
    bit, _, _ = cell_bits(x, bound, cascade, H_GRID)
    assert case["T"] >= CHUNK + 1
    distinct = np.array([len(np.unique(b)) for b in bit])
    chosen, used = [], set()
    for n in np.argsort(-distinct, kind="stable"):                      # rays through many cells first
        if n == miss:
            continue
        cells = set(bit[n].tolist())
        if cells & used:
            continue
        chosen.append(int(n))
        used |= cells
        if len(chosen) == len(STRADDLE_COUNTS):
            break
    assert len(chosen) == len(STRADDLE_COUNTS), f"{name}: {len(chosen)} rays with cells of their own"
    for n, target in zip(chosen, STRADDLE_COUNTS):
        # whole cells are switched (all lattice samples of the ray inside a cell share its bit): a subset of the ray's cells whose sample counts add
        # up to the target, by the subset-sum table over the cells in the order the ray meets them
        order = list(dict.fromkeys(bit[n].tolist()))
        size = [int((bit[n] == b).sum()) for b in order]
        reach = [{0: None}]                                             # reach[k]: sum -> whether cell k - 1 is in, using the first k cells
        for k, s in enumerate(size):
            nxt = {v: False for v in reach[k]}
            for v in reach[k]:
                if v + s <= target and v + s not in nxt:
                    nxt[v + s] = True
            reach.append(nxt)
        assert target in reach[-1], f"{name}: no set of ray {n}'s cells holds exactly {target} samples"
        v = target
        for k in range(len(order), 0, -1):
            b, on = order[k - 1], reach[k][v]
            if on:
                v -= size[k - 1]
                bits[b >> 3] |= np.uint8(1 << (b & 7))
            else:
                bits[b >> 3] &= np.uint8(~(1 << (b & 7)) & 0xFF)
        assert v == 0
    got = occupied(x, bits, bound, cascade, H_GRID).sum(axis=1)
    assert [int(got[n]) for n in chosen] == list(STRADDLE_COUNTS)
    bits.setflags(write=False)
    return bits


def straddle_rays(name):
    """the rows of the three adjusted rays, by their counts"""
    case = C.RUN_CASES[name]
    counts = case_mask(case, straddle_bits(name)).sum(axis=1)
    return {c: np.flatnonzero(counts == c) for c in STRADDLE_COUNTS}
