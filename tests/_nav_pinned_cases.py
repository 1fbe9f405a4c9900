"""What tests/test_nav_pinned_host.py (CPU) and tests/test_gpu_nav_pinned.py (GPU) share: the fields, rays, points and loss weights the fused nav
queries (csrc/nav_field.hip) are held to, the pinned float64 reference of each case, and the comparison rule.

Reference: oracle.callers_oracle with pin_float32 -- float64 arithmetic on the float32 run's own samples, cells and fractions ("Pinned
reference").  Yardstick: the float32 oracle's own distance from that reference, per ray or per point; a kernel may be MARGIN times as far.
Everything here is computed once per process and shared: do not write to what these functions return."""
import functools
import math

import numpy as np
import torch

MARGIN = 16.0                  # the other summation order (FMA chains, block scans against cumprod, up to 4,096 terms) and the device's expf against libm
MASK_THRESHOLD = 1e-4          # nerf/renderer.py:217
# Contrast field: row 0 of sigma_net[1].weight (the log-density row) times GAIN.  Chosen on the CPU so that, over the base rays at 100 steps, the
# colour mask keeps a minority of the samples and the rays spread from translucent to opaque (tests/test_nav_pinned_host.py asserts both conditions).
# A gain alone cannot meet both: up to 20 every sample is kept, from 30 on every ray is opaque (the fog has no large-scale structure, so all rays see
# the same statistics).  The negative constant added to the row thins the medium between the peaks the gain raises: at (120, -3.0) 47 % of the
# samples are kept, 23 % of the rays end below weights_sum 0.99 and 53 % above 0.999.
CONTRAST_GAIN = 120.0
CONTRAST_SHIFT = -3.0          # added to every entry of that row after the gain
ROT30 = None                   # filled below: rotation by 30 degrees about (1, 2, 3) / sqrt(14); not symmetric


def _rot30():
    k = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = math.radians(30.0)
    return (np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)).astype(np.float32)


ROT30 = _rot30()


# ------------------------------------------------------------------------------------------------------------------------
# fields
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field_arrays(kind, bound):
    """(embeddings, offsets, per_level_scale, sigma layers, colour layers), float32 numpy, of field "fog" (torch.manual_seed(11), embeddings in
    +-0.5, default-initialised Linear layers: sigma about 1 everywhere) or "contrast" (fog with the log-density row amplified)"""
    from ngp.field import NGPField
    torch.manual_seed(11)
    field = NGPField(bound=bound)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
    sw = [l.weight.detach().numpy().copy() for l in field.sigma_net]
    cw = [l.weight.detach().numpy().copy() for l in field.color_net]
    if kind == "contrast":
        sw[1][0] = (sw[1][0] * np.float32(CONTRAST_GAIN) + np.float32(CONTRAST_SHIFT)).astype(np.float32)
    elif kind != "fog":
        raise KeyError(kind)
    return field.encoder.embeddings.detach().numpy().copy(), field.encoder.offsets.numpy().copy(), float(field.encoder.per_level_scale), sw, cw


def oracle_field(kind, bound, dtype=torch.float32, pin_float32=False):
    from oracle import callers_oracle as CO
    emb, offsets, pls, sw, cw = field_arrays(kind, bound)
    return CO.DefaultField(emb, offsets, pls, sw, cw, bound, dtype=dtype, pin_float32=pin_float32)


def product_field(kind, bound, dev):
    """ngp.field.NGPField on `dev` holding the same numbers"""
    from ngp.field import NGPField
    emb, _, _, sw, cw = field_arrays(kind, bound)
    field = NGPField(bound=bound).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(emb))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            layer.weight.copy_(torch.from_numpy(w))
    return field


# ------------------------------------------------------------------------------------------------------------------------
# rays
# ------------------------------------------------------------------------------------------------------------------------
def base_rays():
    """the 12 x 12 orbit view plus two rays from inside the box: the 146 rays the contrast field's conditions are stated on"""
    from ngp import workload as W
    o, d = W.get_rays(W.orbit_pose(1), W.intrinsics(12, 12), 12, 12)
    o = np.concatenate([o, [[0.1, 0.2, -0.3], [0.0, 0.0, 0.0]]]).astype(np.float32)
    d = np.concatenate([d, [[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]]]).astype(np.float32)
    return o, d


def special_rays(bound):
    """[(name, origin, direction)]: the rays a batch norm hides"""
    s = 1.0 / math.sqrt(3.0)
    return [("inside_a", (0.1, 0.2, -0.3), (0.0, 0.0, 1.0)), ("inside_b", (0.0, 0.0, 0.0), (0.6, 0.0, 0.8)),
            ("axis_x", (-3.0, 0.3, -0.4), (1.0, 0.0, 0.0)), ("axis_y", (0.25, 3.0, 0.7), (0.0, -1.0, 0.0)), ("axis_z", (-0.6, 0.45, -3.0), (0.0, 0.0, 1.0)),
            ("face", (-3.0, bound, 0.1), (1.0, 0.0, 0.0)),                                  # every sample ties the clip of y
            ("diagonal", (-1.5 * bound,) * 3, (s, s, s)),                                   # corner to corner
            ("miss", (5.0, 5.0, 5.0), (1.0, 0.0, 0.0))]


LONG_ORBIT = (9, 69)            # rows of the 12 x 12 orbit view


@functools.lru_cache(maxsize=None)
def rays(bound, count=None, translucent=False, long=False):
    """(rays_o, rays_d [N,3] float32, index of the miss).  count None: the 144 orbit rays and the eight special rays, the miss in the MIDDLE of the
    batch.  count n >= 8: the eight special rays and n - 8 orbit rays spread over the view, the miss again in the middle.
    translucent: n - 1 rays spread over those of the full batch that the contrast field leaves translucent (float32 oracle, 100 steps: weights_sum
    < 0.9995), and the miss.  For the losses that are flat on an opaque ray: d weights_sum / d ray is rounding noise where weights_sum is 1.
    long: the eight rays of the 513- and 4,096-step cases -- the miss, five special rays and the orbit rays LONG_ORBIT.  inside_b and axis_z are in
    every other batch but not in this one: at 4,096 steps the float32 oracle's OWN image is 1.9e-6 and 1.2e-6 from the pinned reference on them (run()
    sums weights * rgb over a strided axis, a running float32 sum whose rounding walks with the number of terms), above the 1e-6 every case has to
    meet to serve as a yardstick.  The two orbit rays in their place stay translucent through all sixteen chunks (weights_sum 0.9996 and 0.998; the
    float32 oracle's image 1e-7 and 3e-7 from the reference), as do axis_x, axis_y and the diagonal (sample weight above 1e-4 in 15 or 16 chunks)."""
    from ngp import workload as W
    if translucent:
        from oracle import callers_oracle as CO
        o, d, at = rays(bound, None)
        with torch.no_grad():
            ws = CO.run(oracle_field("contrast", bound), torch.from_numpy(o), torch.from_numpy(d), bound, num_steps=100)["weights_sum"].numpy()
        cand = np.flatnonzero((ws < 0.9995) & (np.arange(o.shape[0]) != at))
        pick = cand[np.linspace(0, len(cand) - 1, count - 1).round().astype(int)]
        assert len(set(pick.tolist())) == count - 1
        pick = np.insert(pick, (count - 1) // 2, at)
        return np.ascontiguousarray(o[pick]), np.ascontiguousarray(d[pick]), (count - 1) // 2
    o, d = W.get_rays(W.orbit_pose(1), W.intrinsics(12, 12), 12, 12)
    if long:
        assert count == 8
        o, d = o[list(LONG_ORBIT)], d[list(LONG_ORBIT)]
    elif count is not None:
        pick = np.linspace(0, o.shape[0] - 1, count - 8).round().astype(int) if count > 8 else np.zeros(0, int)
        o, d = o[pick], d[pick]
    sp = special_rays(bound)
    hits = [r for r in sp if r[0] != "miss" and not (long and r[0] in ("inside_b", "axis_z"))]
    miss = [r for r in sp if r[0] == "miss"][0]
    o = np.concatenate([o, np.array([r[1] for r in hits], np.float32).reshape(-1, 3)]).astype(np.float32)
    d = np.concatenate([d, np.array([r[2] for r in hits], np.float32).reshape(-1, 3)]).astype(np.float32)
    at = o.shape[0] // 2
    o = np.insert(o, at, np.array(miss[1], np.float32), axis=0)
    d = np.insert(d, at, np.array(miss[2], np.float32), axis=0)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), at


def loss_weights(n, seed=2):
    """(grad_image [n,3], grad_depth [n], grad_weights_sum [n]) float32 in +-1"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, size=(n, 3)).astype(np.float32), rng.uniform(-1, 1, size=n).astype(np.float32),
            rng.uniform(-1, 1, size=n).astype(np.float32))


def _run_case(field="contrast", T=100, count=None, bound=2.0, bg=1.0, density_scale=1.0, min_near=0.2, terms=("image", "depth", "weights_sum"),
              translucent=False, long=False):
    return dict(field=field, T=T, count=count, bound=bound, bg=bg, density_scale=density_scale, min_near=min_near, terms=tuple(terms),
                translucent=translucent, long=long)


def case_rays(case):
    return rays(case["bound"], case["count"], case["translucent"], case["long"])


BG = (0.1, 0.5, 0.9)
RUN_CASES = {
    "base": _run_case(field="fog", T=100),
    "contrast": _run_case(T=257),
    "chunk_255": _run_case(T=255, count=16),
    "chunk_256": _run_case(T=256, count=16),
    "tiny_1": _run_case(T=1, count=16),
    "tiny_2": _run_case(T=2, count=16),
    "tiny_3": _run_case(T=3, count=16),
    "long_513": _run_case(T=513, count=8, long=True),
    "long_4096": _run_case(T=4096, count=8, long=True),
    "background": _run_case(count=32, bg=BG),
    "scale_2": _run_case(count=32, density_scale=2.0),
    "bound_1": _run_case(count=32, bound=1.0, min_near=0.05),
    "weights_sum_alone": _run_case(count=32, terms=("weights_sum",), translucent=True),
    "depth_alone": _run_case(count=32, terms=("depth",), translucent=True),
}
STEP_COUNTS = sorted({c["T"] for c in RUN_CASES.values()})


def lin_rule(T):
    """torch.linspace(0, 1, T) in float32 as csrc/nav_field.hip's nv_lin states it: step * i below T / 2, ONE rounding of 1 - step * (T - 1 - i) above
    (the product is exact in float64: two 24-bit factors), 0 for T < 2"""
    if T < 2:
        return np.zeros(T, np.float32)
    step = np.float32(1.0) / np.float32(T - 1)
    i = np.arange(T)
    low = (step * i.astype(np.float32)).astype(np.float32)
    high = (1.0 - np.float64(step) * (T - 1 - i).astype(np.float64)).astype(np.float32)
    return np.where(i < T // 2, low, high)


def oracle_run(case, dtype, pin):
    """callers_oracle.run of a case and the gradients of its loss w.r.t. the rays -> dict of numpy arrays in `dtype`"""
    from oracle import callers_oracle as CO
    o, d, _ = case_rays(case)
    G, Gd, Gw = loss_weights(o.shape[0])
    field = oracle_field(case["field"], case["bound"], dtype, pin_float32=pin)
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
    return res


# ------------------------------------------------------------------------------------------------------------------------
# the comparison rule
# ------------------------------------------------------------------------------------------------------------------------
RELATIVE = ("grad_o", "grad_d", "grad_x", "sigma")         # judged relative to the reference's own size per ray / point; the others absolutely


def row_error(got, ref, name):
    """per ray / per point: |got - ref| (Euclidean over the row), divided by |ref| for the arrays in RELATIVE.  float64 numpy [N]; NaN where the reference
    is NaN (the miss ray's depth) or, for a relative array, zero"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    err = np.linalg.norm(got - ref, axis=1)
    if name in RELATIVE:
        size = np.linalg.norm(ref, axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.where(size > 0, err / size, np.nan)
    return err


def carry_floor(T):
    """A floor under the yardstick of image, depth and weights_sum for runs of more than one 256-sample chunk, from the arithmetic (found on the GPU:
    at 4,096 steps the weights_sum of the ray axis_z sat 7.8e-7 from the reference while the float32 oracle, by luck of its roundings, sat 1e-9 from
    it and the p90 of the batch's eight rays was 4e-8, less than one ulp of the value; axis_x in the present batch: 4.2e-7 against 2e-9).  The oracle's transmittance is a sequential cumprod: T[i+1] = fl(T[i] keep[i]), so
    sum(alpha T) telescopes to 1 - T[last] and the roundings of T all but cancel in the three sums.  k_nav_run_fwd multiplies a scan's partial
    products instead: per chunk, `carry *= total` is one rounding on top of the ten behind `total` (six shuffle steps, four wave totals), and that
    error is COMMON to every later sample, so it does not average out in a sum whose weights add up to one.  Behind chunk c stand 11 (c - 1)
    roundings of at most 2^-24 each, independent in sign: 2^-24 sqrt(11 (chunks - 1)) -- 1.9e-7 at two chunks, 7.7e-7 at sixteen.  Zero for one chunk."""
    chunks = (T + 255) // 256
    return 2.0 ** -24 * math.sqrt(11.0 * (chunks - 1))


def yardstick(e32, judged, p90=None, floor=0.0):
    """max(e32[i], p90 of e32 over the judged rows, floor): what MARGIN multiplies.  `p90`: taken over a larger set of the same case (the whole point
    set when a few of its points are judged); `floor`: see carry_floor"""
    if p90 is None:
        p90 = float(np.percentile(e32[judged], 90)) if judged.any() else 0.0
    return np.maximum(np.where(np.isfinite(e32), e32, 0.0), max(p90, floor))


def left_out(ref, miss=None):
    """rows left out of the RELATIVE check of a run case (bool [N]; the miss apart, the host test caps their share at 2 %): a reference gradient norm
    below 1e-6 of the case's median, or a sample whose reference weight lies within 1e-6 relative of the colour mask's threshold"""
    n = ref["grad_o"].shape[0]
    out = np.zeros(n, bool)
    hit = np.ones(n, bool)
    if miss is not None:
        hit[miss] = False
    for k in ("grad_o", "grad_d"):
        size = np.linalg.norm(ref[k].astype(np.float64), axis=1)
        out |= hit & ~(size >= 1e-6 * np.median(size[hit]))
    with np.errstate(invalid="ignore"):
        out |= hit & (np.abs(ref["weights"] - MASK_THRESHOLD) <= 1e-6 * MASK_THRESHOLD).any(axis=1)
    return out


@functools.lru_cache(maxsize=None)
def run_reference(name):
    """dict(ref = the pinned float64 run, f32 = the float32 oracle, miss, judged = rows in the relative check, e32 = {array: per-ray error of f32})"""
    case = RUN_CASES[name]
    _, _, miss = case_rays(case)
    ref, f32 = oracle_run(case, torch.float64, True), oracle_run(case, torch.float32, False)
    hit = np.ones(ref["grad_o"].shape[0], bool)
    hit[miss] = False
    judged = hit & ~left_out(ref, miss)
    e32 = {k: row_error(f32[k], ref[k], k) for k in ("image", "depth", "weights_sum", "grad_o", "grad_d")}
    return dict(case=case, ref=ref, f32=f32, miss=miss, hit=hit, judged=judged, e32=e32)


def judge(label, got, ref, e32, rows, name, p90=None, floor=0.0):
    """The rule: for every row i in `rows`, error(got)[i] <= MARGIN * max(e32[i], p90(e32 over rows), floor).  Prints the largest ratio of error to yardstick
    and returns it; raises AssertionError naming the worst row."""
    ek = row_error(got, ref, name)
    rows = rows & np.isfinite(row_error(ref, ref, name))
    y = yardstick(e32, rows, p90, floor)
    assert np.isfinite(ek[rows]).all(), f"{label} {name}: not finite in rows {np.flatnonzero(rows & ~np.isfinite(ek))[:8].tolist()}"
    if not rows.any():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(ek > 0, ek / y, 0.0)
    ratio = np.where(rows, ratio, 0.0)
    worst = int(np.argmax(ratio))
    print(f"{label} {name}: max error / yardstick {ratio[worst]:.3g} (row {worst}: error {ek[worst]:.3g}, float32 oracle {e32[worst]:.3g}, yardstick {y[worst]:.3g})")
    assert ratio[worst] <= MARGIN, f"{label} {name}: row {worst} is {ratio[worst]:.3g} yardsticks from the pinned reference (margin {MARGIN:g})"
    return float(ratio[worst])


# ------------------------------------------------------------------------------------------------------------------------
# points
# ------------------------------------------------------------------------------------------------------------------------
def level_scale(level, bound):
    from oracle import ngp_oracle as O
    _, _, pls, _, _ = field_arrays("fog", bound)
    scales, _ = O.grid_level_table(16, np.float32(np.log2(pls)), 16)
    return np.float32(scales[level])


def grid_pos32(x, level, bound):
    """pos = x01 * scale + 0.5 of the encoder at one level, in float32 as gridencoder.cu and csrc/ngp_nav_field.h compute it"""
    f = np.float32
    x01 = ((np.asarray(x, f) + f(bound)) * (f(1.0) / f(2 * bound))).astype(f)
    return (x01 * level_scale(level, bound) + f(0.5)).astype(f)


def _lattice_node(level, node, bound):
    """a float32 coordinate whose pos at `level` is exactly the integer `node` (frac == 0)"""
    f = np.float32
    x = f((node - 0.5) / float(level_scale(level, bound)) * 2 * bound - bound)
    for cand in [x] + [_ulps(x, s * k) for k in range(1, 9) for s in (1, -1)]:
        if grid_pos32(cand, level, bound) == f(node):
            return f(cand)
    raise AssertionError(f"no float32 coordinate within 8 ulps lands on node {node} of level {level}")


def _ulps(x, k):
    f = np.float32
    for _ in range(abs(k)):
        x = np.nextafter(x, f(np.inf if k > 0 else -np.inf), dtype=f)
    return x


N_POINTS = 1000
OUTSIDE_NAMES = ("below_x", "below_y", "below_z", "far_a", "far_b", "far_c")


@functools.lru_cache(maxsize=None)
def points(bound):
    """(x [1000,3] float32, names {name: row}): the special points first, then uniform in +-bound.  Applied UNROTATED they are: the 6 face centres and 8
    corners (x01 exactly 0 or 1), nextafter(bound, inf) and nextafter(-bound, -inf) on each axis, the centre, lattice nodes of levels 0-3 (frac == 0),
    points at +-2.5 (outside every bound used)."""
    f = np.float32
    b = f(bound)
    names, rows = {}, []

    def add(name, p):
        names[name] = len(rows)
        rows.append(np.array(p, f))
    for a in range(3):
        for s in (-1, 1):
            p = [0.0, 0.0, 0.0]; p[a] = s * b
            add(f"face_{'xyz'[a]}{'-+'[s > 0]}", p)
    for c in range(8):
        add(f"corner_{c}", [b if c & 1 else -b, b if c & 2 else -b, b if c & 4 else -b])
    up, down = np.nextafter(b, f(np.inf), dtype=f), np.nextafter(-b, f(-np.inf), dtype=f)
    for a in range(3):
        p = [f(0.25) * b, f(-0.4) * b, f(0.1) * b]; p[a] = up
        add(f"above_{'xyz'[a]}", p)                # x + bound ties to even and rounds back onto the face: x01 == 1, INSIDE for encoder and kernel
        q = [f(0.25) * b, f(-0.4) * b, f(0.1) * b]; q[a] = down
        add(f"below_{'xyz'[a]}", q)                # x + bound = -ulp exactly: x01 < 0, outside
    add("centre", [0.0, 0.0, 0.0])
    for level in range(4):
        # nodes from 8 up: there one ulp of the coordinate moves pos by less than pos's own ulp, so some neighbouring float32 lands on the integer
        node = [8, 9, 11] if level == 0 else [16 + level, 17 + 2 * level, 19 + 3 * level]
        add(f"node_{level}", [_lattice_node(level, n, bound) for n in node])
    add("far_a", [2.5, 0.0, 0.0])
    add("far_b", [0.0, -2.5, 0.3])
    add("far_c", [-2.5, 2.5, 2.5])
    rng = np.random.default_rng(7)
    fill = rng.uniform(-bound, bound, size=(N_POINTS - len(rows), 3)).astype(f)
    return np.ascontiguousarray(np.concatenate([np.stack(rows), fill]).astype(f)), names


POINT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
ROTATIONS = {"none": None, "nav": ((0., 0., 1.), (1., 0., 0.), (0., 1., 0.)), "rot30": ROT30}


def point_weights(seed=3):
    """(w [1000] in 0.5..1.5 for sum(w sigma), Gg [1000,15] in +-1 for sum(Gg geo)) float32"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, size=N_POINTS).astype(np.float32), rng.uniform(-1, 1, size=(N_POINTS, 15)).astype(np.float32)


def oracle_points(kind, bound, rot, dtype, pin, with_geo, x=None):
    from oracle import callers_oracle as CO
    if x is None:
        x, _ = points(bound)
    w, Gg = point_weights()
    field = oracle_field(kind, bound, dtype, pin_float32=pin)
    tx = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = CO.point_query(field, tx, rot=rot, pin_float32=pin)
    loss = (out["sigma"] * torch.from_numpy(w).to(dtype)).sum()
    if with_geo:
        loss = loss + (out["geo_feat"] * torch.from_numpy(Gg).to(dtype)).sum()
    (gx,) = torch.autograd.grad(loss, [tx])
    return dict(sigma=out["sigma"].detach().numpy(), geo=out["geo_feat"].detach().numpy(), grad_x=gx.numpy())


@functools.lru_cache(maxsize=None)
def point_reference(kind, bound, rot_name, with_geo=False, prerotated=False):
    """dict(ref, f32, e32, x).  prerotated: the points are rotate_points_float32(points, rot) and the query itself applies no rotation (what the one-lane
    kernels are given)"""
    from oracle import callers_oracle as CO
    x, _ = points(bound)
    rot = ROTATIONS[rot_name]
    if prerotated and rot is not None:
        x, rot = CO.rotate_points_float32(x, rot), None
    ref = oracle_points(kind, bound, rot, torch.float64, True, with_geo, x)
    # the float32 oracle is given the same rotated float32 point (a matrix product in another order lands in other cells); nothing else is pinned in float32
    f32 = oracle_points(kind, bound, rot, torch.float32, True, with_geo, x)
    return dict(ref=ref, f32=f32, x=x, e32={k: row_error(f32[k], ref[k], k) for k in ("sigma", "geo", "grad_x")})
