"""The interest-region contract of DESIGN.md 3.5 "Native interest regions" restated in numpy, from the contract and not from the library: not a test.

  restated_*    float32, every operation its own rounded array (or scalar) operation in the order the contract writes it: what csrc/ngp_features.h must
                reproduce bit for bit
  scipy_*       the same detector in float64 on scipy.ndimage (gaussian_filter(mode="mirror", radius=...), maximum_filter / minimum_filter,
                binary_dilation): what the float32 restatement is held to within a derived bound
  make_*        the images the tests use
"""
import math

import numpy as np

f32 = np.float32
CONTRAST, EDGE, SIGMA, LAYERS, BORDER = 0.04, 10.0, 1.6, 3, 5
MAX_RADIUS, ATTEMPTS, ROUNDS = 12, 5, 4


# ------------------------------------------------------------------------------------------------------------------------
# shapes and weights (host arithmetic in double, as the contract says)
# ------------------------------------------------------------------------------------------------------------------------
def octave_shapes(H, W):
    n_oct = int(math.floor(math.log2(2 * min(H, W)) + 0.5)) - 2
    shapes, h, w = [], 2 * H, 2 * W
    for _ in range(n_oct):
        shapes.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return shapes


def blur_sigmas(sigma=SIGMA, layers=LAYERS):
    """[0] the base image's blur, [i] the blur from level i - 1 to level i; sigma enters as the float32 the configuration holds"""
    sigma = float(f32(sigma))
    k = math.pow(2.0, 1.0 / layers)
    out = [math.sqrt(sigma * sigma - 1.0)]
    for i in range(1, layers + 3):
        prev = sigma * math.pow(k, float(i - 1))
        total = prev * k
        out.append(math.sqrt(total * total - prev * prev))
    return out


def blur_radius(sigma):
    return min(int(4.0 * sigma + 0.5), MAX_RADIUS)


def blur_weights(sigma):
    """float64 weights w[0..r] over their sum w0 + 2 (w1 + ...), before any rounding"""
    r = blur_radius(sigma)
    e = [1.0] + [math.exp(-float(i * i) / (2.0 * sigma * sigma)) for i in range(1, r + 1)]
    total = 1.0
    for i in range(1, r + 1):
        total += 2.0 * e[i]
    return [v / total for v in e]


def fold(i, n):
    """reflect-101 with period 2(n - 1)"""
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


# ------------------------------------------------------------------------------------------------------------------------
# the pyramid, in the working type T (float32: the contract; float64 only for the generic helpers below)
# ------------------------------------------------------------------------------------------------------------------------
def gray_of(image, T=f32):
    im = image.astype(T)
    return (T(0.299) * im[..., 0] + T(0.587) * im[..., 1]) + T(0.114) * im[..., 2]


def upsample(g):
    T = g.dtype.type
    H, W = g.shape
    gp = np.pad(g, ((0, 1), (0, 1)), mode="reflect")                      # index n -> n - 2
    a, b, c, d = gp[:-1, :-1], gp[:-1, 1:], gp[1:, :-1], gp[1:, 1:]
    u = np.empty((2 * H, 2 * W), g.dtype)
    u[0::2, 0::2] = a
    u[0::2, 1::2] = (a + b) * T(0.5)
    u[1::2, 0::2] = (a + c) * T(0.5)
    u[1::2, 1::2] = ((a + b) + (c + d)) * T(0.25)
    return u


def blur_pass(a, w, axis):
    T = a.dtype.type
    r, n = len(w) - 1, a.shape[axis]
    padded = np.take(a, fold(np.arange(-r, n + r), n), axis=axis)
    at = lambda off: np.take(padded, np.arange(r + off, r + off + n), axis=axis)      # noqa: E731
    acc = T(w[0]) * at(0)
    for i in range(1, r + 1):
        acc = acc + T(w[i]) * (at(-i) + at(i))
    return acc


def blur(a, sigma):
    w = [a.dtype.type(v) for v in blur_weights(sigma)]                     # rounded once to the working type
    return blur_pass(blur_pass(a, w, 1), w, 0)


def restated_pyramid(image, sigma=SIGMA, layers=LAYERS, T=f32):
    """[octave][level] arrays of the working type"""
    H, W, _ = image.shape
    sig = blur_sigmas(sigma, layers)
    base = blur(upsample(gray_of(image, T)), sig[0])
    pyramid = []
    for _ in octave_shapes(H, W):
        levels = [base]
        for i in range(1, layers + 3):
            levels.append(blur(levels[-1], sig[i]))
        pyramid.append(levels)
        base = levels[layers][0::2, 0::2]
    return pyramid


# ------------------------------------------------------------------------------------------------------------------------
# candidates and refinement
# ------------------------------------------------------------------------------------------------------------------------
def candidates(dog, threshold, layers=LAYERS, border=BORDER):
    """(s, y, x) of every candidate of one octave; dog [layers + 2] arrays"""
    h, w = dog[0].shape
    out = []
    if h <= 2 * border or w <= 2 * border:
        return out
    inner = (slice(border, h - border), slice(border, w - border))
    for s in range(1, layers + 1):
        c = dog[s][inner]
        above = np.ones(c.shape, bool)
        below = np.ones(c.shape, bool)
        for ds in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    nb = dog[s + ds][border + dy:h - border + dy, border + dx:w - border + dx]
                    above &= ~(nb > c)
                    below &= ~(nb < c)
        found = (np.abs(c) > threshold) & (((c > 0) & above) | ((c < 0) & below))
        for y, x in np.argwhere(found):
            out.append((s, int(y) + border, int(x) + border))
    return out


def refine(dog, s, y, x, contrast=CONTRAST, edge=EDGE, layers=LAYERS, border=BORDER):
    """the contract's step 5 in the type of `dog`; (column position, row position) in the octave, or None"""
    T = dog[0].dtype.type
    h, w = dog[0].shape
    half, quarter, two = T(0.5), T(0.25), T(2.0)
    D = lambda ds, dy, dx: dog[s + ds][y + dy, x + dx]                     # noqa: E731
    for _ in range(ATTEMPTS):
        v = D(0, 0, 0)
        v2 = v * two
        xm, xp, ym, yp, sm, sp = D(0, 0, -1), D(0, 0, 1), D(0, -1, 0), D(0, 1, 0), D(-1, 0, 0), D(1, 0, 0)
        gx, gy, gs = (xp - xm) * half, (yp - ym) * half, (sp - sm) * half
        a, d, f = (xp + xm) - v2, (yp + ym) - v2, (sp + sm) - v2
        b = (((D(0, 1, 1) - D(0, 1, -1)) - D(0, -1, 1)) + D(0, -1, -1)) * quarter
        c = (((D(1, 0, 1) - D(1, 0, -1)) - D(-1, 0, 1)) + D(-1, 0, -1)) * quarter
        e = (((D(1, 1, 0) - D(1, -1, 0)) - D(-1, 1, 0)) + D(-1, -1, 0)) * quarter
        A00, A01, A02 = d * f - e * e, c * e - b * f, b * e - c * d
        A11, A12, A22 = a * f - c * c, b * c - a * e, a * d - b * b
        det = (a * A00 + b * A01) + c * A02
        if det == 0:
            return None
        with np.errstate(over="ignore", invalid="ignore"):
            xc = -(((A00 * gx + A01 * gy) + A02 * gs) / det)
            xr = -(((A01 * gx + A11 * gy) + A12 * gs) / det)
            xs = -(((A02 * gx + A12 * gy) + A22 * gs) / det)
        if abs(xc) < half and abs(xr) < half and abs(xs) < half:
            contr = v + half * ((gx * xc + gy * xr) + gs * xs)
            if not abs(contr) * T(layers) >= T(contrast):
                return None
            tr, det2 = a + d, a * d - b * b
            if not det2 > 0:
                return None
            if not (tr * tr) * T(edge) < ((T(edge) + T(1)) * (T(edge) + T(1))) * det2:
                return None
            return T(x) + xc, T(y) + xr
        if not (abs(xc) <= T(1e6) and abs(xr) <= T(1e6) and abs(xs) <= T(1e6)):
            return None
        x, y, s = x + int(np.rint(xc)), y + int(np.rint(xr)), s + int(np.rint(xs))
        if s < 1 or s > layers or x < border or x >= w - border or y < border or y >= h - border:
            return None
    return None


def keypoints_of(pyramid, contrast=CONTRAST, edge=EDGE, layers=LAYERS, border=BORDER, refined=True):
    """[(octave, row in the image, column in the image)] as floats of the pyramid's type"""
    T = pyramid[0][0].dtype.type
    threshold = (T(0.5) * T(contrast)) / T(layers)
    out = []
    for o, levels in enumerate(pyramid):
        dog = [levels[s + 1] - levels[s] for s in range(layers + 2)]
        scale = T(0.5 * 2 ** o)
        for s, y, x in candidates(dog, threshold, layers, border):
            pos = refine(dog, s, y, x, contrast, edge, layers, border) if refined else (T(x), T(y))
            if pos is not None:
                out.append((o, pos[1] * scale, pos[0] * scale))
    return out


def mask_of(keypoints, H, W):
    mask = np.zeros((H, W), np.uint8)
    for _, y, x in keypoints:
        iy, ix = int(y), int(x)
        if 0 <= iy < H and 0 <= ix < W:
            mask[iy, ix] = 1
    return mask


def restated_mask(image, **cfg):
    H, W, _ = image.shape
    pyr = restated_pyramid(image, cfg.get("sigma", SIGMA), cfg.get("layers", LAYERS))
    return mask_of(keypoints_of(pyr, cfg.get("contrast", CONTRAST), cfg.get("edge", EDGE), cfg.get("layers", LAYERS), cfg.get("border", BORDER)), H, W)


# ------------------------------------------------------------------------------------------------------------------------
# the float64 route on scipy.ndimage
# ------------------------------------------------------------------------------------------------------------------------
def scipy_pyramid(image, sigma=SIGMA, layers=LAYERS):
    from scipy import ndimage
    H, W, _ = image.shape
    sig = blur_sigmas(sigma, layers)
    g = lambda a, s: ndimage.gaussian_filter(a, s, mode="mirror", radius=blur_radius(s))      # noqa: E731
    base = g(upsample(gray_of(image, np.float64)), sig[0])
    pyramid = []
    for _ in octave_shapes(H, W):
        levels = [base]
        for i in range(1, layers + 3):
            levels.append(g(levels[-1], sig[i]))
        pyramid.append(levels)
        base = levels[layers][0::2, 0::2]
    return pyramid


def scipy_keypoints(pyramid, contrast=CONTRAST, edge=EDGE, layers=LAYERS, border=BORDER, conditions=True):
    """Candidates without refinement: no sub-pixel solve and no moves.  conditions=False: the raw extrema of step 4 alone.  conditions=True: the contrast
    and curvature conditions of step 5 taken at the candidate pixel itself (offset 0); without them the ring-shaped side lobe of a blob's response
    yields extrema of its own, which the curvature condition removes.  [(octave, row, column)] in image coordinates."""
    from scipy import ndimage
    threshold = 0.5 * contrast / layers
    out = []
    for o, levels in enumerate(pyramid):
        dog = np.stack([levels[s + 1] - levels[s] for s in range(layers + 2)])
        top = ndimage.maximum_filter(dog, size=3, mode="nearest")
        bottom = ndimage.minimum_filter(dog, size=3, mode="nearest")
        found = (np.abs(dog) > threshold) & (((dog > 0) & (dog == top)) | ((dog < 0) & (dog == bottom)))
        found[0] = found[-1] = False
        _, h, w = dog.shape
        inside = np.zeros((h, w), bool)
        if h > 2 * border and w > 2 * border:
            inside[border:h - border, border:w - border] = True
        for s, y, x in np.argwhere(found & inside[None]):
            d = dog[s]
            v = d[y, x]
            a, c = d[y, x + 1] + d[y, x - 1] - 2 * v, d[y + 1, x] + d[y - 1, x] - 2 * v
            b = (d[y + 1, x + 1] - d[y + 1, x - 1] - d[y - 1, x + 1] + d[y - 1, x - 1]) * 0.25
            tr, det = a + c, a * c - b * b
            if not conditions or (abs(v) * layers >= contrast and det > 0 and tr * tr * edge < (edge + 1) ** 2 * det):
                out.append((o, y * 0.5 * 2 ** o, x * 0.5 * 2 ** o))
    return out


def level_bound(blurs_applied, sigma=SIGMA, layers=LAYERS):
    """How far a float32 level may lie from the float64 one: every value is a convex combination of values in [0, 1], so a pass of t taps adds at most
    (t + 1) 2^-24, accumulated over the passes that precede the level (a blur is two passes; later passes carry an earlier error on unamplified, their
    weights summing to 1).  blurs_applied: the blurs from the base blur on, as indices into blur_sigmas()."""
    eps = 2.0 ** -24
    total = 0.0
    for i in blurs_applied:
        taps = 2 * blur_radius(blur_sigmas(sigma, layers)[i]) + 1
        total += 2 * (taps + 1) * eps                                       # the row pass and the column pass
    return total


def restated_dilation(mask, kernel_size, dil_iter):
    from scipy import ndimage
    return ndimage.binary_dilation(mask.astype(bool), np.ones((kernel_size, kernel_size), bool), iterations=dil_iter).astype(np.uint8)


def restated_regions(mask):
    """coords[mask] of nav/estimator_helpers.py:204 for a square image: ascending column, then row, as (row, col)"""
    return np.argwhere(mask.T)[:, ::-1].astype(np.int32)


def _mix(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def restated_permutation(M, n, n_iter, seed):
    """p[k, j] for j < n: the keyed bijection of [0, M) in uint32 arrays (their arithmetic wraps)"""
    bits = 0
    while (1 << bits) < M:
        bits += 1
    half = np.uint32(max((bits + 1) // 2, 1))
    low = np.uint32((1 << int(half)) - 1)
    with np.errstate(over="ignore"):
        k = np.arange(n_iter, dtype=np.uint32)
        key = _mix(np.uint32(seed) ^ _mix(k + np.uint32(0x9E3779B9)))[:, None]
        v = np.broadcast_to(np.arange(n, dtype=np.uint32)[None, :], (n_iter, n)).copy()
        todo = np.ones(v.shape, bool)
        while todo.any():
            L, R = v >> half, v & low
            for r in range(ROUNDS):
                t = L ^ (_mix((R + key) + np.uint32(r) * np.uint32(0x9E3779B9)) & low)
                L, R = R, t
            v = np.where(todo, (L << half) | R, v)
            todo = v >= np.uint32(M)
    return v


def restated_draw(regions, B, n_iter, seed):
    return regions[restated_permutation(regions.shape[0], B, n_iter, seed).astype(np.int64)]


# ------------------------------------------------------------------------------------------------------------------------
# images [H,W,3] float32 in [0,1]
# ------------------------------------------------------------------------------------------------------------------------
BLOBS_96 = dict(shape=(96, 96), centres=[(20, 24), (30, 70), (66, 40), (75, 80)], sigmas=[2.0, 3.0, 4.5, 2.5], depths=[0.8, 0.7, 0.9, 0.6])
# The second blob of the small image was asked for with sigma 3.  That scale lies between the samples 1.6 k^2 = 2.54 and 1.6 k^3 = 3.2 of octave 1, and with
# the image's lower edge 12 rows away the refined row comes out as 23.99998 (in float64 as well: it is the mirrored edge, not rounding), which int()
# truncates to row 23.  Its sigma is therefore moved onto the sampled scale 1.6 k^2, where the refined position is the centre exactly.
BLOBS_37x53 = dict(shape=(37, 53), centres=[(12, 15), (24, 38)], sigmas=[2.0, 1.6 * 2.0 ** (2.0 / 3.0)], depths=[0.8, 0.7])


def make_blobs(shape, centres, sigmas, depths):
    """dark Gaussian blobs on a white ground, gray (the three channels equal)"""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    g = np.ones((H, W))
    for (cy, cx), s, d in zip(centres, sigmas, depths):
        g -= d * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * s * s))
    return np.repeat(np.clip(g, 0.0, 1.0)[..., None], 3, axis=2).astype(np.float32)


def make_noise(H, W, seed, smooth=1.5):
    """coloured noise from a seeded generator, smoothed and stretched to [0, 1]"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    im = ndimage.gaussian_filter(rng.random((H, W, 3)), (smooth, smooth, 0.0), mode="mirror")
    im = (im - im.min()) / (im.max() - im.min())
    return im.astype(np.float32)


def make_constant(H, W, value=0.5):
    return np.full((H, W, 3), value, np.float32)
