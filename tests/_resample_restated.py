"""The resampled run's contract (include/ngp_hip.h "Resampled run") restated in numpy, shared by tests/test_resample_host.py (CPU) and
tests/test_gpu_resample.py / test_gpu_resample_guard.py (GPU).  Every operation rounds to float32 once, in the order written; the two sums of
sample_pdf are taken in 64-bit fixed point (2^-40 per unit), so the cdf does not depend on an order of summation and the kernels reproduce these bits."""
import numpy as np

import _nav_pinned_cases as C

F = np.float32
SCALE = F(2.0 ** 40)


def u_rule(n):
    """torch.linspace(0.5 / n, 1 - 0.5 / n, n) in float32 by ATen's rule: the ends formed in float64 and rounded, step = (e - s) / (n - 1) in float32,
    fma(step, j, s) below n / 2 and fma(-step, n - 1 - j, e) from there on (each product is exact in float64 and so is its sum: one rounding)"""
    s, e = F(0.5 / n), F(1.0 - 0.5 / n)
    if n < 2:
        return np.full(n, s, F)
    step = F(F(e - s) / F(n - 1))
    j = np.arange(n)
    low = (np.float64(step) * j + np.float64(s)).astype(F)
    high = (np.float64(e) - np.float64(step) * (n - 1 - j)).astype(F)
    return np.where(j < n // 2, low, high)


def fixed(weights):
    """q = (int64) rint((w + 1e-5) * 2^40); negative or NaN counts as 0, above 1024 as 1024"""
    v = (np.asarray(weights, F) + F(1e-5)).astype(F)
    with np.errstate(invalid="ignore"):
        ok = v >= 0
    v = np.where(ok, np.minimum(v, F(1024.0)), F(0.0)).astype(F)
    return np.rint((v * SCALE).astype(F)).astype(np.int64)


def cdf_of(weights):
    """weights [N, Tb - 1] -> cdf [N, Tb] float32: (float) ((double) P_k / (double) S) over the exact integer prefix sums; all 0 where S = 0"""
    q = fixed(weights)
    P = np.concatenate([np.zeros_like(q[:, :1]), np.cumsum(q, axis=1)], axis=1)
    S = P[:, -1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(S > 0, P.astype(np.float64) / S.astype(np.float64), 0.0)
    return c.astype(F)


def sample_pdf(bins, weights, n, u=None):
    """bins [N,Tb], weights [N,Tb-1] -> [N,n].  u None: the deterministic branch"""
    bins, weights = np.asarray(bins, F), np.asarray(weights, F)
    N, Tb = bins.shape
    cdf = cdf_of(weights)
    u = np.broadcast_to(u_rule(n), (N, n)) if u is None else np.asarray(u, F)
    out = np.empty((N, n), F)
    for r in range(N):
        hi = np.searchsorted(cdf[r], u[r], side="right")
        lo = np.maximum(hi - 1, 0)
        hi = np.minimum(hi, Tb - 1)
        c0 = cdf[r][lo]
        denom = (cdf[r][hi] - c0).astype(F)
        denom = np.where(denom < F(1e-5), F(1.0), denom).astype(F)
        t = ((u[r] - c0).astype(F) / denom).astype(F)
        b0, b1 = bins[r][lo], bins[r][hi]
        out[r] = np.minimum((b0 + (t * (b1 - b0).astype(F)).astype(F)).astype(F), b1)
    return out


def merge(z, z_new):
    """the stable sort of cat(z, z_new) by the contract's ranks: coarse i at i + #{j : z_new_j < z_i}, new j at j + #{i : z_i <= z_new_j}"""
    z, z_new = np.asarray(z, F), np.asarray(z_new, F)
    N, Nc = z.shape
    Nf = z_new.shape[1]
    out = np.full((N, Nc + Nf), np.nan, F)
    for r in range(N):
        rc = np.arange(Nc) + (z_new[r][None, :] < z[r][:, None]).sum(axis=1)
        rn = np.arange(Nf) + (z[r][None, :] <= z_new[r][:, None]).sum(axis=1)
        assert len(set(rc.tolist()) | set(rn.tolist())) == Nc + Nf
        out[r, rc] = z[r]
        out[r, rn] = z_new[r]
    return out


def near_far(o, d, bound, min_near):
    from oracle import ngp_oracle as O
    return O.near_far_from_aabb(np.asarray(o, F), np.asarray(d, F), np.array([-bound] * 3 + [bound] * 3, F), min_near)


def coarse_z(near, far, Nc):
    """[N,Nc]: near + (far - near) * lin_rule(Nc): the dense lattice's depths (csrc/nav_field.hip: nv_sample_at)"""
    near, far = np.asarray(near, F), np.asarray(far, F)
    span = (far - near).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        return (near[:, None] + (span[:, None] * C.lin_rule(Nc)[None, :]).astype(F)).astype(F)


def bins_of(z):
    """z + 0.5 * (z[1:] - z[:-1]) (nerf/renderer.py:183)"""
    z = np.asarray(z, F)
    return (z[:, :-1] + (F(0.5) * (z[:, 1:] - z[:, :-1]).astype(F)).astype(F)).astype(F)


def resample(near, far, coarse_weights, Nf):
    """the merged depth list [N, Nc + Nf] from the rays' near / far and the float32 coarse weights [N,Nc]; also returns (z coarse, z_new)"""
    w = np.asarray(coarse_weights, F)
    Nc = w.shape[1]
    z = coarse_z(near, far, Nc)
    z_new = sample_pdf(bins_of(z), w[:, 1:Nc - 1], Nf)
    return merge(z, z_new), z, z_new
