"""GPU: marching cubes of csrc/mesh.hip against its numpy restatement (tests/_mc_restated.py), bit for bit; ngp.mesh's lattice against
the reference's chunked query (nerf/utils.py:150-167); save_mesh on the hand-set ring scene."""
import numpy as np
import pytest
import torch

import _mc_restated as R
from test_mesh_host import edge_counts, noise_field, read_ply, signed_volume, sphere_field

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    return R.case_table()


def gpu_mc(u, thr, dev):
    from ngp.mesh import marching_cubes
    v, t = marching_cubes(torch.from_numpy(np.ascontiguousarray(u)).to(dev), thr)
    torch.cuda.synchronize()
    return v.cpu().numpy(), t.cpu().numpy()


def assert_same_mesh(got, ref):
    (v, t), (v_ref, t_ref) = got, ref
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert v.shape == v_ref.shape and t.shape == t_ref.shape, (v.shape, v_ref.shape, t.shape, t_ref.shape)
    assert np.array_equal(v.view(np.uint32), v_ref.view(np.uint32))
    assert np.array_equal(t, t_ref)


def lattices():
    rng = np.random.default_rng(7)
    out = [("sphere48", sphere_field((48, 48, 48), 20.0)[0], 0.0),
           ("sphere_noncubic", sphere_field((40, 56, 33), 12.5)[0], 0.0),
           ("noncubic_noise", rng.normal(size=(17, 9, 70)).astype(np.float32), 0.1),        # crossings on the lattice's own faces too
           ("empty", np.zeros((5, 6, 7), np.float32), 0.5),
           ("full", np.ones((5, 6, 7), np.float32), 0.5),
           ("at_threshold", rng.integers(0, 3, size=(23, 19, 21)).astype(np.float32), 1.0)]   # a third of the corners exactly at threshold
    for n in (20, 33):
        for seed in range(10):
            out.append((f"noise{n}_{seed}", noise_field(n, seed), 0.5))
    return out


@pytest.mark.parametrize("name,u,thr", lattices(), ids=[c[0] for c in lattices()])
def test_marching_cubes_equals_restatement(dev, table, name, u, thr):
    ref = R.marching_cubes(u, thr, table)
    got = gpu_mc(u, thr, dev)
    assert_same_mesh(got, ref)
    assert_same_mesh(gpu_mc(u, thr, dev), got)                  # run to run: bit-identical
    if name.startswith("noise"):
        assert edge_counts(got[1]).max() == 2 and edge_counts(got[1]).min() == 2
    if name in ("empty", "full"):
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3)


@pytest.mark.parametrize("shape", [(1024, 4, 4), (4, 4, 1024), (3, 1024, 2)])
def test_marching_cubes_long_thin_lattices(dev, table, shape):
    u = np.random.default_rng(1).normal(size=shape).astype(np.float32)
    assert_same_mesh(gpu_mc(u, 0.0, dev), R.marching_cubes(u, 0.0, table))


def test_marching_cubes_several_workgroups_of_a_sphere(dev, table):
    """a 97^3 sphere: 224 workgroups of 4096 points, so the per-workgroup bases and cross-workgroup vertex lookups are exercised"""
    u, _ = sphere_field((97, 97, 97), 44.7)
    got = gpu_mc(u, 0.0, dev)
    assert_same_mesh(got, R.marching_cubes(u, 0.0, table))
    assert edge_counts(got[1]).max() == 2 and signed_volume(*got) > 0


def test_marching_cubes_rejects_bad_input(dev):
    from ngp.mesh import marching_cubes
    with pytest.raises(RuntimeError, match="GPU"):
        marching_cubes(torch.zeros(4, 4, 4), 0.0)
    with pytest.raises(ValueError):
        marching_cubes(torch.zeros(4, 4, device=dev), 0.0)
    with pytest.raises(RuntimeError, match=r"\[2, 1024\]"):
        marching_cubes(torch.zeros(1, 4, 4, device=dev), 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the lattice of extract_fields

def reference_fields(bound_min, bound_max, resolution, query_func, S=128):
    """nerf/utils.py:150-167 as written: CPU linspace, 128^3 chunks, one .cpu() each"""
    X = torch.linspace(bound_min[0], bound_max[0], resolution).split(S)
    Y = torch.linspace(bound_min[1], bound_max[1], resolution).split(S)
    Z = torch.linspace(bound_min[2], bound_max[2], resolution).split(S)
    u = np.zeros([resolution, resolution, resolution], dtype=np.float32)
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    val = query_func(pts).reshape(len(xs), len(ys), len(zs)).detach().cpu().numpy()
                    u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = val
    return u


@pytest.fixture(scope="module")
def ring(dev):
    from ngp import workload as W
    from ngp.field import NGPFieldFF
    from ngp.render import NGPRenderer
    model = W.make_model(0)
    field = NGPFieldFF(bound=W.BOUND).to(dev).load_arrays(model)
    ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
    return dict(W=W, model=model, field=field, ren=ren)


def test_extract_fields_ff_equals_chunked_density_sigma(dev, ring):
    """the fused field's density_sigma is pointwise: the slab query equals the reference's 128^3-chunk query bit for bit"""
    from ngp.mesh import density_query, extract_fields
    q = density_query(ring["field"], fp16=True)
    lo, hi = ring["ren"].aabb_infer[:3], ring["ren"].aabb_infer[3:]
    r = 150                                                     # chunks of 128 and 22 along each axis
    got = extract_fields(lo, hi, r, lambda p: q(p.to(dev)))
    ref = reference_fields(lo.cpu(), hi.cpu(), r, lambda p: q(p.to(dev)))
    assert got.dtype == np.float32 and got.shape == (r, r, r)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert (got > 10).sum() > 1000                              # the scene is there


def test_extract_fields_linear_field_equals_chunked_density(dev, ring):
    """float32 NGPField through the op chain: the slab batches and the reference's chunks may tile the GEMMs differently, so the two
    agree within the op chain's float32 tolerance (tests/test_gpu_callers_parity.py: 2e-5 relative on sigma)"""
    from _util import linear_field_from_model
    from ngp.mesh import extract_fields
    field = linear_field_from_model(ring["model"], dev)
    q = lambda p: field.density(p.to(dev))["sigma"]            # noqa: E731
    lo, hi = torch.tensor([-2.0] * 3), torch.tensor([2.0] * 3)
    r = 136
    got = extract_fields(lo, hi, r, q)
    ref = reference_fields(lo, hi, r, q)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-6)
    assert (got > 10).sum() > 100


def closed_part(v_idx, t, u, thr, r):
    """The hand-set table's occupancy level is hashed (workload.make_model): its collisions put sigma > 10 at stray lattice points all over the
    box, a few of them on the lattice's outer faces, where their surface leaves the lattice and stays open.  So the checks split the mesh:
    every mesh edge is in at most 2 triangles and in 1 only when both its vertices lie on an outer face; the components that touch no outer
    face are returned with the lattice points inside them (6-connected components of u > thr that touch no outer face: with the face rule
    "separate the inside corners" those are what one closed surface encloses)."""
    import scipy.ndimage
    import scipy.sparse
    import scipy.sparse.csgraph
    on_face = np.any((v_idx == 0) | (v_idx == r - 1), axis=1)
    te = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    e, c = np.unique(te, axis=0, return_counts=True)
    assert c.max() == 2
    assert np.all(on_face[e[c == 1]])
    n = len(v_idx)
    nc, lab = scipy.sparse.csgraph.connected_components(scipy.sparse.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)
    touch = np.zeros(nc, bool)
    touch[lab[on_face]] = True
    keep = ~touch[lab[t[:, 0]]]
    inside = u > thr
    L, _ = scipy.ndimage.label(inside)
    outer = np.unique(np.concatenate([L[[0, -1]].ravel(), L[:, [0, -1]].ravel(), L[:, :, [0, -1]].ravel()]))
    return keep, int((inside & ~np.isin(L, outer)).sum())


def test_save_mesh_ring_scene(dev, ring, table, tmp_path):
    from ngp.mesh import density_query, extract_fields, save_mesh
    r, thr = 256, 10.0
    path = tmp_path / "ring.ply"
    v, t = save_mesh(ring["ren"], str(path), resolution=r, threshold=thr)
    assert v.dtype == np.float64 and t.dtype == np.int64 and len(t) > 1000
    # the same mesh as the restatement on the same lattice
    lo, hi = ring["ren"].aabb_infer[:3], ring["ren"].aabb_infer[3:]
    u = extract_fields(lo, hi, r, density_query(ring["field"], fp16=True))
    v_idx, t_ref = R.marching_cubes(u, thr, table)
    b_min, b_max = lo.cpu().numpy(), hi.cpu().numpy()
    assert np.array_equal(t, t_ref.astype(np.int64))
    assert np.array_equal(v, v_idx.astype(np.float64) / (r - 1.0) * (b_max - b_min)[None, :] + b_min[None, :])
    # closed wherever it does not leave the lattice; orientation and size of the closed part against the lattice points it encloses
    keep, n_inside = closed_part(v_idx, t_ref, u, thr, r)
    assert keep.sum() > 0.75 * len(t)
    h = 4.0 / (r - 1)
    vol, vol_pts = signed_volume(v, t[keep]), n_inside * h ** 3
    assert vol > 0
    assert abs(vol / vol_pts - 1.0) < 0.10, (vol, vol_pts)
    # the ring itself: the surface runs round each of the twelve pillars (workload.scene_boxes)
    for k in range(12):
        a = 2 * np.pi * k / 12
        d = np.linalg.norm(v[:, :2] - [0.65 * np.cos(a), 0.65 * np.sin(a)], axis=1)
        near = (d < 0.12) & (v[:, 2] > 0.1) & (v[:, 2] < 0.35)
        assert near.sum() > 50, k
    # the PLY reads back to the same arrays
    _, v2, t2 = read_ply(str(path))
    assert np.array_equal(v2, v.astype(np.float32)) and np.array_equal(t2, t)
