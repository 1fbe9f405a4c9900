"""CPU: the marching-cubes case table of csrc/mesh.hip (read through the C ABI without a GPU), the numpy restatement of its contract
(tests/_mc_restated.py) on analytic spheres and random fields, the PLY writer of ngp.mesh and the argument validation of the new entry points."""
import ctypes

import numpy as np
import pytest

import _mc_restated as R


@pytest.fixture(scope="module")
def table():
    return R.case_table()


def face_cycles():
    """the six cell faces as corner lists in cyclic order"""
    out = []
    for a in range(3):
        b, c = R.other_axes(a)
        for side in (0, 1):
            cyc = []
            for ob, oc in ((0, 0), (1, 0), (1, 1), (0, 1)):
                o = [0, 0, 0]
                o[a], o[b], o[c] = side, ob, oc
                cyc.append(o[0] | (o[1] << 1) | (o[2] << 2))
            out.append(cyc)
    return out


EDGES = [R.edge_corners(e) for e in range(12)]


def edge_of(k0, k1):
    return next(e for e, pq in enumerate(EDGES) if set(pq) == {k0, k1})


def rule_segments(case, cyc):
    """the face rule: one segment across a face with one inside run; on a face whose inside corners sit on one diagonal, a segment
    cutting off each inside corner"""
    ins = [(case >> k) & 1 for k in cyc]
    if sum(ins) in (0, 4):
        return set()
    if sum(ins) == 2 and ins[0] == ins[2]:
        return {frozenset((edge_of(cyc[i], cyc[i - 1]), edge_of(cyc[i], cyc[(i + 1) % 4]))) for i in range(4) if ins[i]}
    cross = [edge_of(cyc[i], cyc[(i + 1) % 4]) for i in range(4) if ins[i] != ins[(i + 1) % 4]]
    return {frozenset(cross)}


def test_table_layout(table):
    assert table.shape == (256, R.ROW)
    assert table[0, 2] == 0 and table[255, 2] == 0
    assert int(table[:, 2].max()) <= R.MAX_TRIS


def test_table_is_the_generated_one(table):
    """csrc/mesh.hip holds exactly what tools/gen_mc_table.py derives from the face rule"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_mc_table.py")
    spec = importlib.util.spec_from_file_location("gen_mc_table", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for case, (mask, tris) in enumerate(gen.table()):
        assert int(table[case, 0]) | (int(table[case, 1]) << 8) == mask, case
        assert R.table_triangles(table, case) == [tuple(t) for t in tris], case


def test_table_uses_exactly_the_crossing_edges(table):
    for case in range(256):
        crossing = {e for e, (p, q) in enumerate(EDGES) if ((case >> p) & 1) != ((case >> q) & 1)}
        mask = int(table[case, 0]) | (int(table[case, 1]) << 8)
        assert mask == sum(1 << e for e in crossing), case
        tris = R.table_triangles(table, case)
        used = {e for t in tris for e in t}
        assert used == crossing, (case, used, crossing)
        for t in tris:
            assert len(set(t)) == 3, (case, t)                       # no triangle degenerate in edge terms
        assert all(v == 255 for v in table[case, 3 + 3 * len(tris):]), case


def test_table_boundary_follows_the_face_rule(table):
    """the sides each case's triangles leave unpaired are exactly the face segments the ambiguity rule prescribes"""
    for case in range(256):
        count = {}
        for t in R.table_triangles(table, case):
            for i in range(3):
                s = frozenset((t[i], t[(i + 1) % 3]))
                count[s] = count.get(s, 0) + 1
        assert all(n in (1, 2) for n in count.values()), case
        boundary = {s for s, n in count.items() if n == 1}
        expected = set()
        for cyc in face_cycles():
            expected |= rule_segments(case, cyc)
        assert boundary == expected, (case, boundary ^ expected)


def test_table_orientation(table):
    """one inside corner: the triangle's normal points away from it (right-hand rule, edge midpoints)"""
    for k in range(8):
        for case, sign in ((1 << k, 1.0), (255 ^ (1 << k), -1.0)):
            (t,) = R.table_triangles(table, case)
            pts = []
            for e in t:
                p, q = EDGES[e]
                pts.append((np.array(R.corner_offset(p)) + np.array(R.corner_offset(q))) / 2.0)
            n = np.cross(pts[1] - pts[0], pts[2] - pts[0])
            assert sign * np.dot(n, pts[0] - np.array(R.corner_offset(k))) > 0, (case, t)


# ---------------------------------------------------------------------------------------------------------------------------------
# mesh checks shared with tests/test_gpu_mesh.py

def edge_counts(tris):
    t = np.asarray(tris, np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return counts


def signed_volume(verts, tris):
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def sphere_field(shape, r):
    c = np.array([(s - 1) / 2.0 + 0.123 for s in shape])
    g = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    d = np.sqrt(sum((gi - ci) ** 2 for gi, ci in zip(g, c)))
    return (r - d).astype(np.float32), c


SPHERES = [((48, 48, 48), 20.0), ((97, 97, 97), 44.7), ((40, 56, 33), 12.5)]


def noise_field(n, seed):
    u = np.random.default_rng(seed).uniform(size=(n, n, n)).astype(np.float32)
    u[[0, -1]] = 0.0
    u[:, [0, -1]] = 0.0
    u[:, :, [0, -1]] = 0.0
    return u


@pytest.mark.parametrize("shape,r", SPHERES)
def test_restated_sphere_is_a_closed_outward_sphere(table, shape, r):
    u, c = sphere_field(shape, r)
    assert min(min(c) - r, min(s - 1 - ci - r for s, ci in zip(shape, c))) >= 3      # a margin of 3 cells
    v, t = R.marching_cubes(u, 0.0, table)
    assert v.dtype == np.float32 and t.dtype == np.int32
    counts = edge_counts(t)
    assert counts.min() == 2 and counts.max() == 2                                   # closed 2-manifold
    assert len(v) - len(counts) + len(t) == 2                                        # Euler characteristic of a sphere
    assert len(np.unique(t)) == len(v)                                               # no unreferenced vertex
    vol = signed_volume(v, t)
    assert vol > 0
    assert abs(vol / (4.0 / 3.0 * np.pi * r ** 3) - 1.0) < 0.02
    dist = np.linalg.norm(v.astype(np.float64) - c, axis=1)
    assert np.max(np.abs(dist - r)) < 0.05


@pytest.mark.parametrize("n", [20, 33])
def test_restated_noise_is_closed(table, n):
    """uniform noise hits every ambiguous face configuration many times: with the face rule the mesh has no crack"""
    for seed in range(10):
        v, t = R.marching_cubes(noise_field(n, seed), 0.5, table)
        counts = edge_counts(t)
        assert len(t) > 0 and counts.min() == 2 and counts.max() == 2, seed


def test_restated_vertex_order_and_degenerate_corners(table):
    """vertices in edge-id order with the contract's coordinates; a corner exactly at threshold is outside"""
    u = np.zeros((3, 3, 3), np.float32)
    u[1, 1, 1] = 2.0
    u[1, 1, 2] = 1.0                                                                 # exactly at threshold: outside
    v, t = R.marching_cubes(u, 1.0, table)
    assert len(v) == 6 and len(t) == 8
    expect = np.array([[0.5, 1, 1], [1, 0.5, 1], [1, 1, 0.5], [1.5, 1, 1], [1, 1.5, 1], [1, 1, 2]], np.float32)   # edge ids 3*4, 3*10+1, 3*12+2, 3*13+0..2
    assert np.array_equal(v, expect)
    assert edge_counts(t).max() == 2 and signed_volume(v, t) > 0
    for full in (np.full((4, 5, 6), 3.0, np.float32), np.zeros((4, 5, 6), np.float32)):
        v, t = R.marching_cubes(full, 1.0, table)
        assert v.shape == (0, 3) and t.shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# host-side pieces

def read_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").split("\n")
    nv = int(next(h for h in header if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in header if h.startswith("element face")).split()[-1])
    body = data[end:]
    v = np.frombuffer(body[:12 * nv], "<f4").reshape(nv, 3)
    f = np.frombuffer(body[12 * nv:], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    assert len(f) == nf and np.all(f["n"] == 3)
    return data[:end], v, f["i"]


def test_write_ply_round_trips(tmp_path):
    from ngp.mesh import write_ply
    rng = np.random.default_rng(3)
    v = rng.normal(size=(7, 3))
    t = rng.integers(0, 7, size=(5, 3)).astype(np.int64)
    path = tmp_path / "m.ply"
    write_ply(str(path), v, t)
    header, v2, t2 = read_ply(str(path))
    assert header == (b"ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
                      b"element face 5\nproperty list uchar int vertex_indices\nend_header\n")
    assert np.array_equal(v2, v.astype(np.float32)) and np.array_equal(t2, t)
    assert path.stat().st_size == len(header) + 7 * 12 + 5 * 13
    write_ply(str(path), np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    header, v2, t2 = read_ply(str(path))
    assert v2.shape == (0, 3) and t2.shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(str(path), v, t + 7)


def test_marching_cubes_validation_needs_no_gpu():
    import ngp_hip
    L = ngp_hip.lib()
    one = ctypes.c_void_p(16)                                     # non-null dummy: validation rejects before any dereference
    V, T = ctypes.c_uint64(), ctypes.c_uint64()
    ws = L.ngp_marching_cubes_workspace(8, 8, 8)
    assert ws >= 8 ** 3 * 3
    for dims in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (1025, 8, 8), (8, 1025, 8), (8, 8, 1025), (0, 0, 0)):
        assert L.ngp_marching_cubes_workspace(*dims) == 0
        assert L.ngp_marching_cubes_count(one, *dims, 0.0, one, 1 << 40, ctypes.byref(V), ctypes.byref(T), None) == -1
        assert b"[2, 1024]" in L.ngp_last_error()
        assert L.ngp_marching_cubes_emit(one, *dims, 0.0, one, 1 << 40, one, 1, one, 1, None) == -1
        assert b"[2, 1024]" in L.ngp_last_error()
    assert L.ngp_marching_cubes_count(None, 8, 8, 8, 0.0, one, ws, ctypes.byref(V), ctypes.byref(T), None) == -1
    assert b"null pointer" in L.ngp_last_error()
    assert L.ngp_marching_cubes_count(one, 8, 8, 8, 0.0, one, ws, None, ctypes.byref(T), None) == -1
    assert L.ngp_marching_cubes_count(one, 8, 8, 8, 0.0, None, ws, ctypes.byref(V), ctypes.byref(T), None) == -1
    assert L.ngp_marching_cubes_count(one, 8, 8, 8, 0.0, one, ws - 1, ctypes.byref(V), ctypes.byref(T), None) == -1
    assert b"workspace too small" in L.ngp_last_error()
    assert L.ngp_marching_cubes_emit(one, 8, 8, 8, 0.0, one, ws, None, 4, one, 4, None) == -1
    assert b"null pointer" in L.ngp_last_error()
    assert L.ngp_marching_cubes_emit(one, 8, 8, 8, 0.0, one, ws, one, 1 << 31, one, 4, None) == -1
    assert b"int32" in L.ngp_last_error()
    assert L.ngp_marching_cubes_emit(one, 8, 8, 8, 0.0, one, ws, None, 0, None, 0, None) == 0      # nothing to write: no launch
    assert L.ngp_marching_cubes_table(None, 1 << 20) == -1
    buf = (ctypes.c_uint8 * 16)()
    assert L.ngp_marching_cubes_table(buf, 16) == -1
    assert b"needs" in L.ngp_last_error()
