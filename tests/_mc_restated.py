"""numpy restatement of the marching-cubes contract of csrc/mesh.hip: the same vertices, bit for bit, in the
same order, and the same triangles.  It reads the case table through ngp_marching_cubes_table, which needs no GPU."""
import ctypes

import numpy as np

MAX_TRIS = 5
ROW = 3 + 3 * MAX_TRIS


def corner_offset(k):
    return (k & 1, (k >> 1) & 1, (k >> 2) & 1)


def other_axes(a):
    return [b for b in range(3) if b != a]


def edge_corners(e):
    """local edge e = 4 * a + j -> (corner at its low end, corner at its high end)"""
    a, j = divmod(e, 4)
    b, c = other_axes(a)
    o = [0, 0, 0]
    o[b], o[c] = j & 1, j >> 1
    k0 = o[0] | (o[1] << 1) | (o[2] << 2)
    return k0, k0 | (1 << a)


def case_table():
    """uint8 [256, ROW] as the library holds it"""
    import ngp_hip
    buf = np.zeros((256, ROW), np.uint8)
    ngp_hip.check(ngp_hip.lib().ngp_marching_cubes_table(buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes), "marching_cubes_table")
    return buf


def table_triangles(table, case):
    """the case's triangles as a list of local-edge triples"""
    n = int(table[case, 2])
    return [tuple(int(e) for e in table[case, 3 + 3 * i: 6 + 3 * i]) for i in range(n)]


def marching_cubes(u, threshold, table=None):
    """(vertices float32 [V,3] in index space, triangles int32 [T,3])"""
    u = np.ascontiguousarray(u, np.float32)
    X, Y, Z = u.shape
    thr = np.float32(threshold)
    table = case_table() if table is None else table
    inside = u > thr
    # crossing bits of the three edges each lattice point owns, and the vertex index of every owned edge
    cross = np.zeros((X, Y, Z, 3), bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)                                  # edge id 3 * point + a
    vid = np.cumsum(flat, dtype=np.int64) - 1
    ids = np.flatnonzero(flat)
    p, a = ids // 3, ids % 3
    x, y, z = p // (Y * Z), (p // Z) % Y, p % Z
    verts = np.stack([x, y, z], 1).astype(np.float32)
    uf = u.reshape(-1)
    stride = np.array([Y * Z, Z, 1], np.int64)
    u0 = uf[p]
    u1 = uf[p + stride[a]]
    with np.errstate(all="ignore"):
        t = (thr - u0) / (u1 - u0)                            # float32 throughout
    verts[np.arange(len(ids)), a] = verts[np.arange(len(ids)), a] + t
    # cases of the cells in linear cell order
    case = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    for k in range(8):
        dx, dy, dz = corner_offset(k)
        case |= inside[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int64) << k
    case = case.reshape(-1)
    ntri = table[case, 2].astype(np.int64)
    cells = np.repeat(np.arange(case.size), ntri)
    slot = np.arange(cells.size) - np.repeat(np.cumsum(ntri) - ntri, ntri)
    cx = cells // ((Y - 1) * (Z - 1))
    cy = (cells // (Z - 1)) % (Y - 1)
    cz = cells % (Z - 1)
    origin = (cx * Y + cy) * Z + cz
    tris = np.zeros((cells.size, 3), np.int32)
    for c in range(3):
        e = table[case[cells], 3 + 3 * slot + c].astype(np.int64)
        ea, ej = e // 4, e % 4
        # the edge's owner point: the cell origin plus its two other offsets (b < c the other axes)
        ob = np.where(ea == 0, stride[1], stride[0])
        oc = np.where(ea == 2, stride[1], stride[2])
        q = origin + (ej & 1) * ob + (ej >> 1) * oc
        tris[:, c] = vid[3 * q + ea]
    return verts, tris
