"""Generates the 256-case marching-cubes table of csrc/mesh.hip and prints it as C.

The table is derived, not copied: for each case the contour segments on the six faces of the cell follow one fixed face
rule, the segments chain into closed loops, and every loop is capped by triangles (`triangulate`).  The face rule, "on a face whose inside
corners sit on one diagonal, separate the inside corners", depends only on the face's four corner values, so the two
cells sharing a face draw the same segments there and the mesh has no cracks.

Conventions (shared with mesh.hip and tests/_mc_restated.py):
  corner k of a cell sits at offset (k & 1, (k >> 1) & 1, (k >> 2) & 1) along (x, y, z); case bit k = corner k inside;
  edge e = 4 * a + j runs along axis a from the corner whose two other offsets (ob, oc), b < c the other axes, give
  j = ob + 2 * oc.
Loops are oriented so that, by the right-hand rule, triangle normals point from the inside corners to the outside ones.

Run: python tools/gen_mc_table.py > table.inc   (the output is pasted into csrc/mesh.hip)"""
import sys

import numpy as np


def corner_offset(k):
    return np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])


def edge_corners(e):
    a, j = divmod(e, 4)
    b, c = [ax for ax in range(3) if ax != a]
    o = [0, 0, 0]
    o[b], o[c] = j & 1, j >> 1
    k0 = o[0] | (o[1] << 1) | (o[2] << 2)
    return k0, k0 | (1 << a)


EDGE = [edge_corners(e) for e in range(12)]
MAX_TRIS = 5                                                      # NGP_MC_MAX_TRIS: the rule never needs more


def edge_between(k0, k1):
    for e, (p, q) in enumerate(EDGE):
        if {p, q} == {k0, k1}:
            return e
    raise ValueError((k0, k1))


def faces():
    """(axis, side, corners in cyclic order around the face)"""
    out = []
    for a in range(3):
        b, c = [ax for ax in range(3) if ax != a]
        for side in (0, 1):
            cyc = []
            for ob, oc in ((0, 0), (1, 0), (1, 1), (0, 1)):
                o = [0, 0, 0]
                o[a], o[b], o[c] = side, ob, oc
                cyc.append(o[0] | (o[1] << 1) | (o[2] << 2))
            out.append((a, side, cyc))
    return out


FACES = faces()


def face_segments(case, cyc):
    """Segments (as unordered edge pairs, each with the inside corner at the first edge's end) the face rule draws on one face."""
    ins = [(case >> k) & 1 for k in cyc]
    n_in = sum(ins)
    if n_in in (0, 4):
        return []
    segs = []
    if n_in == 2 and ins[0] == ins[2]:                            # ambiguous: inside corners on one diagonal -> cut each off
        for i in range(4):
            if ins[i]:
                segs.append((edge_between(cyc[i], cyc[i - 1]), edge_between(cyc[i], cyc[(i + 1) % 4]), cyc[i]))
        return segs
    cross = [edge_between(cyc[i], cyc[(i + 1) % 4]) for i in range(4) if ins[i] != ins[(i + 1) % 4]]
    assert len(cross) == 2
    k_in = next(k for k in EDGE[cross[0]] if (case >> k) & 1)
    segs.append((cross[0], cross[1], k_in))
    return segs


def midpoint(e):
    p, q = EDGE[e]
    return (corner_offset(p) + corner_offset(q)) / 2.0


def oriented_face_segments(case):
    """directed segments (e_from, e_to): with f the face's outward normal, ((to - from) x (-f)) points away from the inside corner"""
    out = []
    for a, side, cyc in FACES:
        f = np.zeros(3)
        f[a] = 1.0 if side else -1.0
        for e1, e2, k_in in face_segments(case, cyc):
            p, q = midpoint(e1), midpoint(e2)
            s = np.dot(np.cross(q - p, -f), corner_offset(k_in) - p)
            assert s != 0
            out.append((e1, e2) if s < 0 else (e2, e1))
    return out


def case_triangles(case):
    segs = oriented_face_segments(case)
    nxt = {}
    for s, t in segs:
        assert s not in nxt, (case, "two segments leave one edge")
        nxt[s] = t
    assert sorted(nxt) == sorted(nxt.values()), (case, "segments do not chain")
    tris, seen = [], set()
    for start in sorted(nxt):                                     # loops in order of their smallest edge; fan from it
        if start in seen:
            continue
        loop = [start]
        while nxt[loop[-1]] != start:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        tris += triangulate(loop)
    return tris


def share_face(e1, e2):
    return any(set(EDGE[e1]) | set(EDGE[e2]) <= set(cyc) for _, _, cyc in FACES)


def polygon_triangulations(poly):
    """every triangulation of the polygon poly (a list of vertices in loop order), the fans from poly[0] first"""
    if len(poly) < 3:
        yield []
        return
    if len(poly) == 3:
        yield [tuple(poly)]
        return
    a, b = poly[0], poly[-1]                                      # the triangle on the closing side (a, b) has its apex at some k
    for k in range(len(poly) - 2, 0, -1):
        for left in polygon_triangulations(poly[:k + 1]):
            for right in polygon_triangulations(poly[k:]):
                yield left + right + [(a, poly[k], b)]


def triangulate(loop):
    """Cap one oriented loop with n - 2 triangles whose chords (triangle sides that are not loop sides) never join two vertices of one
    lattice face: such a chord lies in the face, the cell across it may draw the same chord, and the mesh edge would then belong to four
    triangles.  A chord between edges of no common face lies in this cell only, so with it every mesh edge is in exactly two triangles.
    Among the admissible triangulations the first in a fixed order is taken: fans from each loop vertex in turn, then all the others."""
    n = len(loop)
    sides = {frozenset((loop[i], loop[(i + 1) % n])) for i in range(n)}

    def ok(tris):
        for t in tris:
            for i in range(3):
                s = frozenset((t[i], t[(i + 1) % 3]))
                if s not in sides and share_face(*s):
                    return False
        return True

    for r in range(n):
        rot = loop[r:] + loop[:r]
        fan = [(rot[0], rot[i], rot[i + 1]) for i in range(1, n - 1)]
        if ok(fan):
            return fan
    for tris in polygon_triangulations(loop):
        if ok(tris):
            return tris
    raise AssertionError(("no admissible triangulation", loop))


def edge_mask(case):
    return sum(1 << e for e, (p, q) in enumerate(EDGE) if ((case >> p) & 1) != ((case >> q) & 1))


def table():
    return [(edge_mask(c), case_triangles(c)) for c in range(256)]


def main():
    tab = table()
    maxt = max(len(t) for _, t in tab)
    assert maxt <= MAX_TRIS
    print(f"// generated by tools/gen_mc_table.py: 256 cases, at most {maxt} triangles per case; row = edge mask (lo, hi), count, edges")
    print("#define MC_TABLE_ROWS { \\")
    for c, (m, tris) in enumerate(tab):
        row = [m & 0xFF, m >> 8, len(tris)] + [e for t in tris for e in t]
        row += [0xFF] * (3 + 3 * MAX_TRIS - len(row))
        print("    {" + ", ".join(str(v) for v in row) + "}, \\")
    print("}")
    hist = np.bincount([len(t) for _, t in tab])
    print("// triangles per case: " + ", ".join(f"{n}: {h}" for n, h in enumerate(hist)), file=sys.stderr)


if __name__ == "__main__":
    main()
