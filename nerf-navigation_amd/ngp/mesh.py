"""Mesh export of a fitted scene: what the reference's Trainer.save_mesh -> extract_geometry -> extract_fields does
(nerf/utils.py:150-182, 533-555), without PyMCubes or trimesh.

The density lattice is queried in x-slabs that stay on the device, marching cubes runs on the device (csrc/mesh.hip,
DESIGN.md §3.10), and the mesh is written as a binary PLY.  The only host synchronisations of an extraction are the read
of the vertex and triangle counts and the final copy of the mesh."""
import ctypes

import numpy as np
import torch

import ngp_hip as _hip


def marching_cubes(u, threshold):
    """u: CUDA float32 [X,Y,Z] (2 <= X, Y, Z <= 1024).  Returns (vertices float32 [V,3], triangles int32 [T,3]) on u's device, in INDEX
    space: a vertex on the lattice edge from p to p + e_a sits at p_a + (threshold - u(p)) / (u(p + e_a) - u(p)) along a.  A corner is inside
    iff u > threshold; normals (right-hand rule) point from inside to outside; the mesh has no cracks and is the same bit for bit on every run."""
    _hip.require_cuda(u)
    if u.dim() != 3 or u.dtype != torch.float32:
        raise ValueError(f"marching_cubes: expected a float32 [X,Y,Z] lattice, got {tuple(u.shape)} {u.dtype}")
    u = u.contiguous()
    X, Y, Z = (int(s) for s in u.shape)
    L = _hip.lib()
    thr = float(threshold)
    ws = _hip.workspace(L.ngp_marching_cubes_workspace(X, Y, Z), u.device)
    V, T = ctypes.c_uint64(), ctypes.c_uint64()
    _hip.check(L.ngp_marching_cubes_count(_hip.ptr(u), X, Y, Z, thr, _hip.ptr(ws), ws.numel(), ctypes.byref(V), ctypes.byref(T),
                                          _hip.stream()), "marching_cubes_count")
    verts = torch.empty((V.value, 3), dtype=torch.float32, device=u.device)
    tris = torch.empty((T.value, 3), dtype=torch.int32, device=u.device)
    _hip.check(L.ngp_marching_cubes_emit(_hip.ptr(u), X, Y, Z, thr, _hip.ptr(ws), ws.numel(), _hip.ptr(verts) if V.value else None,
                                         V.value, _hip.ptr(tris) if T.value else None, T.value, _hip.stream()), "marching_cubes_emit")
    return verts, tris


def _host(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu()
    return torch.as_tensor(np.asarray(v))


def _lattice_axes(bound_min, bound_max, resolution):
    """the reference's lattice coordinates: torch.linspace per axis on the CPU (nerf/utils.py:152-154)"""
    lo, hi = _host(bound_min), _host(bound_max)
    return [torch.linspace(lo[i], hi[i], resolution) for i in range(3)]


def _device_lattice(bound_min, bound_max, resolution, query_func, S=128, device=None):
    """sigma over the resolution^3 lattice as a float32 [r,r,r] tensor on the device.  The points are queried in x-slabs of about S^3 points
    (the reference's chunk size) and every slab's result stays on the device."""
    device = torch.device("cuda") if device is None else device
    xs, ys, zs = (a.to(device) for a in _lattice_axes(bound_min, bound_max, resolution))
    r = resolution
    u = torch.empty((r, r, r), dtype=torch.float32, device=device)
    rows = max(1, (S ** 3) // (r * r))
    with torch.no_grad():
        yy, zz = torch.meshgrid(ys, zs, indexing="ij")
        for x0 in range(0, r, rows):
            xb = xs[x0:x0 + rows]
            n = xb.numel()
            pts = torch.stack([xb[:, None, None].expand(n, r, r), yy[None].expand(n, r, r), zz[None].expand(n, r, r)], dim=-1).reshape(-1, 3)
            u[x0:x0 + n] = query_func(pts).reshape(n, r, r).float()
    return u


def extract_fields(bound_min, bound_max, resolution, query_func, S=128):
    """nerf/utils.py:150-167: numpy float32 [r,r,r] of query_func over the lattice of torch.linspace(bound_min[i], bound_max[i], r).
    One copy to the host at the end instead of one per 128^3 chunk."""
    return _device_lattice(bound_min, bound_max, resolution, query_func, S).cpu().numpy()


def _world(vertices, bound_min, bound_max, resolution):
    """index space -> world, in float64 as the reference does it (nerf/utils.py:178)"""
    b_max, b_min = _host(bound_max).numpy(), _host(bound_min).numpy()
    return vertices.astype(np.float64) / (resolution - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func):
    """nerf/utils.py:170-180: (vertices float64 [V,3] in world units, triangles int64 [T,3]) of the threshold surface of query_func.
    The lattice stays on the device and goes straight into marching_cubes."""
    u = _device_lattice(bound_min, bound_max, resolution, query_func)
    verts, tris = marching_cubes(u, threshold)
    return _world(verts.cpu().numpy(), bound_min, bound_max, resolution), tris.cpu().numpy().astype(np.int64)


def density_query(field, fp16=True):
    """The query of Trainer.save_mesh (nerf/utils.py:541-545): sigma of the field under autocast; `density_sigma` (two native launches for
    the default fused field) when the field has it, `density(x)['sigma']` otherwise."""
    def query(pts):
        with torch.no_grad():
            with torch.autocast("cuda", enabled=fp16):
                if hasattr(field, "density_sigma"):
                    return field.density_sigma(pts)
                return field.density(pts)["sigma"]
    return query


def save_mesh(renderer, save_path, resolution=256, threshold=10, fp16=True):
    """Trainer.save_mesh (nerf/utils.py:533-555) on renderer.aabb_infer: the threshold surface of the field's density as a binary PLY.
    Returns (vertices float64 [V,3] world, triangles int64 [T,3]) as written."""
    field = getattr(renderer, "field", renderer)
    aabb = renderer.aabb_infer
    vertices, triangles = extract_geometry(aabb[:3], aabb[3:], resolution, threshold, density_query(field, fp16))
    write_ply(save_path, vertices, triangles)
    return vertices, triangles


def ply_header(n_vertices, n_faces):
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {n_vertices}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {n_faces}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")


def write_ply(path, vertices, triangles):
    """Binary little-endian PLY: vertex float x, y, z; face list uchar int vertex_indices.  vertices [V,3], triangles [T,3] (arrays or tensors)."""
    v = np.ascontiguousarray(_host(vertices).numpy(), dtype="<f4").reshape(-1, 3)
    t = np.asarray(_host(triangles).numpy()).reshape(-1, 3)
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("write_ply: triangle index out of range")
    faces = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    with open(path, "wb") as f:
        f.write(ply_header(len(v), len(t)))
        f.write(v.tobytes())
        f.write(faces.tobytes())
