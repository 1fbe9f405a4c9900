"""Shared synthetic inputs for the tests (seeded, small enough for the CPU oracle)."""
import numpy as np


def blob_bitfield(oracle, cascade=2, H=128, seed=0, n_blobs=40, bound=2.0):
    """Occupancy bitfield [cascade*H^3/8] from random spheres; Morton-ordered cells like the reference's density grid."""
    rng = np.random.default_rng(seed)
    idx = np.arange(H ** 3, dtype=np.int32)
    coords = oracle.morton3D_invert(idx).astype(np.float32)           # cell (x,y,z) of each Morton index
    grid = np.zeros((cascade, H ** 3), np.float32)
    for cas in range(cascade):
        b = min(2.0 ** cas, bound)
        centres = ((coords + 0.5) / H * 2 - 1) * b
        c = rng.uniform(-0.8 * b, 0.8 * b, size=(n_blobs, 3)).astype(np.float32)
        r = rng.uniform(0.05 * b, 0.25 * b, size=n_blobs).astype(np.float32)
        for k in range(n_blobs):
            d2 = ((centres - c[k]) ** 2).sum(1)
            grid[cas, d2 < r[k] ** 2] = 1.0
    return oracle.packbits(grid, 0.5), grid


def blob_bitfield_boxed(oracle, cascade=2, H=128, seed=0, n_blobs=40, bound=2.0):
    """blob_bitfield's bitfield (the same spheres from the same draws, the same float32 arithmetic per cell) for grids too large to test every cell
    against every sphere (256^3: 45 s there, 1 s here): a sphere is tested on the cells of its bounding box, widened by a cell.  Returns the
    bitfield only; callers assert that it equals blob_bitfield's at a size where both are cheap."""
    rng = np.random.default_rng(seed)
    grid = np.zeros((cascade, H ** 3), np.float32)
    for cas in range(cascade):
        b = min(2.0 ** cas, bound)
        axis = ((np.arange(H, dtype=np.int32).astype(np.float32) + 0.5) / H * 2 - 1) * b          # a cell centre's coordinate, as blob_bitfield forms it
        c = rng.uniform(-0.8 * b, 0.8 * b, size=(n_blobs, 3)).astype(np.float32)
        r = rng.uniform(0.05 * b, 0.25 * b, size=n_blobs).astype(np.float32)
        for k in range(n_blobs):
            lo = [max(int(np.searchsorted(axis, c[k, a] - r[k])) - 1, 0) for a in range(3)]
            hi = [min(int(np.searchsorted(axis, c[k, a] + r[k])) + 1, H) for a in range(3)]
            sq = [(axis[lo[a]:hi[a]] - c[k, a]) ** 2 for a in range(3)]
            d2 = (sq[0][:, None, None] + sq[1][None, :, None]) + sq[2][None, None, :]                # numpy's sum over three float32: left to right
            x, y, z = np.nonzero(d2 < r[k] ** 2)
            cells = np.stack([x + lo[0], y + lo[1], z + lo[2]], -1).astype(np.int32)
            if cells.shape[0]:
                grid[cas, oracle.morton3D(cells)] = 1.0
    return oracle.packbits(grid, 0.5)


def camera_rays(n_side=32, radius=3.0, seed=0, jitter=True):
    """Pinhole rays from a camera on an orbit looking at the origin; a few degenerate directions appended."""
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, 2 * np.pi)
    eye = np.array([radius * np.cos(th), radius * np.sin(th), 0.7 * radius * 0.3], np.float32)
    fwd = -eye / np.linalg.norm(eye)
    up = np.array([0, 0, 1], np.float32)
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    u, v = np.meshgrid(np.linspace(-0.6, 0.6, n_side), np.linspace(-0.6, 0.6, n_side))
    d = fwd[None] + u.reshape(-1, 1) * right[None] + v.reshape(-1, 1) * up[None]
    if jitter:
        d += rng.normal(scale=1e-3, size=d.shape)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o = np.broadcast_to(eye, d.shape).astype(np.float32).copy()
    # axis-parallel rays (a zero component in d: 1/d = inf) and a ray that misses the box
    extra_o = np.array([[-3, 0.1, 0.2], [0.3, -3, 0.1], [0.2, 0.1, 3], [5, 5, 5]], np.float32)
    extra_d = np.array([[1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 0, 0]], np.float32)
    return np.concatenate([o, extra_o]), np.concatenate([d, extra_d])


def oracle_field(field, dtype=None):
    """oracle.callers_oracle.DefaultField holding the parameters of a product field module (ngp.field.NGPField or NGPFieldFF):
    the CPU checker the GPU parity tests compare against."""
    import torch
    from oracle import callers_oracle as CO
    dtype = dtype or torch.float32
    emb = field.encoder.embeddings.detach().float().cpu().numpy()
    offsets = field.encoder.offsets.cpu().numpy()
    pls = float(field.encoder.per_level_scale)
    if hasattr(field.sigma_net, "weights"):                                   # FFMLP: flat [64,in] + k [64,64] + [16,64] (ffmlp/ffmlp.py:121-122)
        def split(net):
            w = net.weights.detach().float().cpu().numpy()
            shapes = [(net.hidden_dim, net.input_dim)] + [(net.hidden_dim, net.hidden_dim)] * (net.num_layers - 1) + [(net.padded_output_dim, net.hidden_dim)]
            out, off = [], 0
            for r, c in shapes:
                out.append(w[off:off + r * c].reshape(r, c)); off += r * c
            assert off == w.size
            return out
        return CO.DefaultField(emb, offsets, pls, split(field.sigma_net), split(field.color_net), field.bound, dtype=dtype, ff_layout=True)
    sw = [l.weight.detach().float().cpu().numpy() for l in field.sigma_net]
    cw = [l.weight.detach().float().cpu().numpy() for l in field.color_net]
    return CO.DefaultField(emb, offsets, pls, sw, cw, field.bound, dtype=dtype)


def ff_grads_as_matrices(net):
    """.grad of an FFMLP's flat weights as the list of per-layer matrices (same split as oracle_field)."""
    g = net.weights.grad.detach().float().cpu().numpy()
    shapes = [(net.hidden_dim, net.input_dim)] + [(net.hidden_dim, net.hidden_dim)] * (net.num_layers - 1) + [(net.padded_output_dim, net.hidden_dim)]
    out, off = [], 0
    for r, c in shapes:
        out.append(g[off:off + r * c].reshape(r, c)); off += r * c
    return out


def ff_model_matrices(model):
    """the flat FFMLP weights of a workload.make_model() dict as per-layer matrices (ffmlp/ffmlp.py:121-122: [64,32] + k [64,64] + [16,64]):
    (sigma net [64,32],[64,64],[16,64]; colour net [64,32],[64,64],[64,64],[16,64])"""
    def split(flat, n_hidden):
        shapes = [(64, 32)] + [(64, 64)] * (n_hidden - 1) + [(16, 64)]
        out, off = [], 0
        for r, c in shapes:
            out.append(np.asarray(flat[off:off + r * c], np.float32).reshape(r, c)); off += r * c
        assert off == flat.size
        return out
    return split(model["sigma_weights"], 2), split(model["color_weights"], 3)


def linear_field_from_model(model, dev):
    """ngp.field.NGPField (nn.Linear layers, float32) holding the numbers of a workload.make_model() dict: the FFMLP shapes 32-64-64-16 and
    32-64-64-64-16 as Linear stacks (the colour net's zero input column and its 13 unused output rows dropped, nerf/network_ff.py:67-74)."""
    import torch
    from ngp.field import NGPField
    sw, cw = ff_model_matrices(model)
    field = NGPField(bound=model["bound"], num_layers=3, num_layers_color=4).to(dev)
    cw = [cw[0][:, :31]] + cw[1:-1] + [cw[-1][:3]]
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(model["embeddings"]))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            assert tuple(layer.weight.shape) == w.shape, (layer.weight.shape, w.shape)
            layer.weight.copy_(torch.from_numpy(np.ascontiguousarray(w)))
    return field


# the frame kernel's workspace carve (render_fused.hip: RV_WS_COARSE, RV_WS_AREA; restated, the size is part of the C ABI): the header, and the end of the
# region of the coarse occupancy map, behind which two u32 per 64 rays hold the tile order
FRAME_WS_HEADER = 256
FRAME_WS_AREA = 256 + 48 * 1024


def render_frame(ren, o, d, width, *, tile_order=None, block_skip=None, occupied_box=None, dt_gamma=0.0, min_near=None, max_steps=1024,
                 bitfield=None, workspace_bytes=None, grid_size=None):
    """ngp_render_frame as NGPRenderer.render_fused calls it, through ctypes, with NaN-filled outputs and a 0xAB-filled workspace, so that a value the
    kernel did not write, or a workspace word it relied on without writing it, shows.  The three process-wide switches are set when given (0 / 1) and
    restored afterwards; `bitfield` replaces the renderer's (same cascades and grid size), `workspace_bytes` the size ngp_render_frame_workspace
    asks for, `min_near` and `grid_size` the renderer's.  Returns (outputs, workspace, return code); the outputs stay NaN / -1 when the call refuses."""
    import ctypes

    import ngp_hip as H
    import torch
    L = H.lib()
    N, dev = o.shape[0], o.device
    image = torch.full((N, 3), float("nan"), device=dev)
    depth = torch.full((N,), float("nan"), device=dev)
    weights_sum = torch.full((N,), float("nan"), device=dev)
    stats = torch.full((4,), -1, dtype=torch.int32, device=dev)
    ws_bytes = L.ngp_render_frame_workspace(N) if workspace_bytes is None else int(workspace_bytes)
    ws = torch.full((max(ws_bytes, 16),), 0xAB, dtype=torch.uint8, device=dev)
    bg = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    aabb = (ctypes.c_float * 6)(*[float(v) for v in ren._aabb().tolist()])
    f = ren.field.fused_state(ren.density_scale)
    bits = ren.density_bitfield if bitfield is None else bitfield
    assert bits.numel() == ren.density_bitfield.numel() and bits.dtype == torch.uint8 and bits.is_contiguous()
    setters = ((L.ngp_render_set_tile_order, tile_order), (L.ngp_render_set_block_skip, block_skip), (L.ngp_render_set_occupied_box, occupied_box))
    previous = [(fn, fn(int(value))) for fn, value in setters if value is not None]
    try:
        rc = L.ngp_render_frame(ctypes.byref(f), H.ptr(o), H.ptr(d), N, int(width), aabb, ren.min_near if min_near is None else float(min_near),
                                H.ptr(bits), ren.cascade, ren.grid_size if grid_size is None else int(grid_size), float(dt_gamma), int(max_steps), bg,
                                H.ptr(image), H.ptr(depth), H.ptr(weights_sum), H.ptr(stats), H.ptr(ws), ws_bytes, H.stream())
        torch.cuda.synchronize()
    finally:
        for fn, value in previous:
            fn(value)
    return dict(image=image, depth=depth, weights_sum=weights_sum, stats=stats), ws, rc


NULL = object()                      # render_default_frame(bitfield=NULL): a null pointer, where None means the renderer's own bitfield


def render_default_frame(ren, o, d, width, *, dt_gamma=0.0, min_near=None, max_steps=1024, bitfield=None, grid_size=None, workspace_bytes=None,
                         bg=1.0, camera=None):
    """ngp_nav_render_frame as NGPRenderer._render_default_frame calls it (the field struct and the prepared weights from the renderer's own holder),
    through ctypes, with NaN-filled image / depth / weights_sum, stats of -1 and a 0xAB-filled workspace, so that a value the kernel did not write, or a
    workspace word it relied on without writing it, shows.  `bitfield` replaces the renderer's (NULL: a null pointer), `workspace_bytes` the size
    ngp_nav_render_frame_workspace asks for (the tensor is exactly that long), `min_near` and `grid_size` the renderer's; `bg` a number or three.
    camera=(pose, intrinsics, H, W): ngp_nav_render_frame_camera instead, `o`, `d` and `width` unused (o gives the device).
    Returns (outputs, workspace, return code); the outputs stay NaN / -1 when the call refuses."""
    import ctypes

    import ngp_hip as H
    import torch
    L = H.lib()
    dev = o.device
    N = o.shape[0] if camera is None else int(camera[2]) * int(camera[3])
    image = torch.full((N, 3), float("nan"), device=dev)
    depth = torch.full((N,), float("nan"), device=dev)
    weights_sum = torch.full((N,), float("nan"), device=dev)
    stats = torch.full((4,), -1, dtype=torch.int32, device=dev)
    ws_bytes = int(L.ngp_nav_render_frame_workspace(N)) if workspace_bytes is None else int(workspace_bytes)
    ws = torch.full((max(ws_bytes, 16),), 0xAB, dtype=torch.uint8, device=dev)
    bg3 = (ctypes.c_float * 3)(*([float(bg)] * 3 if np.isscalar(bg) else [float(v) for v in bg]))
    aabb = (ctypes.c_float * 6)(*ren._aabb_host())
    bits = ren.density_bitfield if bitfield is None else bitfield
    if bits is NULL:
        bits = None
    else:
        assert bits.dtype == torch.uint8 and bits.is_contiguous()
    with torch.cuda.device(dev):
        st, prep = ren._default_frame_field("render_default_frame").struct()
        tail = (aabb, ren.min_near if min_near is None else float(min_near), H.ptr(bits), ren.cascade, ren.grid_size if grid_size is None else int(grid_size),
                float(dt_gamma), int(max_steps), bg3, H.ptr(image), H.ptr(depth), H.ptr(weights_sum), H.ptr(stats), H.ptr(ws), ws_bytes, H.stream())
        if camera is None:
            rc = L.ngp_nav_render_frame(ctypes.byref(st), H.ptr(prep), H.ptr(o), H.ptr(d), N, int(width), *tail)
        else:
            pose_h, intr_h = H.camera_args(camera[0], camera[1])
            rc = L.ngp_nav_render_frame_camera(ctypes.byref(st), H.ptr(prep), pose_h, intr_h, int(camera[2]), int(camera[3]), *tail)
        torch.cuda.synchronize()
    return dict(image=image, depth=depth, weights_sum=weights_sum, stats=stats), ws, rc
