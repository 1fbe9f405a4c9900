"""GPU: every op that carves a workspace stays inside it and does not depend on what the workspace held before.

`ngp_hip.workspace` is replaced by one that hands out the middle n bytes of a buffer of n + 512 (offset 256, so the alignment the allocator
gives is kept).  Each op runs through its product wrapper twice, the whole buffer pre-filled with 0xAB and then with 0x00: both 256-byte
guards must be untouched, and the two runs' outputs must be the same bit for bit.  The shapes are the smallest that put more than one piece
of the layout and a partial last block into play (csrc/ngp_workspace.h; the layouts themselves are pinned by tests/test_workspace_host.py)."""
import importlib

import numpy as np
import pytest
import torch

importlib.import_module("nerf-navigation_amd")
pytestmark = pytest.mark.gpu

GUARD = 256


class GuardedWorkspaces:
    def __init__(self, fill):
        self.fill, self.buffers = fill, []

    def __call__(self, nbytes, device):
        n = max(int(nbytes), 16)
        buf = torch.full((n + 2 * GUARD,), self.fill, dtype=torch.uint8, device=device)
        assert buf.data_ptr() % 256 == 0
        self.buffers.append(buf)
        return buf[GUARD:GUARD + n]

    def check(self, at_least):
        assert len(self.buffers) >= at_least, f"{len(self.buffers)} workspaces were allocated through ngp_hip.workspace, expected {at_least}"
        for k, buf in enumerate(self.buffers):
            assert bool((buf[:GUARD] == self.fill).all()), f"workspace {k} ({buf.numel() - 2 * GUARD} bytes): written in front of it"
            assert bool((buf[-GUARD:] == self.fill).all()), f"workspace {k} ({buf.numel() - 2 * GUARD} bytes): written behind it"


@pytest.fixture
def guarded(monkeypatch, dev):
    """guarded(op, at_least): runs op() under both fills, checks the guards of the (at least `at_least`) workspaces it allocated and that its
    outputs (a list of tensors) do not depend on the fill; returns the outputs"""
    import ngp_hip

    def run(op, at_least=1):
        outs = []
        for fill in (0xAB, 0x00):
            spaces = GuardedWorkspaces(fill)
            monkeypatch.setattr(ngp_hip, "workspace", spaces)
            result = [r.detach().clone() for r in op()]
            torch.cuda.synchronize()
            spaces.check(at_least)
            outs.append(result)
        assert len(outs[0]) == len(outs[1]) > 0
        for k, (a, b) in enumerate(zip(*outs)):
            assert a.shape == b.shape and a.dtype == b.dtype and a.numel() > 0, k
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"output {k} depends on what the workspace held"
        return outs[0]
    return run


@pytest.fixture(scope="module")
def scene(dev):
    """the hand-set ring scene: the half-precision field of the frame kernel and of the training step, and its occupancy grid"""
    from ngp import workload as W
    from ngp.field import NGPFieldFF
    return W, NGPFieldFF(bound=W.BOUND).to(dev).load_arrays(W.make_model(0))


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_training_march(guarded, dev):
    """65 rays: two 64-ray blocks, the last with one ray; 16 steps, one cascade of 16^3; the `_full` size, so the t buffer behind the coarse map exists"""
    import raymarching
    from _util import camera_rays
    N, max_steps, C, H, bound = 65, 16, 1, 16, 1.0
    o, d = camera_rays(8, radius=2.2, seed=3)
    o, d = t(o[:N], dev), t(d[:N], dev)
    bits = t(np.random.default_rng(5).integers(0, 256, C * H ** 3 // 8, dtype=np.uint8), dev)
    nears, fars = raymarching.near_far_from_aabb(o, d, t(np.array([-bound] * 3 + [bound] * 3, np.float32), dev), 0.05)

    def op():
        counter = torch.zeros(2, dtype=torch.int32, device=dev)
        x, dd, l, rays = raymarching.march_rays_train(o, d, bound, bits, C, H, nears, fars, counter, -1, False, -1, True, 0.0, max_steps)
        return [x, dd, l, rays, counter]
    x, _, _, rays, counter = guarded(op)
    assert int(counter[0]) == x.shape[0] == int(rays[:, 2].sum()) > 64


def test_compact_alive(guarded, dev):
    """257 entries: two 256-thread blocks, the last with one entry"""
    import raymarching
    rng = np.random.default_rng(1)
    alive = np.where(rng.random(257) < 0.4, -1, rng.integers(0, 1000, 257)).astype(np.int32)
    alive[-1] = 7
    ta = t(alive, dev)

    def op():
        packed, cnt = raymarching.compact_alive(ta, 257)
        return [packed[:int(cnt.item())], cnt]
    packed, cnt = guarded(op)
    assert np.array_equal(packed.cpu().numpy(), alive[alive >= 0]) and int(cnt) == int((alive >= 0).sum()) > 128


def test_update_extra_state(guarded, dev, scene):
    """two cascades of 8^3 = four block sums: a full sweep, then a partial one (occupied-cell lists, n_occ and thresh at the unaligned tail)"""
    from ngp.render import NGPRenderer
    W, field = scene

    def op():
        ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0, grid_size=8).to(dev).train()
        assert ren.cascade == 2
        with torch.autocast("cuda", dtype=torch.float16):       # (the training loop's setting: the density query then takes ngp_field_density)
            ren.update_extra_state()
            full = ren.density_grid.clone()
            ren.iter_density = 16
            ren.update_extra_state()
        return [full, ren.density_grid, ren.density_bitfield, ren._mean_dev]
    full, grid, _, _ = guarded(op, at_least=3)                # the grid workspace and a density-query workspace per sweep
    assert float(full.max()) > 0 and not torch.equal(full, grid)


def test_binned_scatter(guarded, dev):
    """1025 samples: two chunks of 1024, the second with one sample; two levels"""
    from gridencoder import GridEncoder
    from gridencoder import grid as G
    B = 1025
    enc = GridEncoder(num_levels=2, log2_hashmap_size=12, desired_resolution=32).to(dev)
    rng = np.random.default_rng(4)
    x = t(rng.uniform(0, 1, (B, 3)).astype(np.float32), dev)
    grad = t((rng.normal(size=(2, B, 2)) * 0.1).astype(np.float16), dev)

    def op():
        return [G.table_gradient_binned(grad, x, enc.offsets, B, 2, float(np.log2(enc.per_level_scale)), enc.base_resolution, enc.gridtype_id, enc.align_corners)]
    out, = guarded(op)
    assert out.shape == (int(enc.offsets[-1]), 2) and float(out.abs().max()) > 0


def test_field_train_forward_and_backward(guarded, dev, scene):
    """33 samples: two 32-sample pairs, the second with one sample; the live list on (some samples get no gradient)"""
    W, field = scene
    g = torch.Generator(device="cpu").manual_seed(33)
    x = ((torch.rand(33, 3, generator=g) * 2 - 1) * W.BOUND).to(dev)
    d = torch.nn.functional.normalize(torch.randn(33, 3, generator=g), dim=-1).to(dev)
    gs, gc = torch.randn(33, generator=g).to(dev), torch.randn(33, 3, generator=g).to(dev)
    gs[5:9], gc[5:9] = 0.0, 0.0

    def op():
        field.train()
        field.fused_training = True
        for p in field.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.float16):
            sig, rgb = field(x, d)
            loss = (sig * gs).sum() + (rgb.float() * gc).sum()
        loss.backward()
        return [sig, rgb, field.encoder.embeddings.grad, field.sigma_net.weights.grad, field.color_net.weights.grad]
    out = guarded(op, at_least=3)                             # kept features, backward workspace, scatter workspace
    assert all(bool(torch.isfinite(o.float()).all()) for o in out) and float(out[2].abs().max()) > 0


def test_marching_cubes(guarded, dev):
    """17^3 = 4913 lattice points: two spans of 4096, the second partial; count and emit share the workspace"""
    from ngp import mesh
    u = torch.rand(17, 17, 17, generator=torch.Generator().manual_seed(2)).to(dev)
    verts, tris = guarded(lambda: list(mesh.marching_cubes(u, 0.5)))
    assert verts.shape[0] > 1000 and tris.shape[0] > 1000 and 0 <= int(tris.min()) and int(tris.max()) < verts.shape[0]


def test_plan_epochs(guarded, dev, scene):
    """R = 2 rows of states, B = 3 body points, one epoch: 15 points, each piece of the workspace shorter than its 256-byte slot"""
    from ngp import nav
    from ngp.field import NGPField
    from ngp.render import NGPRenderer
    from oracle import nav_oracle as NO
    W, _ = scene
    model = W.make_model(0)
    sw, cw = W.nav_weights(0)
    field = NGPField(bound=W.BOUND).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(model["embeddings"]))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            layer.weight.copy_(torch.from_numpy(w))
    ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=False).to(dev).eval()
    cfg = {"T_final": 2., "steps": 4, "lr": 0.001, "epochs_init": 1, "epochs_update": 1, "fade_out_epoch": 0, "fade_out_sharpness": 10, "mass": 1.,
           "I": torch.eye(3), "g": 10., "body": np.array([[-0.05, 0.05], [-0.05, 0.05], [-0.02, 0.02]]), "nbins": [3, 1, 1]}

    def op():
        queries = nav.NativeNavQueries(ren, (20.0, 20.0, 4.0, 4.0), 8, 8, num_steps=8)
        plan = nav.NativePlanner(NO.state18([0.39, -0.67, 0.2]), NO.state18([-0.4, 0.55, 0.16]), cfg, queries)
        assert plan.R == 2 and plan.robot_body.shape[0] == 3
        adam, losses, per_state = plan.new_adam_state(), torch.empty(1, device=dev), torch.empty(2, plan.S, device=dev)
        plan.run_epochs(0, 1, adam, losses=losses, per_state=per_state)
        return [plan.states, plan.initial_accel, adam, losses, per_state]
    out = guarded(op, at_least=2)                             # the prepared weights and the planner's workspace
    assert all(bool(torch.isfinite(o).all()) for o in out)


def test_render_fused_cameras(guarded, dev, scene):
    """two 8x8 frames in one launch: the cameras travel behind the tile-order area of the frame workspace"""
    from ngp.render import NGPRenderer
    W, field = scene
    ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
    ren.load_density_grid(W.density_grid())
    poses = np.stack([W.orbit_pose(k, 5) for k in range(2)])

    def op():
        out = ren.render_fused_cameras(poses, W.intrinsics(8, 8), 8, 8, bg_color=(0.2, 0.4, 0.9))
        return [out["image"], out["depth"].nan_to_num(), out["weights_sum"], out["stats"]]
    image, _, weights_sum, stats = guarded(op)
    assert image.shape == (2, 8, 8, 3) and float(weights_sum.max()) > 0.5 and int(stats[0]) > 100
