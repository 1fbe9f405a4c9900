"""The frames of the default float32 field (csrc/nav_frame.hip) that tests/test_gpu_default_frame.py renders on the GPU and whose conditioning
tests/test_default_frame_host.py checks on the CPU: fields, rays, occupancy and the CPU reference, built once per process.

Field A: the hand-set nav model (workload.make_model(0, bound) table + workload.nav_weights(0)), as tests/test_gpu_nav_golden.py builds it.
Field B: a random NGPField: torch.manual_seed(11), embeddings uniform_(-0.5, 0.5), drawn on the CPU so that both test files see the same numbers.
Reference: oracle.render_oracle.render_single_march over oracle.callers_oracle.DefaultField, with sigma times density_scale."""
import functools

import numpy as np
import torch

BG = (0.2, 0.5, 0.9)


@functools.lru_cache(maxsize=None)
def field_arrays(which, bound):
    """(embeddings, offsets, per_level_scale, sigma layers, colour layers) of field "A" or "B" at `bound`, float32 numpy"""
    from ngp import workload as W
    if which == "A":
        model = W.make_model(0, bound=bound)
        sw, cw = W.nav_weights(0)
        return model["embeddings"], np.asarray(model["offsets"]), float(model["per_level_scale"]), sw, cw
    from ngp.field import NGPField
    torch.manual_seed(11)
    field = NGPField(bound=bound)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
    return (field.encoder.embeddings.detach().numpy().copy(), field.encoder.offsets.numpy().copy(), float(field.encoder.per_level_scale),
            [l.weight.detach().numpy().copy() for l in field.sigma_net], [l.weight.detach().numpy().copy() for l in field.color_net])


def oracle_field(which, bound, dtype=torch.float32):
    from oracle import callers_oracle as CO
    emb, offsets, pls, sw, cw = field_arrays(which, bound)
    return CO.DefaultField(emb, offsets, pls, sw, cw, bound, dtype=dtype)


def product_field(which, bound, dev):
    """ngp.field.NGPField on `dev` holding the same numbers"""
    from ngp.field import NGPField
    emb, _, _, sw, cw = field_arrays(which, bound)
    field = NGPField(bound=bound).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.copy_(torch.from_numpy(emb))
        for layer, w in zip(list(field.sigma_net) + list(field.color_net), sw + cw):
            layer.weight.copy_(torch.from_numpy(w))
    return field


def field_fn(orc, density_scale=1.0):
    """(xyzs, dirs) -> (sigma * density_scale, rgb), float32 numpy, evaluated in the oracle field's own precision"""
    def fn(x, d):
        with torch.no_grad():
            sigma, rgb = orc(torch.from_numpy(np.ascontiguousarray(x)).to(orc.dtype), torch.from_numpy(np.ascontiguousarray(d)).to(orc.dtype))
            sigma = sigma * torch.tensor(density_scale, dtype=orc.dtype)
        return sigma.numpy().astype(np.float32), rgb.numpy().astype(np.float32)
    return fn


@functools.lru_cache(maxsize=None)
def ring(bound):
    """(grid [C, 128^3], bitfield) of the ring scene: what NGPRenderer(density_thresh=10).load_density_grid(grid) packs"""
    from ngp import workload as W
    grid = W.density_grid(bound=bound)
    bitfield, _ = W.bitfield_from_grid(grid)
    return grid, bitfield


def orbit_rays(k, res_h, res_w=None, **pose_kw):
    from ngp import workload as W
    res_w = res_h if res_w is None else res_w
    return W.get_rays(W.orbit_pose(k, **pose_kw), W.intrinsics(res_h, res_w), res_h, res_w)


def _case(field, bound, rays, *, occupancy="ring", dt_gamma=0.0, max_steps=1024, density_scale=1.0, bg=1.0, image_width=0):
    return dict(field=field, bound=bound, rays=rays, occupancy=occupancy, dt_gamma=dt_gamma, max_steps=max_steps, density_scale=density_scale, bg=bg,
                image_width=image_width)


def _shuffled_subset():
    o, d = orbit_rays(6, 48)
    perm = np.random.default_rng(0).permutation(o.shape[0])[:2001]            # shuffled subset, not a multiple of 64
    return o[perm], d[perm]


def _tiny(n):
    o, d = orbit_rays(2, 48)
    pick = np.random.default_rng(n).permutation(o.shape[0])[:n]
    return o[pick], d[pick]


def _inside(name, res):
    import _frame_poses as FP
    return FP.rays(name, res)


def _blob_rays():
    from _util import camera_rays
    return camera_rays(24, radius=5.5, seed=3)


# name -> the case, lazily (rays are cheap, but the table should import without the package)
CASES = {
    "two_cascades": lambda: _case("A", 2.0, orbit_rays(2, 40), image_width=40),
    "one_cascade": lambda: _case("A", 1.0, orbit_rays(3, 40, radius=1.3, height=0.5), image_width=40),
    "dt_gamma_128": lambda: _case("A", 2.0, orbit_rays(2, 40), dt_gamma=1.0 / 128, image_width=40),
    "dt_gamma_32": lambda: _case("A", 2.0, orbit_rays(2, 40), dt_gamma=1.0 / 32, image_width=40),
    "sample_cap": lambda: _case("A", 2.0, orbit_rays(1, 32), occupancy="full", max_steps=64, image_width=32),
    "odd_count_rgb_background": lambda: _case("A", 2.0, _shuffled_subset(), bg=BG),
    "random_field": lambda: _case("B", 2.0, orbit_rays(2, 32), image_width=32),
    "random_field_scale_8": lambda: _case("B", 2.0, orbit_rays(2, 32), density_scale=8.0, image_width=32),
    "random_field_full_grid": lambda: _case("B", 2.0, orbit_rays(2, 32), occupancy="full", max_steps=128, image_width=32),
    "density_scale_2": lambda: _case("A", 2.0, orbit_rays(2, 32), density_scale=2.0, image_width=32),
    "three_cascades": lambda: _case("B", 4.0, _blob_rays(), occupancy="blobs"),
    "inside_centre": lambda: _case("A", 2.0, _inside("centre", 32), image_width=32),
    "inside_away": lambda: _case("A", 2.0, _inside("away", 32), image_width=32),
    "one_ray": lambda: _case("A", 2.0, _tiny(1)),
    "sixty_five_rays": lambda: _case("A", 2.0, _tiny(65)),
}
# the cases whose inputs' own sensitivity the host test bounds (the issue's cases 1-4, 9 and 10)
CONDITIONED = ("two_cascades", "one_cascade", "dt_gamma_128", "dt_gamma_32", "sample_cap", "random_field", "random_field_scale_8",
               "random_field_full_grid", "density_scale_2")


# The frames tests/test_gpu_default_frame_inside.py renders from INSIDE the ring scene (tests/_frame_poses.py), 33 x 33 (direction components of exactly
# 0.0) and 40 x 40 (8x8 tiles): field A from every pose at bound 2 (nested cascades) and 1.5 (not nested), from the centre at bound 3 (three cascades of
# half-widths 1, 2, 3), and field B with density_scale 8 from inside a pillar and inside the slab (rays that saturate within their first few samples).
INSIDE_SIZES = (33, 40)
INSIDE_BOUNDS = (2.0, 1.5)


def inside_name(pose, res, bound):
    return f"inside_{pose}_{res}_bound_{bound:g}"


def inside_sizes(pose, bound):
    """the two sizes a pose is rendered at.  lintel_top at bound 2 takes 32 x 32 for its even size: at 40 x 40 one ray's float32 transmittance
    crosses the 1e-4 stop one sample away from where the float64 field's does (tests/test_default_frame_host.py's condition on the inputs), so the
    frame would measure the inputs' rounding, not a kernel; 32 is a multiple of 8 as well and meets the condition."""
    return (33, 32) if (pose, bound) == ("lintel_top", 2.0) else INSIDE_SIZES


def _register_inside():
    import _frame_poses as FP
    names, empty = [], []
    for bound in INSIDE_BOUNDS:
        for pose in FP.NAMES:
            for res in inside_sizes(pose, bound):
                name = inside_name(pose, res, bound)
                CASES[name] = lambda pose=pose, res=res, bound=bound: _case("A", bound, _inside(pose, res), image_width=res)
                names.append(name)
                if pose in FP.NO_SAMPLES:
                    empty.append(name)
    CASES["inside_three_cascades"] = lambda: _case("A", 3.0, _inside("centre", 33), image_width=33)
    names.append("inside_three_cascades")
    for pose in ("in_solid", "slab_skim"):
        for res in INSIDE_SIZES:
            name = f"inside_{pose}_{res}_random_field_scale_8"
            CASES[name] = lambda pose=pose, res=res: _case("B", 2.0, _inside(pose, res), density_scale=8.0, image_width=res)
            names.append(name)
    return tuple(names), tuple(empty)


# CONDITIONED_INSIDE: held to the host test's bar like CONDITIONED; INSIDE_NO_SAMPLES: those of them whose frame has no sample at all (FP.NO_SAMPLES)
CONDITIONED_INSIDE, INSIDE_NO_SAMPLES = _register_inside()


def occupancy(case, oracle):
    """(grid or None, bitfield uint8 numpy, cascades) of a case; grid None = every bit set"""
    from ngp import workload as W
    cascades = W.cascade_count(case["bound"])
    if case["occupancy"] == "blobs":
        from _util import blob_bitfield
        bitfield, grid = blob_bitfield(oracle, cascades, 128, seed=4, n_blobs=30, bound=case["bound"])
        return grid, bitfield, cascades
    grid, bitfield = ring(case["bound"])
    if case["occupancy"] == "full":
        return None, np.full_like(bitfield, 255), cascades
    return grid, bitfield, cascades


def reference(name, oracle, dtype=torch.float32, field=None):
    """render_single_march of case `name` over the oracle's field in `dtype` (or over `field`, an oracle field of the caller's)"""
    from oracle import render_oracle as R
    case = CASES[name]()
    _, bitfield, cascades = occupancy(case, oracle)
    orc = field if field is not None else oracle_field(case["field"], case["bound"], dtype)
    o, d = case["rays"]
    bg = np.array(case["bg"], np.float32) if not np.isscalar(case["bg"]) else case["bg"]
    return R.render_single_march(field_fn(orc, case["density_scale"]), o, d, bitfield, case["bound"], cascades, dt_gamma=case["dt_gamma"],
                                 max_steps=case["max_steps"], bg_color=bg)


@functools.lru_cache(maxsize=None)
def _reference32(name):
    from oracle import ngp_oracle
    ngp_oracle.build()
    return reference(name, ngp_oracle)


def reference32(name):
    """the float32 reference of a case, computed once per process and shared (do not write to it)"""
    return _reference32(name)
