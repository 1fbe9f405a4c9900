"""GPU: the float32 frame kernel (nav_frame.hip: ngp_nav_render_frame, ngp_nav_render_frame_camera) with the camera INSIDE the scene, on every grid
and bound its march has a branch for, and every route its launcher can take.  It is the kernel the navigation loop's sensor calls from the vehicle's own
pose, among the pillars; tests/test_gpu_default_frame.py looks at the scene from an orbit, with a 128^3 grid and min_near 0.2 only.

The poses are tests/_frame_poses.py's (in a pillar, in the ground slab, under a lintel, just inside the AABB's wall, looking away), at 33 x 33 (the centre
column and row have direction components of exactly 0.0: 1 / d = inf in the slab test and in cell_exit) and 40 x 40 (8x8 tiles).  The checker is the CPU
oracle's cell-by-cell march (oracle.render_oracle.render_single_march) over oracle.callers_oracle.DefaultField in float32; the bars are
test_gpu_default_frame.check's, unchanged, and the real-field frames are held to the float64 oracle by tests/test_default_frame_host.py (5e-5).

  what the kernel branches on                                  where it is run
  zero direction components (ngp_near_far_inline, 1 / V.dx)    33 x 33 in parts a, b, c
  a march that starts in an occupied cell / at t = 0           in_solid, slab_* with min_near 0.05 and 0 (part a); ngp_lattice_jump's t = 0 branch
  ngp_advance on every empty cell, dt_gamma 0 and 1/128        part a (exact sample counts)
  2 nested cascades | 2 not nested (rbound = 1 / 1.5) | 1      bounds 2.0, 1.5, 0.75 in part a; 2.0 and 1.5 in part b
  3 cascades of half-widths 1, 2, 3 (dt_max from 1 << 2)       test_real_field_three_cascades
  early termination (T < 1e-4) within a round's three samples  field B with density_scale 8 from in_solid and slab_skim; part c
  grids of 2^3 .. 64^3 (hHf, r2H for any power of two)         test_other_grids_against_the_oracle
  C H^3 = 2^25: the binary32 cell index rounds; last_bit       test_grid_of_256_against_the_oracle
  no sample at all                                             away, out_between, behind in parts a, b
  stats[3] >= stats[0]                                         check(), every case
  launcher: image_width 0 | 33 (no tiles) | 40 (tiles)         test_every_route_gives_the_same_frame
  launcher: bitfield at a 4-byte offset, workspace exact / +4K test_every_route_gives_the_same_frame
  launcher: the camera form, 33 x 33 included                  test_camera_gives_the_frame_of_rays_in_memory
  two launches, lanes that finish at very different times      test_repeatable_from_inside_the_slab
  refused: H 48, 96, 127; workspace one byte short;            test_refusals_leave_every_output_untouched
           max_steps 0; null bitfield; C H^3 not whole bytes   test_a_grid_of_fewer_bits_than_a_byte_is_refused (both frame kernels)

Measured maxima on an MI355X over the 447 frames checked here (check() prints each case's figures before it asserts; run with -s): image 3.6e-7,
weights_sum 1.8e-7, depth 1.9e-3 of its per-ray bound; stats[0] equal to the oracle's sample count in every one of them, the real-field frames
included; the sensor's two frames (tests/test_gpu_agent.py): image 1.2e-7, weights_sum 0, depth 4.1e-4 of its bound.  The bars are check()'s.

What a scratch build of nav_frame.hip with one line changed does to this file (each run once, then reverted):
  no clamp of the cell index to last_bit          passes: by construction no ray of test_grid_of_256_against_the_oracle reaches the one cell
                                                  whose index rounds past the end, and the oracle could not be compared there (it does not clamp)
  near = min_near whatever the box                36 cases of test_constant_density_sample_counts (every eye outside the box: corner at bounds 1.5 and
                                                  0.75; slab_skim, slab_out, slab_edge, behind at 0.75) and test_real_field_from_inside[corner-1.5] fail
  t += dt in place of the step to cell_exit       8 cases of test_constant_density_sample_counts fail (slab_skim, slab_out with dt_gamma 1/128).  The
                                                  two marches visit the same lattice of points and differ only where rounding puts a lattice point
                                                  on the other side of a cell's exit, which the exact counts along the slab's long runs notice
  lds_ray of odd lanes holds ray 0, not the ray   27 cases fail: every real-field test (the colour network gets another ray's direction).  (Leaving
                                                  the word unwritten would make the evaluating lane read whatever the LDS held as a ray index, an
                                                  out-of-bounds read when the rays are in memory: not something to run.)
"""
import functools

import numpy as np
import pytest
import torch

import _default_frame_cases as DC
import _frame_poses as FP
from _frame_checks import _same_count_same_weight, _written
from _util import NULL, blob_bitfield, blob_bitfield_boxed, render_default_frame, render_frame
from oracle import render_oracle as R
from test_gpu_default_frame import check, field_on, renderer, t
from test_gpu_frame_inside import _differences

pytestmark = pytest.mark.gpu

ODD, EVEN = 33, 40                  # exact-zero direction components | a multiple of 8: the rays are handed out in 8x8 tiles
BOUNDS = (2.0, 1.5, 0.75)           # 2 nested cascades | 2 cascades that are not nested | 1 cascade narrower than 1
EINVAL, EWORKSPACE = -1, -3         # include/ngp_hip.h


@pytest.fixture(scope="module")
def constant(dev):
    """bound -> renderer of the ring scene's grid over a default NGPField whose networks are all zero, density_scale = FP.DENSITY: sigma = exp(0) *
    FP.DENSITY and rgb = sigmoid(0) = 0.5 everywhere (FP.constant_field), so no ray saturates and every marched sample is composited"""
    from ngp import workload as W
    from ngp.field import NGPField
    from ngp.render import NGPRenderer
    made = {}

    def get(bound):
        if bound not in made:
            field = NGPField(bound=bound).to(dev)
            with torch.no_grad():
                for layer in list(field.sigma_net) + list(field.color_net):
                    layer.weight.zero_()
            ren = NGPRenderer(field, bound=bound, cuda_ray=True, density_scale=FP.DENSITY, density_thresh=10.0).to(dev).eval()
            ren.load_density_grid(W.density_grid(bound=bound))
            bitfield, cascade = FP.scene(bound)
            assert ren.cascade == cascade and np.array_equal(ren.density_bitfield.cpu().numpy(), bitfield)
            made[bound] = ren
        return made[bound]
    return get


@pytest.fixture(scope="module")
def real(dev, oracle):
    """case -> renderer of the case's field, bound and density_scale on the ring scene's grid (test_gpu_default_frame.renderer), one per combination"""
    made = {}

    def get(case):
        key = (case["field"], case["bound"], case["density_scale"], case["occupancy"])
        if key not in made:
            made[key] = renderer(dev, oracle, case)
            assert np.array_equal(made[key].density_bitfield.cpu().numpy(), FP.scene(case["bound"])[0])
        return made[key]
    return get


def _frame(ren, o, d, width, dev, **kw):
    import ngp_hip
    out, ws, rc = render_default_frame(ren, t(o, dev) if isinstance(o, np.ndarray) else o, t(d, dev) if isinstance(d, np.ndarray) else d, width, **kw)
    ngp_hip.check(rc, "nav_render_frame")
    return out, ws


# ------------------------------------------------------------------------------------------------------------------------------------------------
# part a: exact sample counts from inside, constant density
# ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("min_near", (0.2, 0.05, 0.0))
@pytest.mark.parametrize("dt_gamma", (0.0, 1.0 / 128))
@pytest.mark.parametrize("name", FP.NAMES)
def test_constant_density_sample_counts(oracle, dev, constant, name, dt_gamma, min_near, bound):
    """Conditions, not tolerances: the frame's composited samples, its capped rays (none) and its rays with samples are the oracle's exactly, the
    evaluated samples are no fewer; depth is finite exactly where the oracle's is; every element is written; with a constant step (dt_gamma 0) rays
    with equal counts in the oracle have bit-equal weights_sum, more samples strictly more, none exactly 0.  With dt_gamma > 0 the step differs from
    ray to ray, so the per-ray argument does not apply: the totals and check()'s bars do.  The reference is the one test_gpu_frame_inside.py uses
    (FP.reference_constant: shared when both files run in one process), first checked to be inside what makes this valid."""
    ren = constant(bound)
    for res in (ODD, EVEN):
        what = f"{name} {res}x{res} bound {bound} min_near {min_near} dt_gamma {dt_gamma:.4f}"
        o, d = FP.rays(name, res)
        ref = FP.reference_constant(name, res, bound, min_near=min_near, dt_gamma=dt_gamma)
        FP.check_reference_is_clean(ref, bound)
        out, _ = _frame(ren, o, d, res, dev, dt_gamma=dt_gamma, min_near=min_near)
        _written(out, what)
        stats = check(out, ref, DC._case("constant", bound, (o, d), dt_gamma=dt_gamma), oracle, what, min_near=min_near)
        hit = int((ref["consumed"] > 0).sum())
        assert int(stats[0]) == ref["samples"] and int(stats[1]) == 0 and int(stats[2]) == hit and int(stats[3]) >= int(stats[0]), (what, stats, ref["samples"], hit)
        assert np.array_equal(np.isfinite(out["depth"].cpu().numpy()), np.isfinite(ref["depth"])), what
        if dt_gamma == 0.0:
            _same_count_same_weight(out["weights_sum"].cpu().numpy(), ref["marched"], what)
        else:
            assert bool((out["weights_sum"].cpu().numpy()[ref["marched"] == 0] == 0).all()), what


# ------------------------------------------------------------------------------------------------------------------------------------------------
# part b: the real field from inside
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _real_case(real, oracle, dev, cname, pose):
    case = DC.CASES[cname]()
    ref = DC.reference32(cname)
    o, d = case["rays"]
    assert (ref["samples"] == 0) == (pose in FP.NO_SAMPLES), (cname, ref["samples"])
    out, _ = _frame(real(case), o, d, case["image_width"], dev)
    _written(out, cname)
    stats = check(out, ref, case, oracle, cname)
    assert int(stats[1]) == 0, (cname, stats)
    if pose in FP.NO_SAMPLES:
        assert int(stats[0]) == 0 and int(stats[2]) == 0 and int(stats[3]) == 0, (cname, stats)
    return stats, ref


@pytest.mark.parametrize("bound", DC.INSIDE_BOUNDS)
@pytest.mark.parametrize("name", FP.NAMES)
def test_real_field_from_inside(oracle, dev, real, name, bound):
    """field A (the hand-set nav model: rays that saturate inside the solids) at bound 2 (nested cascades) and 1.5 (not nested) from every pose, at
    the sizes DC.inside_sizes gives, against the oracle's single march over the float32 DefaultField; check()'s bars"""
    for res in DC.inside_sizes(name, bound):
        _real_case(real, oracle, dev, DC.inside_name(name, res, bound), name)


def test_real_field_three_cascades(oracle, dev, real):
    """bound 3.0: three cascades of half-widths 1, 2 and 3; the outer cascade's cells are not twice the middle one's, dt_max comes from 1 << 2"""
    assert FP.scene(3.0)[1] == 3
    stats, ref = _real_case(real, oracle, dev, "inside_three_cascades", "centre")
    assert ref["samples"] > 1000


@pytest.mark.parametrize("name", ("in_solid", "slab_skim"))
def test_dense_random_field_from_inside_a_solid(oracle, dev, real, name):
    """field B (random) with density_scale 8 from inside a pillar and inside the slab.  Along the slab rays saturate: a ray's round of three marched
    samples is cut by the T < 1e-4 stop, and what it marched behind that sample is evaluated (stats[3]) but not composited (stats[0]).  From inside
    the pillar this field saturates no ray (the reference says so): those are runs of dozens of samples that start in the march's first cell."""
    for res in DC.INSIDE_SIZES:
        stats, ref = _real_case(real, oracle, dev, f"inside_{name}_{res}_random_field_scale_8", name)
        cut = int((ref["consumed"] < ref["marched"]).sum())
        print(f"{name} {res}: {cut} rays of the reference are cut short by saturation")
        if name == "slab_skim":
            assert cut > 0 and int(stats[3]) > int(stats[0]), (cut, stats)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# part c: other grids
# ------------------------------------------------------------------------------------------------------------------------------------------------
GRID_SCALE = 8.0                    # field B saturates no ray of these frames at density_scale 1 (the reference says so); at 8 it does


def _grid_renderer(dev, grid_h, bitfield):
    """field B, two cascades of grid_h^3 cells holding the oracle's own bits (oracle.packbits)"""
    from ngp.render import NGPRenderer
    ren = NGPRenderer(field_on(dev, "B", 2.0), bound=2.0, cuda_ray=True, density_thresh=0.5, density_scale=GRID_SCALE, grid_size=grid_h).to(dev).eval()
    assert ren.cascade == 2 and ren.density_bitfield.numel() == bitfield.size
    ren.density_bitfield.copy_(t(bitfield, dev))
    return ren


def _grid_reference(o, d, bitfield, grid_h, max_steps=1024):
    return R.render_single_march(DC.field_fn(DC.oracle_field("B", 2.0), GRID_SCALE), o, d, bitfield, 2.0, 2, H=grid_h, max_steps=max_steps)


@pytest.mark.parametrize("grid_h", [2, 4, 8, 16, 32, 64])
def test_other_grids_against_the_oracle(oracle, dev, grid_h):
    """two cascades of 2^3 .. 64^3 cells (the scalings by H in their one-multiply forms hHf = H / 2 and r2H = 2 / H), blobs, from inside the ring
    scene's pillar position at 33 x 33; check()'s bars.  2^3 is the smallest grid whose cascades are whole bytes: oracle.packbits and the oracle's
    march take it as any other."""
    bitfield, grid = blob_bitfield(oracle, 2, grid_h, seed=2, n_blobs=40, bound=2.0)
    assert bitfield.size == 2 * grid_h ** 3 // 8 and 0 < int(grid.sum()) < grid.size
    o, d = FP.rays("in_solid", ODD)
    ref = _grid_reference(o, d, bitfield, grid_h)
    assert ref["samples"] > 500 and int((ref["consumed"] < ref["marched"]).sum()) > 0             # rays end in these cells, some of them early
    case = DC._case("B", 2.0, (o, d), density_scale=GRID_SCALE)
    out, _ = _frame(_grid_renderer(dev, grid_h, bitfield), o, d, ODD, dev)
    _written(out, f"H {grid_h}")
    stats = check(out, ref, case, oracle, f"H {grid_h}")
    assert int(stats[1]) == 0 and int(stats[0]) > 500


@functools.lru_cache(maxsize=None)
def _blobs_256():
    """the blobs of test_other_grids_against_the_oracle on 256^3 cells (blob_bitfield_boxed: shown here to be blob_bitfield's bits at 16^3 and 64^3)"""
    from oracle import ngp_oracle
    for grid_h in (16, 64):
        assert np.array_equal(blob_bitfield_boxed(ngp_oracle, 2, grid_h, seed=2, n_blobs=40, bound=2.0),
                              blob_bitfield(ngp_oracle, 2, grid_h, seed=2, n_blobs=40, bound=2.0)[0])
    return blob_bitfield_boxed(ngp_oracle, 2, 256, seed=2, n_blobs=40, bound=2.0)


@pytest.mark.parametrize("occupancy", ("blobs", "full"))
def test_grid_of_256_against_the_oracle(oracle, dev, occupancy):
    """two cascades of 256^3: C H^3 = 2^25, so the reference's cell index, formed in binary32 (raymarching.cu:783-784, oracle/ngp_oracle.c:363),
    rounds to an even number in cascade 1 -- the kernel and the oracle read the same, neighbouring, bit.  The one index that rounds past the end is
    2^25 - 1, cascade 1's cell (255, 255, 255) at the (+2, +2, +2) corner: the kernel clamps it to the last bit, the oracle does not, so the rays
    (from the scene's centre along -x) are first shown to leave the volume nowhere near that corner.  The same blobs as the smaller grids, and a
    bitfield of all ones with max_steps 128 (every probe is a sample, in both cascades)."""
    from ngp import workload as W
    grid_h = 256
    o, d = W.get_rays(W.look_pose(FP.POSES["centre"][0], (-1.0, 0.0, 0.0)), W.intrinsics(ODD, ODD), ODD, ODD)
    assert int((d == 0).sum()) == 2 * ODD
    nears, fars = oracle.near_far_from_aabb(o, d, np.array([-2.0] * 3 + [2.0] * 3, np.float32), 0.2)
    leaves = o + fars[:, None] * d
    cell = 4.0 / grid_h                                                     # a cell of the outer cascade
    assert np.isfinite(leaves).all() and float(np.min(np.max(np.abs(leaves - 2.0), axis=1))) > 2 * cell
    assert float(np.max(o + nears[:, None] * d)) < 2.0 - 2 * cell         # ... and the march starts nowhere near it either
    if occupancy == "blobs":
        bitfield, max_steps = _blobs_256(), 1024
    else:
        bitfield, max_steps = np.full(2 * grid_h ** 3 // 8, 255, np.uint8), 128
    assert bitfield.size * 8 == 1 << 25
    ref = _grid_reference(o, d, bitfield, grid_h, max_steps=max_steps)
    assert ref["samples"] > 500
    case = DC._case("B", 2.0, (o, d), density_scale=GRID_SCALE, max_steps=max_steps)
    out, _ = _frame(_grid_renderer(dev, grid_h, bitfield), o, d, ODD, dev, max_steps=max_steps)
    _written(out, f"H 256 {occupancy}")
    check(out, ref, case, oracle, f"H 256 {occupancy}")


# ------------------------------------------------------------------------------------------------------------------------------------------------
# part d: routes that must not change a bit
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _route_rays(name, res):
    from ngp import workload as W
    if name == "orbit":
        return W.get_rays(W.orbit_pose(1), W.intrinsics(res, res), res, res)
    return FP.rays(name, res)


def _kind(constant, real, kind):
    return constant(2.0) if kind == "constant" else real(DC._case("A", 2.0, None))


def _unwritten(out, label):
    return [f"{label}: {key}: {int(torch.isnan(out[key]).sum())} values were not written" for key in ("image", "depth", "weights_sum")
            if bool(torch.isnan(out[key]).any())]


@pytest.mark.parametrize("name", ("centre", "in_solid", "away", "orbit"))
@pytest.mark.parametrize("kind", ("constant", "real"))
def test_every_route_gives_the_same_frame(dev, constant, real, kind, name):
    """include/ngp_hip.h: "results do not depend on it, bit for bit" (image_width), and nothing in the kernel reads the bitfield wider than a byte
    or the workspace beyond its header: every route gives the frame of the default call (image_width = the image's width, the renderer's own
    bitfield, a workspace of exactly the size asked for).  All differences are collected before the test fails."""
    import ngp_hip
    L = ngp_hip.lib()
    ren = _kind(constant, real, kind)
    n_bits = ren.density_bitfield.numel()
    holder = torch.zeros(n_bits + 16, dtype=torch.uint8, device=dev)
    shifted = holder[4:4 + n_bits]
    shifted.copy_(ren.density_bitfield)
    assert ren.density_bitfield.data_ptr() % 8 == 0 and shifted.data_ptr() % 8 == 4 and torch.equal(shifted, ren.density_bitfield)
    failures = []
    for res in (EVEN, ODD):
        N = res * res
        need = int(L.ngp_nav_render_frame_workspace(N))
        o, d = _route_rays(name, res)
        o, d = t(o, dev), t(d, dev)
        base, ws = _frame(ren, o, d, res, dev)
        _written(base, f"{name} {res} default")
        assert not bool(torch.isnan(base["depth"]).any())                  # every eye lies inside the AABB: every depth is a number
        assert ws.numel() == need and bool((ws[4:] == 0).all())            # the header was zeroed; only its first word, the queue's head, counts up
        routes = {
            "image_width 0": dict(width=0),
            "bitfield at a 4-byte offset": dict(bitfield=shifted),
            "workspace of exactly the size asked for": dict(workspace_bytes=need),
            "workspace of 4 KiB more": dict(workspace_bytes=need + 4096),
        }
        for route, kw in routes.items():
            kw = dict(kw)
            out, ws_r = _frame(ren, o, d, kw.pop("width", res), dev, **kw)
            failures += _unwritten(out, f"{res}x{res} {route}")
            failures += [f"{res}x{res} {route}: {line}" for line in _differences(out, base)]
            if ws_r.numel() > need and not bool((ws_r[need:] == 0xAB).all()):
                failures.append(f"{res}x{res} {route}: the workspace was written beyond the {need} bytes asked for")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ("constant", "real"))
def test_camera_gives_the_frame_of_rays_in_memory(dev, constant, real, kind):
    """ngp_nav_render_frame_camera forms the rays inside the refill: bit for bit the frame of the same camera's rays in memory (ngp_get_rays) given
    to ngp_nav_render_frame, from a corner of the volume, the scene's centre, inside a pillar and looking away -- 33 x 33 included, where the camera's
    centre pixel has x_cam = y_cam = 0"""
    from ngp import workload as W
    from ngp.nav import get_rays_native
    ren = _kind(constant, real, kind)
    failures = []
    total = 0
    for res in (EVEN, ODD):
        intr = W.intrinsics(res, res)
        for name in ("corner", "centre", "in_solid", "away"):
            pose = FP.pose(name)
            o, d = get_rays_native(pose.tolist(), intr, res, res, device=dev)
            o_np, d_np = FP.rays(name, res)
            assert np.array_equal(o.cpu().numpy(), o_np) and float(np.max(np.abs(d.cpu().numpy() - d_np))) < 1e-6
            base, _ = _frame(ren, o, d, res, dev)
            _written(base, f"{name} {res} rays in memory")
            import ngp_hip
            cam, _, rc = render_default_frame(ren, o, d, res, camera=(pose, intr, res, res))
            ngp_hip.check(rc, "nav_render_frame_camera")
            failures += _unwritten(cam, f"{res}x{res} {name} camera")
            failures += [f"{res}x{res} {name} camera: {line}" for line in _differences(cam, base)]
            assert (int(base["stats"][0]) == 0) == (name == "away")
            total += int(base["stats"][0])
    assert total > 1000
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ("constant", "real"))
def test_repeatable_from_inside_the_slab(dev, constant, real, kind):
    """no float atomics on the data path and no dependence on which lane or workgroup draws which ray: two launches from slab_skim (hundreds of
    samples on some rays, a handful on others: lanes finish at very different times and refill from the queue in another order) are bit-identical"""
    ren = _kind(constant, real, kind)
    for res in (EVEN, ODD):
        o, d = FP.rays("slab_skim", res)
        o, d = t(o, dev), t(d, dev)
        a, _ = _frame(ren, o, d, res, dev, min_near=0.0)
        b, _ = _frame(ren, o, d, res, dev, min_near=0.0)
        _written(a, f"slab_skim {res}")
        assert _differences(a, b) == [] and int(a["stats"][2]) == res * res and int(a["stats"][0]) > 1000, a["stats"]

# ------------------------------------------------------------------------------------------------------------------------------------------------
# part e: refusals
# ------------------------------------------------------------------------------------------------------------------------------------------------
def _untouched(out):
    return (bool(torch.isnan(out["image"]).all()) and bool(torch.isnan(out["depth"]).all()) and bool(torch.isnan(out["weights_sum"]).all())
            and bool((out["stats"] == -1).all()))


def test_refusals_leave_every_output_untouched(dev, constant):
    """every refusal comes before anything reaches the device (include/ngp_hip.h): the error code, outputs still NaN / -1 -- stats included, which a
    launch would zero first -- and the reason named in ngp_last_error.  A grid size that is not a power of two would be read past its end (Morton
    index: H = 48, cell (47, 47, 47) has index 2^18 - 1 > 48^3); the bitfield passed is the 2 x 128^3 one, larger than any index these sizes form."""
    import ngp_hip
    L = ngp_hip.lib()
    ren = constant(2.0)
    o, d = FP.rays("centre", ODD)
    o, d = t(o, dev), t(d, dev)
    need = int(L.ngp_nav_render_frame_workspace(ODD * ODD))
    refusals = [(dict(grid_size=48), EINVAL, b"power of two"), (dict(grid_size=96), EINVAL, b"power of two"), (dict(grid_size=127), EINVAL, b"power of two"),
                (dict(workspace_bytes=need - 1), EWORKSPACE, b"workspace"), (dict(max_steps=0), EINVAL, b"max_steps"), (dict(bitfield=NULL), EINVAL, b"null")]
    for kw, code, reason in refusals:
        for camera in (None, (FP.pose("centre"), [50.0, 50.0, ODD / 2, ODD / 2], ODD, ODD)):
            out, ws, rc = render_default_frame(ren, o, d, ODD, camera=camera, **kw)
            message = L.ngp_last_error()
            assert rc == code and _untouched(out) and bool((ws == 0xAB).all()), (kw, rc, message)
            assert reason in message and message.startswith(b"nav_render_frame_camera:" if camera else b"nav_render_frame:"), (kw, message)
    out, _ = _frame(ren, o, d, ODD, dev)                                   # and the same arguments without the fault render
    _written(out, "after the refusals")


def test_a_grid_of_fewer_bits_than_a_byte_is_refused(dev, constant):
    """H = 1 with two cascades is a bitfield of 2 bits: C H^3 / 8 rounds to no byte at all.  Both frame launchers refuse a grid whose C H^3 is not a
    multiple of 8 before anything is launched (H = 2 is whole bytes for every C and is rendered in test_other_grids_against_the_oracle)."""
    import ngp_hip
    from ngp.field import NGPFieldFF
    from ngp.render import NGPRenderer
    L = ngp_hip.lib()
    o, d = FP.rays("centre", ODD)
    o, d = t(o, dev), t(d, dev)
    out, ws, rc = render_default_frame(constant(2.0), o, d, ODD, grid_size=1)
    assert rc == EINVAL and _untouched(out) and bool((ws == 0xAB).all()) and b"whole number of bytes" in L.ngp_last_error(), (rc, L.ngp_last_error())
    half = NGPRenderer(NGPFieldFF(bound=2.0).to(dev), bound=2.0, cuda_ray=True).to(dev).eval()
    half.density_bitfield.fill_(255)
    out, ws, rc = render_frame(half, o, d, ODD, grid_size=1)
    assert rc == EINVAL and _untouched(out) and bool((ws == 0xAB).all()) and b"whole number of bytes" in L.ngp_last_error(), (rc, L.ngp_last_error())
    out, _, rc = render_frame(half, o, d, ODD)
    assert rc == 0 and not bool(torch.isnan(out["image"]).any())
