"""Camera poses INSIDE the ring scene, shared by test_frame_poses_host.py (CPU) and test_gpu_frame_inside.py: the frames a vehicle flying among the
obstacles takes, where every other frame test looks at the scene from an orbit outside everything occupied.

name -> (eye, forward); `ngp.workload.look_pose` makes the pose.  What each one reaches is asserted on the CPU oracle by
`check_reaches`, so that a later change of the scene cannot hollow the set out:

  centre       origin inside the box of everything occupied, level, along +x
  in_solid     origin inside a pillar: the first sample lies in an occupied cell (every ray has samples once min_near lets the march start there)
  slab_skim    inside the ground slab, along its diagonal: long occupied runs (hundreds of samples on a ray)
  slab_out     the same run the other way: the long occupied runs leave the occupied box through its UPPER x and y sides, obliquely
  slab_edge    inside the slab's outermost 4^3 blocks on its upper x side, along the edge: half the rays never come nearer to the middle than the eye, so
               they have their hundreds of samples only as long as the occupied box reaches out to the last occupied block
  lintel_top   level with the upper part of a lintel, looking at it: the eye is in the TOPMOST occupied blocks, the upper z side of the occupied box a few
               cells above it and parallel to the view
  up           under a lintel, looking straight up (z cannot be the pose's up vector)
  away         inside the occupied box with nothing ahead: no sample at all, every tile costs 0
  out_between  level, leaves the occupied box at once through the gap between two pillars: no sample
  corner       just inside the wall of the bound-2 AABB, looking at the scene along the diagonal: near = min_near
  behind       outside the occupied box, looking away from it: the box lies wholly behind the camera
"""
import functools

import numpy as np

POSES = {
    "centre": ((0.0, 0.0, 0.25), (1.0, 0.0, 0.0)),
    "in_solid": ((0.65, 0.0, 0.2), (-1.0, 0.0, 0.0)),
    "slab_skim": ((0.9, 0.9, -0.025), (-1.0, -1.0, 0.0)),
    "slab_out": ((-0.9, -0.9, -0.025), (1.0, 1.0, 0.0)),
    "slab_edge": ((0.97, 0.0, -0.025), (0.0, 1.0, 0.0)),
    "lintel_top": ((0.3, 0.15, 0.515), (1.0, 0.0, 0.0)),
    "up": ((0.6, 0.15, 0.2), (0.0, 0.0, 1.0)),
    "away": ((0.3, 0.3, 0.3), (0.0, 0.0, 1.0)),
    "out_between": ((0.5, 0.1, 0.2), (1.0, 0.2, 0.0)),
    "corner": ((1.95, 1.95, 1.9), (-1.0, -1.0, -1.0)),
    "behind": ((1.5, 0.3, 0.8), (1.0, 0.2, 0.3)),
}
NAMES = tuple(POSES)

# Direction components that are exactly 0.0 in an image of odd width and height n (the centre column has x_cam = 0, the centre row y_cam = 0): an axis-aligned
# pose maps each of the two onto one world axis (2 n components); a level pose that is not along an axis has only its `down` axis on a world axis (n); a pose
# with no camera axis on a world axis has none.  An even size has no centre column or row: none at all.
ZERO_COMPONENTS = {"centre": 2, "lintel_top": 2, "slab_edge": 2, "in_solid": 2, "up": 2, "away": 2, "slab_skim": 1, "slab_out": 1, "out_between": 1, "corner": 0, "behind": 0}     # times n
NO_SAMPLES = ("away", "out_between", "behind")           # frames without a single sample, whatever min_near and dt_gamma
DENSITY = 1e-3                                             # the constant density of the sample-count tests


def pose(name):
    from ngp import workload as W
    eye, forward = POSES[name]
    return W.look_pose(eye, forward)


def rays(name, res):
    """rays_o, rays_d [res * res, 3] float32 of pose `name` at res x res pixels (workload.get_rays, workload.intrinsics)"""
    from ngp import workload as W
    return W.get_rays(pose(name), W.intrinsics(res, res), res, res)


@functools.lru_cache(maxsize=None)
def scene(bound):
    """(bitfield, cascades) of the ring scene in a volume of half-width `bound`"""
    from ngp import workload as W
    bitfield, _ = W.bitfield_from_grid(W.density_grid(bound=bound))
    return bitfield, W.cascade_count(bound)


def constant_field(xyzs, dirs):
    """the field of all-zero networks: sigma = DENSITY * exp(0), rgb = sigmoid(0)"""
    n = xyzs.shape[0]
    return np.full(n, DENSITY, np.float32), np.full((n, 3), 0.5, np.float32)


@functools.lru_cache(maxsize=None)
def reference_constant(name, res, bound, min_near=0.2, dt_gamma=0.0):
    """the constant field's reference does not depend on which kernel is tested: computed once per process and shared by the GPU files that render
    these poses (the key is the call as written: pass min_near and dt_gamma by keyword; do not write to the result)"""
    from oracle import render_oracle as R
    o, d = rays(name, res)
    bitfield, cascade = scene(bound)
    return R.render_single_march(constant_field, o, d, bitfield, bound, cascade, min_near=min_near, dt_gamma=dt_gamma)


def check_reference_is_clean(ref, bound):
    """what makes the exact conditions valid, asserted on the reference before anything is compared with it: the compositor consumed every marched sample
    (no ray saturated), no ray ran into the cap of 1,024 samples, and weights_sum stays far from 1: at most 1 - exp(-DENSITY * the AABB's diagonal)"""
    assert np.array_equal(ref["consumed"], ref["marched"])
    assert int(ref["marched"].max()) < 1024
    assert float(ref["weights_sum"].max()) <= 1.0 - np.exp(-DENSITY * 2.0 * bound * np.sqrt(3.0)) + 1e-6


def check_reaches(name, res, refs):
    """the pose table's claims, on the CPU oracle at bound 2 with the constant field.  refs: {min_near: reference_constant(name, res, 2.0, min_near)} for
    min_near 0.2 and 0.0."""
    _, d = rays(name, res)
    n_rays = res * res
    assert int((d == 0).sum()) == (ZERO_COMPONENTS[name] * res if res % 2 else 0), name
    hit = {mn: int((ref["consumed"] > 0).sum()) for mn, ref in refs.items()}
    longest = {mn: int(ref["marched"].max()) for mn, ref in refs.items()}
    for mn, ref in refs.items():
        assert (ref["samples"] == 0) == (name in NO_SAMPLES), (name, mn, ref["samples"])
        assert np.isfinite(ref["depth"]).all(), name             # every eye lies inside the bound-2 AABB: every ray has a near and a far
    from ngp import workload as W
    lo = np.min([b[0] for b in W.scene_boxes()], axis=0)         # the bounding box of the solids: the box of everything occupied is this, rounded outwards
    hi = np.max([b[1] for b in W.scene_boxes()], axis=0)         # to the 4^3 blocks of the grid and widened by one more block (at most 0.25 at bound 2)
    eye = np.array(POSES[name][0])
    if name in ("centre", "in_solid", "slab_skim", "slab_out", "slab_edge", "lintel_top", "up", "away", "out_between"):
        assert bool(np.all(eye > lo) and np.all(eye < hi)), name
    if name in ("in_solid", "slab_skim", "slab_out", "slab_edge"):
        assert bool(W.inside(eye[None])[0]), name
    if name == "slab_edge":                                      # within one 4^3 block of cascade 0 (0.0625) of the slab's side; the rays that lean outwards hit too
        outwards = d[:, 0] > 0
        assert hi[0] - 0.0625 < eye[0] < hi[0] and hit[0.0] == n_rays and int(refs[0.0]["marched"][outwards].min()) > 10, (name, hit)
    if name == "lintel_top":                                     # within one 4^3 block of cascade 0 (0.0625) of the top of everything solid
        assert hi[2] - 0.0625 < eye[2] < hi[2] and 0 < hit[0.2] < n_rays, (name, hit)
    if name == "corner":                                         # inside the AABB, within one cell of cascade 1 (4 / 128) times two of its wall
        assert bool(np.all(np.abs(eye) < 2.0) and np.all(2.0 - eye < 0.125)), name
    if name == "behind":                                         # beyond the widened box on the x axis and every ray goes further that way: both crossings of
        assert eye[0] > hi[0] + 0.25 and float(d[:, 0].min()) > 0.0           # the box's x slab lie behind the origin, so the slab test's far is negative
    if name == "in_solid":                                       # from inside a pillar every ray starts in an occupied cell; min_near 0.2 steps out of it
        assert hit[0.0] == n_rays and hit[0.2] < n_rays, hit
    if name in ("slab_skim", "slab_out"):
        assert hit[0.0] == n_rays and longest[0.0] > 500, (hit, longest)
    if name == "up":                                             # the lintel is overhead on every ray
        assert hit[0.2] == n_rays, hit
    if name in ("centre", "corner"):                             # pillars ahead of some rays, gaps ahead of others
        assert 0 < hit[0.2] < n_rays and refs[0.2]["samples"] > 20 * hit[0.2], (hit, refs[0.2]["samples"])
