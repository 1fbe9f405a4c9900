"""CPU: `workload.look_pose` and the table of inside poses (tests/_frame_poses.py) that test_gpu_frame_inside.py renders: the helper builds a right-handed
orthonormal camera frame the way `orbit_pose` does, looking straight up and down included; through it an image of odd width has direction components that are
exactly 0.0 where the pose table says; and what each pose is in the table FOR (no sample at all, every ray hit, the box behind the camera ...) holds on the
CPU oracle, here at 17 x 17, so that the table is guarded on every machine and not only where a GPU is."""
import numpy as np
import pytest

import _frame_poses as FP


def _axes(pose):
    return pose[:3, 0].astype(np.float64), pose[:3, 1].astype(np.float64), pose[:3, 2].astype(np.float64)


@pytest.mark.parametrize("forward", [(1, 0, 0), (0, -1, 0), (-1, -1, 0), (1, 0.2, 0), (-1, -1, -1), (0.3, -2.0, 0.7), (0, 0, 1), (0, 0, -1), (0, 0, 5.0),
                                     (1e-4, 0, 1)])
def test_look_pose_is_a_right_handed_orthonormal_frame(forward):
    from ngp import workload as W
    eye = (0.3, -0.2, 0.1)
    pose = W.look_pose(eye, forward)
    assert pose.shape == (4, 4) and pose.dtype == np.float32
    assert np.array_equal(pose[3], [0, 0, 0, 1]) and np.array_equal(pose[:3, 3], np.array(eye, np.float32))
    right, down, fwd = _axes(pose)
    f = np.array(forward, np.float64)
    assert np.allclose(fwd, f / np.linalg.norm(f), atol=1e-7)                            # the third column is the forward direction
    R = pose[:3, :3].astype(np.float64)
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-6)                                    # orthonormal ...
    assert abs(np.linalg.det(R) - 1.0) < 1e-6 and np.allclose(np.cross(right, down), fwd, atol=1e-6)   # ... and right-handed: x right, y down, z forward
    if abs(fwd[2]) < 0.999:
        assert abs(right[2]) < 1e-7 and down[2] < 0                                      # level horizon, z up (image rows run downwards)
    else:
        assert np.isfinite(pose).all() and abs(down[1]) > 0.99                           # straight up / down: +y takes the place of z


def test_look_pose_agrees_with_orbit_pose():
    """the same camera as orbit_pose when given its eye and its viewing direction (orbit_pose itself is unchanged)"""
    from ngp import workload as W
    for k in range(8):
        ref = W.orbit_pose(k)
        assert np.allclose(W.look_pose(ref[:3, 3], -ref[:3, 3].astype(np.float64)), ref, atol=1e-6)
    assert W.orbit_pose(1).tolist() == W.orbit_pose(1, 8, 1.6, 0.6).tolist()


@pytest.mark.parametrize("name", FP.NAMES)
def test_exact_zero_direction_components(name):
    """odd width: the centre column and row have a camera-space coordinate of exactly 0, which an axis-aligned pose carries into the world direction
    (1 / d = inf in the slab tests and the cell exits); even width: no such pixel"""
    for res in (17, 33):
        _, d = FP.rays(name, res)
        assert int((d == 0).sum()) == FP.ZERO_COMPONENTS[name] * res, name
        assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6)
    for res in (16, 40):
        assert int((FP.rays(name, res)[1] == 0).sum()) == 0
    if name == "centre":                                          # along +x with z up: the centre column has d_y = 0, the centre row d_z = 0
        d = FP.rays(name, 17)[1].reshape(17, 17, 3)
        assert bool((d[:, 8, 1] == 0).all()) and bool((d[8, :, 2] == 0).all()) and bool((d[..., 0] > 0.9).all())
    if name == "up":
        d = FP.rays(name, 17)[1].reshape(17, 17, 3)
        assert bool((d[..., 2] > 0.9).all()) and d[8, 8].tolist() == [0.0, 0.0, 1.0]


@pytest.mark.parametrize("name", FP.NAMES)
def test_each_pose_reaches_what_the_table_says(oracle, name):
    refs = {mn: FP.reference_constant(name, 17, 2.0, min_near=mn) for mn in (0.2, 0.0)}
    for ref in refs.values():
        FP.check_reference_is_clean(ref, 2.0)
    FP.check_reaches(name, 17, refs)


def test_the_empty_poses_stay_empty_at_every_bound_and_step_rule(oracle):
    for name in FP.NO_SAMPLES:
        for bound in (2.0, 1.5, 0.75):
            for dt_gamma in (0.0, 1.0 / 128):
                assert FP.reference_constant(name, 17, bound, min_near=0.0, dt_gamma=dt_gamma)["samples"] == 0, (name, bound, dt_gamma)
