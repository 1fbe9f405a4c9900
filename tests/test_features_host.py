"""CPU: the pose filter's native interest regions (csrc/ngp_features.h, csrc/nav_features.hip) through their host twins, which run the header's functions
pixel after pixel: held bit for bit to the numpy restatement of the contract (tests/_features_restated.py, DESIGN.md 3.5 "Native interest regions"), and
the restatement to a float64 route on scipy.ndimage; dilation, list and draw against scipy / numpy; refusals; the header under sanitizers."""
import ctypes
import importlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

importlib.import_module("nerf-navigation_amd")

import _features_restated as FR  # noqa: E402

from _features_helpers import NGP_EINVAL, NGP_EWORKSPACE, NOISE_SHAPES, ROOT, _p, default_cfg, host_detect, host_draw, host_regions, layout, levels_of  # noqa: E402,F401


@pytest.fixture(scope="module")
def noise():
    """per shape: image, the restated pyramid and mask, the host twin's mask and workspace -- computed once, never changed"""
    out = {}
    for H, W in NOISE_SHAPES:
        image = FR.make_noise(H, W, seed=H * 1000 + W)
        pyr = FR.restated_pyramid(image)
        mask = FR.mask_of(FR.keypoints_of(pyr), H, W)
        got, ws = host_detect(image)
        out[(H, W)] = dict(image=image, pyramid=pyr, mask=mask, host_mask=got, host_ws=ws)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# host twins against the restatement, bit for bit
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", NOISE_SHAPES)
def test_host_mask_equals_the_restatement(noise, shape):
    n = noise[shape]
    print(shape, "keypoint pixels", int(n["mask"].sum()))
    assert np.array_equal(n["host_mask"], n["mask"])
    if shape != (16, 16):
        assert n["mask"].sum() > 0                                          # the comparison is not one of two empty masks


def test_octave_shapes_are_the_contracts():
    assert FR.octave_shapes(37, 53) == [(74, 106), (37, 53), (19, 27), (10, 14)]
    for H, W in NOISE_SHAPES + [(800, 800), (4096, 16)]:
        assert [(h, w) for h, w, _ in layout(H, W)["octaves"]] == FR.octave_shapes(H, W)
    assert FR.blur_radius(FR.blur_sigmas()[5]) == 12 and FR.blur_radius(FR.blur_sigmas()[0]) == 5
    assert min(FR.octave_shapes(37, 53)[-1]) - 1 < 12                       # the last octaves are narrower than the radius: the fold wraps more than once


@pytest.mark.parametrize("shape", [(37, 53), (64, 64)])
def test_host_pyramid_equals_the_restatement_level_by_level(noise, shape):
    n = noise[shape]
    got = levels_of(n["host_ws"], *shape)
    assert len(got) == len(n["pyramid"])
    for o, levels in enumerate(n["pyramid"]):
        for i, ref in enumerate(levels):
            assert ref.dtype == np.float32
            assert np.array_equal(got[o][i].view(np.uint32), ref.view(np.uint32)), (o, i)


# ------------------------------------------------------------------------------------------------------------------------
# the restatement against float64 on scipy.ndimage
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 53), (64, 64)])
def test_restated_pyramid_against_float64(noise, shape):
    n = noise[shape]
    ref = FR.scipy_pyramid(n["image"])
    chain = [0]                                                             # the blurs applied so far, as indices into blur_sigmas()
    worst = 0.0
    for o, levels in enumerate(n["pyramid"]):
        for i, lv in enumerate(levels):
            done = chain + list(range(1, i + 1))
            bound = FR.level_bound(done)
            err = float(np.abs(lv.astype(np.float64) - ref[o][i]).max())
            worst = max(worst, err / bound)
            assert err <= bound, (o, i, err, bound)
            assert 0.0 <= lv.min() and lv.max() <= 1.0 + bound
        chain = chain + [1, 2, 3]                                           # the next octave starts from level 3
    print(shape, "largest error / bound", worst)


BLOB_IMAGES = [FR.BLOBS_96, FR.BLOBS_37x53]


@pytest.mark.parametrize("spec", BLOB_IMAGES, ids=["96x96", "37x53"])
def test_blobs_give_one_keypoint_each_at_their_centres(spec):
    image = FR.make_blobs(**spec)
    H, W = spec["shape"]
    want = np.zeros((H, W), np.uint8)
    for cy, cx in spec["centres"]:
        want[cy, cx] = 1
    # 1. float64, no refinement: exactly one keypoint per blob, at the centre pixel
    pyr64 = FR.scipy_pyramid(image)
    raw = FR.scipy_keypoints(pyr64, conditions=False)
    kp64 = FR.scipy_keypoints(pyr64)
    print(spec["shape"], "raw float64 extrema", len(raw), "of which at a blob's centre", sum((int(y), int(x)) in spec["centres"] for _, y, x in raw),
          "; after the contrast and curvature conditions at the pixel", len(kp64))
    print(spec["shape"], "float64 keypoints (octave, row, col):", kp64)
    assert sorted((int(y), int(x)) for _, y, x in kp64) == sorted(spec["centres"])
    assert all(float(y) == int(y) and float(x) == int(x) for _, y, x in kp64)
    # 2. the restatement (with refinement): the same set
    kp32 = FR.keypoints_of(FR.restated_pyramid(image))
    print(spec["shape"], "restated keypoints:", [(o, float(y), float(x)) for o, y, x in kp32])
    assert np.array_equal(FR.mask_of(kp32, H, W), want)
    assert np.array_equal(FR.mask_of(kp64, H, W), want)
    # 3. the host twin
    got, _ = host_detect(image)
    assert np.array_equal(got, want)


def test_constant_image_has_no_keypoints():
    got, _ = host_detect(FR.make_constant(37, 53))
    assert got.sum() == 0 and FR.restated_mask(FR.make_constant(37, 53)).sum() == 0


# ------------------------------------------------------------------------------------------------------------------------
# dilation and list
# ------------------------------------------------------------------------------------------------------------------------
def _dilation_masks():
    out = {}
    for name, (r, c) in dict(corner00=(0, 0), corner0w=(0, 52), cornerh0=(36, 0), cornerhw=(36, 52), edge=(0, 20), inner=(17, 30)).items():
        m = np.zeros((37, 53), np.uint8)
        m[r, c] = 1
        out[name] = m
    for spec, name in zip(BLOB_IMAGES, ("blobs96", "blobs37x53")):
        m = np.zeros(spec["shape"], np.uint8)
        for cy, cx in spec["centres"]:
            m[cy, cx] = 1
        out[name] = m
    return out


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("it", [1, 3])
def test_dilation_equals_scipy(k, it):
    for name, m in _dilation_masks().items():
        regions, M, dilated = host_regions(m, k, it)
        ref = FR.restated_dilation(m, k, it)
        assert np.array_equal(dilated, ref), (name, k, it)
        assert M == int(ref.sum())
        assert np.array_equal(regions[:M], FR.restated_regions(ref)), (name, k, it)


def _list_masks():
    rng = np.random.default_rng(11)
    single = np.zeros((37, 53), np.uint8)
    single[30, 7] = 1
    return dict(empty=np.zeros((37, 53), np.uint8), single=single, ones=np.ones((37, 53), np.uint8),
                random=(rng.random((255, 257)) < 0.3).astype(np.uint8))            # 65,535 pixels: 63 full chunks and one of 1,023


@pytest.mark.parametrize("name", ["empty", "single", "ones", "random"])
def test_list_is_numpys_transposed_argwhere(name):
    m = _list_masks()[name]
    regions, M, dilated = host_regions(m, 1, 1)                             # a 1 x 1 kernel: the mask itself
    assert np.array_equal(dilated, m)
    ref = np.argwhere(m.T)[:, ::-1]
    assert M == ref.shape[0] == int(m.sum())
    assert np.array_equal(regions[:M], ref)
    assert np.all(regions[M:] == -1)                                        # nothing written past the count


# ------------------------------------------------------------------------------------------------------------------------
# draw
# ------------------------------------------------------------------------------------------------------------------------
def _fake_regions(M):
    i = np.arange(M, dtype=np.int64)
    return np.stack([i % 4099, i // 4099], axis=1).astype(np.int32)          # distinct pairs: a repeated pair would be a repeated index


@pytest.mark.parametrize("B", [1, 64, 1024])
def test_draw_equals_the_integer_restatement(B):
    for M in sorted({B, B + 1, 1000, 65537, 200000}):
        if M < B:
            continue
        regions = _fake_regions(M)
        got = {}
        for seed in (0, 0xDEADBEEF):
            got[seed] = host_draw(regions, B, 7, seed)
            assert np.array_equal(got[seed], FR.restated_draw(regions, B, 7, seed)), (M, B, seed)
            index = got[seed][..., 0].astype(np.int64) + 4099 * got[seed][..., 1]
            assert index.min() >= 0 and index.max() < M
            for k in range(7):
                assert np.unique(index[k]).size == B                        # without replacement
        if M >= 1000:                                                       # (with M = B = 1 there is one possible batch)
            assert not np.array_equal(got[0], got[0xDEADBEEF])
            assert all(not np.array_equal(got[0][0], got[0][k]) for k in range(1, 7))


def test_draw_includes_every_index_equally_often():
    """M = 5,000, B = 64, K = 2,000 batches: the inclusion count of an index is binomial(K, p = B / M) under a uniform draw without replacement, so
    sum (c - K p)^2 / (K p (1 - p)) is about chi-square with M - 1 degrees of freedom: within (M - 1) +- 6 sqrt(2 (M - 1))."""
    M, B, K = 5000, 64, 2000
    regions = np.stack([np.arange(M), np.zeros(M)], axis=1).astype(np.int32)
    for seed in (1, 2):
        counts = np.bincount(host_draw(regions, B, K, seed)[..., 0].ravel(), minlength=M).astype(np.float64)
        p = B / M
        chi = float(((counts - K * p) ** 2).sum() / (K * p * (1 - p)))
        print("seed", seed, "chi-square", chi, "expected", M - 1, "+-", 6 * np.sqrt(2 * (M - 1)))
        assert abs(chi - (M - 1)) <= 6 * np.sqrt(2 * (M - 1))
        # and the first entry of a batch alone (position 0 of the permutation) is spread over [0, M) too
        first = np.bincount(host_draw(regions, 1, 20000, seed)[..., 0].ravel(), minlength=M).astype(np.float64)
        chi0 = float(((first - 4.0) ** 2 / 4.0).sum())
        assert abs(chi0 - (M - 1)) <= 6 * np.sqrt(2 * (M - 1))


# ------------------------------------------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------------------------------------------
def test_workspace_sizes_are_pinned():
    import ngp_hip
    L = ngp_hip.lib()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_sizes_features.json")))
    assert len(golden) >= 8
    for key, size in golden.items():
        H, W = (int(v) for v in key.split("x"))
        assert L.ngp_features_workspace(H, W) == size, key
    for H, W in ((15, 16), (16, 15), (4097, 16), (16, 4097), (0, 0)):
        assert golden[f"{H}x{W}"] == 0
    # the pyramid dominates: 6 float32 levels per octave of the 2x upsample
    H, W = 37, 53
    floats = sum(6 * h * w for h, w in FR.octave_shapes(H, W))
    assert 4 * floats + H * W <= golden["37x53"] <= 4 * floats + H * W + 4 * 256 + 4 * 2 + 8 * 16 * 2


def test_refusals_need_no_device():
    import ngp_hip
    L = ngp_hip.lib()
    one = ctypes.c_void_p(4096)
    H, W = 37, 53
    need = L.ngp_features_workspace(H, W)

    def cfg(**kw):
        c = default_cfg()
        for k, v in kw.items():
            setattr(c, k, v)
        return ctypes.byref(c)
    for entry, tail in ((L.ngp_features_detect, (None,)), (L.ngp_features_detect_host, ())):
        assert entry(None, H, W, cfg(), one, one, need, *tail) == NGP_EINVAL and b"null pointer" in L.ngp_last_error()
        assert entry(one, H, W, None, one, one, need, *tail) == NGP_EINVAL
        assert entry(one, H, W, cfg(), None, one, need, *tail) == NGP_EINVAL
        for h, w in ((15, 53), (37, 15), (4097, 53), (37, 4097)):
            assert entry(one, h, w, cfg(), one, one, need, *tail) == NGP_EINVAL and b"supported from 16 to 4096" in L.ngp_last_error()
        assert entry(one, H, W, cfg(layers=0), one, one, need, *tail) == NGP_EINVAL and b"layers" in L.ngp_last_error()
        assert entry(one, H, W, cfg(layers=4), one, one, need, *tail) == NGP_EINVAL
        assert entry(one, H, W, cfg(border=0), one, one, need, *tail) == NGP_EINVAL and b"border" in L.ngp_last_error()
        assert entry(one, H, W, cfg(sigma=1.0), one, one, need, *tail) == NGP_EINVAL and b"sigma" in L.ngp_last_error()
        assert entry(one, H, W, cfg(edge=0.0), one, one, need, *tail) == NGP_EINVAL and b"edge" in L.ngp_last_error()
        assert entry(one, H, W, cfg(), one, one, need - 1, *tail) == NGP_EWORKSPACE and b"ngp_features_workspace" in L.ngp_last_error()
        assert entry(one, H, W, cfg(), one, None, need, *tail) == NGP_EWORKSPACE
    for entry, tail in ((L.ngp_features_regions, (None,)), (L.ngp_features_regions_host, ())):
        assert entry(None, H, W, 5, 3, one, one, one, need, *tail) == NGP_EINVAL and b"null pointer" in L.ngp_last_error()
        assert entry(one, H, W, 5, 3, None, one, one, need, *tail) == NGP_EINVAL
        assert entry(one, H, W, 5, 3, one, None, one, need, *tail) == NGP_EINVAL
        assert entry(one, 15, W, 5, 3, one, one, one, need, *tail) == NGP_EINVAL
        assert entry(one, H, W, 4, 3, one, one, one, need, *tail) == NGP_EINVAL and b"kernel_size = 4 must be odd" in L.ngp_last_error()
        assert entry(one, H, W, 0, 3, one, one, one, need, *tail) == NGP_EINVAL and b"kernel_size" in L.ngp_last_error()
        assert entry(one, H, W, 5, 0, one, one, one, need, *tail) == NGP_EINVAL and b"dil_iter = 0" in L.ngp_last_error()
        assert entry(one, H, W, 5, 3, one, one, one, need - 1, *tail) == NGP_EWORKSPACE and b"workspace" in L.ngp_last_error()
        assert entry(one, H, W, 5, 3, one, one, None, need, *tail) == NGP_EWORKSPACE
    for entry, tail in ((L.ngp_features_draw, (None,)), (L.ngp_features_draw_host, ())):
        assert entry(None, 100, 10, 3, 0, one, *tail) == NGP_EINVAL and b"null pointer" in L.ngp_last_error()
        assert entry(one, 100, 10, 3, 0, None, *tail) == NGP_EINVAL
        assert entry(one, 100, 0, 3, 0, one, *tail) == NGP_EINVAL and b"B = 0" in L.ngp_last_error()
        assert entry(one, 0, 10, 3, 0, one, *tail) == NGP_EINVAL and b"M = 0" in L.ngp_last_error()
        assert entry(one, 9, 10, 3, 0, one, *tail) == NGP_EINVAL
        assert b"9 interest points cannot fill a batch of 10 without replacement" in L.ngp_last_error()
        assert entry(one, 1 << 24, 1 << 20, 1 << 11, 0, one, *tail) == NGP_EINVAL and b"2^31" in L.ngp_last_error()
        assert entry(one, (1 << 24) + 1, 10, 3, 0, one, *tail) == NGP_EINVAL and b"an image holds at most 16777216 pixels" in L.ngp_last_error()
    assert L.ngp_features_layout(H, W, None) == NGP_EINVAL
    assert L.ngp_features_layout(15, W, one) == NGP_EINVAL
    assert L.ngp_abi_version() == 1


def test_default_cfg_is_opencvs():
    c = default_cfg()
    assert (c.contrast, c.edge, c.sigma, c.layers, c.border) == (np.float32(0.04), 10.0, np.float32(1.6), 3, 5)
    assert ctypes.sizeof(c) == 20


def test_header_and_ctypes_signatures_agree():
    import ngp_hip
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    kinds = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int, "void": None}
    names = ("ngp_features_default_cfg", "ngp_features_workspace", "ngp_features_layout", "ngp_features_detect", "ngp_features_regions", "ngp_features_draw",
             "ngp_features_detect_host", "ngp_features_regions_host", "ngp_features_draw_host")
    for name in names:
        m = re.search(r"\b(size_t|int|void)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        params = [p.strip() for p in m.group(2).split(",")]
        want = [ctypes.c_void_p if "*" in p else kinds[p.rsplit(" ", 1)[0].replace("const ", "").strip()] for p in params]
        assert name in ngp_hip.EXPORTS
        fn = getattr(ngp_hip.lib().raw, name)
        assert fn.restype is kinds[m.group(1)] and list(fn.argtypes) == want, (name, params)


# ------------------------------------------------------------------------------------------------------------------------
# the header under AddressSanitizer and UBSan, as a stand-alone program
# ------------------------------------------------------------------------------------------------------------------------
def test_features_header_under_address_and_ub_sanitizers(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "features_check")
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) and "clang" not in os.path.basename(cxx) else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    *static, "-I", os.path.join(ROOT, "nerf-navigation_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "features_check.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("features ok"), run.stdout + run.stderr
