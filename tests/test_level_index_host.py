"""How a level of the hash grid is indexed (csrc/ngp_device.h: ngp_classify_level), held to oracle/ngp_oracle.c row by row.  No GPU.
  (a) a stand-alone program includes ngp_device.h, prints the classifier's strides and kind for each case and the row that kind gives at
      each lattice corner; built host-only with hipcc, once plainly and once under AddressSanitizer + UBSan;
  (b) oracle/callers_oracle.py's _grid_index at the same corners;
  (c) the fused nav queries refuse a field with a wrapped level (their kernels add a dense level's strides without a modulo), in every
      query's argument check and in ngp_nav_field_prepare, and accept the default field.
The expected rows come from the oracle's forward on a one-level float32 table whose row r holds the value r (exact below 2^24), at points
that sit on a lattice corner, so that this corner has weight 1 and the seven others weight 0."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (rows, side, kind, s1, s2)
CASES = [
    (4913, 17, "exact", 17, 289),
    (1 << 19, 80, "exact", 80, 6400),
    (1 << 19, 81, "hashed", 81, 6561),
    (1 << 19, 725, "hashed", 725, 0),                  # the second stride no longer fits
    (1 << 19, 65536, "wrapped", 65536, 0),             # the square is 2^32 = 0
    (1 << 19, 65537, "wrapped", 65537, 131073),
    (1 << 19, 131073, "wrapped", 131073, 262145),
    (1 << 19, 262145, "hashed", 262145, 0),
    (1 << 19, 524289, "hashed", 0, 0),
    (500000, 100, "hashed", 100, 10000),               # rows not 2^k: the modulo path
    (1 << 24, 1626, "wrapped", 1626, 2643876),         # a wrap well below a side of 2^16
    (1 << 24, 1625, "hashed", 1625, 2640625),
    (1 << 22, 1 << 22, "wrapped", 1 << 22, 0),         # the cube, 2^66, wraps in 64 bits as well: not exact
]
NRANDOM = 200

PROGRAM = r"""
#include "ngp_device.h"
thread_local char ngp_err_buf[512];

// the row each kind of level gives, from nothing but the classifier's answer
static uint32_t row_of(const ngp_level_index& ix, uint32_t rows, uint32_t x, uint32_t y, uint32_t z) {
    if (ix.exact) return x + y * ix.s1 + z * ix.s2;
    const uint32_t i = ix.dense ? x + y * ix.s1 + z * ix.s2 : x ^ (y * NGP_HASH_P1) ^ (z * NGP_HASH_P2);
    return (rows & (rows - 1u)) == 0u ? (i & (rows - 1u)) : i % rows;
}

int main() {          // stdin: per case `rows side n` and n corners `x y z`; stdout: `s1 s2 kind` and n rows
    uint32_t rows, side, n;
    while (scanf("%u %u %u", &rows, &side, &n) == 3) {
        const ngp_level_index ix = ngp_classify_level(rows, side);
        printf("%u %u %s\n", ix.s1, ix.s2, ix.exact ? "exact" : ix.dense ? "wrapped" : "hashed");
        for (uint32_t k = 0; k < n; k++) {
            uint32_t x, y, z;
            if (scanf("%u %u %u", &x, &y, &z) != 3) return 1;
            printf("%u\n", row_of(ix, rows, x, y, z));
        }
    }
    return 0;
}
"""


def _corners(side, seed):
    """[2 + NRANDOM, 3] lattice points: the origin, (side-1, side-1, side-1) and seeded random ones in between.  With align_corners the oracle's
    position is fl(fl(k / scale) * scale), scale = side - 1: the random coordinates are drawn among the k that this returns unchanged."""
    scale = np.float32(side - 1)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, side, size=8 * NRANDOM * 3, dtype=np.int64)
    k = k[(k.astype(np.float32) / scale) * scale == k.astype(np.float32)][:NRANDOM * 3]
    assert k.size == NRANDOM * 3
    return np.concatenate([np.zeros((1, 3), np.int64), np.full((1, 3), side - 1, np.int64), k.reshape(NRANDOM, 3)])


@pytest.fixture(scope="module")
def expected(oracle):
    """per case: (corners [N,3] int64, the oracle's rows [N] int64), computed once"""
    out = []
    for n, (rows, side, _, _, _) in enumerate(CASES):
        pts = _corners(side, 1000 + n)
        x = pts.astype(np.float32) / np.float32(side - 1)
        assert np.array_equal(x * np.float32(side - 1), pts.astype(np.float32)) and x.min() >= 0 and x.max() <= 1
        table = np.arange(rows, dtype=np.float32).reshape(rows, 1)
        # one level, align_corners: scale = side - 1, and get_grid_index multiplies its stride by `resolution` = side
        got, _ = oracle.grid_encode_forward(x, table, np.array([0, rows], np.int32), 1.0, side, gridtype=0, align_corners=True)
        ref = got.reshape(-1).astype(np.int64)
        assert np.array_equal(ref.astype(np.float32), got.reshape(-1)) and ref.min() >= 0 and ref.max() < rows
        out.append((pts, ref))
    return out


def _build_and_run(tmp_path, name, extra, stdin):
    src = tmp_path / "level_index_check.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / name)
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-Werror", *extra,
                    "-I", os.path.join(ROOT, "nerf-navigation_amd", "csrc"), str(src), "-o", exe], check=True, timeout=600)
    run = subprocess.run([exe], input=stdin, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not run.stderr.strip(), run.stderr[-2000:]
    return run.stdout.split("\n")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_classifier_rows_equal_the_oracle(tmp_path, expected, sanitize):
    stdin = "".join("%d %d %d\n" % (rows, side, len(pts)) + "".join("%d %d %d\n" % tuple(p) for p in pts)
                    for (rows, side, _, _, _), (pts, _) in zip(CASES, expected))
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    lines = _build_and_run(tmp_path, "check_san" if sanitize else "check", extra, stdin)
    at = 0
    for (rows, side, kind, s1, s2), (pts, ref) in zip(CASES, expected):
        assert lines[at].split() == [str(s1), str(s2), kind], (rows, side, lines[at])
        got = np.array([int(v) for v in lines[at + 1:at + 1 + len(pts)]], np.int64)
        at += 1 + len(pts)
        wrong = np.flatnonzero(got != ref)
        assert wrong.size == 0, (rows, side, kind, wrong.size, pts[wrong[:4]].tolist(), got[wrong[:4]].tolist(), ref[wrong[:4]].tolist())
    assert lines[at:] == [""]


def test_callers_oracle_grid_index_equals_the_oracle(expected):
    from oracle import callers_oracle
    failed = {}
    for (rows, side, kind, _, _), (pts, ref) in zip(CASES, expected):
        loc = [torch.from_numpy(np.ascontiguousarray(pts[:, d])) for d in range(3)]
        got = callers_oracle._grid_index(loc, rows, side - 1, 0, False).numpy()
        if not np.array_equal(got, ref):
            failed[(rows, side, kind)] = int((got != ref).sum())
    assert not failed, failed


def _nav_field(bound):
    """ngp_nav_field_t of NGPField(bound)'s encoder with dummy non-null pointers (nothing here dereferences them) + what it must keep alive"""
    import ngp_hip
    from gridencoder import GridEncoder
    enc = GridEncoder(desired_resolution=2048 * bound)
    offsets = (ctypes.c_int32 * 17)(*[int(v) for v in enc.offsets.tolist()])
    f = ngp_hip.ngp_nav_field_t(16, ctypes.cast(offsets, ctypes.c_void_p), 16, 16, 16, 16, 16, 16, enc.base_resolution,
                                float(np.log2(enc.per_level_scale)), float(bound), 1.0)
    return f, offsets


def test_nav_queries_refuse_a_wrapped_level_without_a_gpu():
    import ngp_hip
    L = ngp_hip.lib()
    one = ctypes.c_void_p(16)
    size = L.ngp_nav_field_workspace()
    big, keep_big = _nav_field(256)                             # S = 1, H = 16, 2^19 rows: sides 65,537 and 131,073 at levels 12 and 13
    assert (big.H, big.S, keep_big[13] - keep_big[12]) == (16, 1.0, 1 << 19)
    default, keep_default = _nav_field(1)
    # M = 0: the field is checked, nothing is launched
    assert L.ngp_nav_density_forward(ctypes.byref(big), one, None, 0, None, None, None) == -1
    message = L.ngp_last_error().decode()
    assert "level 12" in message and "65537" in message and str(1 << 19) in message and "NavQueries" in message, message
    assert L.ngp_nav_density_forward(ctypes.byref(default), one, None, 0, None, None, None) == 0
    # ngp_nav_field_prepare judges the field as the queries do, before anything else.  Its success path launches the transposes, which a test
    # with dummy pointers must not reach: the default field is shown to pass the field check by the NEXT refusal, a workspace one byte short.
    assert L.ngp_nav_field_prepare(ctypes.byref(big), one, size, None) == -1
    assert "level 12" in L.ngp_last_error().decode()
    assert L.ngp_nav_field_prepare(ctypes.byref(default), one, size - 1, None) == -1
    assert L.ngp_last_error().decode() == "nav_field_prepare: bad argument"
    assert L.ngp_nav_field_prepare(ctypes.byref(big), one, size - 1, None) == -1
    assert "level 12" in L.ngp_last_error().decode()
