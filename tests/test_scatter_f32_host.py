"""CPU: the float32 binned scatter's host side (csrc/gridencoder.hip: gsf_layout, ngp_grid_scatter_binned_f32): workspace sizes pinned against
tests/golden/workspace_sizes_scatter_f32.json (recorded from the library; sizes are part of the C ABI), refusals with their codes before any
device is touched, and the declaration in include/ngp_hip.h against the ctypes signature in ngp_hip.py."""
import ctypes
import importlib
import json
import os
import re

importlib.import_module("nerf-navigation_amd")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NGP_EINVAL, NGP_EWORKSPACE = -1, -3
SIZES = (0, 1, 1024, 1025, 1 << 22, (1 << 22) + 1)


def test_workspace_sizes_are_pinned():
    import ngp_hip
    lib = ngp_hip.lib()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_sizes_scatter_f32.json")))
    assert sorted(int(k) for k in golden["L16"]) == sorted(SIZES)
    for B in SIZES:
        assert lib.ngp_grid_scatter_binned_f32_workspace(B, 16) == golden["L16"][str(B)], B
    # 10 bytes per possible entry (two binary32 planes and a u16 row), 8,192 entries per 1,024-sample chunk and level, plus the directory and the ticket
    chunks = lambda B: (min(B, 1 << 22) + 1023) // 1024                   # noqa: E731
    for B in SIZES:
        entries = 16 * chunks(B) * 8192
        directory = 16 * 129 * chunks(B) * 2
        assert entries * 10 <= golden["L16"][str(B)] <= entries * 10 + directory + 3 * 256 + 256
    assert golden["L16"][str((1 << 22) + 1)] == golden["L16"][str(1 << 22)]  # beyond one pass the workspace stops growing


def test_refusals_need_no_device():
    import ngp_hip
    L = ngp_hip.lib()
    one = ctypes.c_void_p(4096)                                             # non-null dummies: every refusal comes before any dereference
    need = L.ngp_grid_scatter_binned_f32_workspace(1025, 16)
    ok = dict(grad=one, inputs=one, offsets=one, out=one, B=1025, L=16, rows=1 << 19, ws=one, ws_bytes=need)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ngp_grid_scatter_binned_f32(a["grad"], a["inputs"], a["offsets"], a["out"], a["B"], a["L"], 1.0, 16, a["rows"], 0, 0, 1.0, a["ws"], a["ws_bytes"], None)
    for name in ("grad", "inputs", "offsets", "out"):
        assert call(**{name: None}) == NGP_EINVAL, name
        assert b"null pointer" in L.ngp_last_error()
    assert call(L=0) == NGP_EINVAL and call(L=33) == NGP_EINVAL
    assert b"1..32" in L.ngp_last_error()
    assert call(rows=(1 << 19) + 1) == NGP_EINVAL
    assert b"2^19" in L.ngp_last_error()
    assert call(rows=0) == NGP_EINVAL
    assert call(ws_bytes=need - 1) == NGP_EWORKSPACE
    assert b"workspace" in L.ngp_last_error()
    assert call(ws=None) == NGP_EWORKSPACE
    assert call(B=0, grad=None, inputs=None, ws_bytes=0) == NGP_EWORKSPACE  # an empty batch still needs its (ticket-sized) workspace


def test_header_and_ctypes_signatures_agree():
    import ngp_hip
    header = open(os.path.join(ROOT, "include", "ngp_hip.h")).read()
    kinds = {"size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int, "float": ctypes.c_float}
    for name in ("ngp_grid_scatter_binned_f32_workspace", "ngp_grid_scatter_binned_f32"):
        m = re.search(r"\b(size_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        params = [p.strip() for p in m.group(2).split(",")]
        want = [ctypes.c_void_p if "*" in p else kinds[p.rsplit(" ", 1)[0].replace("const ", "").strip()] for p in params]
        assert name in ngp_hip.EXPORTS
        fn = getattr(ngp_hip.lib().raw, name)
        assert fn.restype is kinds[m.group(1)] and list(fn.argtypes) == want, (name, params)
