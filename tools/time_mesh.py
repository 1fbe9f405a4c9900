"""Time mesh extraction (ngp/mesh.py, csrc/mesh.hip) on cuda:0 for the hand-set ring scene (workload.make_model(0), NGPFieldFF,
bound 2) at resolution 256 and 512: the density lattice, marching cubes split into count (classify + scan + the read-back of V, T) and emit, V and T,
the marching-cubes passes' bytes over time against 8 TB/s, and, labelled as such, the reference-structured extract_fields loop (128^3 chunks, one
.cpu() each; nerf/utils.py:150-167).  Device events; warm-up, then the median of several back-to-back repeats; the first call after a 200 ms idle
gap is reported on its own (profiles/HISTORY.md §4.2: the clocks come back over several launches)."""
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("nerf-navigation_amd")
import ngp_hip as H  # noqa: E402
from ngp import workload as W  # noqa: E402
from ngp.field import NGPFieldFF  # noqa: E402
from ngp.mesh import _device_lattice, density_query  # noqa: E402

HBM = 8.0e12
REPEATS = int(os.environ.get("REPEATS", "7"))


def events_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def reference_loop(lo, hi, r, query, S=128):
    X, Y, Z = (torch.linspace(lo[i], hi[i], r).split(S) for i in range(3))
    u = np.zeros([r, r, r], dtype=np.float32)
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = \
                        query(pts).reshape(len(xs), len(ys), len(zs)).detach().cpu().numpy()
    return u


def main():
    assert torch.cuda.is_available(), "time_mesh.py needs a GPU"
    dev = torch.device("cuda:0")
    field = NGPFieldFF(bound=W.BOUND).to(dev).load_arrays(W.make_model(0))
    lo, hi = torch.tensor([-W.BOUND] * 3), torch.tensor([W.BOUND] * 3)
    query = density_query(field, fp16=True)
    L = H.lib()
    results = []
    for r in (256, 512):
        lattice = lambda: _device_lattice(lo, hi, r, query, device=dev)      # noqa: E731
        u = lattice()
        ws = H.workspace(L.ngp_marching_cubes_workspace(r, r, r), dev)
        V, T = ctypes.c_uint64(), ctypes.c_uint64()

        def count():
            H.check(L.ngp_marching_cubes_count(H.ptr(u), r, r, r, 10.0, H.ptr(ws), ws.numel(), ctypes.byref(V), ctypes.byref(T), H.stream()), "count")

        count()
        verts = torch.empty((V.value, 3), dtype=torch.float32, device=dev)
        tris = torch.empty((T.value, 3), dtype=torch.int32, device=dev)

        def emit():
            H.check(L.ngp_marching_cubes_emit(H.ptr(u), r, r, r, 10.0, H.ptr(ws), ws.numel(), H.ptr(verts), V.value, H.ptr(tris), T.value,
                                              H.stream()), "emit")

        for _ in range(3):                                                    # warm-up of every shape
            lattice(); count(); emit()
        torch.cuda.synchronize()
        time.sleep(0.2)
        idle_count, idle_emit = events_ms(count, 1)[0], events_ms(emit, 1)[0]
        for _ in range(3):
            count(); emit()
        t_lat = events_ms(lattice, REPEATS)
        t_count = events_ms(count, REPEATS)
        t_emit = events_ms(emit, REPEATS)
        N = r ** 3
        bytes_count = 4 * N + 3 * N                                           # lattice read once, bits + loc written
        bytes_emit = 4 * N + 3 * N + 12 * V.value + 12 * T.value             # lattice, bits, loc read; mesh written
        mc_ms = statistics.median(t_count) + statistics.median(t_emit)
        ref_s = None
        if r <= 512:
            reference_loop(lo, hi, r, lambda p: query(p.to(dev)))            # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reference_loop(lo, hi, r, lambda p: query(p.to(dev)))
            torch.cuda.synchronize()
            ref_s = time.perf_counter() - t0
        row = dict(resolution=r, V=V.value, T=T.value,
                   lattice_ms=statistics.median(t_lat), count_ms=statistics.median(t_count), emit_ms=statistics.median(t_emit),
                   count_ms_after_idle=idle_count, emit_ms_after_idle=idle_emit,
                   mc_bytes=bytes_count + bytes_emit, mc_TBps=(bytes_count + bytes_emit) / (mc_ms * 1e-3) / 1e12,
                   mc_frac_of_8TBps=(bytes_count + bytes_emit) / (mc_ms * 1e-3) / HBM,
                   reference_structured_lattice_ms=None if ref_s is None else ref_s * 1e3,
                   spread=dict(lattice=[min(t_lat), max(t_lat)], count=[min(t_count), max(t_count)], emit=[min(t_emit), max(t_emit)]))
        results.append(row)
        print(f"r={r}: V={V.value} T={T.value}  lattice {row['lattice_ms']:.2f} ms  count {row['count_ms']:.3f} ms  emit {row['emit_ms']:.3f} ms"
              f"  (after idle: {idle_count:.3f} / {idle_emit:.3f})  MC {row['mc_bytes'] / 1e9:.2f} GB at {row['mc_TBps']:.2f} TB/s"
              f" = {row['mc_frac_of_8TBps']:.2f} of 8 TB/s;  reference-structured lattice loop {row['reference_structured_lattice_ms']:.1f} ms",
              flush=True)
        del u, ws, verts, tris
        torch.cuda.empty_cache()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
