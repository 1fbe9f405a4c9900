"""Packing / march statistics of one fused 800x800 frame (needs a -DRV_COUNTERS build for rounds and march trips):
   NGP_HIP_LIB=.../libngp_counters.so python tools/frame_counters.py [res] [--trained STEPS] [--frames P] [--hist-offset BYTES]
--trained STEPS renders a student fitted for STEPS steps to the hand-set scene (bench.py --model trained) instead of the hand-set model.
--frames P renders bench's first P orbit poses in ONE launch (ngp_render_frames_camera) instead of one frame.
--hist-offset: byte offset of the RV_TIMELINE histogram in the workspace (render_fused.hip RV_WS_HIST; before the tile order it was 49408)."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("nerf-navigation_amd")
from ngp import workload as W  # noqa: E402
from ngp.field import NGPFieldFF  # noqa: E402
from ngp.render import NGPRenderer  # noqa: E402

dev = torch.device("cuda:0")
trained = int(sys.argv[sys.argv.index("--trained") + 1]) if "--trained" in sys.argv else 0
res = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 800
frames = int(sys.argv[sys.argv.index("--frames") + 1]) if "--frames" in sys.argv else 1
hist_off = int(sys.argv[sys.argv.index("--hist-offset") + 1]) if "--hist-offset" in sys.argv else 256 + 36 * 1024
model = W.make_model(0)
field = NGPFieldFF(bound=W.BOUND).to(dev).load_arrays(model)
ren = NGPRenderer(field, bound=W.BOUND, cuda_ray=True, density_thresh=10.0).to(dev).eval()
ren.load_density_grid(W.density_grid())
if trained:
    import argparse
    import bench
    ren, fit = bench.fit_model(argparse.Namespace(workload="ring", fit_steps=trained), dev, W, ren)
    print("student:", fit)
if frames > 1:
    poses = np.stack([W.orbit_pose(k) for k in range(frames)]).astype(np.float32)
    intr = W.intrinsics(res, res)
    run = lambda **kw: ren.render_fused_cameras(poses, intr, res, res, bg_color=1, **kw)  # noqa: E731
else:
    o, d = W.get_rays(W.orbit_pose(1), W.intrinsics(res, res), res, res)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    run = lambda **kw: ren.render_fused(o[None], d[None], bg_color=1, image_width=res, **kw)  # noqa: E731
for _ in range(3):                                      # warm-up launches: the counters below are those of a warm frame
    run()
out = run(return_workspace=True)
torch.cuda.synchronize()
st = out["stats"].cpu().numpy().astype(np.int64)
ws = out["workspace"][:128].view(torch.int32).cpu().numpy().astype(np.int64)
print("samples", st[0], "rays with samples", st[2], "tiles", st[3], "fill %.3f" % (st[0] / (16.0 * max(st[3], 1))))
if ws[1]:
    print("wave rounds", ws[1], "march trips", ws[2], "tiles/round %.2f" % (st[3] / ws[1]), "trips/round %.2f" % (ws[2] / ws[1]),
          "samples/round %.1f" % (st[0] / ws[1]))
    print("lane probes: fine-tested", ws[3], "(of which samples", st[0], ") coarse-empty", ws[4], "super-empty", ws[5], "; samples evaluated behind a terminated ray:", ws[6])

    c = out["workspace"][32:88].view(torch.int64).cpu().numpy().view(np.uint64)
    nw = 2048.0                                             # 256 workgroups x 8 waves
    cmin = float(np.uint64(0xFFFFFFFFFFFFFFFF) - c[6])
    print("wave cycles (mean per wave, M): refill %.2f march %.2f tiles %.2f composite %.2f total %.2f | max %.2f min %.2f" % (
        float(c[0]) / nw / 1e6, float(c[1]) / nw / 1e6, float(c[2]) / nw / 1e6, float(c[3]) / nw / 1e6, float(c[4]) / nw / 1e6,
        float(c[5]) / 1e6, cmin / 1e6))
    # timeline (-DRV_COUNTERS -DRV_TIMELINE build; its atomics perturb the cycle counters above): 20 us bins of samples / wave-rounds / live lanes at round start / waves finishing
    off = hist_off
    if out["workspace"].numel() >= off + 4 * 2048:
        h = out["workspace"][off:off + 4 * 2048].view(torch.int32).cpu().numpy().astype(np.int64).reshape(4, 512)
        last = int(np.nonzero(h[1])[0].max()) + 1 if h[1].any() else 0
        step = 5
        print("timeline, %d us bins: t_us  Gsamples/s  rounds  live-lanes/round  samples/round  waves-finished(cum)" % (20 * step))
        fin = 0
        for b in range(0, last, step):
            smp, rnd, live, f = (int(h[k, b:b + step].sum()) for k in range(4))
            fin += f
            print("  %5d  %6.2f  %6d  %5.1f  %6.1f  %5d" % (20 * b, smp / (20e-6 * step) / 1e9, rnd, live / max(rnd, 1), smp / max(rnd, 1), fin))
        # ramp = until the 20 us rate first reaches 90 % of the median rate of the frame's middle half; first retire = first bin in which a wave finished
        rate = h[0, :last].astype(np.float64)
        mid = float(np.median(rate[last // 4: 3 * last // 4])) if last >= 4 else 0.0
        ramp = int(np.argmax(rate >= 0.9 * mid)) if mid > 0 else 0
        first = int(np.nonzero(h[3, :last + 1])[0].min()) if h[3].any() else last
        print("summary: frame %d us, ramp %d us (%.1f %%), first wave retires at %d us (%.1f %% of the frame), steady %.2f G samples/s" % (
            20 * last, 20 * ramp, 100.0 * ramp / max(last, 1), 20 * first, 100.0 * first / max(last, 1), mid / 20e-6 / 1e9))
