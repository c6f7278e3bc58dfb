"""Point rendering time: ops.render_points (include/pcc_geo.h "point rendering") against utils/render.render_host on the same seeded
clouds, both checked to give the same image and rows.

    python tools/bench_render.py [--reps 10] [--out profiles/render_bench.json] [--gpu_only]

Cases: 10^6 uniform points at 1024^2 with s = 1 and 3; the 527k-point shell of tests/_normals_ref.shell(1024, 0.2, 0.5) at 1024^2; a far
camera that puts the 10^6 points on fewer than 16 pixels (every point hits one of a handful of z-buffer words: the atomic-bound
case).  GPU: device events around the whole call (host checks, upload, memset, kernels, the copy back), median of --reps after a
warm-up.  Host: median wall clock of --host_reps calls.  Kernel times come from a separate rocprofv3 --kernel-trace --stats run
of this script with --gpu_only."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from _normals_ref import shell  # noqa: E402
from pcc_geo_cnn_v2_amd import ops  # noqa: E402
from pcc_geo_cnn_v2_amd.utils import render  # noqa: E402


def cases():
    rng = np.random.default_rng(0)
    u = rng.random((1000000, 3)) * 1024
    cu = rng.integers(0, 256, (len(u), 3)).astype(np.uint8)
    sh, _ = shell(1024, radius=0.2, half_width=0.5)                # 527k points (tools/bench_metrics.py)
    csh = rng.integers(0, 256, (len(sh), 3)).astype(np.uint8)
    cam_u = render.default_camera(u, 1024, 1024, front=(1, 1, 1))
    far = render.default_camera(u, 1024, 1024, zoom=3000.0)
    return [('uniform1e6_s1', u, cu, cam_u, 1), ('uniform1e6_s3', u, cu, cam_u, 3),
            ('shell%dk_s1' % (len(sh) // 1000), sh, csh, render.default_camera(sh, 1024, 1024, front=(1, 1, 1)), 1),
            ('far_camera1e6_s1', u, cu, far, 1)]


def gpu_time(ctx, fn, reps):
    stream = torch.cuda.current_stream(ctx.device)
    out = fn()                                                # warm-up (allocations, code objects)
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    return out, {'median': float(np.median(ev)), 'min': float(np.min(ev))}


def host_time(fn, reps):
    out, t = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return out, float(np.median(t)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host_reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--gpu_only', action='store_true', help='skip the host side (profiling runs)')
    args = ap.parse_args()
    ctx = ops.get_context()
    results = []
    for name, pts, col, cam, s in cases():
        (img, rows), t = gpu_time(ctx, lambda: ops.render_points(ctx, pts, cam, col, s, return_rows=True), args.reps)
        _, t_img = gpu_time(ctx, lambda: ops.render_points(ctx, pts, cam, col, s), args.reps)
        row = {'case': name, 'n': len(pts), 'width': cam.width, 'height': cam.height, 'point_size': s,
               'covered_pixels': int((rows >= 0).sum()), 'render_points_event_ms': t_img, 'render_points_with_rows_event_ms': t}
        if not args.gpu_only:
            (himg, hrows), row['host_render_ms'] = host_time(lambda: render.render_host(pts, cam, col, s, return_rows=True), args.host_reps)
            row['equal_to_host'] = bool(np.array_equal(img, himg) and np.array_equal(rows, hrows))
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(ctx.device), 'reps': args.reps, 'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
