"""Colour transfer and colour distortion time: the GPU engine (ops.map_colors / ops.cloud_color_distortion, include/pcc_geo.h "cloud
colours") against the host paths on the same seeded clouds, with ops.cloud_nearest beside map_colors for scale.

    python tools/bench_color.py [--reps 10] [--out profiles/color_bench.json]

Cases: 10^6 uniform points in a 1024^3 box and the ~614k-point shell of tools/bench_metrics.py, each against a decoded-like copy
(20 % dropped, 30 % of the rest moved by one voxel).  GPU: device events around the whole call (index builds, uploads, kernels,
the copy back), median of --reps after a warm-up; cloud_nearest is timed with its index build so that the two calls do the same
work apart from the visitor.  Host: the reference's map_color (cKDTree k = 2 over the original, then the colour gather) and
pc_metric.color_tally_host, median wall clock of --host_reps calls.  Both sides are checked to agree."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_metrics import decoded_like  # noqa: E402
from _normals_ref import shell  # noqa: E402
from pcc_geo_cnn_v2_amd import ops  # noqa: E402
from pcc_geo_cnn_v2_amd.utils import pc_metric  # noqa: E402


def cases():
    rng = np.random.default_rng(0)
    u = rng.integers(0, 1024, (1000000, 3))
    s614, _ = shell(1024, radius=0.216, half_width=0.5, seed=1)
    out = []
    for i, (name, a) in enumerate((('uniform1e6', u), ('cloud614k', s614))):
        a = a.astype(np.int32)
        b = decoded_like(a, 10 + i, 1023).astype(np.int32)
        out.append((name, a, rng.integers(0, 256, (len(a), 3)).astype(np.uint8), b, rng.integers(0, 256, (len(b), 3)).astype(np.uint8)))
    return out


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
    ap.add_argument('--host_reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--gpu_only', action='store_true', help='skip the host side (profiling runs)')
    args = ap.parse_args()
    ctx = ops.get_context()
    results = []
    for name, a, ca, b, cb in cases():
        mapped, t_map = gpu_time(ctx, lambda: ops.map_colors(ctx, a, ca, b, rank=2), args.reps)
        _, t_near = gpu_time(ctx, lambda: ops.cloud_nearest(ctx, ops.CloudIndex(ctx, a), b), args.reps)
        tally, t_dist = gpu_time(ctx, lambda: ops.cloud_color_distortion(ctx, a, ca, b, cb), args.reps)
        row = {'case': name, 'n_a': len(a), 'n_b': len(b),
               'map_colors_event_ms': t_map, 'cloud_nearest_event_ms': t_near, 'color_distortion_event_ms': t_dist}
        if not args.gpu_only:
            af, bf = a.astype(np.float64), b.astype(np.float64)
            ref_map, row['host_map_color_ms'] = host_time(lambda: ca[cKDTree(af).query(bf, k=2, workers=-1)[1][:, 1]], args.host_reps)
            host_tally, row['host_color_tally_ms'] = host_time(lambda: pc_metric.color_tally_host(af, ca, bf, cb), args.host_reps)
            row['map_equal_to_ckdtree_share'] = float((mapped == ref_map).all(1).mean())     # < 1 only where cKDTree breaks a tie
            row['tally_rel_diff_max'] = float(np.max(np.abs(tally - host_tally) / np.abs(host_tally)))
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(ctx.device), 'reps': args.reps, 'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
