"""Whole-cloud D1 / D2 metric time: the GPU engine (pc_metric.cloud_metrics_batch_gpu, include/pcc_geo.h "cloud metrics") against the
host path (pc_metric.cloud_metrics_batch, scipy KD-trees) on the same seeded clouds.

    python tools/bench_metrics.py [--reps 10] [--out profiles/metrics_bench.json]

Cases: the 1024^3 shell of tests/_normals_ref.shell against a perturbed copy; 10^6 uniform points in a 1024^3 box against a perturbed
copy; a ~614k-point shell against one and two decoded-like candidates (20 % dropped, 30 % of the rest moved by one voxel), D1 alone and
D1 + D2.  GPU: device events around the whole call (index builds, uploads, kernels, the tally copy), median of --reps after a
warm-up; also the wall clock.  Host: median wall clock of --host_reps calls.  Both sides are checked to give the same D1."""
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
from pcc_geo_cnn_v2_amd.utils import pc_metric  # noqa: E402


def decoded_like(p, seed, top):
    rng = np.random.default_rng(seed)
    keep = rng.random(len(p)) < 0.8
    q = p[keep].astype(np.int64)
    q += rng.integers(-1, 2, q.shape) * (rng.random((len(q), 1)) < 0.3)
    return np.clip(q, 0, top).astype(np.float64)


def cases():
    rng = np.random.default_rng(0)
    s1024, _ = shell(1024, radius=0.2, half_width=0.5)                # 527k points (tools/bench_normals.py)
    u = rng.integers(0, 1024, (1000000, 3))
    s614, _ = shell(1024, radius=0.216, half_width=0.5, seed=1)        # ~614k points: the configs2 cloud size
    out = [('shell1024', s1024, [decoded_like(s1024, 1, 1023)], 1023, False),
           ('uniform1e6', u, [decoded_like(u, 2, 1023)], 1023, False),
           ('cloud614k_1cand', s614, [decoded_like(s614, 3, 1023)], 1023, False),
           ('cloud614k_2cand', s614, [decoded_like(s614, 3, 1023), decoded_like(s614, 4, 1023)], 1023, False),
           ('cloud614k_2cand_d2', s614, [decoded_like(s614, 3, 1023), decoded_like(s614, 4, 1023)], 1023, True)]
    return [(n, a.astype(np.float64), c, r, d2) for n, a, c, r, d2 in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host_reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--gpu_only', action='store_true', help='skip the host side (profiling runs)')
    args = ap.parse_args()
    ctx = ops.get_context()
    stream = torch.cuda.current_stream(ctx.device)
    results = []
    for name, a, cands, peak, with_d2 in cases():
        nrm = ops.estimate_normals(ctx, a) if with_d2 else None
        run = lambda: pc_metric.cloud_metrics_batch_gpu(ctx, a, cands, peak, nrm)
        gpu = run()                                           # warm-up (allocations, code objects)
        ev, wall = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            run()
            e1.record(stream)
            e1.synchronize()
            wall.append(time.perf_counter() - t0)
            ev.append(e0.elapsed_time(e1))
        row = {'case': name, 'n_a': len(a), 'n_b': [len(c) for c in cands], 'd2': with_d2,
               'gpu_event_ms_median': float(np.median(ev)), 'gpu_event_ms_min': float(np.min(ev)),
               'gpu_wall_ms_median': float(np.median(wall)) * 1e3}
        if not args.gpu_only:
            host_t = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                host = pc_metric.cloud_metrics_batch(a, cands, peak, nrm)
                host_t.append(time.perf_counter() - t0)
            row['host_wall_ms_median'] = float(np.median(host_t)) * 1e3
            row['d1_equal'] = all(g['d1_sum_AB'] == h['d1_sum_AB'] and g['d1_sum_BA'] == h['d1_sum_BA'] for g, h in zip(gpu, host))
            if with_d2:
                row['d2_mse_rel_diff_max'] = float(max(abs(g['d2_mse'] / h['d2_mse'] - 1) for g, h in zip(gpu, host)))
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(ctx.device), 'reps': args.reps, 'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
