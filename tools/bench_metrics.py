"""Whole-cloud D1 / D2 metric time: the GPU engine (pc_metric.cloud_metrics_batch_gpu, include/pcc_geo.h "cloud metrics") against the
host path (pc_metric.cloud_metrics_batch, scipy KD-trees) on the same seeded clouds.

    python tools/bench_metrics.py [--reps 10] [--out profiles/metrics_bench.json]

Cases: the 1024^3 shell of tests/_normals_ref.shell against a perturbed copy; 10^6 uniform points in a 1024^3 box against a perturbed
copy; a ~614k-point shell against one and two decoded-like candidates (20 % dropped, 30 % of the rest moved by one voxel), D1 alone and
D1 + D2.  GPU: device events around the whole call (index builds, uploads, kernels, the tally copy), median of --reps after a
warm-up; also the wall clock.  Host: median wall clock of --host_reps calls.  Both sides are checked to give the same D1.

    python tools/bench_metrics.py --ties mean [--reps 10] [--out profiles/metrics_bench.json]

times the tie-averaged D2 (cloud_metrics_batch_gpu(..., ties='mean'), DESIGN.md "Tie-averaged D2") beside the default rule on the
D1 + D2 cases (the 614k-point cloud and the 10^6-point cloud, one candidate each): the two rules alternate inside one process, device
events around each whole call; the rows go under the key "ties_mean" of --out, whose other keys are kept."""
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


def time_call(run, stream, reps):
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        run()
        e1.record(stream)
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    return ev


def ties_rows(ctx, stream, args):
    """pick and mean on the same clouds, alternating rep by rep; the host `mean` once, for the agreement columns."""
    rng = np.random.default_rng(0)
    s614, _ = shell(1024, radius=0.216, half_width=0.5, seed=1)
    u = rng.integers(0, 1024, (1000000, 3))
    rows = []
    for name, a, seed in (('cloud614k_1cand_d2', s614, 3), ('uniform1e6_1cand_d2', u, 2)):
        a = a.astype(np.float64)
        cands = [decoded_like(a, seed, 1023)]
        nrm = ops.estimate_normals(ctx, a)
        run = {t: (lambda t=t: pc_metric.cloud_metrics_batch_gpu(ctx, a, cands, 1023, nrm, ties=t)) for t in ('pick', 'mean')}
        got = {t: run[t]() for t in run}                      # warm-up
        ev = {t: [] for t in run}
        for _ in range(args.reps):
            for t in run:
                ev[t] += time_call(run[t], stream, 1)
        index_a = ops.CloudIndex(ctx, a)
        _, status = ops.cloud_distortion_launch(ctx, index_a, cands[0], nrm, ties='mean')
        pairs, over = status.cpu().tolist()
        row = {'case': name, 'n_a': len(a), 'n_b': len(cands[0]), 'tie_pairs': pairs, 'pair_capacity': ops.tie_pair_capacity(len(a)),
               'capacity_exceeded': bool(over), 'pick_event_ms_median': float(np.median(ev['pick'])),
               'pick_event_ms_min': float(np.min(ev['pick'])), 'mean_event_ms_median': float(np.median(ev['mean'])),
               'mean_event_ms_min': float(np.min(ev['mean']))}
        row['mean_over_pick'] = row['mean_event_ms_median'] / row['pick_event_ms_median']
        row['d2_mse_pick_vs_mean_rel'] = float(abs(got['pick'][0]['d2_mse'] / got['mean'][0]['d2_mse'] - 1))
        if not args.gpu_only:
            t0 = time.perf_counter()
            host = pc_metric.cloud_metrics_batch(a, cands, 1023, nrm, ties='mean')
            row['host_mean_wall_ms'] = (time.perf_counter() - t0) * 1e3
            row['d1_equal'] = all(g['d1_sum_AB'] == h['d1_sum_AB'] and g['d1_sum_BA'] == h['d1_sum_BA'] for g, h in zip(got['mean'], host))
            row['d2_mse_gpu_vs_host_mean_rel'] = float(abs(got['mean'][0]['d2_mse'] / host[0]['d2_mse'] - 1))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ties', choices=('pick', 'mean'), default='pick', help='mean: time the tie-averaged D2 beside the default rule')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host_reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--gpu_only', action='store_true', help='skip the host side (profiling runs)')
    args = ap.parse_args()
    ctx = ops.get_context()
    stream = torch.cuda.current_stream(ctx.device)
    if args.ties == 'mean':
        rows = ties_rows(ctx, stream, args)
        if args.out:
            doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
            doc['ties_mean'] = {'device': torch.cuda.get_device_name(ctx.device), 'reps': args.reps, 'results': rows}
            with open(args.out, 'w') as f:
                json.dump(doc, f, indent=1)
        return
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
