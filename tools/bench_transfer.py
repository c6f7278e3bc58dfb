"""Colour transfer time and what it buys: ops.transfer_colors beside ops.map_colors rank 1 on the same inputs in the same process,
the host restatement's time, and the colour PSNR of a decoded cloud coloured by rank 1, rank 2 and the transfer.

    python tools/bench_transfer.py [--reps 10] [--out profiles/transfer_bench.json]

Cases: those of tools/bench_color.py (10^6 uniform points and the shell, each onto its decoded-like copy).  GPU: device events
around the whole call (index builds, uploads, kernels, the copy back), median of --reps after a warm-up.  The transfer searches B's
index twice per original point (the distance, then the scatter) and A's index once per decoded point that nobody voted for;
map_colors searches A's index once per decoded point: the number to read is their ratio.  Host: pc_metric.transfer_colors_host,
median wall clock of --host_reps calls, checked to give the GPU's bytes.  PSNR: ops.cloud_color_distortion + pc_metric.color_table
of the decoded cloud under each of the three colourings (max of both directions, as every report of the project)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_color import cases, gpu_time, host_time  # noqa: E402
from pcc_geo_cnn_v2_amd import ops  # noqa: E402
from pcc_geo_cnn_v2_amd.utils import pc_metric  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host_reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--gpu_only', action='store_true', help='skip the host restatement')
    args = ap.parse_args()
    ctx = ops.get_context()
    results = []
    for name, a, ca, b, _ in cases():
        (transfer, votes), t_transfer = gpu_time(ctx, lambda: ops.transfer_colors(ctx, a, ca, b, return_votes=True), args.reps)
        rank1, t_rank1 = gpu_time(ctx, lambda: ops.map_colors(ctx, a, ca, b, rank=1), args.reps)
        rank2 = ops.map_colors(ctx, a, ca, b, rank=2)
        index_a = ops.CloudIndex(ctx, a)
        row = {'case': name, 'n_a': len(a), 'n_b': len(b), 'fallback_share': float((votes == 0).mean()), 'max_votes': int(votes.max()),
               'transfer_colors_event_ms': t_transfer, 'map_colors_rank1_event_ms': t_rank1,
               'transfer_over_rank1': t_transfer['median'] / t_rank1['median']}
        for key, colours in (('rank1', rank1), ('rank2', rank2), ('transfer', transfer)):
            tally = ops.cloud_color_distortion(ctx, index_a, ca, b, colours)
            table = pc_metric.color_table(tally, len(a), len(b))
            row[f'{key}_psnr'] = {k: float(table[f'{k}_psnr']) for k in pc_metric.COLOR_KEYS}
            row[f'{key}_ab_mse'] = [float(v) / len(a) for v in tally[:3]]
        if not args.gpu_only:
            (host, host_votes), row['host_transfer_ms'] = host_time(lambda: pc_metric.transfer_colors_host(a, ca, b), args.host_reps)
            row['equal_to_host'] = bool(np.array_equal(host, transfer) and np.array_equal(host_votes, votes))
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(ctx.device), 'reps': args.reps, 'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
