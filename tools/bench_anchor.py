"""Octree anchor codec (pcc_geo_cnn_v2_amd/anchor_octree.py): where the time goes and what the streams cost.

    python tools/bench_anchor.py [--reps 10] [--host_reps 3] [--out profiles/anchor_bench.json]

Inputs: the 527k-point 1024^3 shell and 10^6 uniform points in 1024^3, the stand-ins of the other bench tools.  Per input and device
(gpu = the HIP tree, host = the numpy tree; the entropy coder is the same host C++ on both), at scale 1/1:
  tree_ms    the tree and its contexts: gpu = device events around upload, kernels and the one copy back; host = wall clock;
  coder_ms   the host range coder over all occupancy bytes, wall clock;
  encode_ms / decode_ms   the whole call, wall clock (the call ends with the data on the host).
Medians of --reps (gpu) / --host_reps (host) after a warm-up.  Per input: bits per input point at the six default rates of
ev_run_anchor and losslessly, with and without the neighbour contexts (the same build, no_context=True), both devices checked to
give the same bytes.  The numbers are this codec's: it is not G-PCC and nothing here compares with G-PCC."""
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
from pcc_geo_cnn_v2_amd import anchor_octree as A  # noqa: E402
from pcc_geo_cnn_v2_amd import ev_run_anchor, ops  # noqa: E402


def wall(fn, reps):
    out, t = fn(), []                                     # warm-up
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t))


def events(ctx, fn, reps):
    stream = torch.cuda.current_stream(ctx.device)
    out, t = fn(), []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return out, float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host_reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = ops.get_context()
    s1024, _ = shell(1024, radius=0.2, half_width=0.5)
    uniform = np.random.default_rng(0).integers(0, 1024, (1000000, 3))
    results = []
    for name, cloud in (('shell1024', s1024), ('uniform1e6', uniform)):
        row = {'cloud': name, 'points': int(len(cloud)), 'resolution': 1024}
        (counts, occ, n6), row['gpu_tree_ms'] = events(ctx, lambda: A.tree(cloud, (1, 1), 'gpu', ctx), args.reps)
        tree_host, row['host_tree_ms'] = wall(lambda: A.tree(cloud, (1, 1), 'host'), args.host_reps)
        row['tree_identical'] = bool(all(np.array_equal(a, b) for a, b in zip((counts, occ, n6), tree_host)))
        row['tree_speedup'] = row['host_tree_ms'] / row['gpu_tree_ms']
        row['internal_nodes'] = int(len(occ))
        _, row['coder_ms'] = wall(lambda: ops.anchor_encode_nodes(occ, n6), args.host_reps)
        for dev, reps in (('gpu', args.reps), ('host', args.host_reps)):
            data, row[f'{dev}_encode_ms'] = wall(lambda: A.encode(cloud, 1024, (1, 1), dev, ctx), reps)
            _, row[f'{dev}_decode_ms'] = wall(lambda: A.decode(data, dev, ctx), reps)
        rates = dict(ev_run_anchor.DEFAULT_RATES, lossless=(1, 1))
        row['bits_per_input_point'], row['bits_per_input_point_no_context'], same = {}, {}, True
        for rate, scale in rates.items():
            data = A.encode(cloud, 1024, scale, 'gpu', ctx)
            same = same and data == A.encode(cloud, 1024, scale, 'host')
            plain = A.encode(cloud, 1024, scale, 'gpu', ctx, no_context=True)
            assert np.array_equal(A.decode(plain, 'gpu', ctx, no_context=True), A.reconstruct(cloud, 1024, scale))
            row['bits_per_input_point'][rate] = 8 * len(data) / len(cloud)
            row['bits_per_input_point_no_context'][rate] = 8 * len(plain) / len(cloud)
        row['bytes_identical'] = bool(same)
        row['context_gain_lossless'] = 1 - row['bits_per_input_point']['lossless'] / row['bits_per_input_point_no_context']['lossless']
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(ctx.device), 'reps': args.reps, 'host_reps': args.host_reps,
                       'note': 'octree anchor of this project; not G-PCC, not comparable with G-PCC numbers', 'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
