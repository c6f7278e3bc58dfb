"""Mesh -> voxelised cloud time: ops.mesh_to_points (include/pcc_geo.h "mesh sampling") beside the host path
utils/mesh_sampling.mesh_to_points, which returns the same bits.

    python tools/bench_mesh.py [--reps 10] [--host_reps 3] [--out profiles/mesh_bench.json]

Meshes: a 10^5-triangle random soup (areas 1e-12 .. 1) and an icosphere of 1.31 * 10^6 triangles.  Configurations: 5 * 10^5 samples
at vg 64 and 10^7 samples at vg 1024.  GPU: device events around the whole call (host checks, uploads, the kernels, the count and
the copy back of the voxels), median of --reps after a warm-up.  Host: median wall clock of --host_reps calls.  Both outputs are
checked to be identical."""
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

import _mesh_ref as R  # noqa: E402
from pcc_geo_cnn_v2_amd import ops  # noqa: E402
from pcc_geo_cnn_v2_amd.utils import mesh_sampling as MS  # noqa: E402


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
    meshes = (('soup1e5', R.soup(100000, 0, zero=100)), ('icosphere1.3e6', R.icosphere(8)))
    results = []
    for name, (v, f) in meshes:
        for n, vg in ((500000, 64), (10000000, 1024)):
            pts, t = gpu_time(ctx, lambda: ops.mesh_to_points(ctx, v, f, n, vg, 0), args.reps)
            row = {'mesh': name, 'triangles': int(len(f)), 'n_samples': n, 'vg_size': vg, 'points': int(len(pts)), 'gpu_event_ms': t}
            if not args.gpu_only:
                ref, row['host_ms'] = host_time(lambda: MS.mesh_to_points(v, f, n, vg, 0), args.host_reps)
                row['identical'] = bool(ref.tobytes() == pts.tobytes())
                row['speedup'] = row['host_ms'] / t['median']
            print(json.dumps(row), flush=True)
            results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(ctx.device), 'reps': args.reps, 'host_reps': args.host_reps,
                       'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
