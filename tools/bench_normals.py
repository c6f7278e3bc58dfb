#!/usr/bin/env python
"""Time point-normal estimation (pcc_estimate_normals, csrc/normals.hip) on one MI355X, beside the numpy / scipy restatement of the
same definition (tests/_normals_ref.py: cKDTree kNN + exact int64 scatter matrices + numpy.linalg.eigh) on the host.

Clouds: the voxelised sphere shell at 1024^3 of the tests (~5.3e5 points), a larger shell of ~1e6 points, and 1e6 uniform random
points in a 1024^3 cube.  GPU figures: median over --iters calls of HIP events around the C call alone (input on the device,
workspace allocated once), and the whole ops.estimate_normals call (host numpy in, host numpy out).  One JSON line per cloud.

    timeout -k 10 600 python tools/bench_normals.py [--k 16] [--iters 20] [--cpu] [--out normals.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def clouds():
    import _normals_ref as R
    rng = np.random.default_rng(0)
    yield 'shell_1024', R.shell(1024, radius=0.2, half_width=0.5)[0]
    yield 'shell_1e6', R.shell(1024, radius=0.275, half_width=0.5)[0]
    yield 'uniform_1e6', rng.integers(0, 1024, (1000000, 3)).astype(np.int32)


def cpu_restatement(p, k):
    import _normals_ref as R
    t0 = time.perf_counter()
    knn = R.knn_ref(p, k)
    M = R.scatter_ref(p, knn).astype(np.float64)
    np.linalg.eigh(M)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--cpu', action='store_true', help='also time the host restatement (seconds per cloud)')
    ap.add_argument('--only', default=None, help='comma-separated cloud names')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from pcc_geo_cnn_v2_amd import _lib as L, ops
    ctx = ops.get_context(torch.device('cuda', 0))
    rows = []
    for name, p in clouds():
        if args.only and name not in args.only.split(','):
            continue
        n = len(p)
        pts = torch.from_numpy(p).to(ctx.device)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=ctx.device)
        ws = torch.empty((L.lib().pcc_normals_workspace_bytes(n, args.k),), dtype=torch.uint8, device=ctx.device)

        def call():
            L.check(L.lib().pcc_estimate_normals(ctx.handle, C.c_void_p(pts.data_ptr()), n, args.k, None, C.c_void_p(nrm.data_ptr()),
                                                 None, C.c_void_p(ws.data_ptr()), ctx.stream), 'pcc_estimate_normals')
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        dev_ms = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            dev_ms.append(a.elapsed_time(b))
        e2e_ms = []
        for _ in range(max(3, args.iters // 4)):
            t0 = time.perf_counter()
            ops.estimate_normals(ctx, p, k=args.k)
            e2e_ms.append((time.perf_counter() - t0) * 1e3)
        row = dict(cloud=name, points=n, k=args.k, gpu_call_ms_median=float(np.median(dev_ms)), gpu_call_ms_min=float(np.min(dev_ms)),
                   gpu_call_ms_max=float(np.max(dev_ms)), ops_call_ms_median=float(np.median(e2e_ms)))
        if args.cpu:
            row['cpu_restatement_s'] = cpu_restatement(p, args.k)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
