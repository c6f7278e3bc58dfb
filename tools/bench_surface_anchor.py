"""Surface anchor codec (pcc_geo_cnn_v2_amd/anchor_surface.py): where the time goes and what the streams cost, beside
the octree anchor on the same clouds.

    python tools/bench_surface_anchor.py [--reps 10] [--host_reps 1] [--out profiles/surface_anchor_bench.json] [--device both|host]

Inputs: the 527k-point 1024^3 shell and 10^6 uniform points in 1024^3, the stand-ins of the other bench tools.  Per input, rate
(node_log2 of ev_run_anchor's four default rates) and device (gpu = csrc/surface_anchor.hip, host = the numpy path; the entropy coder
and the block stream's coder are the same host C++ on both):
  fit_ms          leaves, edge list and vertices: gpu = device events around upload, kernels and the copies back; host = wall clock;
  reconstruct_ms  the decoder's count, raster, sort and unique from leaves, edge list and vertices, timed the same way;
  encode_ms / decode_ms   the whole call, wall clock (the call ends with the data on the host).
Medians of --reps (gpu, after a warm-up) / --host_reps (host, at least 1).  Per input and rate: bits per input point and D1 PSNR (peak 1023) of the
surface anchor, and of the octree anchor at its six default rates.  --device host skips everything that needs a GPU: sizes and PSNR
do not depend on the device.  The numbers are these codecs': neither is G-PCC and nothing here compares with G-PCC."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from _normals_ref import shell  # noqa: E402
from pcc_geo_cnn_v2_amd import anchor_octree as A  # noqa: E402
from pcc_geo_cnn_v2_amd import anchor_surface as S  # noqa: E402
from pcc_geo_cnn_v2_amd import ev_run_anchor  # noqa: E402
from pcc_geo_cnn_v2_amd.utils.pc_metric import compute_metrics  # noqa: E402


def wall(fn, reps, warm=True):
    out, t = (fn() if warm else None), []                 # warm-up (the numpy path has nothing to warm)
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(t))


def events(ctx, fn, reps):
    import torch
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
    ap.add_argument('--host_reps', type=int, default=1)
    ap.add_argument('--device', choices=('both', 'host'), default='both')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx, device_name = None, None
    if args.device == 'both':
        import torch
        from pcc_geo_cnn_v2_amd import ops
        ctx = ops.get_context()
        device_name = torch.cuda.get_device_name(ctx.device)
    s1024, _ = shell(1024, radius=0.2, half_width=0.5)
    uniform = np.random.default_rng(0).integers(0, 1024, (1000000, 3))
    results = []
    for name, cloud in (('shell1024', s1024), ('uniform1e6', uniform)):
        row = {'cloud': name, 'points': int(len(cloud)), 'resolution': 1024, 'surface': {}, 'octree': {}}
        for rate, k in ev_run_anchor.SURFACE_DEFAULT_RATES.items():
            r = {'node_log2': k}
            model, r['host_fit_ms'] = wall(lambda: S.vertices(cloud, 1024, k, 'host'), args.host_reps, warm=False)
            dec, r['host_reconstruct_ms'] = wall(lambda: S.surface_points(*model, 1024, k, 'host'), args.host_reps, warm=False)
            data, r['host_encode_ms'] = wall(lambda: S.encode(cloud, 1024, k, 'host'), args.host_reps, warm=False)
            _, r['host_decode_ms'] = wall(lambda: S.decode(data, 'host'), args.host_reps, warm=False)
            if ctx is not None:
                got, r['gpu_fit_ms'] = events(ctx, lambda: S.vertices(cloud, 1024, k, 'gpu', ctx), args.reps)
                got_dec, r['gpu_reconstruct_ms'] = events(ctx, lambda: S.surface_points(*model, 1024, k, 'gpu', ctx), args.reps)
                gpu_data, r['gpu_encode_ms'] = wall(lambda: S.encode(cloud, 1024, k, 'gpu', ctx), args.reps)
                _, r['gpu_decode_ms'] = wall(lambda: S.decode(data, 'gpu', ctx), args.reps)
                r['identical'] = bool(all(np.array_equal(a, b) for a, b in zip(got, model)) and np.array_equal(got_dec, dec) and gpu_data == data)
            h = S.read_header(data)
            r.update(leaves=h['leaves'], edges=h['edges'], vertices=h['vertices'], decoded_points=int(len(dec)), bytes=len(data),
                     block_stream_bytes=h['octree_len'], bits_per_input_point=8 * len(data) / len(cloud),
                     d1_psnr=float(compute_metrics(cloud, dec, 1023)['d1_psnr']))
            row['surface'][rate] = r
            print(json.dumps({'cloud': name, 'rate': rate, **r}), flush=True)
        for rate, scale in ev_run_anchor.DEFAULT_RATES.items():
            data = A.encode(cloud, 1024, scale, 'host')
            dec = A.decode(data, 'host')
            row['octree'][rate] = {'scale': f'{scale[0]}/{scale[1]}', 'bytes': len(data), 'decoded_points': int(len(dec)),
                                   'bits_per_input_point': 8 * len(data) / len(cloud), 'd1_psnr': float(compute_metrics(cloud, dec, 1023)['d1_psnr'])}
            print(json.dumps({'cloud': name, 'rate': rate, **row['octree'][rate]}), flush=True)
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': device_name, 'times': 'gpu and host' if ctx is not None else 'host only; gpu not measured', 'reps': args.reps,
                       'host_reps': args.host_reps, 'note': 'surface and octree anchors of this project; not G-PCC, not trisoup-conformant, not '
                       'comparable with G-PCC numbers', 'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
