"""Colour anchor codec (pcc_geo_cnn_v2_amd/anchor_color.py): where the time goes and what the streams cost.

    python tools/bench_color_anchor.py [--reps 10] [--host_reps 1] [--out profiles/color_anchor_bench.json] [--device both|host]

Inputs, seeded and built here: the 527k-point 1024^3 shell with a smooth colour field, and 10^6 distinct uniform points in 1024^3 with
uniform random colours (the worst case: nothing to decorrelate).  Per input, at qstep 16, and per device (gpu =
csrc/color_anchor.hip, host = the numpy path; the entropy coder is the same host C++ on both):
  forward_ms   the tree plan and the forward transform: gpu = device events around upload, kernels and the copy back; host = wall clock;
  inverse_ms   the tree plan and the inverse transform, timed the same way;
  coder_encode_ms / coder_decode_ms   the host coefficient coder alone, wall clock;
  encode_ms / decode_ms   the whole call, wall clock (the call ends with the data on the host).
Medians of --reps (gpu, after a warm-up) / --host_reps (host, at least 1).  Per input and qstep (ev_run_anchor's six default colour steps
and 1 = lossless): bits per input point and BT.709 y/u/v PSNR (peak 255) of the decoded colours against the input's.  --device host
skips everything that needs a GPU: sizes and PSNR do not depend on the device.  The numbers are this codec's: it is not G-PCC, not
RAHT-conformant, and nothing here compares with G-PCC."""
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
from pcc_geo_cnn_v2_amd import anchor_color as C  # noqa: E402
from pcc_geo_cnn_v2_amd import ev_run_anchor  # noqa: E402
from pcc_geo_cnn_v2_amd.utils.pc_metric import psnr, yuv_terms  # noqa: E402

TIMED_QSTEP = 16


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


def smooth_field(points):
    p = np.asarray(points, np.float64) / 1024.0
    c = np.stack([128 + 100 * np.sin(9 * p[:, 0] + 4 * p[:, 1]), 128 + 100 * np.cos(7 * p[:, 1] - 5 * p[:, 2]),
                  128 + 100 * np.sin(6 * p[:, 0] + 8 * p[:, 2])], axis=1)
    return np.clip(np.round(c), 0, 255).astype(np.uint8)


def inputs():
    s1024, _ = shell(1024, radius=0.2, half_width=0.5)
    s1024 = np.unique(np.asarray(s1024, np.int64), axis=0)
    rng = np.random.default_rng(0)
    uniform = rng.permutation(np.unique(rng.integers(0, 1024, (1010000, 3)), axis=0))[:1000000]
    assert len(uniform) == 1000000
    return (('shell1024_smooth', s1024, smooth_field(s1024)), ('uniform1e6_random', uniform, rng.integers(0, 256, (1000000, 3)).astype(np.uint8)))


def yuv_psnr(a, b):
    mse = yuv_terms(a, np.asarray(b, np.float64)).mean(axis=0)
    return {f'{k}_psnr': float(psnr(m, 255 ** 2)) for k, m in zip('yuv', mse)}


def host_forward(p, colors, q):
    plan = C.HostPlan(p)
    return (plan.counts,) + C.forward_host(plan, colors, q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host_reps', type=int, default=1)
    ap.add_argument('--device', choices=('both', 'host'), default='both')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx, device_name, ops = None, None, None
    if args.device == 'both':
        import torch
        from pcc_geo_cnn_v2_amd import ops
        ctx = ops.get_context()
        device_name = torch.cuda.get_device_name(ctx.device)
    results = []
    for name, cloud, colors in inputs():
        from pcc_geo_cnn_v2_amd import ops as O
        n, q = len(cloud), TIMED_QSTEP
        p64, p32, depth = C.check_points(cloud), np.ascontiguousarray(cloud, np.int32), C.depth_of(cloud.max())
        row = {'cloud': name, 'points': int(n), 'resolution': 1024, 'timed_qstep': q, 'rates': {}}
        (counts, dc, coef), row['host_forward_ms'] = wall(lambda: host_forward(p64, colors, q), args.host_reps, warm=False)
        rec, row['host_inverse_ms'] = wall(lambda: C.inverse_host(C.HostPlan(p64), dc, coef, q), args.host_reps, warm=False)
        payload, row['coder_encode_ms'] = wall(lambda: O.color_anchor_encode_coefficients(coef, counts[:3 * depth]), max(args.host_reps, 3))
        _, row['coder_decode_ms'] = wall(lambda: O.color_anchor_decode_coefficients(payload, counts[:3 * depth], n - 1), max(args.host_reps, 3))
        data, row['host_encode_ms'] = wall(lambda: C.encode(cloud, colors, q, 'host'), args.host_reps, warm=False)
        _, row['host_decode_ms'] = wall(lambda: C.decode(data, cloud, 'host'), args.host_reps, warm=False)
        if ctx is not None:
            got, row['gpu_forward_ms'] = events(ctx, lambda: ops.color_anchor_transform(ctx, p32, colors, depth, q), args.reps)
            grec, row['gpu_inverse_ms'] = events(ctx, lambda: ops.color_anchor_inverse(ctx, ops.color_anchor_plan(ctx, p32, depth)[0], coef, dc, n,
                                                                                          depth, q), args.reps)
            gdata, row['gpu_encode_ms'] = wall(lambda: C.encode(cloud, colors, q, 'gpu', ctx), args.reps)
            gdec, row['gpu_decode_ms'] = wall(lambda: C.decode(data, cloud, 'gpu', ctx), args.reps)
            row['identical'] = bool(np.array_equal(got[0], counts) and np.array_equal(got[2], dc) and np.array_equal(got[3], coef) and
                                    np.array_equal(grec, rec) and gdata == data and np.array_equal(gdec, rec))
            row['forward_speedup'] = row['host_forward_ms'] / row['gpu_forward_ms']
            row['inverse_speedup'] = row['host_inverse_ms'] / row['gpu_inverse_ms']
        print(json.dumps({k: v for k, v in row.items() if k != 'rates'}), flush=True)
        for rate, qs in (('lossless', 1), *ev_run_anchor.COLOR_DEFAULT_RATES.items()):
            stream = C.encode(cloud, colors, qs, 'host')
            dec = C.decode(stream, cloud, 'host')
            assert qs != 1 or np.array_equal(dec, colors)
            row['rates'][rate] = {'qstep': qs, 'bytes': len(stream), 'bits_per_input_point': 8 * len(stream) / n, **yuv_psnr(colors, dec)}
            print(json.dumps({'cloud': name, 'rate': rate, **row['rates'][rate]}), flush=True)
        results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': device_name, 'times': 'gpu and host' if ctx is not None else 'host only; gpu not measured', 'reps': args.reps,
                       'host_reps': args.host_reps, 'note': 'colour anchor of this project; not G-PCC, not RAHT-conformant, not comparable with '
                       'G-PCC numbers', 'results': results}, f, indent=1)


if __name__ == '__main__':
    main()
