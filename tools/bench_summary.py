#!/usr/bin/env python
"""Time the training summaries (pcc_tensor_histogram / pcc_occupancy_scores, csrc/summary.hip) on one MI355X.

1. One full c3p summary at batch 32, 64^3 (the eleven tensor histograms + the scores; x_tilde_quant's histogram follows from the
   scores) on the tensors of a real forward, three ways in one process: the HIP calls, a torch-on-device restatement
   (torch.bucketize on float64 copies, torch.bincount / min / max / sum) and tf_summary.histogram_host on host copies.
2. pcc_tensor_histogram alone on 32 x 64^3 floats of {0,1} data, a trained-looking x_tilde and N(0,1), each beside the time to read
   the tensor's 33.5 MB at 8 TB/s.
3. Trainer steps per second over --train_steps steps with summary_interval 0 and 100.

Device events, median of --iters after --warmup; host figures are wall clock.

    timeout -k 10 900 python tools/bench_summary.py [--out profiles/summary_bench.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pcc_geo_cnn_v2_amd import ops, train  # noqa: E402
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType  # noqa: E402
from pcc_geo_cnn_v2_amd.utils import tf_summary  # noqa: E402
from tools.bench_train import seeded_blocks  # noqa: E402


def device_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def torch_histogram(t, limits):
    """The fields of pcc_histogram with torch operators on the device."""
    v = t.reshape(-1)
    fin = torch.isfinite(v)
    d = v[fin].double()
    counts = torch.bincount(torch.bucketize(d, limits, right=True), minlength=tf_summary.NUM_BUCKETS)
    return counts, fin.sum(), d.min(), d.max(), d.sum(), (d * d).sum()


def torch_scores(x, xt):
    q, qt = torch.round(torch.clamp(x.reshape(-1), 0, 1)) == 1, torch.round(torch.clamp(xt.reshape(-1), 0, 1)) == 1
    return (qt & q).sum(), (~qt & ~q).sum(), (qt & ~q).sum(), (~qt & q).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch_size', type=int, default=32)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--train_steps', type=int, default=300)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    pctx = train.training_context(torch.device('cuda', 0))
    R, B = a.resolution, a.batch_size
    res = dict(model='c3p', batch_size=B, resolution=R, device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup)

    # 1. one full summary
    model = ModelConfigType['c3p'].build(seed=42)
    model.compress([1, 1, R, R, R])
    graph = train.TrainGraph(model, pctx)
    blocks = seeded_blocks(B, R)
    x = torch.from_numpy(blocks).cuda()
    gen = torch.Generator(device='cuda')
    gen.manual_seed(0)
    noise = [torch.rand(s, generator=gen, device='cuda') - .5 for s in graph.latent_shapes(tuple(x.shape))]
    with torch.no_grad():
        out = graph.loss(x, noise, 1e-4, tensors=True)
    t = out['tensors']
    names = list(t)
    tensors = [t[k].contiguous() for k in names]
    res['summary_tensors'] = {k: int(v.numel()) for k, v in zip(names, tensors)}
    limits = torch.from_numpy(np.array(tf_summary.default_bucket_limits())).cuda()

    def hip():
        ops.tensor_histograms_launch(pctx, tensors)
        ops.occupancy_scores_launch(pctx, t['x'], t['x_tilde'])

    def torch_dev():
        for v in tensors:
            torch_histogram(v, limits)
        torch_scores(t['x'], t['x_tilde'])

    def host():
        t0 = time.perf_counter()
        for v in tensors:
            tf_summary.histogram_host(v.cpu().numpy())
        return (time.perf_counter() - t0) * 1e3

    s = dict(hip_calls=device_ms(hip, a.iters, a.warmup), torch_on_device=device_ms(torch_dev, a.iters, a.warmup))
    s['histogram_host_on_copies_ms'] = float(np.median([host() for _ in range(3)]))
    wall = []
    for _ in range(a.warmup + a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train.summarize(pctx, out)
        wall.append((time.perf_counter() - t0) * 1e3)
    s['summarize_wall_ms'] = float(np.median(wall[a.warmup:]))
    s['torch_over_hip'] = s['torch_on_device']['median_ms'] / s['hip_calls']['median_ms']
    res['full_summary'] = s
    print(json.dumps(dict(full_summary=s)), flush=True)

    # 2. the 8.4 M-element kernel alone
    n = B * R ** 3
    rng = np.random.default_rng(1)
    trained = np.where(blocks.reshape(-1) > 0, 1 - np.abs(rng.normal(0, .02, n)), np.abs(rng.normal(0, .002, n))).astype(np.float32)
    inputs = {'binary': x.reshape(-1), 'trained_x_tilde': torch.from_numpy(trained).cuda(),
              'normal': torch.from_numpy(rng.standard_normal(n, dtype=np.float32)).cuda()}
    roof_ms = n * 4 / 8e12 * 1e3
    k = {}
    for name, v in inputs.items():
        r = device_ms(lambda: ops.tensor_histograms_launch(pctx, [v]), a.iters, a.warmup)
        r['read_at_8TBs_ms'] = roof_ms
        r['roof_fraction'] = roof_ms / r['median_ms']
        k[name] = r
    res['kernel_alone'] = k
    print(json.dumps(dict(kernel_alone=k)), flush=True)

    # 3. trainer steps per second with and without summaries
    pts = [np.argwhere(b > 0) for b in seeded_blocks(2 * B, R, seed=3)]
    tr = {}
    for interval in (0, 100):
        d = tempfile.mkdtemp(prefix='bench_summary_')
        try:
            trainer = train.Trainer(ModelConfigType['c3p'].build(seed=42), d, pts, pts[:B], resolution=R, batch_size=B, max_steps=a.train_steps,
                                    validation_interval=10 ** 9, validation_steps=1, log=None, summary_interval=interval)
            trainer.last_val = 0              # no validation: the steps alone
            trainer.max_steps = 5
            trainer.run()                     # warm-up
            trainer.max_steps = 5 + a.train_steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.run()
            torch.cuda.synchronize()
            tr[f'summary_interval_{interval}'] = dict(steps=a.train_steps, steps_per_s=a.train_steps / (time.perf_counter() - t0))
        finally:
            shutil.rmtree(d, ignore_errors=True)
    res['trainer'] = tr
    print(json.dumps(dict(trainer=tr)), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
