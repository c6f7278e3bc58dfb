"""Count-matched thresholding (cnt1) on one chunk of 32 blocks of 64^3: what the top-k selection costs beside the two
policies the codec already has.

The blocks are the first 32 occupied 64^3 blocks of tools/rd_sweep.py's synthetic 512^3 shell, x_hat comes from c3p under
init_checkpoint.make_synthetic_weights.  The script records
  * HIP-event medians on that x_hat: ops.topk_compact (k = the input points of each block), ops.threshold_compact (fixed threshold, clipped)
    and the D1 search's statistics call (ops.d1_threshold_stats, its results fetched);
  * the whole compress_blocks call on the same 32 blocks under the three policies -- adaptive search, --fixed_threshold, count_scale = 1 --
    as wall-clock medians, with the bytes of the strings and the D1 PSNR the encoder reports; compress_blocks includes the whole-cloud
    metrics of the candidate (host KD-trees, whose time grows with the decoded points), encode_block_range is the per-block part alone.
Synthetic weights are not trained weights: bytes and PSNR say what the three code paths do with THESE scores, nothing about a trained model.

    python tools/bench_topk.py --out profiles/topk_bench.json [--commit <id>]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_rans import _commit, _median_ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--blocks', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--model_reps', type=int, default=5)
    ap.add_argument('--commit', default=None, help='what to record as the measured commit (default: git describe)')
    a = ap.parse_args(argv)
    import torch
    from pcc_geo_cnn_v2_amd import ops
    from pcc_geo_cnn_v2_amd.init_checkpoint import make_synthetic_weights
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree
    from tools.rd_sweep import synthetic_cloud

    ctx = ops.get_context(torch.device('cuda', 0))
    res, level = 512, 3
    edge = res >> level
    full = synthetic_cloud(res)
    cell = (full[:, :3] // edge).astype(np.int64)
    ident = (cell[:, 0] * 64 + cell[:, 1]) * 64 + cell[:, 2]
    keep = np.unique(ident)[:a.blocks]
    cloud = full[np.isin(ident, keep)]
    blocks, binstr = partition_octree(cloud, [0, 0, 0], [res] * 3, level)
    assert len(blocks) == len(keep)
    dhw = (edge,) * 3
    n = edge ** 3

    m = ModelConfigType['c3p'].build(batch_size=a.blocks)
    m.compress([1, 1] + list(dhw))
    m.set_weights(make_synthetic_weights('c3p'))
    mc = m._ctx(ctx)
    x = m._voxelize(mc, blocks, dhw)
    x_hat = ops.codec_encode(mc, m._codec(mc), x.contiguous())['x_hat']
    positive = (x_hat > 0).sum(dim=(1, 2, 3)).cpu().numpy()
    k = torch.tensor([len(b) for b in blocks], dtype=torch.int32, device=ctx.device)
    half = len(m.thresholds) // 2
    thr = m._thr_tensor(mc, [half] * len(blocks))
    table = m._dev(mc, 'thr_table', np.array([m._thr32(t) for t in range(len(m.thresholds))], np.float32))
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(b)[:, :3] for b in blocks]).astype(np.int32))).to(ctx.device)
    bof = torch.from_numpy(np.concatenate([np.full(len(b), i, np.int32) for i, b in enumerate(blocks)])).to(ctx.device)
    _, counts = ops.topk_compact(mc, x_hat, k)
    kernels = dict(
        topk_compact_device_ms=_median_ms(lambda: ops.topk_compact(mc, x_hat, k), a.reps, a.warmup),
        threshold_compact_device_ms=_median_ms(lambda: ops.threshold_compact(mc, x_hat, thr, clip=True), a.reps, a.warmup),
        d1_search_stats_device_ms=_median_ms(lambda: ops.d1_threshold_stats(mc, x_hat, table, pts, bof), a.reps, a.warmup))
    kernels['topk_over_threshold_compact'] = kernels['topk_compact_device_ms'] / kernels['threshold_compact_device_ms']
    kernels['topk_over_d1_search'] = kernels['topk_compact_device_ms'] / kernels['d1_search_stats_device_ms']
    print(json.dumps(kernels), flush=True)

    policies = []
    for name, how in (('search', {}), ('fixed', dict(fixed_threshold=True)), ('count', dict(count_scale=1.0))):
        wall = []
        for rep in range(a.model_reps + 1):                  # (the first call warms the pools and caches up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data, meta, _ = m.compress_blocks(ctx, blocks, binstr, cloud, res, level, opt_metrics=('d1_mse',), **how)
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        block_part = []                                      # the per-block part alone: no whole-cloud metrics, no KD-tree over the decoded cloud
        for rep in range(a.model_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.encode_block_range(ctx, blocks, res, opt_metrics=('d1_mse',), **how)
            torch.cuda.synchronize()
            block_part.append(1e3 * (time.perf_counter() - t0))
        row = dict(policy=name, compress_blocks_wall_ms=statistics.median(wall[1:]), encode_block_range_wall_ms=statistics.median(block_part),
                   string_bytes=sum(len(v) for s, _ in data[0] for v in s), threshold_bytes=len(data[0]),
                   d1_psnr=float(meta[0]['metrics']['d1_psnr']), decoded_points=int(len(meta[0]['blocks_full'])))
        print(json.dumps(row), flush=True)
        policies.append(row)

    result = dict(commit=a.commit or _commit(), device=torch.cuda.get_device_name(0), blocks=len(blocks), block_edge=edge,
                  chunk_mbytes=len(blocks) * n * 4 / 2 ** 20, input_points=int(len(cloud)), reps=a.reps, model_reps=a.model_reps,
                  positive_voxels_per_block_median=float(np.median(positive)), positive_share=float(positive.sum() / (len(blocks) * n)),
                  topk_points=int(counts.sum().item()), kernels=kernels, policies=policies,
                  note='synthetic weights: bytes and PSNR describe these scores, not a trained model')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
