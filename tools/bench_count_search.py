"""Count search on one chunk of 32 blocks of 64^3: what scoring a ladder of candidate counts costs beside the threshold
search it mirrors.

The setting is tools/bench_topk.py's: the first 32 occupied 64^3 blocks of tools/rd_sweep.py's synthetic 512^3 shell, x_hat from c3p under
init_checkpoint.make_synthetic_weights.  The script records
  * HIP-event medians on that x_hat: ops.rank_levels alone (J = 33 and J = 255), ops.d1_count_stats at J = 33 and J = 255 (results
    fetched) beside ops.d1_threshold_stats with the encoder's 256 thresholds on the same tensor;
  * encode_block_range (the per-block part of the encoder, wall clock) under the adaptive threshold search, count_scale = 1 and
    count_search = the CLI's default ladder.
No time is a pass/fail condition.  Synthetic weights are not trained weights: no rate-distortion claim is made.

    python tools/bench_count_search.py --out profiles/count_search_bench.json [--commit <id>]
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
    from pcc_geo_cnn_v2_amd import model_opt as MO
    from pcc_geo_cnn_v2_amd import ops
    from pcc_geo_cnn_v2_amd.compress_octree import COUNT_SEARCH_DEFAULT
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
    table = m._dev(mc, 'thr_table', np.array([m._thr32(t) for t in range(len(m.thresholds))], np.float32))
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(b)[:, :3] for b in blocks]).astype(np.int32))).to(ctx.device)
    bof = torch.from_numpy(np.concatenate([np.full(len(b), i, np.int32) for i, b in enumerate(blocks)])).to(ctx.device)
    lo, hi, _ = COUNT_SEARCH_DEFAULT
    rows = {J: torch.from_numpy(MO.count_rows(blocks, MO.count_ladder(lo, hi, J), n)).to(ctx.device) for J in (33, 255)}
    live = {J: int(ops.d1_count_stats(mc, x_hat, rows[J], pts, bof)[3].max()) for J in rows}
    kernels = dict(
        rank_levels_j33_device_ms=_median_ms(lambda: ops.rank_levels(mc, x_hat, rows[33]), a.reps, a.warmup),
        rank_levels_j255_device_ms=_median_ms(lambda: ops.rank_levels(mc, x_hat, rows[255]), a.reps, a.warmup),
        d1_count_stats_j33_device_ms=_median_ms(lambda: ops.d1_count_stats(mc, x_hat, rows[33], pts, bof), a.reps, a.warmup),
        d1_count_stats_j255_device_ms=_median_ms(lambda: ops.d1_count_stats(mc, x_hat, rows[255], pts, bof), a.reps, a.warmup),
        d1_threshold_stats_t256_device_ms=_median_ms(lambda: ops.d1_threshold_stats(mc, x_hat, table, pts, bof), a.reps, a.warmup))
    kernels['live_levels'] = {'j33': live[33], 'j255': live[255], 't256': int(ops.d1_threshold_stats(mc, x_hat, table, pts, bof)[3].max())}
    kernels['rank_share_of_count_stats_j33'] = kernels['rank_levels_j33_device_ms'] / kernels['d1_count_stats_j33_device_ms']
    kernels['rank_share_of_count_stats_j255'] = kernels['rank_levels_j255_device_ms'] / kernels['d1_count_stats_j255_device_ms']
    kernels['count_j33_over_threshold_t256'] = kernels['d1_count_stats_j33_device_ms'] / kernels['d1_threshold_stats_t256_device_ms']
    print(json.dumps(kernels), flush=True)

    policies = []
    for name, how in (('search', {}), ('count', dict(count_scale=1.0)), ('count_search', dict(count_search=COUNT_SEARCH_DEFAULT))):
        wall = []
        for rep in range(a.model_reps + 1):                  # (the first call warms the pools and caches up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            strings, _, points, names, _ = m.encode_block_range(ctx, blocks, res, opt_metrics=('d1_mse',), **how)
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        row = dict(policy=name, encode_block_range_wall_ms=statistics.median(wall[1:]), string_bytes=sum(len(v) for s in strings for v in s),
                   decoded_points=int(sum(len(p[0]) for p in points)))
        print(json.dumps(row), flush=True)
        policies.append(row)

    result = dict(commit=a.commit or _commit(), device=torch.cuda.get_device_name(0), blocks=len(blocks), block_edge=edge,
                  chunk_mbytes=len(blocks) * n * 4 / 2 ** 20, input_points=int(len(cloud)), reps=a.reps, model_reps=a.model_reps,
                  positive_voxels_per_block_median=float(np.median(positive)), positive_share=float(positive.sum() / (len(blocks) * n)),
                  count_ladder=list(COUNT_SEARCH_DEFAULT), kernels=kernels, policies=policies,
                  note='synthetic weights: times describe these scores, no rate-distortion claim is made')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
