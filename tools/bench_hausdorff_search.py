"""What the Hausdorff forms of the search statistics cost beside the plain calls, on tools/bench_count_search.py's chunk:
the first 32 occupied 64^3 blocks of tools/rd_sweep.py's synthetic 512^3 shell, x_hat from c3p under init_checkpoint.make_synthetic_weights,
the encoder's 256 thresholds.

The script records HIP-event medians (results fetched, as the search does) of ops.d1_threshold_stats and ops.d12_threshold_stats (ties to the
lowest (x, y, z); radial unit normals) with and without hausdorff=True -- the same process, the same inputs, the calls interleaved -- and the
ratio of each pair.  No time is a pass/fail condition: nobody has measured this cost before.  The plain calls' numbers are also what a later
comparison against the parent commit's plain call starts from.

    python tools/bench_hausdorff_search.py --out profiles/hausdorff_search_bench.json [--commit <id>]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_rans import _commit, _median_ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--blocks', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
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
    cloud = full[np.isin(ident, keep)][:, :3]
    radial = cloud - cloud.mean(0)
    radial = (radial / np.maximum(np.linalg.norm(radial, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    blocks, binstr = partition_octree(np.hstack([cloud, radial]), [0, 0, 0], [res] * 3, level)
    assert len(blocks) == len(keep)
    dhw = (edge,) * 3

    m = ModelConfigType['c3p'].build(batch_size=a.blocks)
    m.compress([1, 1] + list(dhw))
    m.set_weights(make_synthetic_weights('c3p'))
    mc = m._ctx(ctx)
    x_hat = ops.codec_encode(mc, m._codec(mc), m._voxelize(mc, blocks, dhw).contiguous())['x_hat']
    table = m._dev(mc, 'thr_table', np.array([m._thr32(t) for t in range(len(m.thresholds))], np.float32))
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(ctx.device)
    sizes = [len(b) for b in blocks]
    pts = dev(np.concatenate([np.asarray(b)[:, :3] for b in blocks]).astype(np.int32))
    nrm = dev(np.concatenate([np.asarray(b)[:, 3:6] for b in blocks]).astype(np.float32))
    bof = dev(np.repeat(np.arange(len(blocks), dtype=np.int32), sizes))
    start = dev(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))

    d1 = lambda hd: ops.d1_threshold_stats(mc, x_hat, table, pts, bof, hausdorff=hd)
    d12 = lambda hd: ops.d12_threshold_stats(mc, x_hat, table, pts, bof, start, nrm, hausdorff=hd)
    plain, hd = d12(False), d12(True)
    assert all(np.array_equal(p, h) for p, h in zip(plain, hd)), 'the Hausdorff form changed a shared output'
    times = {}
    for rnd in range(2):          # two interleaved rounds; the second is recorded (the first also warms the workspaces up)
        for name, fn in (('d1_threshold_stats', d1), ('d12_threshold_stats_pick', d12)):
            times[f'{name}_plain_device_ms'] = _median_ms(lambda: fn(False), a.reps, a.warmup)
            times[f'{name}_hausdorff_device_ms'] = _median_ms(lambda: fn(True), a.reps, a.warmup)
    for name in ('d1_threshold_stats', 'd12_threshold_stats_pick'):
        times[f'{name}_hausdorff_over_plain'] = times[f'{name}_hausdorff_device_ms'] / times[f'{name}_plain_device_ms']
    print(json.dumps(times), flush=True)
    live = int(plain[3].max())
    result = dict(commit=a.commit or _commit(), device=torch.cuda.get_device_name(0), blocks=len(blocks), block_edge=edge,
                  input_points=int(len(cloud)), thresholds=int(table.numel()), live_levels=live, reps=a.reps, times=times,
                  largest=dict(d1_hausdorff_AB=int(hd[6].max()), d1_hausdorff_BA=int(hd[7].max()), d2_hausdorff_AB=float(hd[8].max()),
                               d2_hausdorff_BA=float(hd[9].max())),
                  note='synthetic weights: times describe these scores; no pass mark, the comparison to make later is against the parent '
                       "commit's plain call")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
