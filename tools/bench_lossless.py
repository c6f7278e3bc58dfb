"""The lossless occupancy layer (occ1) on one cloud at the six designed c3p rate points: what it costs in bytes and time.

The cloud is tools/rd_sweep.py's synthetic 512^3 shell at octree level 3 (64^3 blocks).  For each designed weight set
(init_checkpoint.make_cell_codec_weights, levels 1..6) the script records
  * over ALL blocks: base bytes (y + z strings), occupancy bytes, and total bits per input point -- strings only and with the
    container's 5 bytes per block -- beside the octree anchor's lossless bits per point on the same cloud;
  * over the first chunk of --blocks blocks: coded symbols m and lanes L per block (m from the host restatement tests/_occ_ref.py,
    L from the strings' first byte), and HIP-event medians of the occ1 encode launch, the occ1 decode launch (upload of the strings
    included) and the synthesis transform of the same chunk (per-layer forward on y_hat).
Designed weights are not trained weights: the rates say what the format costs under THESE models, nothing about a trained one.

    python tools/bench_lossless.py --out profiles/lossless_bench.json [--commit <id>]
"""
import argparse
import collections
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from tools.bench_rans import _commit, _median_ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--levels', type=int, nargs='+', default=[1, 2, 3, 4, 5, 6])
    ap.add_argument('--blocks', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--commit', default=None, help='what to record as the measured commit (default: git describe)')
    a = ap.parse_args(argv)
    import torch
    import _occ_ref as R
    from pcc_geo_cnn_v2_amd import anchor_octree, ops
    from pcc_geo_cnn_v2_amd.init_checkpoint import make_cell_codec_weights
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree
    from tools.rd_sweep import synthetic_cloud

    ctx = ops.get_context(torch.device('cuda', 0))
    res, level = 512, 3
    cloud = synthetic_cloud(res)
    blocks, binstr = partition_octree(cloud, [0, 0, 0], [res] * 3, level)
    dhw = (res >> level,) * 3
    n_points = len(cloud)
    anchor_bytes = len(anchor_octree.encode(cloud, res, (1, 1), 'gpu', ctx))
    result = dict(commit=a.commit or _commit(), device=torch.cuda.get_device_name(0), cloud_points=n_points, blocks=len(blocks),
                  chunk_blocks=min(a.blocks, len(blocks)), block_edge=dhw[0], reps=a.reps,
                  anchor_lossless_bits_per_input_point=8 * anchor_bytes / n_points, points=[])
    for lv in a.levels:
        with tempfile.TemporaryDirectory() as ck:
            np.savez(os.path.join(ck, 'model.npz'), **make_cell_codec_weights(lv))
            m = ModelConfigType['c3p'].build(batch_size=a.blocks, lossless=True)
            m.compress([1, 1] + list(dhw))
            m.restore(ck)
        mc = m._ctx(ctx)
        strings, thr, _, _, _ = m.encode_block_range(ctx, blocks, res, fixed_threshold=True)
        dec, _ = m.decompress_blocks(ctx, [(s, t[0]) for s, t in zip(strings, thr)], dhw)
        rows = lambda p: np.unique(np.asarray(p, np.float32).reshape(-1, 3), axis=0)
        assert all(np.array_equal(rows(d), rows(np.asarray(b)[:, :3])) for d, b in zip(dec, blocks)), 'the lossless decode is not the input'
        base = sum(len(v) for s in strings for v in s[:-1])
        occ = sum(len(s[-1]) for s in strings)
        container = 5 * len(blocks) + 2 * len(blocks)            # threshold byte + 2 length fields, + the third length field
        # the first chunk: m, L and the launch times
        chunk = blocks[:a.blocks]
        x = m._voxelize(mc, chunk, dhw)
        t = ops.codec_encode(mc, m._codec(mc), x.contiguous())
        x_hat, y_hat = t['x_hat'], t['y_hat']
        occ_strings = ops.occ_encode_batch(mc, x_hat, x)
        assert occ_strings == [s[-1] for s in strings[:len(chunk)]]
        xh = x_hat.cpu().numpy()
        xo = x.cpu().numpy()
        coded = []
        for b in range(len(chunk)):
            info = {}
            assert R.encode(xh[b].reshape(-1), xo[b].reshape(-1), info=info) == occ_strings[b]
            coded.append(info['m'])
        enc_ms = _median_ms(lambda: ops.occ_encode_launch(mc, x_hat, x), a.reps, a.warmup)
        dec_ms = _median_ms(lambda: ops.occ_decode_batch(mc, x_hat, occ_strings, check=False), a.reps, a.warmup)
        syn_ms = _median_ms(lambda: m.synthesis_transform.forward_ndhwc(mc, y_hat), a.reps, a.warmup)
        point = dict(level=lv, base_bytes=base, occ_bytes=occ, bits_per_input_point_strings=8 * (base + occ) / n_points,
                     bits_per_input_point_with_container=8 * (base + occ + container + 8 + len(binstr)) / n_points,
                     base_bits_per_input_point=8 * base / n_points, coded_symbols_per_block=coded,
                     coded_symbols_median=statistics.median(coded), voxels_per_block=int(np.prod(dhw)),
                     lanes=dict(sorted(collections.Counter(1 << s[0] for s in occ_strings if s).items())),
                     occ_encode_device_ms=enc_ms, occ_decode_device_ms=dec_ms, synthesis_device_ms=syn_ms)
        print(json.dumps(point), flush=True)
        result['points'].append(point)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
