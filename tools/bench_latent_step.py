"""Latent step on one chunk of 32 blocks of 64^3: what the rate ladder costs beside the analysis + hyper pass it rides
on, what the stepped element-wise kernels cost beside their twins, and what a few steps of the ladder do to the strings.

The setting is tools/bench_count_search.py's: the first 32 occupied 64^3 blocks of tools/rd_sweep.py's synthetic 512^3 shell, c3p under
init_checkpoint.make_synthetic_weights.  The script records
  * HIP-event medians: the analysis + hyper pass (analysis, hyper-analysis, z quantiser, hyper-synthesis: the first pass of a rate target
    without the ladder), ops.rate_ladder at J = 64 and J = 1 on its y and sigma-hat, and each stepped kernel (q = 24 in every block)
    beside its un-stepped twin on the same tensors;
  * the y/z string bytes, the container bytes and the whole-cloud D1 PSNR of compress_blocks at q = 8, 16, 24, 32, 40 (fixed threshold).
No time is a pass/fail condition.  Synthetic weights are not trained weights: no RD claim is made.

    python tools/bench_latent_step.py --out profiles/latent_step_bench.json [--commit <id>]
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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--commit', default=None, help='what to record as the measured commit (default: git describe)')
    a = ap.parse_args(argv)
    import torch
    from pcc_geo_cnn_v2_amd import _lib as L
    from pcc_geo_cnn_v2_amd import model_syntax as MS
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

    m = ModelConfigType['c3p'].build(batch_size=a.blocks)
    m.compress([1, 1] + list(dhw))
    m.set_weights(make_synthetic_weights('c3p'))
    mc = m._ctx(ctx)
    x = m._voxelize(mc, blocks, dhw)
    t = m._analysis_hyper(mc, x)
    y, sigma = t['y'], t['sigma_hat']
    tab, gc = m._scale_table_dev(mc), m.conditional_bottleneck.table
    B = len(blocks)
    q = torch.full((B,), 24, dtype=torch.uint8, device=ctx.device)
    cf = m.data_format == 'channels_first'
    dst16 = torch.empty(y.shape, dtype=torch.int16, device=ctx.device)
    dst8 = torch.empty(y.shape, dtype=torch.uint8, device=ctx.device)
    tmax = torch.empty((L.lib().pcc_symbols_tiles(B, y[0].numel() // y.shape[-1], y.shape[-1]),), dtype=torch.int32, device=ctx.device)
    sym, deq, idx = torch.empty(y.shape, dtype=torch.int32, device=ctx.device), torch.empty_like(y), torch.empty(y.shape, dtype=torch.int32, device=ctx.device)
    med = lambda fn: _median_ms(fn, a.reps, a.warmup)
    kernels = dict(
        analysis_hyper_pass_device_ms=med(lambda: m._analysis_hyper(mc, x)),
        rate_ladder_j64_device_ms=med(lambda: ops.rate_ladder(mc, y, sigma, np.arange(64), tab, gc, m.round_mode)),
        rate_ladder_j1_device_ms=med(lambda: ops.rate_ladder(mc, y, sigma, [16], tab, gc, m.round_mode)),
        quantize_pack_device_ms=med(lambda: ops.quantize_pack(mc, y, None, m.round_mode, cf, dst16.data_ptr(), 2, tmax.data_ptr(), sym=sym, deq=deq)),
        quantize_step_pack_device_ms=med(lambda: ops.quantize_step_pack(mc, y, None, m.round_mode, cf, dst16.data_ptr(), 2, q, tmax.data_ptr(), sym=sym, deq=deq)),
        index_pack_device_ms=med(lambda: ops.index_pack(mc, sigma, tab, cf, dst8.data_ptr(), 1, idx=idx)),
        index_pack_step_device_ms=med(lambda: ops.index_pack_step(mc, sigma, tab, cf, dst8.data_ptr(), 1, q, idx=idx)),
        unpack_dequantize_device_ms=med(lambda: ops.unpack_dequantize(mc, dst16, y.shape, cf, None, sym=sym, deq=deq)),
        unpack_dequantize_step_device_ms=med(lambda: ops.unpack_dequantize_step(mc, dst16, y.shape, cf, q, None, sym=sym, deq=deq)))
    kernels['rate_ladder_j64_over_analysis_hyper_pass'] = kernels['rate_ladder_j64_device_ms'] / kernels['analysis_hyper_pass_device_ms']
    kernels['cost_table_kbytes'] = int(np.prod(ops.device_cost_table(mc, gc)[0].shape)) * 4 / 1024
    kernels['latent_elements'] = int(y.numel())
    print(json.dumps(kernels), flush=True)

    steps = []
    for qq in (8, 16, 24, 32, 40):
        data, meta, _ = m.compress_blocks(ctx, blocks, binstr, cloud, res, level, fixed_threshold=True, metrics_device='gpu', latent_step=qq)
        psnr = float(meta[0]['metrics']['d1_psnr'])
        try:
            container = len(MS.save_compressed_file(binstr, data[0], res, level, strict=True))
        except AssertionError:              # a y string beyond the container's 65535 bytes per string
            container = None
        row = dict(latent_step=qq, latent_step_size=MS.latent_step(qq), y_bytes=sum(len(s[0]) for s, _ in data[0]), z_bytes=sum(len(s[1]) for s, _ in data[0]),
                   container_bytes=container, d1_psnr=psnr if np.isfinite(psnr) else None)      # (null: nothing was decoded)
        print(json.dumps(row), flush=True)
        steps.append(row)
    _, target = m.choose_latent_step(ctx, blocks, binstr, len(cloud), 1e9)
    for row in steps:           # (the prediction carries the measured margin of model_types.rate_margin_bits16)
        row['predicted_container_bytes'] = target['predictions'][row['latent_step']]

    result = dict(commit=a.commit or _commit(), device=torch.cuda.get_device_name(0), blocks=B, block_edge=edge, input_points=int(len(cloud)),
                  reps=a.reps, kernels=kernels, steps=steps,
                  note='synthetic weights: times and sizes describe these latents, no RD claim is made')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1, allow_nan=False)
        fh.write('\n')


if __name__ == '__main__':
    main()
