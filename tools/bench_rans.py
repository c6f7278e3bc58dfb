"""Device rANS coder against the host range coder on the symbols of one codec chunk.

For a 32-block c3p chunk of 64^3 blocks at each of the six designed rate points of tools/rd_sweep.py (init_checkpoint.make_cell_codec_weights,
levels 1..6) the script takes the y / z symbols and CDF rows the compress graph produces and measures
  * device time of the rANS encode launches (y and z) and of the decode launches (upload of the strings included), HIP events, median;
  * wall time and process CPU seconds of the host range coder on the same symbols (the narrow stream-order arrays the codec ships) at
    coder_threads 1, 4 and 16, encode and decode;
  * process CPU seconds per chunk of the rANS path (launch, fetch of the strings, upload, decode, flags);
  * total string bytes under both coders and their ratio, and the distribution of the lane count L the rule chose.

    python tools/bench_rans.py --out profiles/rans_bench.json [--commit <id>]
"""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _commit():
    try:
        out = subprocess.run(['git', 'describe', '--always', '--dirty'], cwd=ROOT, capture_output=True, text=True, check=True)
        return out.stdout.strip()
    except Exception:
        return 'unknown'


def _median_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def _host(fn, reps, warmup):
    """(median wall ms, median process CPU seconds) of fn()"""
    for _ in range(warmup):
        fn()
    wall, cpu = [], []
    for _ in range(reps):
        c0, t0 = time.process_time(), time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t0))
        cpu.append(time.process_time() - c0)
    return statistics.median(wall), statistics.median(cpu)


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
    from pcc_geo_cnn_v2_amd import ops
    from pcc_geo_cnn_v2_amd.init_checkpoint import make_cell_codec_weights
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree
    from tools.rd_sweep import synthetic_cloud

    ctx = ops.get_context(torch.device('cuda', 0))
    res, level = 512, 3
    blocks, _ = partition_octree(synthetic_cloud(res), [0, 0, 0], [res] * 3, level)
    blocks = sorted(blocks, key=len, reverse=True)[:a.blocks]
    B, dhw = len(blocks), (res >> level,) * 3
    result = dict(commit=a.commit or _commit(), device=torch.cuda.get_device_name(0), blocks=B, block_edge=dhw[0], reps=a.reps, points=[])
    for lv in a.levels:
        with tempfile.TemporaryDirectory() as ck:
            np.savez(os.path.join(ck, 'model.npz'), **make_cell_codec_weights(lv))
            m = ModelConfigType['c3p'].build(batch_size=B, entropy_coder='rans')
            m.compress([1, 1] + list(dhw))
            m.restore(ck)
        mc = m._ctx(ctx)
        x = m._voxelize(mc, blocks, dhw)
        t = ops.codec_encode(mc, m._codec(mc), x.contiguous())
        ysym, zsym, idx = t['symbols'], t['z_symbols'], t['indexes']
        eb, gc = m.entropy_bottleneck, m.conditional_bottleneck
        ny, nz = ysym[0].numel(), zsym[0].numel()
        zrows, zmod, ch = m._rans_layout(mc, nz, True)

        def rans_encode():
            return [ops.rans_encode_launch(mc, gc.table, ysym, None, idx, 0, ch), ops.rans_encode_launch(mc, eb.table, zsym, None, zrows, zmod, ch)]
        ys, zs = (ops.rans_encode_fetch(*l) for l in rans_encode())

        def rans_decode():
            zo, zst = ops.rans_decode_batch(mc, eb.table, zs, [nz] * B, zrows, zmod, ch, out=torch.empty_like(zsym), check=False)
            yo, yst = ops.rans_decode_batch(mc, gc.table, ys, [ny] * B, idx, 0, ch, out=torch.empty_like(ysym), check=False)
            return zo, zst, yo, yst
        zo, zst, yo, yst = rans_decode()
        ops.rans_check_status(zst)
        ops.rans_check_status(yst)
        assert torch.equal(zo, zsym) and torch.equal(yo, ysym)
        enc_ms = _median_ms(rans_encode, a.reps, a.warmup)
        dec_ms = _median_ms(rans_decode, a.reps, a.warmup)

        def rans_chunk():               # what a chunk costs the host under rans: launches, string fetch, upload, decode, flags
            s = [ops.rans_encode_fetch(*l) for l in rans_encode()]
            out = rans_decode()
            ops.rans_check_status(out[1])
            ops.rans_check_status(out[3])
            return s
        rans_wall, rans_cpu = _host(rans_chunk, a.reps, a.warmup)

        # the host range coder on the same symbols, in the narrow stream-order arrays the codec ships
        ys_h = m._to_stream_order(ysym).cpu().numpy().astype(np.int16).reshape(B, -1)
        zs_h = m._to_stream_order(zsym).cpu().numpy().astype(np.int16).reshape(B, -1)
        idx_h = m._to_stream_order(idx).cpu().numpy().astype(np.uint8).reshape(B, -1)
        rows, mod = m._eb_rows(nz, m.num_filters)
        host = {}
        for threads in (1, 4, 16):
            enc = lambda: (ops.range_encode_batch(gc.table, ys_h, idx_h, 0, threads), ops.range_encode_batch(eb.table, zs_h, rows, mod, threads))
            ry, rz = enc()
            oy, oz = np.empty_like(ys_h), np.empty_like(zs_h)
            dec = lambda: (ops.range_decode_batch(eb.table, rz, [nz] * B, rows, mod, threads, out=oz),
                           ops.range_decode_batch(gc.table, ry, [ny] * B, idx_h, 0, threads, out=oy))
            dec()
            assert np.array_equal(oy, ys_h) and np.array_equal(oz, zs_h)
            ew, ec = _host(enc, a.reps, a.warmup)
            dw, dc = _host(dec, a.reps, a.warmup)
            host[str(threads)] = dict(encode_wall_ms=ew, decode_wall_ms=dw, encode_cpu_s=ec, decode_cpu_s=dc, chunk_cpu_s=ec + dc)
        rans_bytes = sum(map(len, ys)) + sum(map(len, zs))
        range_bytes = sum(map(len, ry)) + sum(map(len, rz))
        lanes = lambda ss: dict(sorted(collections.Counter(1 << s[0] for s in ss if s).items()))
        point = dict(level=lv, y_symbols_per_block=ny, z_symbols_per_block=nz, rans_encode_device_ms=enc_ms, rans_decode_device_ms=dec_ms,
                     rans_chunk_wall_ms=rans_wall, rans_chunk_cpu_s=rans_cpu, range_host=host, rans_bytes=rans_bytes, range_bytes=range_bytes,
                     bytes_ratio=rans_bytes / range_bytes, y_bytes=dict(rans=sum(map(len, ys)), range=sum(map(len, ry))),
                     z_bytes=dict(rans=sum(map(len, zs)), range=sum(map(len, rz))), lanes_y=lanes(ys), lanes_z=lanes(zs))
        print(json.dumps(point), flush=True)
        result['points'].append(point)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
