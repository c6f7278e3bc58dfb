"""GPU: the device rANS coder (csrc/rans_coder.hip) against its host restatement (tests/_rans_ref.py), damaged strings, and the codec /
CLIs under entropy_coder='rans' against the range-coder runs on the same weights and blocks."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _rans_ref as R
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_syntax, ops
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
from pcc_geo_cnn_v2_amd.utils import pc_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = (1, 2, 4, 8, 16, 32, 64)


@pytest.fixture(scope='module')
def gauss(oracle):
    tab = oracle.scale_table()
    cdf, size, off = oracle.gaussian_tables(tab)
    return tab, (cdf, size, off), ops.HostCdfTable(cdf, size, off)


def gauss_stream(tab, n, seed, scales=(0.3, 1.0, 5.0)):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 64, n).astype(np.int32)
    return np.rint(rng.standard_normal(n) * tab[idx] * rng.choice(scales, n)).astype(np.int32), idx


def padded(ctx, arrs):
    n_max = max(max(a.size for a in arrs), 1)
    out = np.zeros((len(arrs), n_max), np.int32)
    for s, a in enumerate(arrs):
        out[s, :a.size] = a
    return torch.from_numpy(out).to(ctx.device)


def check_batch(ctx, ref_table, table, datas, idxs=None, index_mod=0, lanes=0):
    """device strings == reference strings, each side decodes the other's, and the device decodes to the symbols"""
    n_list = [d.size for d in datas]
    dev_idx = None if idxs is None else padded(ctx, idxs)
    strings = ops.rans_encode_batch(ctx, table, padded(ctx, datas), n_list, dev_idx, index_mod, lanes=lanes)
    ref = [R.encode(*ref_table, d, None if idxs is None else idxs[s], index_mod, lanes=lanes) for s, d in enumerate(datas)]
    for s, (a, b) in enumerate(zip(strings, ref)):
        assert a == b, f'stream {s} (n {n_list[s]}): device {len(a)} bytes, reference {len(b)} bytes'
    for s, d in enumerate(datas):                  # the reference decodes the device's strings
        assert np.array_equal(R.decode(*ref_table, strings[s], d.size, None if idxs is None else idxs[s], index_mod), d)
    out, _ = ops.rans_decode_batch(ctx, table, ref, n_list, dev_idx, index_mod)       # the device decodes the reference's strings
    out = out.cpu().numpy()
    for s, d in enumerate(datas):
        assert np.array_equal(out[s, :d.size], d), f'stream {s}'
    return strings


BATCHES = {'one_32768': [32768], 'three': [4096 + 17, 1, 0],
           'thirty_three': [0, 1, 63, 64, 65, 127] + [int(v) for v in np.random.default_rng(5).integers(2, 300, 27)]}


@pytest.mark.parametrize('name', list(BATCHES))
def test_device_strings_equal_the_reference_with_the_lane_rule(ctx, gauss, name):
    tab, ref_table, table = gauss
    pairs = [gauss_stream(tab, n, 100 + s) for s, n in enumerate(BATCHES[name])]
    datas, idxs = [p[0] for p in pairs], [p[1] for p in pairs]
    strings = check_batch(ctx, ref_table, table, datas, idxs)
    assert all((len(s) == 0) == (d.size == 0) for s, d in zip(strings, datas))
    # two encodes of the same input: identical bytes
    assert ops.rans_encode_batch(ctx, table, padded(ctx, datas), [d.size for d in datas], padded(ctx, idxs)) == strings
    if name == 'one_32768':
        assert strings[0][0] == 6                   # a long stream takes all 64 lanes


@pytest.mark.parametrize('lanes', LANES)
def test_every_forced_lane_count(ctx, gauss, lanes):
    tab, ref_table, table = gauss
    pairs = [gauss_stream(tab, n, 200 + n) for n in (0, 1, 63, 64, 65, 127, 1000)]
    strings = check_batch(ctx, ref_table, table, [p[0] for p in pairs], [p[1] for p in pairs], lanes=lanes)
    assert all(s[0] == lanes.bit_length() - 1 for s in strings if s)


def test_escapes_none_all_and_the_one_row_table(ctx, gauss):
    tab, ref_table, table = gauss
    quiet = [gauss_stream(tab, n, 300 + n, scales=(0.05,)) for n in (65, 700)]            # far inside every row: no escapes
    info = {}
    R.encode(*ref_table, quiet[1][0], quiet[1][1], info=info)
    assert info['n_escapes'] == 0
    check_batch(ctx, ref_table, table, [p[0] for p in quiet], [p[1] for p in quiet])
    one = (np.array([[0, 1 << 15, 1 << 16]], np.int32), np.array([3], np.int32), np.array([0], np.int32))
    one_t = ops.HostCdfTable(*one)
    rng = np.random.default_rng(3)
    all_esc = [rng.integers(1, 2 ** 31 - 1, n).astype(np.int32) * rng.choice([-1, 1], n).astype(np.int32) for n in (1, 64, 333)]
    mixed = [rng.integers(0, 2, n).astype(np.int32) for n in (127, 2500)]
    for lanes in (0, 8):
        s = check_batch(ctx, one, one_t, all_esc + mixed, None, 1, lanes=lanes)
        assert len(s[2]) >= 4 * 333


def test_per_channel_mode_with_eight_channels(ctx, oracle):
    from test_rans_cpu import channel_table
    ref_table = channel_table(oracle)
    table = ops.HostCdfTable(*ref_table)
    rng = np.random.default_rng(1)
    vox, Cn = 4 * 4 * 4, 8
    data = rng.integers(-14, 15, (3, vox, Cn)).astype(np.int32)
    check_batch(ctx, ref_table, table, [d.reshape(-1) for d in data], None, Cn)
    # channel-major streams straight from the (vox, C) tensors: symbol i at (i % vox) * C + i / vox, rows read at the same place
    x = torch.from_numpy(data).to(ctx.device)
    rows = torch.arange(Cn, dtype=torch.int32, device=ctx.device).repeat(vox)
    strings = ops.rans_encode_batch(ctx, table, x, None, rows, 0, channels=Cn)
    for s in range(3):
        assert strings[s] == R.encode(*ref_table, data[s].T.reshape(-1), np.repeat(np.arange(Cn), vox))
    out = torch.zeros_like(x)
    ops.rans_decode_batch(ctx, table, strings, [vox * Cn] * 3, rows, 0, channels=Cn, out=out)
    assert torch.equal(out, x)


def test_damaged_strings_are_refused_and_the_context_keeps_working(ctx, gauss):
    tab, ref_table, table = gauss
    data, idx = gauss_stream(tab, 3000, 9)
    (good,) = ops.rans_encode_batch(ctx, table, padded(ctx, [data]), None, padded(ctx, [idx]), lanes=8)
    assert good == R.encode(*ref_table, data, idx, lanes=8)
    dev_idx = padded(ctx, [idx])
    bad = {'cut by one byte': good[:-1], 'cut inside its states': good[:2 + 4 * 3 + 1], 'wrong lane byte': bytes([good[0] ^ 1]) + good[1:],
           'lane byte 7': bytes([7]) + good[1:], 'escape count too large': good[:1] + b'\xff\xff\xff\x7f' + good[2:],
           'a word changed': good[:60] + bytes([good[60] ^ 0x55]) + good[61:]}
    for what, s in bad.items():
        with pytest.raises(L.PccError, match=f'status {L.PCC_ERR_CORRUPT}'):
            ops.rans_decode_batch(ctx, table, [s], [data.size], dev_idx)
            pytest.fail(what)
        out, _ = ops.rans_decode_batch(ctx, table, [good], [data.size], dev_idx)
        assert np.array_equal(out.cpu().numpy()[0], data), what
    # the kernel's own test (no host check in front of it): the same strings straight into the ABI
    for what, s in bad.items():
        blob = torch.from_numpy(np.frombuffer(s + b'\0' * 8, np.uint8).copy()).to(ctx.device)
        off, ln = torch.zeros(1, dtype=torch.int64, device=ctx.device), torch.tensor([len(s)], dtype=torch.int32, device=ctx.device)
        n = torch.tensor([data.size], dtype=torch.int32, device=ctx.device)
        out, st = torch.zeros((1, data.size), dtype=torch.int32, device=ctx.device), torch.zeros(1, dtype=torch.int32, device=ctx.device)
        st_host = np.zeros(1, np.int32)
        rc = L.lib().pcc_rans_decode_batch(ctx.handle, C.byref(table.struct), 1, blob.data_ptr(), len(s), off.data_ptr(), ln.data_ptr(), dev_idx.data_ptr(),
                                           0, 0, 0, n.data_ptr(), data.size, out.data_ptr(), data.size, st.data_ptr(), st_host.ctypes.data,
                                           ctx.stream)
        assert rc == L.PCC_ERR_CORRUPT, what
    out, _ = ops.rans_decode_batch(ctx, table, [good], [data.size], dev_idx)
    assert np.array_equal(out.cpu().numpy()[0], data)


def test_a_table_the_format_cannot_code_is_refused(ctx):
    t = ops.HostCdfTable(np.array([[0, 1 << 16]], np.int32), [2], [0])                    # one bin of frequency 2^16
    with pytest.raises(AssertionError, match='frequencies'):
        ops.rans_encode_batch(ctx, t, torch.zeros((1, 4), dtype=torch.int32, device=ctx.device), None, None, 1)
    t12 = ops.HostCdfTable(np.array([[0, 1 << 11, 1 << 12]], np.int32), [3], [0], precision=12)
    with pytest.raises(AssertionError, match='16-bit'):
        ops.rans_encode_batch(ctx, t12, torch.zeros((1, 4), dtype=torch.int32, device=ctx.device), None, None, 1)


@pytest.mark.parametrize('layerwise', [False, True])
@pytest.mark.parametrize('cfg,res', [('c3p', 16), ('c1', 32)])
def test_codec_under_rans_decodes_what_the_range_model_decodes(ctx, monkeypatch, cfg, res, layerwise):
    from test_codec_gpu import make_blocks, scaled_weights
    if layerwise:
        monkeypatch.setenv('PCC_LAYERWISE', '1')
    B = 3
    models = {}
    for coder in ('range', 'rans'):
        m = ModelConfigType[cfg].build(batch_size=B, entropy_coder=coder)
        m.compress([1, 1, res, res, res])
        m.set_weights(scaled_weights(m, 2.2))
        models[coder] = m
    assert (models['rans']._codec(ctx) is None) == layerwise
    x = models['range']._voxelize(ctx, make_blocks(B, res, seed=2), (res,) * 3)
    thr = models['range']._thr_tensor(ctx, [128] * B)
    got = {}
    for coder, m in models.items():
        enc = m._encode_batch(ctx, x, debug=True, thr=thr)
        strings = enc['finish']()
        st = m._decode_phase_a(ctx, strings, (res,) * 3)
        dec = m._decode_phase_b(ctx, st, (res,) * 3, True, thr=thr)
        torch.cuda.synchronize()
        got[coder] = (enc, strings, dec)
    (e1, s1, d1), (e2, s2, d2) = got['range'], got['rans']
    assert s1 != s2 and all(len(a) == len(b) for a, b in zip(s1, s2))
    assert torch.equal(d1['x_hat'], d2['x_hat']) and torch.equal(e1['x_hat'], e2['x_hat'])
    assert torch.equal(d1['counts'], d2['counts'])
    for b in range(B):
        n = int(d1['counts'][b])
        assert n > 0 and np.array_equal(d1['xyz'][b, :n].cpu().numpy(), d2['xyz'][b, :n].cpu().numpy())
        for k in e1['debug'][b]:
            assert np.array_equal(e1['debug'][b][k], e2['debug'][b][k]), k
        for k in d1['debug'][b]:
            assert np.array_equal(d1['debug'][b][k], d2['debug'][b][k]), k
        assert np.array_equal(e2['debug'][b]['x_hat'], d2['debug'][b]['x_hat'])
    # every rans string is what the host restatement writes for the encoder's symbols
    m = models['rans']
    eb = m.entropy_bottleneck
    order = lambda a: np.moveaxis(a[0], -1, 0).reshape(-1)                 # (1,D,H,W,C) -> channel-major (channels_first streams)
    for b in range(B):
        dbg = e2['debug'][b]
        if cfg == 'c1':
            sym = order(dbg['symbols'])
            rows = np.repeat(np.arange(m.num_filters), sym.size // m.num_filters)
            assert s2[b][0] == R.encode(eb.table.cdf, eb.table.cdf_size, eb.table.offset, sym, rows)
        else:
            gc = m.conditional_bottleneck
            assert s2[b][0] == R.encode(gc.table.cdf, gc.table.cdf_size, gc.table.offset, order(dbg['symbols']), order(dbg['indexes']))
            z = order(dbg['z_symbols'])
            assert s2[b][1] == R.encode(eb.table.cdf, eb.table.cdf_size, eb.table.offset, z, np.repeat(np.arange(m.num_filters), z.size // m.num_filters))


def test_compress_blocks_and_roundtrip_stream_under_both_coders(ctx):
    from test_codec_gpu import make_blocks, scaled_weights
    res, B = 16, 2
    pts = {}
    for coder in ('range', 'rans'):
        m = ModelConfigType['c3p'].build(batch_size=B, entropy_coder=coder)
        m.compress([1, 1, res, res, res])
        m.set_weights(scaled_weights(m, 2.2))
        chunks = [m._voxelize(ctx, make_blocks(B, res, seed=s), (res,) * 3) for s in (2, 3)]
        out = list(m.roundtrip_stream(ctx, chunks))
        assert len(out) == 2
        pts[coder] = [p for _, _, plist in out for p in plist]
        strings = [s for ss, _, _ in out for s in ss]
        dec, _ = m.decompress_blocks(ctx, [(s, 128) for s in strings], [res] * 3)          # (3 chunks of 2, 2, 0 .. the pipelined decoder)
        for a, b in zip(dec, pts[coder]):
            assert np.array_equal(a, b)
    assert sum(len(p) for p in pts['range']) > 0
    for a, b in zip(pts['range'], pts['rans']):
        assert np.array_equal(a, b)


def test_cli_rans_stream_names_its_coder(tmp_path):
    """The CLIs' own entry points (compress_octree.compress / decompress_octree.decompress on parsed arguments), in this process."""
    from pcc_geo_cnn_v2_amd import compress_octree, decompress_octree, init_checkpoint
    from test_cli_gpu import _cloud
    res, level, cfg = 128, 2, 'c3p'
    src = str(tmp_path / 'in.ply')
    pc_io.write_df(src, pc_io.pa_to_df(_cloud(res, 0)))
    ck = str(tmp_path / 'ckpt')
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, '-m', 'pcc_geo_cnn_v2_amd.init_checkpoint', '--model_config', cfg, '--checkpoint_dir', ck], cwd=ROOT, env=env,
                   check=True, capture_output=True, text=True)

    def enc(out, *extra):
        compress_octree.compress(compress_octree.build_parser().parse_args(
            ['--input_files', src, '--output_files', out, '--checkpoint_dir', ck, '--model_config', cfg, '--resolution', str(res),
             '--octree_level', str(level), '--opt_metrics', 'd1_mse', '--fixed_threshold', '--batch_size', '5', *extra]))

    def dec(inp, out):
        decompress_octree.decompress(decompress_octree.build_parser().parse_args(
            ['--input_files', inp, '--output_files', out, '--checkpoint_dir', ck, '--model_config', cfg, '--batch_size', '7']))

    f_def, f_range, f_rans = (str(tmp_path / n) for n in ('default.bin', 'range.bin', 'rans.bin'))
    enc(f_def)
    enc(f_range, '--entropy_coder', 'range')
    enc(f_rans, '--entropy_coder', 'rans')
    assert open(f_def, 'rb').read() == open(f_range, 'rb').read()
    tag, tag_r = model_syntax.read_gzip_tag(f_def), model_syntax.read_gzip_tag(f_rans)
    assert tag_r == tag + '/rans1' and not tag.endswith('/rans1')
    assert json.load(open(f_rans + '.enc.metric.json'))['codec_numerics'] == tag_r
    assert json.load(open(f_def + '.enc.metric.json'))['codec_numerics'] == tag
    d_def, d_rans = str(tmp_path / 'd_def.ply'), str(tmp_path / 'd_rans.ply')
    dec(f_def, d_def)
    dec(f_rans, d_rans)                             # no flag: the stream names its coder
    a, b = pc_io.load_pc(d_def), pc_io.load_pc(d_rans)
    assert len(a) > 0 and np.array_equal(a, b)
    # the same payload under an unknown coder suffix is refused
    with gzip.open(f_rans, 'rb') as fh:
        payload = fh.read()
    f_bad = str(tmp_path / 'bad.bin')
    model_syntax.write_tagged_gzip(f_bad, payload, tag + '/rans9')
    with pytest.raises(RuntimeError, match='rans9'):
        dec(f_bad, str(tmp_path / 'd_bad.ply'))
    assert not os.path.exists(str(tmp_path / 'd_bad.ply'))
