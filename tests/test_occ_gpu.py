"""GPU: the device occupancy coder (csrc/occ_coder.hip) against its host restatement (tests/_occ_ref.py), damaged strings, and the
lossless layer through the model classes and the CLIs."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest
import torch

import _occ_ref as O
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_syntax, ops
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
from pcc_geo_cnn_v2_amd.utils import pc_io

pytestmark = pytest.mark.gpu
LANES = (0, 1, 2, 64)
GROUPS = {}                                        # voxels per block -> [(name, x_hat, occ)]: one launch per group
for _name, _x, _o in O.cases():
    GROUPS.setdefault(_x.size, []).append((_name, _x, _o))
_REF = {}


def ref_strings(n, lanes):
    """the restatement's strings of a group, computed once and shared"""
    if (n, lanes) not in _REF:
        _REF[n, lanes] = [O.encode(x, o, lanes=lanes) for _, x, o in GROUPS[n]]
    return _REF[n, lanes]


def on_device(ctx, arrs, pad=0):
    """rows of a (S, n + pad) tensor: streams whose stride is larger than their length when pad > 0"""
    n = arrs[0].size
    host = np.full((len(arrs), n + pad), 7.0, np.float32)
    for s, a in enumerate(arrs):
        host[s, :n] = a
    return torch.from_numpy(host).to(ctx.device)[:, :n]


@pytest.mark.parametrize('lanes', LANES)
@pytest.mark.parametrize('n', list(GROUPS))
def test_device_strings_equal_the_reference_and_each_side_decodes_the_other(ctx, n, lanes):
    group = GROUPS[n]
    x = on_device(ctx, [g[1] for g in group])
    occ = on_device(ctx, [g[2].astype(np.float32) for g in group])
    want = ref_strings(n, lanes)
    got = ops.occ_encode_batch(ctx, x, occ, lanes=lanes)
    for (name, _, _), a, b in zip(group, got, want):
        assert a == b, f'{name}: device {len(a)} bytes, reference {len(b)} bytes'
        assert lanes == 0 or a[0] == lanes.bit_length() - 1
    dec, _ = ops.occ_decode_batch(ctx, x, want)                        # the device decodes the reference's strings
    assert torch.equal(dec, (occ != 0).float())
    if lanes == 0:
        for (name, xh, o), s in zip(group, got):                       # the reference decodes the device's strings
            assert np.array_equal(O.decode(xh, s), o), name
        assert ops.occ_encode_batch(ctx, x, occ) == got                # two encodes: the same bytes


def test_a_batch_of_three_streams_with_strides_larger_than_n(ctx):
    group = [g for g in GROUPS[4097] if g[0] in ('n4097-half-uniform', 'n4097-single-falloff', 'n4097-full-equal')]
    assert len(group) == 3
    x = on_device(ctx, [g[1] for g in group], pad=5)
    occ = on_device(ctx, [g[2].astype(np.float32) for g in group], pad=11)
    assert x.stride(0) == 4102 and occ.stride(0) == 4108
    got = ops.occ_encode_batch(ctx, x, occ)
    assert got == [O.encode(g[1], g[2]) for g in group] and len(set(got)) == 3
    dec, _ = ops.occ_decode_batch(ctx, x, got)
    assert torch.equal(dec, (occ != 0).float())
    # a (B, D, H, W) pair as the model passes it
    x4, o4 = x[:, :4096].reshape(3, 16, 16, 16), occ[:, :4096].reshape(3, 16, 16, 16).contiguous()
    s4 = ops.occ_encode_batch(ctx, x4.contiguous(), o4)
    assert s4 == [O.encode(g[1][:4096], g[2][:4096]) for g in group]


@pytest.mark.parametrize('name', ['n4097-half-uniform', 'n65-half-falloff', 'n4097-empty-zero', 'shell64-falloff'])
def test_damaged_strings_set_the_corrupt_flag_and_write_nothing_outside_the_grid(ctx, name):
    _, xh, o = next(g for grp in GROUPS.values() for g in grp if g[0] == name)
    n = xh.size
    x = on_device(ctx, [xh])
    good = ref_strings(n, 0)[[g[0] for g in GROUPS[n]].index(name)]
    bad = {'cut by one byte': good[:-1], 'cut by two bytes': good[:-2], 'two bytes appended': good + b'\0\0',
           'lane byte 7': bytes([7]) + good[1:], 'the empty string': b''}
    guard = 64
    ws = torch.empty((int(L.lib().pcc_occ_workspace_bytes(1, n)) + 16,), dtype=torch.uint8, device=ctx.device)
    for what, s in bad.items():
        # through the wrapper: the host check or the device flag, the same error either way
        with pytest.raises(L.PccError, match=f'status {L.PCC_ERR_CORRUPT}'):
            ops.occ_decode_batch(ctx, x, [s])
            pytest.fail(what)
        # the kernel's own test (no host check in front of it): the string straight into the ABI, sentinels around the output grid
        blob = torch.from_numpy(np.frombuffer(s + b'\0' * 8, np.uint8).copy()).to(ctx.device)
        off, ln = torch.zeros(1, dtype=torch.int64, device=ctx.device), torch.tensor([len(s)], dtype=torch.int32, device=ctx.device)
        buf = torch.full((n + 2 * guard,), -3.0, dtype=torch.float32, device=ctx.device)
        st, st_host = torch.zeros(1, dtype=torch.int32, device=ctx.device), np.zeros(1, np.int32)
        rc = L.lib().pcc_occ_decode_batch(ctx.handle, x.data_ptr(), n, 1, n, blob.data_ptr(), len(s), off.data_ptr(), ln.data_ptr(),
                                          buf.data_ptr() + 4 * guard, n, st.data_ptr(), st_host.ctypes.data, ws.data_ptr(), ws.numel(), ctx.stream)
        assert rc == L.PCC_ERR_CORRUPT and st_host[0] != 0, what
        b = buf.cpu().numpy()
        assert (b[:guard] == -3.0).all() and (b[-guard:] == -3.0).all(), what
        assert np.isin(b[guard:-guard], (0.0, 1.0)).all(), what
    dec, _ = ops.occ_decode_batch(ctx, x, [good])                       # the context keeps working
    assert np.array_equal(dec.cpu().numpy()[0] != 0, o)


def test_wrapper_and_abi_refuse_what_the_contract_excludes(ctx):
    x = torch.zeros((2, 64), dtype=torch.float32, device=ctx.device)
    with pytest.raises(AssertionError):
        ops.occ_encode_launch(ctx, x, x[:1])
    out = torch.zeros((2, 8), dtype=torch.uint8, device=ctx.device)
    meta = torch.zeros((2, 2), dtype=torch.int32, device=ctx.device)
    ws = torch.zeros((4096,), dtype=torch.uint8, device=ctx.device)
    call = lambda lanes, cap: L.lib().pcc_occ_encode_batch(ctx.handle, x.data_ptr(), 64, x.data_ptr(), 64, 2, 64, lanes, out.data_ptr(), cap,
                                                           meta[0].data_ptr(), meta[1].data_ptr(), ws.data_ptr(), ws.numel(), ctx.stream)
    assert call(3, 8) == L.PCC_ERR_ARG and call(128, 8) == L.PCC_ERR_ARG and call(0, 8) == L.PCC_ERR_SPACE
    assert ops.occ_encode_batch(ctx, x[:0], x[:0]) == []
    assert ops.occ_encode_batch(ctx, x[:, :0], x[:, :0]) == [b'', b'']
    assert ops.occ_decode_batch(ctx, x[:, :0], [b'', b''])[0].shape == (2, 0)
    with pytest.raises(L.PccError, match=f'status {L.PCC_ERR_CORRUPT}'):
        ops.occ_decode_batch(ctx, x[:, :0], [b'', b'\0'])


# ---- model level: init_checkpoint weights, the 128^3 shell of tests/test_cli_gpu.py at octree level 1 (eight 64^3 blocks) ----------
RES, LEVEL = 128, 1


@pytest.fixture(scope='module')
def shell():
    from test_cli_gpu import _cloud
    from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree
    pts = _cloud(RES, 0)
    blocks, binstr = partition_octree(pts, [0, 0, 0], [RES] * 3, LEVEL)
    assert len(blocks) == 8
    return pts, blocks, binstr


def build(cfg, lossless, **kw):
    from pcc_geo_cnn_v2_amd.init_checkpoint import make_synthetic_weights
    m = ModelConfigType[cfg].build(batch_size=3, lossless=lossless, **kw)
    m.compress([1, 1] + [RES >> LEVEL] * 3)
    m.set_weights(make_synthetic_weights(cfg))
    return m


def rows(a):
    a = np.asarray(a, np.float32).reshape(-1, 3)
    return a[np.lexsort(a.T[::-1])]


@pytest.mark.parametrize('cfg,fixed,kw', [('c3p', False, {}), ('c1', True, {}), ('c3p', True, dict(entropy_coder='rans')),
                                          ('c3p', True, dict(precision='fp16'))])
def test_model_roundtrip_is_exact_and_the_base_layer_is_the_stream_without_the_flag(ctx, shell, cfg, fixed, kw):
    pts, blocks, binstr = shell
    n_base = 1 if cfg == 'c1' else 2
    coded = {}
    for lossless in (True, False):
        m = build(cfg, lossless, **kw)
        data, meta, _ = m.compress_blocks(ctx, blocks, binstr, pts, RES, LEVEL, opt_metrics=('d1_mse',), fixed_threshold=fixed, need_points=False)
        coded[lossless] = (m, data[0])
    (m, full), (m0, base) = coded[True], coded[False]
    assert all(len(s) == n_base + 1 for s, _ in full) and all(len(s) == n_base for s, _ in base)
    assert [(tuple(s[:n_base]), t) for s, t in full] == [(tuple(s), t) for s, t in base]          # the y/z strings and thresholds are untouched
    print(cfg, kw, 'occ bytes per block', [len(s[-1]) for s, _ in full], 'base', [sum(len(v) for v in s[:-1]) for s, _ in full])
    shape = [RES >> LEVEL] * 3
    dec, _ = m.decompress_blocks(ctx, full, shape)
    for b, (got, want) in enumerate(zip(dec, blocks)):
        assert np.array_equal(rows(got), rows(np.asarray(want)[:, :3])), f'block {b}'
    lossy, _ = m0.decompress_blocks(ctx, base, shape)
    for layers_of, stream in ((m, full), (m0, full)):
        again, _ = layers_of.decompress_blocks(ctx, stream, shape, layers='base')
        assert all(np.array_equal(a, b) for a, b in zip(again, lossy))
    same, _ = m0.decompress_blocks(ctx, base, shape, layers='all')      # no layer in the stream: 'all' is today's decode
    assert all(np.array_equal(a, b) for a, b in zip(same, lossy))
    # a damaged occupancy string is refused after the chunk's launches
    s, t = full[4]
    broken = full[:4] + [(tuple(s[:-1]) + (s[-1][:-2],), t)] + full[5:]
    with pytest.raises(L.PccError, match=f'status {L.PCC_ERR_CORRUPT}'):
        m.decompress_blocks(ctx, broken, shape)


# ---- CLI -----------------------------------------------------------------------------------------------------------------------
def test_cli_lossless_roundtrip_base_only_and_the_files_without_the_flag(tmp_path, monkeypatch):
    """The CLIs' own entry points (compress_octree.compress / decompress_octree.decompress on parsed arguments), in this process."""
    from pcc_geo_cnn_v2_amd import compress_octree, decompress_octree
    from pcc_geo_cnn_v2_amd.init_checkpoint import make_synthetic_weights
    from test_cli_gpu import _cloud
    cfg = 'c3p'
    pts = _cloud(RES, 0)
    src = str(tmp_path / 'in.ply')
    pc_io.write_df(src, pc_io.pa_to_df(pts))
    ck = str(tmp_path / 'ckpt')
    os.makedirs(ck)
    np.savez(os.path.join(ck, 'model.npz'), **make_synthetic_weights(cfg))

    def enc(out, *extra):
        compress_octree.compress(compress_octree.build_parser().parse_args(
            ['--input_files', src, '--output_files', out, '--checkpoint_dir', ck, '--model_config', cfg, '--resolution', str(RES),
             '--octree_level', str(LEVEL), '--opt_metrics', 'd1_mse', '--fixed_threshold', '--batch_size', '5', *extra]))

    def dec(inp, out, *extra):
        decompress_octree.decompress(decompress_octree.build_parser().parse_args(
            ['--input_files', inp, '--output_files', out, '--checkpoint_dir', ck, '--model_config', cfg, '--batch_size', '3', *extra]))

    f_ll, f_base, d_enc = str(tmp_path / 'll.bin'), str(tmp_path / 'base.bin'), str(tmp_path / 'enc.ply')
    enc(f_ll, '--lossless', '--dec_files', d_enc)
    enc(f_base)
    tag, tag_ll = model_syntax.read_gzip_tag(f_base), model_syntax.read_gzip_tag(f_ll)
    assert tag_ll == tag + '/occ1' and 'occ1' not in tag
    per_block = {}
    for f in (f_ll, f_base):
        with gzip.open(f, 'rb') as fh:
            per_block[f] = {len(s) for s, _ in model_syntax.load_compressed_file(fh)[3]}
    assert per_block[f_ll] == {3} and per_block[f_base] == {2}
    j_ll, j_base = json.load(open(f_ll + '.enc.metric.json')), json.load(open(f_base + '.enc.metric.json'))
    new = {'lossless', 'base_bytes', 'occ_bytes', 'bits_per_input_point_lossless'}
    assert set(j_ll) - set(j_base) == new and not new & set(j_base)
    assert j_ll['lossless'] is True and j_ll['occ_bytes'] > 0 and j_ll['base_bytes'] > 0 and j_ll['codec_numerics'] == tag_ll
    assert j_ll['bits_per_input_point_lossless'] == 8.0 * os.path.getsize(f_ll) / len(pts)
    d_ll, d_bo, d_base, d_noop = (str(tmp_path / n) for n in ('ll.ply', 'bo.ply', 'base.ply', 'noop.ply'))
    dec(f_ll, d_ll)                                 # no flag: the stream names its layer
    assert np.array_equal(rows(pc_io.load_pc(d_ll)), rows(pts))
    dec(f_ll, d_bo, '--base_only')
    dec(f_base, d_base)
    dec(f_base, d_noop, '--base_only')              # a no-op with a warning
    assert open(d_bo, 'rb').read() == open(d_base, 'rb').read() == open(d_noop, 'rb').read()
    assert np.array_equal(pc_io.load_pc(d_enc), pc_io.load_pc(d_base))  # --dec_files: still the base candidate
    # sharded lossless coding is refused before the process group or the GPU is touched
    monkeypatch.setenv('WORLD_SIZE', '2')
    f_no = str(tmp_path / 'no.bin')
    with pytest.raises(AssertionError, match='single-process'):
        enc(f_no, '--lossless')
    assert not os.path.exists(f_no)
