"""GPU: the top-k selection kernels (csrc/topk_select.hip) against the host restatement (tests/_topk_ref.py), and count-matched thresholding
("cnt1") through the model classes and the CLIs."""
import ctypes as C
import gzip
import json
import os
import struct

import numpy as np
import pytest
import torch

import _topk_ref as T
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_syntax, ops
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
from pcc_geo_cnn_v2_amd.utils import pc_io

pytestmark = pytest.mark.gpu
_WANT = {}


def want(dhw):
    """the restatement's (rows, k_eff) of every case of a shape, computed once and shared"""
    if dhw not in _WANT:
        _WANT[dhw] = [T.select(x, k, dhw) for _, x, k in T.cases(dhw)]
    return _WANT[dhw]


def on_device(ctx, arrs, dhw, pad):
    """(B, D, H, W) view of a (B, n + pad) buffer: blocks further apart than their voxels, a sentinel behind each"""
    n = arrs[0].size
    buf = torch.from_numpy(T.strided(arrs, pad)).to(ctx.device)
    return buf, buf[:, :n].view(len(arrs), *dhw)


def k_tensor(ctx, ks):
    return torch.tensor(list(ks), dtype=torch.int32, device=ctx.device)


@pytest.mark.parametrize('dhw', T.SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_kernel_equals_the_restatement_on_every_case_in_one_launch(ctx, dhw):
    group = T.cases(dhw)
    n = int(np.prod(dhw))
    buf, x = on_device(ctx, [g[1] for g in group], dhw, pad=13)
    assert x.stride(0) == n + 13 and not x.is_contiguous()
    xyz, counts = ops.topk_compact(ctx, x, k_tensor(ctx, [g[2] for g in group]))
    assert xyz.shape == (len(group), n, 3) and xyz.dtype == torch.float32 and counts.dtype == torch.int32
    got_n = counts.cpu().numpy()
    for b, ((name, _, _), (rows, ke)) in enumerate(zip(group, want(dhw))):
        assert got_n[b] == ke, f'{name}: {got_n[b]} points, the rule gives {ke}'
        assert np.array_equal(xyz[b, :ke].cpu().numpy(), rows), name
    # the input and its sentinels are untouched (bit patterns: a row holds a NaN)
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), T.strided([g[1] for g in group], 13).view(np.uint32))


def abi(ctx, x, stride, B, dhw, k, xyz, counts, cap, ws, ws_bytes=None):
    return L.lib().pcc_topk_compact(ctx.handle, C.c_void_p(x), stride, B, *dhw, C.c_void_p(k), C.c_void_p(xyz), C.c_void_p(counts), cap,
                                    C.c_void_p(ws.data_ptr()), ws.numel() if ws_bytes is None else ws_bytes, ctx.stream)


def workspace(ctx, B, n):
    return torch.empty((int(L.lib().pcc_topk_workspace_bytes(B, n)),), dtype=torch.uint8, device=ctx.device)


@pytest.mark.parametrize('dhw,cap', [((8, 8, 8), 5), ((16, 8, 24), 100), ((64, 64, 64), 4097)])
def test_a_cap_below_k_eff_reports_k_eff_and_writes_exactly_cap_rows(ctx, dhw, cap):
    group = [g for g in T.cases(dhw) if g[0].split('-')[1] in ('uniform', 'constant', 'relu97', 'last') and g[2] >= 0][:24]
    refs = [w for g, w in zip(T.cases(dhw), want(dhw)) if g[0].split('-')[1] in ('uniform', 'constant', 'relu97', 'last') and g[2] >= 0][:24]
    B, n, guard = len(group), int(np.prod(dhw)), 96
    assert any(ke > cap for _, ke in refs) and any(0 < ke < cap for _, ke in refs)
    _, x = on_device(ctx, [g[1] for g in group], dhw, pad=3)
    k = k_tensor(ctx, [g[2] for g in group])
    out = torch.full((guard + B * cap * 3 + guard,), -7.0, dtype=torch.float32, device=ctx.device)
    counts = torch.full((B,), -1, dtype=torch.int32, device=ctx.device)
    ws = workspace(ctx, B, n)
    assert abi(ctx, x.data_ptr(), x.stride(0), B, dhw, k.data_ptr(), out.data_ptr() + 4 * guard, counts.data_ptr(), cap, ws) == 0
    o = out.cpu().numpy()
    assert (o[:guard] == -7.0).all() and (o[-guard:] == -7.0).all()
    slots = o[guard:-guard].reshape(B, cap, 3)
    for b, ((name, _, _), (rows, ke)) in enumerate(zip(group, refs)):
        assert counts[b].item() == ke, name
        m = min(ke, cap)
        assert np.array_equal(slots[b, :m], rows[:m]), name
        assert (slots[b, m:] == -7.0).all(), name                       # nothing behind the rows that exist
    # the wrapper's cap
    xyz, cnt = ops.topk_compact(ctx, x, k, cap=cap)
    assert xyz.shape == (B, cap, 3) and cnt.cpu().tolist() == [ke for _, ke in refs]


def test_rows_do_not_depend_on_the_batch_or_the_position_in_it(ctx):
    dhw = (64, 64, 64)
    n = 64 ** 3
    picked = {}
    for name, x, k in T.cases(dhw):
        kind = name.split('-')[1]
        if kind in ('uniform', 'levels8', 'relu97') and kind not in picked and 2 < k < n:
            picked[kind] = (x, k)
    assert len(picked) == 3
    xs, ks = [v[0] for v in picked.values()], [v[1] for v in picked.values()]
    single = []
    for x, k in zip(xs, ks):
        xyz, cnt = ops.topk_compact(ctx, torch.from_numpy(x).to(ctx.device).view(1, *dhw), k_tensor(ctx, [k]))
        single.append(xyz[0, :cnt.item()].clone())
    for order in ((0, 1, 2), (2, 0, 1)):
        _, x3 = on_device(ctx, [xs[i] for i in order], dhw, pad=1 + order[0])
        xyz, cnt = ops.topk_compact(ctx, x3, k_tensor(ctx, [ks[i] for i in order]))
        for slot, i in enumerate(order):
            assert cnt[slot].item() == single[i].shape[0] > 0
            assert torch.equal(xyz[slot, :cnt[slot].item()], single[i])


def test_wrapper_and_abi_refuse_what_the_contract_excludes(ctx):
    dhw = (8, 8, 8)
    n, B = 512, 2
    x = torch.rand((B,) + dhw, dtype=torch.float32, device=ctx.device)
    k = k_tensor(ctx, [5, 7])
    for bad_x in (x.permute(0, 3, 2, 1), x[..., ::2], x.double(), x.half(), x[0]):
        with pytest.raises(AssertionError, match='topk_compact'):
            ops.topk_compact(ctx, bad_x, k)
    for bad_k in (k_tensor(ctx, [5]), k_tensor(ctx, [5, 7, 9]), k.long(), k.float(), k.view(2, 1), k.cpu()):
        with pytest.raises(AssertionError, match='topk_compact'):
            ops.topk_compact(ctx, x, bad_k)
    xyz = torch.full((B, n, 3), -7.0, dtype=torch.float32, device=ctx.device)
    counts = torch.full((B,), -1, dtype=torch.int32, device=ctx.device)
    ws = workspace(ctx, B, n)
    call = lambda **kw: abi(ctx, **{**dict(x=x.data_ptr(), stride=n, B=B, dhw=dhw, k=k.data_ptr(), xyz=xyz.data_ptr(), counts=counts.data_ptr(),
                                          cap=n, ws=ws), **kw})
    assert call(ws_bytes=ws.numel() - 1) == L.PCC_ERR_ARG and call(ws_bytes=0) == L.PCC_ERR_ARG
    assert b'workspace' in L.lib().pcc_last_error()
    for null in ('x', 'k', 'xyz', 'counts'):
        assert call(**{null: None}) == L.PCC_ERR_ARG, null
    assert call(dhw=(1024, 1024, 257)) == L.PCC_ERR_ARG and call(stride=n - 1) == L.PCC_ERR_ARG and call(cap=-1) == L.PCC_ERR_ARG
    assert call(B=-1) == L.PCC_ERR_ARG
    assert (xyz == -7.0).all() and (counts == -1).all()                 # a refused call launches nothing
    assert call(B=0) == 0 and (counts == -1).all()
    assert call(dhw=(8, 0, 8)) == 0 and counts.cpu().tolist() == [0, 0] and (xyz == -7.0).all()
    # the wrapper on empty shapes, and the call that works
    e_xyz, e_cnt = ops.topk_compact(ctx, x[:0], k[:0])
    assert e_xyz.shape == (0, n, 3) and e_cnt.shape == (0,)
    z_xyz, z_cnt = ops.topk_compact(ctx, x[:, :, :0], k)
    assert z_xyz.shape == (B, 0, 3) and z_cnt.cpu().tolist() == [0, 0]
    assert call() == 0 and counts.cpu().tolist() == [5, 7]


# ---- model level: the setting of tests/test_occ_gpu.py -- the 128^3 shell at octree level 1 (eight 64^3 blocks), synthetic weights ------
RES, LEVEL = 128, 1
SHAPE = [RES >> LEVEL] * 3


@pytest.fixture(scope='module')
def shell():
    from test_cli_gpu import _cloud
    from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree
    pts = _cloud(RES, 0)
    blocks, binstr = partition_octree(pts, [0, 0, 0], [RES] * 3, LEVEL)
    assert len(blocks) == 8
    return pts, blocks, binstr


def build(cfg, **kw):
    from pcc_geo_cnn_v2_amd.init_checkpoint import make_synthetic_weights
    m = ModelConfigType[cfg].build(batch_size=3, **kw)
    m.compress([1, 1] + SHAPE)
    m.set_weights(make_synthetic_weights(cfg))
    return m


@pytest.mark.parametrize('cfg,kw', [('c3p', {}), ('c1', {}), ('c3p', dict(entropy_coder='rans')), ('c3p', dict(precision='fp16'))])
def test_model_count_stream_is_the_fixed_stream_plus_counts_and_decodes_to_the_top_k(ctx, shell, cfg, kw):
    from pcc_geo_cnn_v2_amd.model_types import block_count
    pts, blocks, binstr = shell
    n_base = 1 if cfg == 'c1' else 2
    m, mf = build(cfg, **kw), build(cfg, **kw)
    encode = lambda model, **how: model.compress_blocks(ctx, blocks, binstr, pts, RES, LEVEL, opt_metrics=('d1_mse',), **how)
    data, meta, _ = encode(m, count_scale=1.0)
    fdata, _, _ = encode(mf, fixed_threshold=True)
    stream, fixed = data[0], fdata[0]
    assert all(len(s) == n_base + 1 for s, _ in stream) and all(len(s) == n_base for s, _ in fixed)
    assert [(tuple(s[:n_base]), t) for s, t in stream] == [(tuple(s), t) for s, t in fixed]      # the y/z strings and threshold bytes
    assert {t for _, t in stream} == {len(m.thresholds) // 2}
    assert [s[-1] for s, _ in stream] == [struct.pack('<I', len(b)) for b in blocks]
    dec, dbg = m.decompress_blocks(ctx, stream, SHAPE, debug=True, layers='count')
    print(cfg, kw, 'points per block in / out', [(len(b), len(d)) for b, d in zip(blocks, dec)])
    for b, (got, info) in enumerate(zip(dec, dbg)):
        rows, ke = T.select(info['x_hat'], len(blocks[b]), tuple(SHAPE))
        assert got.dtype == np.float32 and np.array_equal(got, rows), f'block {b}: {len(got)} rows, the rule gives {ke}'
        assert np.array_equal(got, meta[0]['x_hat_list'][b]), f'block {b}: the encoder\'s candidate'
    base, _ = m.decompress_blocks(ctx, stream, SHAPE, layers='base')
    lossy, _ = mf.decompress_blocks(ctx, fixed, SHAPE)
    assert all(np.array_equal(a, b) for a, b in zip(base, lossy))
    # a count string that is not 4 bytes long is refused before anything is launched
    s, t = stream[4]
    broken = stream[:4] + [(tuple(s[:-1]) + (s[-1][:3],), t)] + stream[5:]
    with pytest.raises(L.PccError, match=f'status {L.PCC_ERR_CORRUPT}'):
        m.decompress_blocks(ctx, broken, SHAPE, layers='count')
    with pytest.raises(L.PccError, match=f'status {L.PCC_ERR_CORRUPT}'):
        m.decompress_blocks(ctx, fixed, SHAPE, layers='count')           # no count string at all
    # rho = 0.5
    half, hmeta, _ = encode(m, count_scale=0.5)
    limit = [block_count(len(b), 0.5, 64 ** 3) for b in blocks]
    assert limit == [int(np.floor(0.5 * len(b) + 0.5)) for b in blocks]
    assert [s[-1] for s, _ in half[0]] == [struct.pack('<I', k) for k in limit]
    hdec, _ = m.decompress_blocks(ctx, half[0], SHAPE, layers='count')
    assert all(len(d) <= k for d, k in zip(hdec, limit)) and any(len(d) for d in hdec)
    assert all(np.array_equal(a, b) for a, b in zip(hdec, hmeta[0]['x_hat_list']))


def test_model_refuses_count_scale_with_the_other_policies(ctx, shell):
    pts, blocks, binstr = shell
    args = (ctx, blocks[:1], binstr, pts, RES, LEVEL)
    with pytest.raises(AssertionError, match='count_scale'):
        build('c1').compress_blocks(*args, fixed_threshold=True, count_scale=1.0)
    with pytest.raises(AssertionError, match='count_scale'):
        build('c1', lossless=True).compress_blocks(*args, count_scale=1.0)
    with pytest.raises(AssertionError, match='count_scale'):
        build('c1').compress_blocks(*args, count_scale=0.0)
    with pytest.raises(AssertionError, match='layers'):
        build('c1').decompress_blocks(ctx, [], SHAPE, layers='counts')


# ---- CLI -----------------------------------------------------------------------------------------------------------------------
def test_cli_count_threshold_roundtrip_base_only_and_the_files_without_the_flag(ctx, tmp_path):
    """The CLIs' own entry points (compress_octree.compress / decompress_octree.decompress on parsed arguments), in this process."""
    from pcc_geo_cnn_v2_amd import compress_octree, decompress_octree
    from pcc_geo_cnn_v2_amd.init_checkpoint import make_synthetic_weights
    from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree
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
             '--octree_level', str(LEVEL), '--opt_metrics', 'd1_mse', '--batch_size', '5', *extra]))

    def dec(inp, out, *extra):
        decompress_octree.decompress(decompress_octree.build_parser().parse_args(
            ['--input_files', inp, '--output_files', out, '--checkpoint_dir', ck, '--model_config', cfg, '--batch_size', '3', *extra]))

    def container(f):
        with gzip.open(f, 'rb') as fh:
            return model_syntax.load_compressed_file(fh)

    f_cnt, f_half, f_fixed, f_search, d_enc = (str(tmp_path / n) for n in ('cnt.bin', 'half.bin', 'fixed.bin', 'search.bin', 'enc.ply'))
    enc(f_cnt, '--count_threshold', '--dec_files', d_enc)
    enc(f_half, '--count_threshold', '0.5')
    enc(f_fixed, '--fixed_threshold')
    enc(f_search)
    tag = model_syntax.read_gzip_tag(f_fixed)
    assert model_syntax.read_gzip_tag(f_cnt) == model_syntax.read_gzip_tag(f_half) == tag + '/cnt1'
    assert 'cnt1' not in tag and model_syntax.read_gzip_tag(f_search) == tag
    blocks, _ = partition_octree(pts, [0, 0, 0], [RES] * 3, LEVEL)
    b_cnt, b_fixed = container(f_cnt)[3], container(f_fixed)[3]
    assert {len(s) for s, _ in b_cnt} == {3} and {len(s) for s, _ in b_fixed} == {len(s) for s, _ in container(f_search)[3]} == {2}
    assert [(s[:2], t) for s, t in b_cnt] == b_fixed
    assert [s[2] for s, _ in b_cnt] == [struct.pack('<I', len(b)) for b in blocks]
    assert [s[2] for s, _ in container(f_half)[3]] == [struct.pack('<I', int(np.floor(0.5 * len(b) + 0.5))) for b in blocks]
    # a file written without the flag: the bytes of the writer as it was before the flag existed (container + coder_tag), for --fixed_threshold
    m = build(cfg)
    m.batch_size = 5
    binstr = container(f_fixed)[2]
    data, _, _ = m.compress_blocks(ctx, blocks, list(binstr), pts, RES, LEVEL, opt_metrics=('d1_mse',), fixed_threshold=True)
    old = str(tmp_path / 'old.bin')
    model_syntax.write_tagged_gzip(old, model_syntax.save_compressed_file(list(binstr), data[0], RES, LEVEL, strict=True),
                                   model_syntax.coder_tag(ctx.numerics_tag('fp32'), 'range'))
    assert open(old, 'rb').read() == open(f_fixed, 'rb').read()
    new = {'threshold_policy', 'count_scale', 'count_bytes'}
    j = {f: json.load(open(f + '.enc.metric.json')) for f in (f_cnt, f_half, f_fixed, f_search)}
    assert set(j[f_cnt]) - set(j[f_fixed]) == new and not new & set(j[f_fixed]) and not new & set(j[f_search])
    assert set(j[f_fixed]) == set(j[f_search])
    assert (j[f_cnt]['threshold_policy'], j[f_cnt]['count_scale'], j[f_cnt]['count_bytes']) == ('count', 1.0, 4 * len(blocks))
    assert j[f_half]['count_scale'] == 0.5 and j[f_cnt]['codec_numerics'] == tag + '/cnt1'
    d_cnt, d_bo, d_fixed = (str(tmp_path / n) for n in ('cnt.ply', 'bo.ply', 'fixed.ply'))
    dec(f_cnt, d_cnt)                               # no flag: the stream names its layer
    assert open(d_cnt, 'rb').read() == open(d_enc, 'rb').read()
    dec(f_cnt, d_bo, '--base_only')
    dec(f_fixed, d_fixed)
    assert open(d_bo, 'rb').read() == open(d_fixed, 'rb').read()
    assert open(d_cnt, 'rb').read() != open(d_fixed, 'rb').read()
    print('points: input', len(pts), 'count', len(pc_io.load_pc(d_cnt)), 'fixed', len(pc_io.load_pc(d_fixed)))
