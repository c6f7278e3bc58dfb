"""Count search on the GPU: the rank-level kernel against its restatement, the count-indexed statistics against the
threshold-indexed ones on a surrogate field, what is scored against what is decoded, the model and the CLI.  Every comparison is exact."""
import gzip
import json
import os
import struct

import numpy as np
import pytest
import torch

import _count_search_ref as R
import _search_adversarial as SA
import _topk_ref as T
from pcc_geo_cnn_v2_amd import model_opt as MO
from pcc_geo_cnn_v2_amd import model_syntax, ops
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
from pcc_geo_cnn_v2_amd.utils import pc_io
from test_topk_gpu import on_device

pytestmark = pytest.mark.gpu

# _topk_ref.SHAPES plus the fused (W % 16 == 0) and fall-back distance-transform paths and a block of two 4096-voxel segments
SHAPES = T.SHAPES[:3] + ((8, 8, 16), (5, 7, 16), (16, 16, 32)) + T.SHAPES[3:]
BIG = (64, 64, 64)
ids = lambda s: 'x'.join(map(str, s)) if isinstance(s, tuple) else str(s)
_LEVELS = {}


def cases(dhw):
    """{ladder name: [(input name, scores, row, lev, tcount)]} of a shape: the restatement of every (input, ladder), computed once and
    shared.  At 64^3 three inputs (the zero bulk, one tie run over every segment, the special values) under four ladders."""
    if dhw not in _LEVELS:
        inputs = R.inputs(dhw) if dhw in T.SHAPES else _inputs_of(dhw)
        if dhw == BIG:
            inputs = {k: v for k, v in inputs.items() if k.split('-')[-1] in ('relu97', 'constant', 'special')}
        out = {}
        for name, x in inputs.items():
            for lname, c in R.ladders(x).items():
                if dhw == BIG and lname not in ('J1', 'J255', 'above-P', 'tie-cut'):
                    continue
                out.setdefault(lname, []).append((name, x, c) + R.levels_lexsort(x, c))
        _LEVELS[dhw] = out
    return _LEVELS[dhw]


def _inputs_of(dhw):
    n = int(np.prod(dhw))
    return {f'{ids(dhw)}-{name}': x for name, (x, _) in T._inputs(n, np.random.default_rng(2000 + n)).items()}


def rows_tensor(rows):
    return torch.from_numpy(np.ascontiguousarray(np.stack(rows), np.int32))


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dhw', SHAPES, ids=ids)
def test_rank_levels_equal_the_restatement_bit_for_bit(ctx, dhw):
    n = int(np.prod(dhw))
    for lname, group in cases(dhw).items():
        xs = [g[1] for g in group]
        buf, x = on_device(ctx, xs, dhw, pad=13)
        assert len(group) == 1 or (x.stride(0) == n + 13 and not x.is_contiguous())
        lev, tcount = ops.rank_levels(ctx, x, rows_tensor([g[2] for g in group]))
        assert lev.shape == (len(group), *dhw) and lev.dtype == torch.uint8 and tcount.dtype == torch.int32
        got, got_t = lev.cpu().numpy().reshape(len(group), n), tcount.cpu().numpy()
        for b, (name, _, c, want, want_t) in enumerate(group):
            assert got_t[b] == want_t, f'{name} {lname}: tcount {got_t[b]}, the rule gives {want_t}'
            assert np.array_equal(got[b], want), f'{name} {lname}: {np.count_nonzero(got[b] != want)} voxels differ'
        # the input and its sentinels are untouched (bit patterns: a row holds a NaN)
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), T.strided(xs, 13).view(np.uint32))


@pytest.mark.parametrize('dhw', [(16, 8, 24), BIG], ids=ids)
def test_levels_of_a_block_do_not_depend_on_the_batch_or_the_position_in_it(ctx, dhw):
    group = cases(dhw)['tie-cut']
    name, x0, c0, want, want_t = group[0]
    others = [g for g in group[1:]] + [g for g in cases(dhw)['above-P']][:2]
    pad = lambda c: np.concatenate([c, np.full(6 - len(c), c[-1], np.int32)])        # one J per launch: a row repeats its last entry
    want6, want6_t = R.levels_lexsort(x0, pad(c0))
    _, alone = on_device(ctx, [x0], dhw, pad=0)
    lev_a, t_a = ops.rank_levels(ctx, alone, rows_tensor([pad(c0)]))
    xs = [others[0][1], x0] + [g[1] for g in others[1:]] + [x0]
    cs = [pad(others[0][2]), pad(c0)] + [pad(g[2]) for g in others[1:]] + [pad(c0)]
    _, many = on_device(ctx, xs, dhw, pad=29)
    lev_m, t_m = ops.rank_levels(ctx, many, rows_tensor(cs))
    a = lev_a.cpu().numpy().ravel()
    assert np.array_equal(a, want6) and int(t_a[0]) == want6_t
    for pos in (1, len(xs) - 1):
        assert np.array_equal(lev_m[pos].cpu().numpy().ravel(), a) and int(t_m[pos]) == want6_t, f'position {pos} of {len(xs)}'


# ---- 2. count source = threshold source on a surrogate field ------------------------------------------------------------------------------
def _blocks_for(dhw, B, seed):
    """B blocks of rows (xyz + unit normals, float64) scattered over the grid, in row-major order"""
    import _metrics_ref as M
    n = int(np.prod(dhw))
    out = []
    for b in range(B):
        a = SA._scatter(dhw, max(3, min(n // 6, 700)), seed + b)
        out.append(np.hstack([a.astype(np.float64), M.unit_normals(len(a), seed + 50 + b)]))
    return out


def _surrogate_case(dhw):
    """(scores (B,n), rows (B,J), surrogate field (B,n) whose threshold levels under T256 are the rank levels, P per block)"""
    inputs = R.inputs(dhw) if dhw in T.SHAPES else _inputs_of(dhw)
    pick = [k for k in inputs if k.split('-')[-1] in ('uniform', 'levels8', 'relu97', 'special')]
    xs, rows, fields, Ps = [], [], [], []
    for i, k in enumerate(pick):
        x = inputs[k]
        P = int(np.count_nonzero(T.keys(x)))
        rho = MO.count_ladder(0.05, 1.2, 33)                      # counts from above P down to a twentieth of it, with duplicates at small P
        c = np.array([int(np.floor(r * P + 0.5)) for r in rho], np.int32)
        lev, _ = R.levels_lexsort(x, c)
        xs.append(x), rows.append(c), fields.append(SA.field_from_levels(lev)), Ps.append(P)
    return np.stack(xs), np.stack(rows), np.stack(fields).astype(np.float32), Ps


@pytest.mark.parametrize('dhw', SHAPES, ids=ids)
def test_count_statistics_equal_threshold_statistics_of_the_surrogate_field(ctx, dhw):
    xs, rows, fields, Ps = _surrogate_case(dhw)
    B, J = rows.shape
    blocks = _blocks_for(dhw, B, 300 + int(np.prod(dhw)) % 97)
    thr, xyz, bof, start, nrm = MO._upload_blocks(ctx, blocks, SA.T256, np.float32)
    x_hat = torch.from_numpy(xs).to(ctx.device).view(B, *dhw)
    x_sur = torch.from_numpy(fields).to(ctx.device).view(B, *dhw)
    want1 = ops.d1_threshold_stats(ctx, x_sur, thr, xyz, bof, clip=True)
    got1 = ops.d1_count_stats(ctx, x_hat, rows_tensor(list(rows)), xyz, bof)
    for nm, g, w in zip(('s_ab', 's_ba', 'n_b', 'tcount'), got1, want1):
        assert g.dtype == w.dtype and np.array_equal(g, w), f'd1 {nm}'
    want2 = ops.d12_threshold_stats(ctx, x_sur, thr, xyz, bof, start, nrm, clip=True)
    got2 = ops.d12_count_stats(ctx, x_hat, rows_tensor(list(rows)), xyz, bof, start, nrm)
    for nm, g, w in zip(('s_ab', 's_ba', 'n_b', 'tcount', 'd2_ab', 'd2_ba'), got2, want2):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.int64 if g.dtype == np.float64 else g.dtype),
                                                     w.view(np.int64 if w.dtype == np.float64 else w.dtype)), f'd12 {nm}'
    for nm, g, w in zip(('s_ab', 's_ba', 'n_b', 'tcount'), got2, got1):
        assert np.array_equal(g, w), f'd12 against d1: {nm}'
    n_b, tcount = got1[2], got1[3]
    for b in range(B):
        assert tcount[b] == (np.count_nonzero(rows[b] >= 1) if Ps[b] else 0)
        assert np.array_equal(n_b[b, :J], np.minimum(rows[b], Ps[b])), f'block {b}: n_b is min(c, P)'
        assert not n_b[b, J:].any()


# ---- 3. what is scored is what is decoded -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dhw', [(5, 7, 16), (16, 16, 32), BIG], ids=ids)
def test_the_scored_sets_are_the_sets_topk_compact_decodes(ctx, dhw):
    xs, rows, _, _ = _surrogate_case(dhw)
    B, J = rows.shape
    x_hat = torch.from_numpy(xs).to(ctx.device).view(B, *dhw)
    lev = ops.rank_levels(ctx, x_hat, rows_tensor(list(rows)))[0].cpu().numpy().reshape(B, -1)
    for j in (0, 1, J // 2, J - 2, J - 1):
        xyz, counts = ops.topk_compact(ctx, x_hat, torch.from_numpy(np.ascontiguousarray(rows[:, j])).to(ctx.device))
        counts = counts.cpu().numpy()
        for b in range(B):
            want = T.rows_of(np.flatnonzero(lev[b] > j), dhw)
            assert counts[b] == len(want) and np.array_equal(xyz[b, :counts[b]].cpu().numpy(), want), f'block {b}, candidate {j}'


# ---- 4. model: the setting of tests/test_topk_gpu.py -- the 128^3 shell at octree level 1 (64^3 blocks), synthetic weights ----------------
RES, LEVEL = 128, 1
SHAPE = [RES >> LEVEL] * 3
LADDER = (0.6, 1.6, 7)


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


def test_model_chooses_the_argmin_count_and_codes_it_behind_the_count_scale_strings(ctx, shell):
    _, blocks, _ = shell
    blocks = blocks[:4]                                            # two chunks of the batch size 3
    m = build('c3p')
    metrics, deltas = ('d1_mse', 'd1_sum_mean'), (np.inf, 1.3)
    strings, thr, points, names, dbg = m.encode_block_range(ctx, blocks, RES, opt_metrics=metrics, max_deltas=deltas, debug=True,
                                                            count_search=LADDER)
    ref, _, _, _, _ = build('c3p').encode_block_range(ctx, blocks, RES, opt_metrics=metrics, max_deltas=deltas, count_scale=1.0)
    n_base = m.n_strings
    assert names == [f'{mt}_{d}' for d in deltas for mt in metrics]
    rows = MO.count_rows(blocks, MO.count_ladder(*LADDER), 64 ** 3)
    chosen = []
    for b, blk in enumerate(blocks):
        x_hat = dbg[b]['x_hat'].reshape(-1)
        want_names, want_k = R.brute_choice(blk, x_hat, rows[b], SHAPE, RES, metrics, deltas)
        got_k = [struct.unpack('<I', s)[0] for s in strings[b][n_base:]]
        print('block', b, 'rows', len(blk), 'ladder', rows[b].tolist(), 'chosen', dict(zip(names, got_k)))
        assert want_names == names and got_k == want_k, f'block {b}: chosen {got_k}, brute force {want_k}'
        assert len(strings[b]) == n_base + len(names) and tuple(strings[b][:n_base]) == tuple(ref[b][:n_base])
        assert thr[b] == [len(m.thresholds) // 2] * len(names)
        for i, k in enumerate(got_k):
            assert np.array_equal(points[b][i], T.select(x_hat, k, tuple(SHAPE))[0]), f'block {b}, {names[i]}: the candidate'
        chosen.append(got_k)
    # every name's stream decodes to its own candidates
    for i in range(len(names)):
        stream = [(tuple(s[:n_base]) + (s[n_base + i],), t[i]) for s, t in zip(strings, thr)]
        dec, _ = m.decompress_blocks(ctx, stream, SHAPE, layers='count')
        assert all(np.array_equal(d, points[b][i]) for b, d in enumerate(dec)), names[i]


def test_model_d1_and_d2_outputs_carry_their_own_counts_and_decode_to_their_own_candidates(ctx, shell):
    import _metrics_ref as M
    pts, blocks, binstr = shell
    normals = M.unit_normals(len(pts), 77)
    cloud = np.hstack([pts, normals]).astype(np.float32)
    from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree
    nblocks, nbin = partition_octree(cloud, [0, 0, 0], [RES] * 3, LEVEL)
    assert len(nblocks) == 8
    m = build('c3p')
    m.d2_search = 'gpu'
    data, meta, _ = m.compress_blocks(ctx, nblocks, nbin, cloud, RES, LEVEL, with_normals=True, opt_metrics=('d1_mse', 'd2_mse'),
                                      count_search=LADDER)
    ref, _, _ = build('c3p').compress_blocks(ctx, nblocks, nbin, cloud, RES, LEVEL, with_normals=True, opt_metrics=('d1_mse',), count_scale=1.0)
    assert len(data) == 2 and sorted(x['idx'] for x in meta) == [0, 1]
    rows = MO.count_rows(nblocks, MO.count_ladder(*LADDER), 64 ** 3)
    for out, info in zip(data, meta):
        assert all(len(s) == m.n_strings + 1 and len(s[-1]) == 4 for s, _ in out)
        assert [tuple(s[:-1]) for s, _ in out] == [tuple(s[:-1]) for s, _ in ref[0]] and {t for _, t in out} == {len(m.thresholds) // 2}
        ks = [struct.unpack('<I', s[-1])[0] for s, _ in out]
        assert all(k == 0 or k in rows[b] for b, k in enumerate(ks))
        dec, _ = m.decompress_blocks(ctx, out, SHAPE, layers='count')
        assert all(np.array_equal(d, c) for d, c in zip(dec, info['x_hat_list'])), f'output {info["idx"]}'
        print('output', info['idx'], 'counts', ks)


# ---- 5. CLI ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_count_search_roundtrip_and_count_threshold_unchanged(ctx, tmp_path):
    """The CLIs' own entry points on parsed arguments, in this process (the setting of test_topk_gpu's CLI test)."""
    from pcc_geo_cnn_v2_amd import compress_octree, decompress_octree
    from pcc_geo_cnn_v2_amd.init_checkpoint import make_synthetic_weights
    from pcc_geo_cnn_v2_amd.model_types import block_count
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

    def container(f):
        with gzip.open(f, 'rb') as fh:
            return model_syntax.load_compressed_file(fh)

    f_cs, f_cnt, f_fixed, d_enc, d_dec = (str(tmp_path / n) for n in ('cs.bin', 'cnt.bin', 'fixed.bin', 'enc.ply', 'dec.ply'))
    enc(f_cs, '--dec_files', d_enc, '--count_search', '0.6', '1.6', '7')
    enc(f_cnt, '--count_threshold', '0.75')
    enc(f_fixed, '--fixed_threshold')
    decompress_octree.decompress(decompress_octree.build_parser().parse_args(
        ['--input_files', f_cs, '--output_files', d_dec, '--checkpoint_dir', ck, '--model_config', cfg, '--batch_size', '3']))
    assert open(d_dec, 'rb').read() == open(d_enc, 'rb').read()
    tag = model_syntax.read_gzip_tag(f_fixed)
    assert model_syntax.read_gzip_tag(f_cs) == tag + '/cnt1' and model_syntax.read_gzip_tag(f_cs).endswith('/cnt1')
    blocks, _ = partition_octree(pts, [0, 0, 0], [RES] * 3, LEVEL)
    b_cs, b_cnt, b_fixed = container(f_cs)[3], container(f_cnt)[3], container(f_fixed)[3]
    assert {len(s) for s, _ in b_cs} == {3} and [(s[:2], t) for s, t in b_cs] == b_fixed
    rows = MO.count_rows(blocks, MO.count_ladder(0.6, 1.6, 7), 64 ** 3)
    ks = [struct.unpack('<I', s[2])[0] for s, _ in b_cs]
    assert all(k == 0 or k in rows[b] for b, k in enumerate(ks))
    j = json.load(open(f_cs + '.enc.metric.json'))
    assert j['threshold_policy'] == 'count_search' and j['count_ladder'] == [0.6, 1.6, 7] and j['count_bytes'] == 4 * len(blocks)
    assert j['codec_numerics'] == tag + '/cnt1' and 'count_scale' not in j
    # --count_threshold on the same tree: the bytes of the rule as it was -- the fixed stream plus k = block_count(rows, rho, voxels)
    assert model_syntax.read_gzip_tag(f_cnt) == tag + '/cnt1'
    assert [(s[:2], t) for s, t in b_cnt] == b_fixed
    assert [s[2] for s, _ in b_cnt] == [struct.pack('<I', block_count(len(b), 0.75, 64 ** 3)) for b in blocks]
    binstr = container(f_fixed)[2]
    old = str(tmp_path / 'old.bin')
    data = [(tuple(s) + (struct.pack('<I', block_count(len(b), 0.75, 64 ** 3)),), t) for (s, t), b in zip(b_fixed, blocks)]
    model_syntax.write_tagged_gzip(old, model_syntax.save_compressed_file(list(binstr), data, RES, LEVEL, strict=True), tag + '/cnt1')
    assert open(old, 'rb').read() == open(f_cnt, 'rb').read()
    jc = json.load(open(f_cnt + '.enc.metric.json'))
    assert (jc['threshold_policy'], jc['count_scale'], jc['count_bytes']) == ('count', 0.75, 4 * len(blocks)) and 'count_ladder' not in jc
    print('counts chosen', ks, 'input rows', [len(b) for b in blocks])
