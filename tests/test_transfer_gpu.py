"""GPU: the colour transfer (include/pcc_geo.h "cloud colours", pcc_cloud_transfer_colors) against its host restatement
utils/pc_metric.transfer_colors_host -- colours and votes exactly, on the cases of tests/_transfer_cases.py -- its independence of
row order and input kind, and the paths that use it: map_color --mode transfer and the recolor step of ev_experiment."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import _transfer_cases as T
from pcc_geo_cnn_v2_amd import map_color, ops
from pcc_geo_cnn_v2_amd.utils import pc_io, pc_metric

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = T.cases()
_HOST = {}


def _host(name):
    """The host restatement of a case, computed once and never written to."""
    if name not in _HOST:
        col, votes = pc_metric.transfer_colors_host(*CASES[name])
        col.setflags(write=False)
        votes.setflags(write=False)
        _HOST[name] = (col, votes)
    return _HOST[name]


@pytest.mark.parametrize('name', sorted(CASES))
def test_colours_and_votes_equal_the_host_restatement(ctx, name):
    a, ca, b = CASES[name]
    got, votes = ops.transfer_colors(ctx, a, ca, b, return_votes=True)
    ref, ref_votes = _host(name)
    assert got.dtype == np.uint8 and got.shape == (len(b), 3) and votes.dtype == np.int32 and votes.shape == (len(b),)
    bad = np.nonzero(votes != ref_votes)[0]
    assert len(bad) == 0, (name, len(bad), bad[:3], votes[bad[:3]], ref_votes[bad[:3]])
    bad = np.nonzero((got != ref).any(1))[0]
    assert len(bad) == 0, (name, len(bad), bad[:3], got[bad[:3]], ref[bad[:3]])
    assert np.array_equal(ops.transfer_colors(ctx, a, ca, b), got)             # without the votes output


def test_a_cloud_onto_itself_keeps_its_colours_with_one_vote_each(ctx):
    a, ca, b = CASES['identity']
    got, votes = ops.transfer_colors(ctx, a, ca, b, return_votes=True)
    assert np.array_equal(got, ca) and (votes == 1).all()


def test_half_rounds_up_and_all_votes_arrive(ctx):
    got, votes = ops.transfer_colors(ctx, *CASES['rounding'], return_votes=True)
    assert got.tolist() == [[1, 0, 2]] and votes.tolist() == [2]
    a, ca, b = CASES['many_voters']
    got, votes = ops.transfer_colors(ctx, a, ca, b, return_votes=True)
    s = ca.astype(np.int64).sum(0)
    assert votes.tolist() == [len(a)] and got.tolist() == [((2 * s + len(a)) // (2 * len(a))).tolist()]


@pytest.mark.parametrize('name', ['fallback_jitter', 'duplicates', 'random256'])
def test_same_bits_on_every_call_and_under_row_permutations(ctx, name):
    a, ca, b = CASES[name]
    ref, ref_votes = ops.transfer_colors(ctx, a, ca, b, return_votes=True)
    again, again_votes = ops.transfer_colors(ctx, a, ca, b, return_votes=True)
    assert again.tobytes() == ref.tobytes() and again_votes.tobytes() == ref_votes.tobytes()
    rng = np.random.default_rng(4)
    pa, pb = rng.permutation(len(a)), rng.permutation(len(b))
    got, votes = ops.transfer_colors(ctx, a[pa], ca[pa], b, return_votes=True)
    assert np.array_equal(got, ref) and np.array_equal(votes, ref_votes)
    got, votes = ops.transfer_colors(ctx, a, ca, b[pb], return_votes=True)
    assert np.array_equal(got, ref[pb]) and np.array_equal(votes, ref_votes[pb])


def test_duplicate_rows_of_b_get_identical_colours_and_votes(ctx):
    a, ca, b = CASES['duplicates']
    got, votes = ops.transfer_colors(ctx, a, ca, b, return_votes=True)
    _, first, inv = np.unique(b, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    assert np.array_equal(got, got[first][inv]) and np.array_equal(votes, votes[first][inv])


def test_indices_and_device_tensors_change_nothing(ctx):
    a, ca, b = CASES['fallback_jitter']
    ref, ref_votes = _host('fallback_jitter')
    ia, ib = ops.CloudIndex(ctx, a), ops.CloudIndex(ctx, b)
    dev = lambda x: torch.from_numpy(x).to(ctx.device)
    for src, q in ((ia, b), (a, ib), (ia, ib), (a, dev(b)), (dev(a), dev(b)), (ia, dev(b))):
        got, votes = ops.transfer_colors(ctx, src, ca, q, return_votes=True)
        assert np.array_equal(got, ref) and np.array_equal(votes, ref_votes)
    assert np.array_equal(ops.transfer_colors(ctx, ia, dev(ca), ib), ref)
    # the same indices serve map_colors, which takes an index of the queries too
    for rank in (1, 2):
        assert np.array_equal(ops.map_colors(ctx, ia, ca, ib, rank=rank), ops.map_colors(ctx, a, ca, b, rank=rank))


def _write_pair(tmp_path, a, ca, b):
    ori = pd.DataFrame({'x': a[:, 0].astype(np.float32), 'y': a[:, 1].astype(np.float32), 'z': a[:, 2].astype(np.float32),
                        'red': ca[:, 0], 'green': ca[:, 1], 'blue': ca[:, 2]})
    tgt = pd.DataFrame({'x': b[:, 0].astype(np.int32), 'y': b[:, 1].astype(np.int32), 'z': b[:, 2].astype(np.float64)})
    pc_io.write_ply(str(tmp_path / 'a.ply'), ori)
    pc_io.write_ply(str(tmp_path / 'b.ply'), tgt)
    return str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply')


def test_map_color_mode_transfer_and_the_unchanged_default(ctx, tmp_path):
    a, ca, b = CASES['fallback_jitter']
    ori, tgt = _write_pair(tmp_path, a, ca, b)
    out = str(tmp_path / 'transfer.ply')
    subprocess.run([sys.executable, '-m', 'pcc_geo_cnn_v2_amd.map_color', ori, tgt, out, '--mode', 'transfer'], check=True, cwd=ROOT,
                   timeout=600)
    df = pc_io.read_ply(out)
    assert list(df.columns) == ['x', 'y', 'z', 'red', 'green', 'blue']
    assert [df[c].dtype for c in df.columns] == [np.int32, np.int32, np.float64, np.uint8, np.uint8, np.uint8]
    assert np.array_equal(df[['x', 'y', 'z']].values, b)
    assert np.array_equal(pc_io.load_colors(out), ops.transfer_colors(ctx, a, ca, b))
    assert np.array_equal(pc_io.load_colors(out), _host('fallback_jitter')[0])
    # the default mode: the file map_color(...) writes without the argument, which is rank 2
    files = [str(tmp_path / f) for f in ('plain.ply', 'rank.ply', 'both.ply')]
    got = map_color.map_color(ori, tgt, files[0], ctx=ctx)
    map_color.map_color(ori, tgt, files[1], ctx=ctx, mode='rank')
    map_color.map_color(ori, tgt, files[2], 2, ctx, 'rank')
    assert np.array_equal(got, ops.map_colors(ctx, a, ca, b, rank=2))
    assert open(files[0], 'rb').read() == open(files[1], 'rb').read() == open(files[2], 'rb').read()
    assert np.array_equal(map_color.map_color(ori, tgt, files[1], ctx=ctx, mode='transfer'), _host('fallback_jitter')[0])
    assert open(files[1], 'rb').read() == open(out, 'rb').read()


def test_anchor_colour_step_under_recolor_transfer(ctx, tmp_path):
    """ev_run_anchor --color with the YAML key recolor: transfer -- the decoded cloud carries the op's colours, the colour anchor
    codes those, and report_color.json names the rule."""
    import yaml
    from pcc_geo_cnn_v2_amd import ev_run_anchor
    points = T.sphere_shell(64)
    colors = T.colors(len(points), 41)
    os.makedirs(tmp_path / 'exp')
    os.makedirs(tmp_path / 'dataset')
    pc_io.write_df(str(tmp_path / 'dataset' / 'shell.ply'), pc_io.pa_to_df(np.concatenate([points.astype(np.float64), colors], axis=1)))
    exp = {'EXPERIMENT_DIR': str(tmp_path / 'exp'), 'MPEG_DATASET_DIR': str(tmp_path / 'dataset'), 'anchor_device': 'gpu', 'metrics_device': 'gpu',
           'model_configs': [{'id': 'c4', 'config': 'c3p', 'lambdas': [3.0e-4], 'label': 'c4'}], 'opt_metrics': ['d1_mse'], 'bd_ignore': [],
           'mpeg_modes': [{'id': 'octree-anchor', 'label': 'octree anchor'}],
           'eval_modes': [{'id': 'main', 'no_legend': True, 'modes': [{'id': 'c4'}, {'id': 'octree-anchor'}]}],
           'anchor_rates': {'r01': [1, 2]}, 'color_rates': {'r01': 8}, 'recolor': 'transfer',
           'data': [{'pc_name': 'shell', 'input_pc': 'shell.ply', 'resolution': 64}]}
    yml = str(tmp_path / 'experiment.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(exp, f)
    assert ev_run_anchor.main([yml, '--color']) == 0
    d = tmp_path / 'exp' / 'gpcc' / 'octree-anchor' / 'shell' / 'r01'
    dec = str(d / 'shell.ply.bin.decoded.ply')
    b = pc_io.load_pc(dec)
    assert len(b) > 0
    assert np.array_equal(pc_io.load_colors(dec + '.color.ply'), ops.transfer_colors(ctx, points, colors, b))
    with open(d / 'report_color.json') as f:
        rep = json.load(f)
    assert rep['recolor'] == 'transfer' and rep['color_qstep'] == 8
    with open(d / 'report.json') as f:
        assert 'recolor' not in json.load(f)


def test_experiment_recolor_transfer(ctx, tmp_path):
    """One fixed-threshold job on the 256^3 synthetic shell with designed weights (as tests/test_experiment_gpu.py), coloured:
    recolor='transfer' puts the op's colours on the decoded cloud and "recolor" into the report; the default adds no key."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import rd_sweep
    from pcc_geo_cnn_v2_amd.ev_experiment import Resident, _recolor, run_experiment
    from pcc_geo_cnn_v2_amd.init_checkpoint import make_cell_codec_weights
    pts = rd_sweep.synthetic_cloud(256)
    colors = T.colors(len(pts), 31)
    src = str(tmp_path / 'colored.ply')
    pc_io.write_df(src, pc_io.pa_to_df(np.hstack([pts, colors.astype(np.float32)])))
    ckpt = str(tmp_path / 'ckpt')
    os.makedirs(ckpt)
    np.savez(os.path.join(ckpt, 'model.npz'), **make_cell_codec_weights(4))
    out = str(tmp_path / 'out')
    job = dict(output_dir=out, model_dir=ckpt, model_config='c3p', pc_name='shell', input_pc=src, fixed_threshold=True, resolution=256,
               octree_level=2, batch_size=16)
    resident = Resident()
    report = run_experiment(resident=resident, recolor='transfer', **job)['d1']
    assert report['recolor'] == 'transfer'
    with open(os.path.join(out, 'report_d1.json')) as f:
        assert json.load(f) == report
    dec = os.path.join(out, 'shell_d1.ply.bin.ply')
    b = pc_io.load_pc(dec)
    want = ops.transfer_colors(ctx, pts, colors, b)
    assert np.array_equal(pc_io.load_colors(dec + '.color.ply'), want)
    assert np.array_equal(pc_io.load_pc(dec + '.color.ply'), b)
    # the default: rank 2 colours, and a report without the key (made again from the files that are there)
    os.remove(os.path.join(out, 'report_d1.json'))
    os.remove(dec + '.color.ply')
    plain = run_experiment(resident=resident, **job)['d1']
    assert 'recolor' not in plain and plain == {k: v for k, v in report.items() if k != 'recolor'}
    assert np.array_equal(pc_io.load_colors(dec + '.color.ply'), ops.map_colors(ctx, pts, colors, b, rank=2))
    original = resident.original(src, None, False, 16)
    _recolor(resident, original, dec, str(tmp_path / 'direct.ply'), 'transfer')
    assert np.array_equal(pc_io.load_colors(str(tmp_path / 'direct.ply')), want)
