"""GPU: colour transfer and colour distortion (include/pcc_geo.h "cloud colours") against the numpy / scipy restatement in
tests/_color_ref.py -- mapped rows and colours exactly, the colour tally to 1e-12 -- against the reference's map_color rule
(cKDTree k = 2, second neighbour) where no tie is involved, and through the map_color CLI and `ev_report --color` end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch
from scipy.spatial import cKDTree

import _color_ref as R
from pcc_geo_cnn_v2_amd import ev_report, ops
from pcc_geo_cnn_v2_amd.utils import pc_io, pc_metric

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = R.color_pairs()


def _rel(x, y):
    return np.abs(x - y) / np.maximum(np.abs(y), 1e-300)


@pytest.mark.parametrize('rank', [1, 2])
@pytest.mark.parametrize('name', sorted(PAIRS))
def test_mapped_rows_and_colours_match_the_restatement(ctx, name, rank):
    a, ca, b, cb = PAIRS[name]
    for src, csrc, dst in ((a, ca, b), (b, cb, a)):
        if rank > len(src):
            continue
        got, rows = ops.map_colors(ctx, src, csrc, dst, rank=rank, return_rows=True)
        ref, ref_rows = R.map_ref(src, csrc, dst, rank)
        assert got.dtype == np.uint8 and got.shape == (len(dst), 3) and rows.dtype == np.int32
        bad = np.nonzero(rows != ref_rows)[0]
        assert len(bad) == 0, (name, rank, len(bad), bad[:3], rows[bad[:3]], ref_rows[bad[:3]])
        assert np.array_equal(got, ref)
    if rank == 1:                                                          # rank 1 is cloud_nearest's row
        idx = ops.CloudIndex(ctx, a)
        assert np.array_equal(ops.map_colors(ctx, idx, ca, b, rank=1, return_rows=True)[1], ops.cloud_nearest(ctx, idx, b)[0])


def test_rank_two_is_the_reference_map_color_on_tie_free_clouds(ctx):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 21, (200000, 3))
    q = np.concatenate([a[rng.permutation(len(a))[:20000]], rng.integers(0, 1 << 21, (80000, 3))])     # some queries ARE originals
    ca = R.random_colors(len(a), 6)
    d, idx = cKDTree(a.astype(np.float64)).query(q.astype(np.float64), k=3)
    d2 = ((a[idx] - q[:, None, :]) ** 2).sum(-1)                           # exact: the fixture has no ties among the first three
    assert (np.diff(d2, axis=1) > 0).all()
    got, rows = ops.map_colors(ctx, a, ca, q, return_rows=True)
    assert np.array_equal(rows, idx[:, 1]) and np.array_equal(got, ca[idx[:, 1]])


def test_rank_one_of_a_cloud_onto_itself_returns_its_colours(ctx):
    a, ca, _, _ = PAIRS['uniform']
    assert len(np.unique(a, axis=0)) == len(a)
    assert np.array_equal(ops.map_colors(ctx, a, ca, a, rank=1), ca)
    s, cs, _, _ = PAIRS['shell_perturbed']
    assert np.array_equal(ops.map_colors(ctx, s, cs, torch.from_numpy(s).to(ctx.device), rank=1), cs)      # device tensor queries


@pytest.mark.parametrize('name', sorted(PAIRS))
def test_color_tally_matches_the_restatement(ctx, name):
    a, ca, b, cb = PAIRS[name]
    got = ops.cloud_color_distortion(ctx, a, ca, b, cb)
    ref = R.tally_ref(a, ca, b, cb)
    assert got.dtype == np.float64 and got.shape == (6,)
    assert np.all(_rel(got, ref) <= 1e-12), (name, got, ref)


def test_identical_clouds_give_zero_and_infinite_psnr(ctx):
    for name in ('uniform', 'duplicates_in_a'):
        a, ca, _, _ = PAIRS[name]
        if name == 'duplicates_in_a':                        # duplicates carry one colour each, or the mean of a tie differs
            a = np.unique(a, axis=0)
            ca = R.random_colors(len(a), 9)
        t = ops.cloud_color_distortion(ctx, a, ca, a, ca)
        assert np.array_equal(t, np.zeros(6))
        m = pc_metric.color_table(t, len(a), len(a))
        assert all(m[f'{k}_mse'] == 0 and m[f'{k}_psnr'] == np.inf for k in 'yuv')


def test_permuting_the_decoded_rows_leaves_the_tally_unchanged(ctx):
    # lattice against sub-lattice: up to eight equidistant neighbours; a lowest-row rule would pick colours by row and fail this
    for name in ('lattice_sublattice', 'sublattice_lattice'):
        a, ca, b, cb = PAIRS[name]
        t = ops.cloud_color_distortion(ctx, a, ca, b, cb)
        for seed in (1, 2):
            p = np.random.default_rng(seed).permutation(len(b))
            tp = ops.cloud_color_distortion(ctx, a, ca, b[p], cb[p])
            assert np.all(_rel(tp, t) <= 1e-12), (name, tp, t)


@pytest.mark.parametrize('name', ['shell_perturbed', 'lattice_sublattice', 'duplicates_in_a'])
def test_two_calls_give_identical_bits(ctx, name):
    a, ca, b, cb = PAIRS[name]
    index = ops.CloudIndex(ctx, a)
    t1 = ops.cloud_color_distortion(ctx, index, ca, b, cb)
    t2 = ops.cloud_color_distortion(ctx, index, ca, b, cb)
    assert t1.tobytes() == t2.tobytes()
    assert ops.map_colors(ctx, index, ca, b).tobytes() == ops.map_colors(ctx, index, ca, b).tobytes()


def test_map_color_cli_writes_the_target_with_mapped_colours(ctx, tmp_path):
    a, ca, b, _ = PAIRS['shell_perturbed']
    ori = pd.DataFrame({'x': a[:, 0].astype(np.float32), 'y': a[:, 1].astype(np.float32), 'z': a[:, 2].astype(np.float32),
                        'red': ca[:, 0], 'green': ca[:, 1], 'blue': ca[:, 2]})
    tgt = pd.DataFrame({'x': b[:, 0].astype(np.int32), 'y': b[:, 1].astype(np.int32), 'z': b[:, 2].astype(np.float64)})
    pc_io.write_ply(str(tmp_path / 'a.ply'), ori)
    pc_io.write_ply(str(tmp_path / 'b.ply'), tgt, as_text=True)
    for rank in (2, 1):
        out = tmp_path / f'o{rank}.ply'
        cmd = [sys.executable, '-m', 'pcc_geo_cnn_v2_amd.map_color', str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply'), str(out)]
        subprocess.run(cmd + (['--rank', '1'] if rank == 1 else []), check=True, cwd=ROOT, timeout=600)
        assert open(out, 'rb').read().split(b'\n')[1] == b'format binary_little_endian 1.0'
        df = pc_io.read_ply(str(out))
        assert list(df.columns) == ['x', 'y', 'z', 'red', 'green', 'blue']
        assert [df[c].dtype for c in df.columns] == [np.int32, np.int32, np.float64, np.uint8, np.uint8, np.uint8]
        assert np.array_equal(df[['x', 'y', 'z']].values, b)
        assert np.array_equal(df[['red', 'green', 'blue']].values, ops.map_colors(ctx, a, ca, b, rank=rank))
        assert np.array_equal(pc_io.load_colors(str(out)), R.map_ref(a, ca, b, rank)[0])


def test_gpu_report_with_color_equals_host_mode(ctx, tmp_path):
    for name in ('shell_perturbed', 'lattice_sublattice'):
        a, ca, b, cb = PAIRS[name]
        for f, p, c in (('a.ply', a, ca), ('b.ply', b, cb)):
            pc_io.write_ply(str(tmp_path / f), pd.DataFrame({'x': p[:, 0].astype(np.float32), 'y': p[:, 1].astype(np.float32),
                                                             'z': p[:, 2].astype(np.float32), 'red': c[:, 0], 'green': c[:, 1],
                                                             'blue': c[:, 2]}))
        open(tmp_path / 'a.bin', 'wb').write(b'\x00' * 1000)
        paths = [str(tmp_path / f) for f in ('a.ply', 'b.ply', 'a.bin')]
        host = ev_report.build_report(*paths, 1024, color=True)
        gpu = ev_report.build_report(*paths, 1024, metrics_device='gpu', color=True)
        assert set(gpu) == set(host)
        for k in 'yuv':
            assert _rel(gpu[f'{k}_mse'], host[f'{k}_mse']) <= 1e-12, (name, k, gpu, host)
            assert abs(gpu[f'{k}_psnr'] - host[f'{k}_psnr']) <= 1e-9, (name, k, gpu, host)
        assert gpu['d1_mse'] == host['d1_mse']
        assert ev_report.build_report(*paths, 1024, metrics_device='gpu') == {k: v for k, v in gpu.items() if k[0] not in 'yuv'}
