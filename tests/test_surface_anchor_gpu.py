"""GPU: the HIP side of the surface anchor codec (csrc/surface_anchor.hip) against the restatement in tests/_surface_ref.py and against
the package's numpy host path.  Every test runs under its own time limit (a watchdog that ends the process: a stuck kernel must not
keep the card); malformed streams are tested on the host checks only (tests/test_surface_anchor_cpu.py)."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import yaml

import _surface_ref as R
from _normals_ref import shell
from pcc_geo_cnn_v2_amd import anchor_surface as S
from pcc_geo_cnn_v2_amd.utils import pc_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT = 300          # seconds per test
NAMES = sorted(R.small_clouds())


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize('name', NAMES)
def test_vertex_arrays_and_voxels_equal_the_restatement(ctx, name):
    points, resolution = R.small_clouds()[name]
    for k in R.KS:
        ref = R.coded(name, k)
        leaf_keys, edge_keys, flags, t = S.vertices(points, resolution, k, device='gpu', ctx=ctx)
        for got, key in ((leaf_keys, 'leaf_keys'), (edge_keys, 'edge_keys'), (flags, 'flags'), (t, 't')):
            assert np.array_equal(got, ref[key]), (k, key)
        got = S.surface_points(ref['leaf_keys'], ref['edge_keys'], ref['flags'], ref['t'], resolution, k, device='gpu', ctx=ctx)
        assert got.dtype == np.int32 and np.array_equal(got, ref['decoded']), k


@pytest.mark.parametrize('name', NAMES)
def test_codec_equal_on_both_devices_and_to_the_restatement(ctx, name):
    points, resolution = R.small_clouds()[name]
    for k in R.KS:
        host = S.encode(points, resolution, k, device='host')
        gpu = S.encode(points, resolution, k, device='gpu', ctx=ctx)
        assert gpu == host and gpu == R.coded(name, k)['stream'], k
        assert S.encode(points, resolution, k, device='gpu', ctx=ctx) == gpu, k                   # two calls, the same bytes
        want = S.reconstruct(points, resolution, k)
        dec_gpu, dec_host = S.decode(gpu, device='gpu', ctx=ctx), S.decode(gpu, device='host')    # one stream, both decoders
        assert dec_gpu.dtype == dec_host.dtype == np.int32
        assert np.array_equal(dec_gpu, dec_host) and np.array_equal(dec_gpu, want), k


@pytest.mark.parametrize('k', [5, 6])
def test_the_large_blocks_equal_the_host_path(ctx, k):
    """k = 5 and 6 take the four-wave kernel with the largest voxel maps: against the host path and against the restatement."""
    for name in ('shell128', 'res100'):
        points, resolution = R.small_clouds()[name]
        gpu = S.encode(points, resolution, k, device='gpu', ctx=ctx)
        assert gpu == S.encode(points, resolution, k, device='host')
        dec = S.decode(gpu, device='gpu', ctx=ctx)
        assert np.array_equal(dec, S.reconstruct(points, resolution, k))
        ref = R.coded(name, k)                                             # R.coded_points, once per (cloud, k)
        assert gpu == ref['stream'] and dec.dtype == np.int32 and np.array_equal(dec, ref['decoded'])


@pytest.mark.parametrize('k', [2, 4])
def test_the_527k_shell_agrees_with_the_host_path(ctx, k):
    points, _ = shell(1024, radius=0.2, half_width=0.5)
    gpu = S.encode(points, 1024, k, device='gpu', ctx=ctx)
    assert gpu == S.encode(points, 1024, k, device='host')
    dec = S.decode(gpu, device='gpu', ctx=ctx)
    assert np.array_equal(dec, S.reconstruct(points, 1024, k))
    R.hausdorff_condition(points, dec, k, k)


def test_ev_run_anchor_both_codecs_feed_ev_run_compare(tmp_path):
    points = R.small_clouds()['shell128'][0]
    os.makedirs(tmp_path / 'exp')
    os.makedirs(tmp_path / 'dataset')
    pc_io.write_df(str(tmp_path / 'dataset' / 'shell.ply'), pc_io.pa_to_df(points.astype(np.float32)))
    ids = ('octree-anchor', 'surface-anchor')
    exp = {'EXPERIMENT_DIR': str(tmp_path / 'exp'), 'MPEG_DATASET_DIR': str(tmp_path / 'dataset'),
           'model_configs': [{'id': 'c4', 'config': 'c3p', 'lambdas': [3.0e-4], 'label': 'c4'}], 'opt_metrics': ['d1_mse'], 'bd_ignore': [],
           'anchor_device': 'gpu', 'metrics_device': 'gpu', 'anchor_rates': {'r01': [1, 8], 'r02': [1, 4], 'r03': [1, 2], 'r04': [3, 4]},
           'mpeg_modes': [{'id': ids[0], 'label': 'octree anchor'}, {'id': ids[1], 'label': 'surface anchor'}],
           'eval_modes': [{'id': 'main', 'no_legend': True, 'modes': [{'id': 'c4'}, {'id': ids[0]}, {'id': ids[1]}]}],
           'data': [{'pc_name': 'shell', 'input_pc': 'shell.ply', 'resolution': 128}]}
    yml = str(tmp_path / 'experiment.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(exp, f)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-m', 'pcc_geo_cnn_v2_amd.ev_run_anchor', yml, '--codec', 'both'], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=STEP_LIMIT)
    assert r.returncode == 0, r.stderr[-3000:]
    reports = {}
    for anchor_id, rates in ((ids[0], exp['anchor_rates']), (ids[1], {'r01': 5, 'r02': 4, 'r03': 3, 'r04': 2})):
        for rate, par in rates.items():
            d = tmp_path / 'exp' / 'gpcc' / anchor_id / 'shell' / rate
            assert sorted(os.listdir(d)) == ['report.json', 'shell.ply.bin', 'shell.ply.bin.decoded.ply'], (anchor_id, rate)
            if anchor_id == ids[1]:
                assert (d / 'shell.ply.bin').read_bytes() == S.encode(points, 128, par, device='host')
            with open(d / 'report.json') as f:
                reports[anchor_id, rate] = json.load(f)
    # one model's report tree, hand-made as in tests/test_anchor_cpu.py: the surface anchor's curve, a little better
    for rate, lmbda in (('r01', '3.00e-04'), ('r02', '1.00e-04'), ('r03', '5.00e-05'), ('r04', '2.00e-05')):
        rep = reports[ids[1], rate]
        d = tmp_path / 'exp' / 'shell' / 'c4' / lmbda
        os.makedirs(d)
        with open(d / 'report_d1.json', 'w') as f:
            json.dump({'pos_bits_per_input_point': rep['pos_bits_per_input_point'] * 0.8, 'd1_psnr': rep['d1_psnr'] + 1.0, 'input_point_count': 1}, f)
    r = subprocess.run([sys.executable, '-m', 'pcc_geo_cnn_v2_amd.ev_run_compare', yml], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=STEP_LIMIT)
    assert r.returncode == 0, r.stderr[-3000:]
    for table in ('bdrate', 'bdsnr'):
        tab = pd.read_csv(tmp_path / 'exp' / 'results' / f'{table}.csv', index_col=0)
        assert set(ids) <= set(tab.columns) and set(tab.mode_id) == {'c4', *ids}
        row = tab[(tab.mode_id == 'c4') & (tab.pc_name == 'shell')].iloc[0]
        assert np.isfinite(row[ids[1]]) and row[ids[1]] != 0
