"""GPU: the HIP side of the colour anchor codec (csrc/color_anchor.hip) against the package's numpy host path, which
tests/test_color_anchor_cpu.py holds against the restatement.  Every test runs under its own time limit (a watchdog that ends the
process: a stuck kernel must not keep the card); malformed streams are tested on the host checks only."""
import faulthandler
import json
import os

import numpy as np
import pytest
import yaml

import _color_anchor_ref as R
from pcc_geo_cnn_v2_amd import anchor_color as C
from pcc_geo_cnn_v2_amd import ev_report, ev_run_anchor
from pcc_geo_cnn_v2_amd.utils import pc_io

pytestmark = pytest.mark.gpu
STEP_LIMIT = 300          # seconds per test
QS = (1, 16, 255)


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _random_cloud(n, bits, seed):
    """n distinct points in [0, 2^bits)^3 with random colours."""
    rng = np.random.default_rng(seed)
    pts = np.unique(rng.integers(0, 1 << bits, (2 * n + 8, 3)), axis=0)
    pts = rng.permutation(pts)[:n]
    assert len(pts) == n
    return pts, rng.integers(0, 256, (n, 3)).astype(np.uint8)


def _cases():
    shell = R.shell()
    wide, wide_colors = _random_cloud(20000, 21, 20)
    wide[0] = (1 << 21) - 1                                  # 63-bit keys
    assert len(np.unique(wide, axis=0)) == len(wide)
    out = {f'n{n}': _random_cloud(n, 7, n) for n in (1, 2, 3, 64, 65, 257)}
    out.update(shell_smooth=(shell, R.smooth_colors(shell)), shell_alternating=(shell, R.alternating_colors(shell)),
               wide_random=(wide, wide_colors), wide_alternating=(wide[:3000], R.alternating_colors(wide[:3000])))
    return out


CASES = _cases()


@pytest.mark.parametrize('name', sorted(CASES))
def test_both_devices_give_the_same_bytes_and_arrays(ctx, name):
    points, colors = CASES[name]
    for q in QS:
        host = C.encode(points, colors, q, device='host')
        gpu = C.encode(points, colors, q, device='gpu', ctx=ctx)
        assert gpu == host, q
        want = C.reconstruct(points, colors, q)
        for data in (host, gpu):                                  # streams crossed both ways
            assert np.array_equal(C.decode(data, points, device='gpu', ctx=ctx), want), q
            assert np.array_equal(C.decode(data, points, device='host'), want), q
        if q == 1:
            assert np.array_equal(want, colors)
        hc, hdc, hcoef = C.coefficients(points, colors, q, device='host')
        gc, gdc, gcoef = C.coefficients(points, colors, q, device='gpu', ctx=ctx)
        assert gcoef.dtype == hcoef.dtype and gcoef.shape == hcoef.shape == (len(points) - 1, 3)
        assert np.array_equal(gc, hc) and np.array_equal(gdc, hdc) and np.array_equal(gcoef, hcoef), q


def test_rows_follow_the_callers_points_on_the_device(ctx):
    points, colors = CASES['shell_smooth']
    perm = np.random.default_rng(1).permutation(len(points))
    data = C.encode(points, colors, 16, device='gpu', ctx=ctx)
    assert C.encode(points[perm], colors[perm], 16, device='gpu', ctx=ctx) == data
    assert np.array_equal(C.decode(data, points[perm], device='gpu', ctx=ctx), C.reconstruct(points, colors, 16)[perm])


def test_duplicate_positions_raise_from_the_device_path(ctx):
    points, colors = CASES['n65']
    points, colors = np.concatenate([points, points[7:9]]), np.concatenate([colors, colors[7:9]])
    with pytest.raises(ValueError):
        C.encode(points, colors, 8, device='gpu', ctx=ctx)
    with pytest.raises(ValueError):
        C.coefficients(points, colors, 8, device='gpu', ctx=ctx)
    base = points[:-2]
    data = C.encode(base, colors[:-2], 8, device='host')
    twice, j = base.copy(), int(np.argmin(base.max(axis=1)))
    twice[j] = base[(j + 1) % len(base)]                           # N and D of the stream, one position twice
    assert int(twice.max()).bit_length() == int(base.max()).bit_length()
    with pytest.raises(ValueError, match='pairwise distinct'):
        C.decode(data, twice, device='gpu', ctx=ctx)


def test_ev_run_anchor_color_step(tmp_path):
    points = R.shell()
    colors = R.smooth_colors(points)
    os.makedirs(tmp_path / 'exp')
    os.makedirs(tmp_path / 'dataset')
    src = str(tmp_path / 'dataset' / 'shell.ply')
    pc_io.write_df(src, pc_io.pa_to_df(np.concatenate([points.astype(np.float64), colors], axis=1)))
    exp = {'EXPERIMENT_DIR': str(tmp_path / 'exp'), 'MPEG_DATASET_DIR': str(tmp_path / 'dataset'), 'anchor_device': 'gpu', 'metrics_device': 'gpu',
           'model_configs': [{'id': 'c4', 'config': 'c3p', 'lambdas': [3.0e-4], 'label': 'c4'}], 'opt_metrics': ['d1_mse'], 'bd_ignore': [],
           'mpeg_modes': [{'id': 'octree-anchor', 'label': 'octree anchor'}],
           'eval_modes': [{'id': 'main', 'no_legend': True, 'modes': [{'id': 'c4'}, {'id': 'octree-anchor'}]}],
           'anchor_rates': {'r01': [1, 2], 'r02': [1, 1]}, 'color_rates': {'r01': 32, 'r02': 4},
           'data': [{'pc_name': 'shell', 'input_pc': 'shell.ply', 'resolution': 64}]}
    yml = str(tmp_path / 'experiment.yml')
    with open(yml, 'w') as f:
        yaml.safe_dump(exp, f)
    plain = ['report.json', 'shell.ply.bin', 'shell.ply.bin.decoded.ply', 'shell.ply.bin.decoded.ply.color.ply']
    new = ['report_color.json', 'shell.ply.bin.color.bin', 'shell.ply.bin.decoded.ply.coded.color.ply']
    rate_dir = lambda rate: tmp_path / 'exp' / 'gpcc' / 'octree-anchor' / 'shell' / rate
    assert ev_run_anchor.main([yml]) == 0
    before = {}
    for rate in exp['anchor_rates']:
        assert sorted(os.listdir(rate_dir(rate))) == sorted(plain), rate                  # without --color: none of the three files
        before[rate] = {n: (rate_dir(rate) / n).read_bytes() for n in plain}
    assert ev_run_anchor.main([yml, '--color']) == 0
    for rate, q in exp['color_rates'].items():
        d = rate_dir(rate)
        assert sorted(os.listdir(d)) == sorted(plain + new), rate
        assert before[rate] == {n: (d / n).read_bytes() for n in plain}, rate             # what was there is untouched
        dec = str(d / 'shell.ply.bin.decoded.ply')
        pts, mapped = pc_io.load_pc(dec + '.color.ply'), pc_io.load_colors(dec + '.color.ply')
        stream = (d / 'shell.ply.bin.color.bin').read_bytes()
        assert stream == C.encode(pts, mapped, q, device='host')
        assert np.array_equal(pc_io.load_pc(dec + '.coded.color.ply'), pts)
        assert np.array_equal(pc_io.load_colors(dec + '.coded.color.ply'), C.reconstruct(pts, mapped, q))
        with open(d / 'report_color.json') as f:
            rep = json.load(f)
        with open(d / 'report.json') as f:
            geo = json.load(f)
        assert rep['color_total_size_in_bytes'] == len(stream) and rep['color_bits_per_input_point'] == len(stream) * 8 / len(points)
        assert rep['total_bits_per_input_point'] == (geo['pos_total_size_in_bytes'] + len(stream)) * 8 / len(points)
        want = ev_report.build_report(src, dec + '.coded.color.ply', str(d / 'shell.ply.bin'), 64, metrics_device='gpu', color=True)
        for k in ('y_mse', 'u_mse', 'v_mse', 'y_psnr', 'u_psnr', 'v_psnr'):
            assert rep[k] == want[k], (rate, k)
