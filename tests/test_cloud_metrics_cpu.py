"""CPU: the cloud-metric surface that needs no GPU -- C ABI symbols, the --metrics_device / --hausdorff command-line contract,
the input checks that run before any GPU call, hausdorff_table on hand-computed tallies and the host-mode --hausdorff report."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import compress_octree, ev_report, model_types, ops
from pcc_geo_cnn_v2_amd.utils import pc_io, pc_metric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pcc_cloud_index_bytes', 'pcc_cloud_index_build', 'pcc_cloud_nearest', 'pcc_cloud_distortion_workspace_bytes', 'pcc_cloud_distortion')


def test_cloud_metric_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'pcc_geo.h')).read()
    for name in NEW:
        assert re.search(rf'\b{name}\s*\(', hdr), name
        assert name in L.EXPORTS
        assert hasattr(C.CDLL(L.LIB_PATH), name)
    assert L.lib().pcc_abi_version() == 4


def test_size_functions_refuse_sizes_outside_the_range():
    lib = L.lib()
    assert lib.pcc_cloud_index_bytes(0) == 0 and lib.pcc_cloud_index_bytes(1 << 31) == 0
    assert lib.pcc_cloud_index_bytes(1) > 0 and lib.pcc_cloud_index_bytes(1000) > lib.pcc_cloud_index_bytes(10)
    assert lib.pcc_cloud_distortion_workspace_bytes(0, 5) == 0 and lib.pcc_cloud_distortion_workspace_bytes(5, 0) == 0
    assert lib.pcc_cloud_distortion_workspace_bytes(100, 50) > 0


def _args(*extra):
    return compress_octree.build_parser().parse_args(['--input_files', 'a.ply', '--output_files', 'a.bin', '--checkpoint_dir', 'ck',
                                                      '--model_config', 'c3p', '--opt_metrics', 'd1_mse', *extra])


def test_compress_octree_metrics_device_flag():
    assert _args().metrics_device == 'host'
    assert _args('--metrics_device', 'gpu').metrics_device == 'gpu'
    with pytest.raises(SystemExit):
        _args('--metrics_device', 'cpu')
    compress_octree.check_encode_options(_args('--metrics_device', 'gpu'), 1)
    compress_octree.check_encode_options(_args(), 4)
    with pytest.raises(AssertionError, match='single-process only'):
        compress_octree.check_encode_options(_args('--metrics_device', 'gpu'), 2)


def test_compress_blocks_refuses_gpu_metrics_under_a_sharded_run(monkeypatch):
    from pcc_geo_cnn_v2_amd import sharding
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    monkeypatch.setattr(sharding, 'world_info', lambda: (0, 2))
    model = ModelConfigType['c3p'].build()
    with pytest.raises(AssertionError, match='single-process only'):
        model.compress_blocks(None, [], [], np.zeros((0, 3)), 64, 1, metrics_device='gpu')
    with pytest.raises(AssertionError, match='metrics_device'):
        model_types.select_best_per_opt_metric([], [], 1, [], np.zeros((0, 3)), 64, False, metrics_device='cuda')


def test_metric_json_gains_the_device_only_in_gpu_mode(tmp_path):
    info = {'metrics': {'d1_mse': np.float64(0.5), 'd1_psnr': np.float64(60.0)}, 'numerics_tag': 'tag', 'blocks_full': None}
    for dev in ('host', 'gpu'):
        a = _args('--metrics_device', dev)
        target = str(tmp_path / dev / 'a.bin')
        compress_octree._write_rate_point(target, None, [1, 0, 0, 0, 0, 0, 0, 0], [([b'ab', b'c'], 7)], info, a, [], [])
        rec = json.load(open(target + '.enc.metric.json'))
        assert rec == dict({'d1_mse': 0.5, 'd1_psnr': 60.0, 'codec_numerics': 'tag'}, **({'metrics_device': 'gpu'} if dev == 'gpu' else {}))


class _NoGpu:
    """A context that fails on use: the input checks must raise before anything touches it."""
    def __getattr__(self, name):
        raise AssertionError(f'GPU context used ({name}) before the inputs were checked')


@pytest.mark.parametrize('pts,what', [
    (np.array([[0.5, 1, 2]], np.float32), 'integers'),
    (np.array([[0, 1, np.inf]], np.float64), 'integers'),
    (np.array([[-1, 0, 0]], np.int32), r'\[0, 2097152\)'),
    (np.array([[0, 0, 1 << 21]], np.int64), r'\[0, 2097152\)'),
    (np.zeros((0, 3), np.int32), r'\(N, 3\)'),
    (np.zeros((4, 2), np.int32), r'\(N, 3\)'),
    (np.array([['a', 'b', 'c']]), 'dtype'),
])
def test_bad_coordinates_raise_before_any_gpu_call(pts, what):
    good = np.array([[1, 2, 3], [4, 5, 6]], np.int32)
    with pytest.raises(L.PccError, match=what):
        ops.CloudIndex(_NoGpu(), pts)
    with pytest.raises(L.PccError, match=what):
        ops.cloud_distortion(_NoGpu(), pts, good)
    with pytest.raises(L.PccError, match=what):
        ops.cloud_distortion(_NoGpu(), good, pts)
    if len(pts):
        with pytest.raises(L.PccError, match=what):
            ops.cloud_nearest(_NoGpu(), None, pts)


def test_bad_normals_raise_before_any_gpu_call():
    good = np.array([[1, 2, 3], [4, 5, 6]], np.int32)
    with pytest.raises(L.PccError, match=r'\(2, 3\)'):
        ops.cloud_distortion(_NoGpu(), good, good, a_normals=np.zeros((3, 3), np.float32))
    with pytest.raises(L.PccError, match='floating point'):
        ops.cloud_distortion(_NoGpu(), good, good, a_normals=np.zeros((2, 3), np.int32))


def test_hausdorff_table_on_hand_computed_tallies():
    t = np.array([5, 10, 12, 3, 4, 9, 4, 2.25, 0.5])
    h = pc_metric.hausdorff_table(t, 63)
    assert set(h) == {'d1_hausdorff_AB', 'd1_hausdorff_BA', 'd1_hausdorff', 'd1_hausdorff_psnr'}
    assert (h['d1_hausdorff_AB'], h['d1_hausdorff_BA'], h['d1_hausdorff']) == (9, 4, 9)
    assert h['d1_hausdorff_psnr'] == 10 * np.log10(3 * 63 * 63 / 9)
    h2 = pc_metric.hausdorff_table(t, 1023, with_normals=True)
    assert (h2['d2_hausdorff_AB'], h2['d2_hausdorff_BA'], h2['d2_hausdorff']) == (2.25, 0.5, 2.25)
    assert h2['d2_hausdorff_psnr'] == 10 * np.log10(3 * 1023 * 1023 / 2.25)
    assert h2['d1_hausdorff_psnr'] == 10 * np.log10(3 * 1023 * 1023 / 9)
    zero = pc_metric.hausdorff_table(np.zeros(9), 63)                     # identical clouds: infinite PSNR, like psnr()
    assert zero['d1_hausdorff'] == 0 and zero['d1_hausdorff_psnr'] == np.inf
    arr = pc_metric.hausdorff_table(np.stack([t, t * 2]), 63)
    assert np.array_equal(arr['d1_hausdorff'], [9, 18])


def test_host_tally_restates_the_hausdorff_terms():
    a = np.array([[0, 0, 0], [10, 0, 0], [0, 5, 0]], np.float64)
    b = np.array([[0, 0, 1], [10, 0, 3]], np.float64)
    n = np.array([[0, 0, 1], [1, 0, 0], [0, 0, 1]], np.float64)
    t = pc_metric.cloud_tally_host(a, b, n)
    # A->B: 1, 9, 26 (point (0,5,0) to (0,0,1)); B->A: 1, 9
    assert list(t[:3]) == [2, 36, 10] and (t[5], t[6]) == (26, 9)
    # decoded normals: b0 <- mean(n0, n2) = (0,0,1), b1 <- n1 = (1,0,0); plane terms A->B: 1, 0, 1; B->A: 1, 0
    assert (t[3], t[4], t[7], t[8]) == (2, 1, 1, 1)
    m = pc_metric.compute_metrics(a, b, 63, p1_n=n)
    assert (m['d1_sum_AB'], m['d1_sum_BA'], m['d2_sum_AB'], m['d2_sum_BA']) == (36, 10, 2, 1)


def test_host_report_with_hausdorff(tmp_path):
    rng = np.random.default_rng(0)
    a = np.unique(rng.integers(0, 64, (500, 3)), axis=0).astype(np.float32)
    b = a.copy()
    b[::7, 0] = np.clip(b[::7, 0] + 1, 0, 63)
    b[::50, 1] = np.clip(b[::50, 1] + 3, 0, 63)
    b = np.unique(b, axis=0)
    pc_io.write_pc(str(tmp_path / 'a.ply'), a)
    pc_io.write_pc(str(tmp_path / 'b.ply'), b)
    open(tmp_path / 'a.bin', 'wb').write(b'\x00' * 250)
    plain = ev_report.build_report(str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply'), str(tmp_path / 'a.bin'), 64)
    r = ev_report.build_report(str(tmp_path / 'a.ply'), str(tmp_path / 'b.ply'), str(tmp_path / 'a.bin'), 64, hausdorff=True)
    assert {k: r[k] for k in plain} == plain
    assert set(r) - set(plain) == {'d1_hausdorff_AB', 'd1_hausdorff_BA', 'd1_hausdorff', 'd1_hausdorff_psnr'}
    A, B = a.astype(np.int64), b.astype(np.int64)
    d = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)                     # brute force
    assert r['d1_hausdorff_AB'] == d.min(1).max() and r['d1_hausdorff_BA'] == d.min(0).max()
    assert r['d1_hausdorff'] == max(d.min(1).max(), d.min(0).max())
    assert r['d1_hausdorff_psnr'] == 10 * np.log10(3 * 63 * 63 / r['d1_hausdorff'])
    out = tmp_path / 'r.json'
    cmd = [sys.executable, '-m', 'pcc_geo_cnn_v2_amd.ev_report', '--input_pc', str(tmp_path / 'a.ply'), '--decoded_pc', str(tmp_path / 'b.ply'),
           '--enc_pc', str(tmp_path / 'a.bin'), '--resolution', '64', '--hausdorff', '--output', str(out)]
    subprocess.run(cmd, check=True, cwd=ROOT)
    assert json.load(open(out)) == r
    bad = subprocess.run(cmd[:-2] + ['--metrics_device', 'tpu', '--output', str(out)], cwd=ROOT, capture_output=True)
    assert bad.returncode != 0
