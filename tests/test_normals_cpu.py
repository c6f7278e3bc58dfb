"""CPU: the point-normal surface that needs no GPU -- C ABI symbols, the command-line contract of --estimate_normals, the input
checks that run before any GPU call, and the `_n.ply` layout the estimate_normals tool writes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import compress_octree, ops
from pcc_geo_cnn_v2_amd.estimate_normals import normals_frame
from pcc_geo_cnn_v2_amd.utils import pc_io, pc_metric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_normals_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'pcc_geo.h')).read()
    for name in ('pcc_normals_workspace_bytes', 'pcc_estimate_normals'):
        assert re.search(rf'\b{name}\s*\(', hdr), name
        assert name in L.EXPORTS
        assert hasattr(C.CDLL(L.LIB_PATH), name)
    assert L.lib().pcc_abi_version() == 4
    assert pc_metric.estimate_normals is not None


def _args(**kw):
    a = compress_octree.build_parser().parse_args(['--input_files', 'a.ply', '--output_files', 'a1.bin', 'a2.bin', '--checkpoint_dir', 'ck',
                                                   '--model_config', 'c3p', '--opt_metrics', 'd1_mse', 'd2_mse'] + kw.pop('extra', []))
    return a


def test_plan_accepts_estimate_normals_with_d2_metrics():
    clouds, with_normals = compress_octree._plan(_args(extra=['--estimate_normals']))
    assert with_normals and len(clouds) == 1 and clouds[0].targets == ['a1.bin', 'a2.bin']
    a = _args(extra=['--estimate_normals', '--normals_k', '24'])
    assert a.normals_k == 24


def test_plan_rejects_estimate_normals_with_input_normals():
    with pytest.raises(AssertionError, match='mutually exclusive'):
        compress_octree._plan(_args(extra=['--estimate_normals', '--input_normals', 'a_n.ply']))


def test_plan_without_normals_still_rejects_d2():
    with pytest.raises(AssertionError, match='not available without normals'):
        compress_octree._plan(_args())


@pytest.mark.parametrize('pts,what', [
    (np.array([[0.5, 1, 2]], np.float32), 'integers'),
    (np.array([[0, 1, np.nan]], np.float64), 'integers'),
    (np.array([[-1, 0, 0]], np.int32), r'\[0, 2097152\)'),
    (np.array([[0, 0, 1 << 21]], np.int64), r'\[0, 2097152\)'),
    (np.array([[0, 0, 2097152.0]], np.float64), r'\[0, 2097152\)'),
    (np.zeros((0, 3), np.int32), r'\(N, 3\)'),
    (np.zeros((4, 2), np.int32), r'\(N, 3\)'),
])
def test_bad_coordinates_raise_before_any_gpu_call(pts, what):
    # ctx=None: the checks must fire before the context is touched
    with pytest.raises(L.PccError, match=what):
        ops.estimate_normals(None, pts)


@pytest.mark.parametrize('k', [2, 65])
def test_k_outside_range_raises(k):
    with pytest.raises(L.PccError, match='outside'):
        ops.estimate_normals(None, np.zeros((4, 3), np.int32), k=k)


def test_bad_viewpoint_raises():
    with pytest.raises(L.PccError, match='viewpoint'):
        ops.estimate_normals(None, np.zeros((4, 3), np.int32), viewpoint=(1, 2))


def test_voxel_points_accepts_integral_floats_and_edges():
    a = ops._voxel_points(np.array([[0.0, 2097151.0, 5.0]], np.float32))
    assert a.dtype == np.int32 and a.tolist() == [[0, 2097151, 5]]


def test_normals_ply_reads_back_through_load_normals(tmp_path):
    rng = np.random.default_rng(0)
    pts = rng.integers(0, 1024, (50, 3)).astype(np.float32)
    nrm = rng.standard_normal((50, 3)).astype(np.float32)
    path = str(tmp_path / 'a_n.ply')
    pc_io.write_df(path, normals_frame(pts, nrm))
    df = pc_io.read_ply(path)
    assert list(df.columns) == ['x', 'y', 'z', 'nx', 'ny', 'nz']
    assert all(df[c].dtype == np.float32 for c in df.columns)
    assert np.array_equal(pc_io.load_normals(path), nrm)
    assert np.array_equal(pc_io.load_pc(path), pts)


def test_ev_report_rejects_both_normal_sources(tmp_path):
    from pcc_geo_cnn_v2_amd.ev_report import build_report
    with pytest.raises(AssertionError, match='mutually exclusive'):
        build_report('a.ply', 'b.ply', 'c.bin', 64, input_norm='a_n.ply', estimate_normals=True)
