"""CPU: the cloud-colour surface that needs no GPU -- C ABI symbols and argument refusals, the input checks of ops.map_colors /
ops.cloud_color_distortion that run before any GPU call, pc_io.load_colors, pc_metric.color_table and color_tally_host, the host-mode
`ev_report --color` report and the map_color CLI on an empty target."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import _color_ref as R
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ev_report, ops
from pcc_geo_cnn_v2_amd.utils import pc_io, pc_metric

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pcc_cloud_map_colors', 'pcc_cloud_color_workspace_bytes', 'pcc_cloud_color_distortion')
COLOR_KEYS = {'y_mse', 'u_mse', 'v_mse', 'y_psnr', 'u_psnr', 'v_psnr'}


def test_color_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'pcc_geo.h')).read()
    for name in NEW:
        assert re.search(rf'\b{name}\s*\(', hdr), name
        assert name in L.EXPORTS
        assert hasattr(C.CDLL(L.LIB_PATH), name)
    assert L.lib().pcc_abi_version() == 4


def test_sizes_and_ranks_outside_the_range_are_refused():
    lib = L.lib()
    ws = lib.pcc_cloud_color_workspace_bytes
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(1 << 31, 5) == 0 and ws(5, -1) == 0
    assert ws(1, 1) > 0 and ws(1000, 50) > ws(10, 50)
    # refused before the context is touched: a dummy non-NULL handle never gets dereferenced
    h, p = C.c_void_p(16), C.c_void_p(256)
    call = lambda n, nq, rank: lib.pcc_cloud_map_colors(h, p, n, p, p, nq, rank, p, None, None)
    assert call(0, 5, 1) == L.PCC_ERR_ARG and call(5, 0, 1) == L.PCC_ERR_ARG and call(1 << 31, 5, 1) == L.PCC_ERR_ARG
    assert call(5, 5, 0) == L.PCC_ERR_ARG and call(5, 5, 3) == L.PCC_ERR_ARG
    assert call(1, 5, 2) == L.PCC_ERR_ARG                                   # rank 2 needs two indexed points
    assert 'rank 2' in lib.pcc_last_error().decode()
    dist = lambda na, nb: lib.pcc_cloud_color_distortion(h, p, na, p, p, nb, p, p, p, None)
    assert dist(0, 5) == L.PCC_ERR_ARG and dist(5, 0) == L.PCC_ERR_ARG and dist(5, 1 << 31) == L.PCC_ERR_ARG
    assert lib.pcc_cloud_map_colors(None, p, 5, p, p, 5, 1, p, None, None) == L.PCC_ERR_ARG


class _NoGpu:
    """A context that fails on use: the input checks must raise before anything touches it."""
    def __getattr__(self, name):
        raise AssertionError(f'GPU context used ({name}) before the inputs were checked')


GOOD = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.int32)
GOOD_C = np.array([[1, 2, 3], [4, 5, 6], [250, 0, 9]], np.uint8)


@pytest.mark.parametrize('kw,what', [
    (dict(rank=3), 'rank'),
    (dict(rank=0), 'rank'),
    (dict(index_a=GOOD[:1], a_colors=GOOD_C[:1]), 'at least 2'),
    (dict(a_colors=GOOD_C[:2]), r'\(3, 3\)'),
    (dict(a_colors=GOOD_C.astype(np.float32)), 'integers in 0..255'),
    (dict(a_colors=GOOD_C.astype(np.int16) + 200), 'integers in 0..255'),
    (dict(a_colors=GOOD_C.astype(np.int32) - 10), 'integers in 0..255'),
    (dict(index_a=np.array([[0.5, 1, 2], [1, 1, 1], [2, 2, 2]])), 'integers'),
    (dict(queries=np.array([[-1, 0, 0]])), r'\[0, 2097152\)'),
    (dict(queries=np.array([[0, 0, 1 << 21]])), r'\[0, 2097152\)'),
    (dict(queries=np.zeros((2, 2), np.int32)), r'\(N, 3\)'),
])
def test_map_colors_checks_its_inputs_before_any_gpu_call(kw, what):
    args = dict(index_a=GOOD, a_colors=GOOD_C, queries=GOOD, rank=2)
    args.update(kw)
    with pytest.raises(L.PccError, match=what):
        ops.map_colors(_NoGpu(), args['index_a'], args['a_colors'], args['queries'], rank=args['rank'])


def test_map_colors_of_no_queries_is_empty_and_needs_no_gpu():
    out = ops.map_colors(_NoGpu(), GOOD, GOOD_C, np.zeros((0, 3), np.int32))
    assert out.shape == (0, 3) and out.dtype == np.uint8
    out, rows = ops.map_colors(_NoGpu(), GOOD, GOOD_C, np.zeros((0, 3)), rank=1, return_rows=True)
    assert out.shape == (0, 3) and rows.shape == (0,) and rows.dtype == np.int32


@pytest.mark.parametrize('kw,what', [
    (dict(a_colors=GOOD_C[:2]), r'\(3, 3\)'),
    (dict(b_colors=GOOD_C[:2]), r'\(3, 3\)'),
    (dict(b_colors=GOOD_C.astype(np.float64)), 'integers in 0..255'),
    (dict(b_colors=GOOD_C.astype(np.int32) * 2), 'integers in 0..255'),
    (dict(index_a=np.zeros((0, 3), np.int32), a_colors=np.zeros((0, 3), np.uint8)), r'\(N, 3\)'),
    (dict(b_points=np.zeros((0, 3), np.int32), b_colors=np.zeros((0, 3), np.uint8)), r'\(N, 3\)'),
    (dict(b_points=GOOD + (1 << 21)), r'\[0, 2097152\)'),
    (dict(b_points=GOOD + 0.25), 'integers'),
])
def test_color_distortion_checks_its_inputs_before_any_gpu_call(kw, what):
    args = dict(index_a=GOOD, a_colors=GOOD_C, b_points=GOOD, b_colors=GOOD_C)
    args.update(kw)
    with pytest.raises(L.PccError, match=what):
        ops.cloud_color_distortion(_NoGpu(), args['index_a'], args['a_colors'], args['b_points'], args['b_colors'])


def _cloud_df(pts, colors=None, xyz_dtype=np.float32):
    d = {c: pts[:, k].astype(xyz_dtype) for k, c in enumerate('xyz')}
    if colors is not None:
        d.update({c: np.asarray(colors)[:, k] for k, c in enumerate(('red', 'green', 'blue'))})
    return pd.DataFrame(d)


@pytest.mark.parametrize('as_text', [False, True])
def test_load_colors_round_trip(tmp_path, as_text):
    pts = np.arange(30).reshape(10, 3)
    col = R.random_colors(10, 0)
    col[0] = (0, 255, 7)
    path = str(tmp_path / 'c.ply')
    pc_io.write_ply(path, _cloud_df(pts, col), as_text=as_text)
    header = open(path, 'rb').read().split(b'end_header')[0].decode()
    for c in ('red', 'green', 'blue'):
        assert f'property uchar {c}' in header                            # uint8 columns are written as uchar
    got = pc_io.load_colors(path)
    assert got.dtype == np.uint8 and np.array_equal(got, col)
    assert np.array_equal(pc_io.load_pc(path), pts)                       # the geometry reader ignores the colour columns


def test_load_colors_refuses_files_without_valid_colours(tmp_path):
    pts = np.arange(12).reshape(4, 3)
    plain = str(tmp_path / 'plain.ply')
    pc_io.write_pc(plain, pts.astype(np.float32))
    with pytest.raises(ValueError, match=re.escape(plain) + '.*no colour'):
        pc_io.load_colors(plain)
    wide = str(tmp_path / 'wide.ply')
    pc_io.write_ply(wide, _cloud_df(pts, np.array([[0, 0, 0], [1, 2, 3], [300, 0, 0], [4, 5, 6]], np.int16)))
    with pytest.raises(ValueError, match=re.escape(wide) + '.*0..255'):
        pc_io.load_colors(wide)
    frac = str(tmp_path / 'frac.ply')
    pc_io.write_ply(frac, _cloud_df(pts, np.full((4, 3), 0.5, np.float32)))
    with pytest.raises(ValueError, match=re.escape(frac)):
        pc_io.load_colors(frac)


def test_color_table_on_hand_computed_tallies():
    t = np.array([40.0, 20.0, 0.0, 30.0, 50.0, 0.0])
    m = pc_metric.color_table(t, 4, 5)
    assert set(m) == COLOR_KEYS
    assert (m['y_mse'], m['u_mse'], m['v_mse']) == (10.0, 10.0, 0.0)      # max(40/4, 30/5), max(20/4, 50/5), identical
    assert m['y_psnr'] == 10 * np.log10(255 ** 2 / 10.0) and m['u_psnr'] == m['y_psnr']
    assert m['v_psnr'] == np.inf
    arr = pc_metric.color_table(np.stack([t, 2 * t]), 4, 5)
    assert np.array_equal(arr['u_mse'], [10.0, 20.0])


def test_host_tally_matches_the_restatement_and_ignores_row_order():
    pairs = R.color_pairs(with_shell=False)
    for name, (a, ca, b, cb) in pairs.items():
        host = pc_metric.color_tally_host(a.astype(np.float64), ca, b.astype(np.float64), cb)
        ref = R.tally_ref(a, ca, b, cb)
        assert np.all(np.abs(host - ref) <= 1e-12 * np.abs(ref)), (name, host, ref)
        p = np.random.default_rng(1).permutation(len(b))
        perm = pc_metric.color_tally_host(a.astype(np.float64), ca, b[p].astype(np.float64), cb[p])
        assert np.all(np.abs(perm - host) <= 1e-12 * np.abs(host)), name
    a, ca, _, _ = pairs['uniform']
    assert np.array_equal(pc_metric.color_tally_host(a, ca, a, ca), np.zeros(6))


def _write_pair(tmp_path, with_b_colors=True):
    rng = np.random.default_rng(3)
    a = np.unique(rng.integers(0, 64, (600, 3)), axis=0)
    b = a[rng.random(len(a)) < 0.8].copy()
    b[::5, 0] = np.clip(b[::5, 0] + 1, 0, 63)
    b = np.unique(b, axis=0)
    ca, cb = R.random_colors(len(a), 5), R.random_colors(len(b), 6)
    pc_io.write_ply(str(tmp_path / 'a.ply'), _cloud_df(a, ca))
    pc_io.write_ply(str(tmp_path / 'b.ply'), _cloud_df(b, cb if with_b_colors else None))
    open(tmp_path / 'a.bin', 'wb').write(b'\x00' * 300)
    return a, ca, b, cb


def test_host_report_with_color(tmp_path):
    a, ca, b, cb = _write_pair(tmp_path)
    paths = [str(tmp_path / f) for f in ('a.ply', 'b.ply', 'a.bin')]
    plain = ev_report.build_report(*paths, 64)
    assert set(plain) == {'pos_total_size_in_bytes', 'pos_bits_per_input_point', 'input_point_count', 'd1_mse', 'd1_psnr'}
    r = ev_report.build_report(*paths, 64, color=True)
    assert {k: r[k] for k in plain} == plain
    assert set(r) - set(plain) == COLOR_KEYS
    ref = pc_metric.color_table(R.tally_ref(a, ca, b, cb), len(a), len(b))
    for k in COLOR_KEYS:
        assert abs(r[k] - ref[k]) <= 1e-12 * abs(ref[k]), (k, r[k], ref[k])
    out = tmp_path / 'r.json'
    cmd = [sys.executable, '-m', 'pcc_geo_cnn_v2_amd.ev_report', '--input_pc', paths[0], '--decoded_pc', paths[1], '--enc_pc', paths[2],
           '--resolution', '64', '--output', str(out)]
    subprocess.run(cmd + ['--color'], check=True, cwd=ROOT)
    assert json.load(open(out)) == r
    subprocess.run(cmd, check=True, cwd=ROOT)                            # without --color: the report of before
    assert json.load(open(out)) == plain


def test_report_refuses_a_decoded_cloud_without_colour(tmp_path):
    _write_pair(tmp_path, with_b_colors=False)
    paths = [str(tmp_path / f) for f in ('a.ply', 'b.ply', 'a.bin')]
    with pytest.raises(ValueError, match='map_color'):
        ev_report.build_report(*paths, 64, color=True)
    ev_report.build_report(*paths, 64)                                    # fine without --color
    bad = subprocess.run([sys.executable, '-m', 'pcc_geo_cnn_v2_amd.ev_report', '--input_pc', paths[0], '--decoded_pc', paths[1],
                          '--enc_pc', paths[2], '--resolution', '64', '--color', '--output', str(tmp_path / 'r.json')],
                         cwd=ROOT, capture_output=True, text=True)
    assert bad.returncode != 0 and 'map_color' in bad.stderr and 'b.ply' in bad.stderr


def test_map_color_cli_on_an_empty_target_writes_a_header_only_file(tmp_path):
    _write_pair(tmp_path)
    empty = pd.DataFrame({'x': np.zeros(0, np.int32), 'y': np.zeros(0, np.int32), 'z': np.zeros(0, np.int32)})
    pc_io.write_ply(str(tmp_path / 'e.ply'), empty)
    out = tmp_path / 'o.ply'
    subprocess.run([sys.executable, '-m', 'pcc_geo_cnn_v2_amd.map_color', str(tmp_path / 'a.ply'), str(tmp_path / 'e.ply'), str(out)],
                   check=True, cwd=ROOT)
    data = open(out, 'rb').read()
    assert data.endswith(b'end_header\n')
    assert b'element vertex 0' in data and b'property int x' in data and b'property uchar blue' in data
    df = pc_io.read_ply(str(out))
    assert list(df.columns) == ['x', 'y', 'z', 'red', 'green', 'blue'] and len(df) == 0
    bad = subprocess.run([sys.executable, '-m', 'pcc_geo_cnn_v2_amd.map_color', str(tmp_path / 'a.ply'), str(tmp_path / 'e.ply'), str(out),
                          '--rank', '3'], cwd=ROOT, capture_output=True)
    assert bad.returncode != 0
