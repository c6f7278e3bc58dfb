"""The colour anchor codec without a GPU: the numpy host path and the C++ coefficient coder against the restatement
in tests/_color_anchor_ref.py, the round trips, the stream checks, the size conditions, the ABI and the CLI."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import _color_anchor_ref as R
from pcc_geo_cnn_v2_amd import _lib, ops
from pcc_geo_cnn_v2_amd import anchor_color as C
from pcc_geo_cnn_v2_amd.anchor_octree import AnchorStreamError
from pcc_geo_cnn_v2_amd.utils import pc_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (1, 2, 16, 255)
SMALL = R.small_cases()
SHELL = R.shell()
SHELL_COLORS = {'smooth': R.smooth_colors(SHELL), 'random': R.random_colors(len(SHELL)), 'alternating': R.alternating_colors(SHELL)}
CASES = {**SMALL, **{f'shell_{k}': (SHELL, v) for k, v in SHELL_COLORS.items()}}
FMT = struct.Struct('<4sBBBI3h')
NEW_EXPORTS = ('pcc_color_anchor_workspace_bytes', 'pcc_color_anchor_plan', 'pcc_color_anchor_forward', 'pcc_color_anchor_inverse',
               'pcc_color_anchor_encode', 'pcc_color_anchor_decode')


def luma(c):
    c = c.astype(np.int64)
    co = c[:, 0] - c[:, 2]
    t = c[:, 2] + (co >> 1)
    return t + ((c[:, 1] - t) >> 1)


def psnr_y(a, b):
    return 10 * np.log10(255.0 ** 2 / max(np.mean((luma(a) - luma(b)) ** 2.0), 1e-12))


def test_the_cases_are_what_they_claim():
    assert FMT.size == 17 and 4500 <= len(SHELL) <= 5500 and len(np.unique(SHELL, axis=0)) == len(SHELL)
    assert [len(SMALL[k][0]) for k in ('n1', 'n2', 'n3', 'cell2')] == [1, 2, 3, 8]
    assert SMALL['depth1'][0].max() == 1 and SMALL['top'][0].max() == (1 << 21) - 1


@pytest.mark.parametrize('q', QS)
@pytest.mark.parametrize('name', sorted(CASES))
def test_host_path_gives_the_restatement_bytes_and_arrays(name, q):
    points, colors = CASES[name]
    data = C.encode(points, colors, q, device='host')
    assert data == R.encode(points, colors, q)
    dec = C.decode(data, points, device='host')
    assert dec.dtype == np.uint8 and dec.shape == colors.shape
    assert np.array_equal(dec, R.decode(data, points))
    assert np.array_equal(dec, C.reconstruct(points, colors, q))
    if q == 1:
        assert np.array_equal(dec, colors)
    counts, dc, coef = C.coefficients(points, colors, q, device='host')
    rcounts, rdc, rcoef = R.coefficients(points, colors, q)
    n = len(points)
    assert coef.shape == (n - 1, 3) and coef.dtype == np.int16 and int(counts.sum()) == n - 1 and counts.shape == (64,)
    assert counts.tolist() == rcounts and list(dc) == list(rdc) and [tuple(r) for r in coef.tolist()] == rcoef
    assert np.abs(coef).max(initial=0) <= 510
    h = C.read_header(data)
    assert (h['qstep'], h['points'], h['dc']) == (q, n, tuple(rdc))


@pytest.mark.parametrize('q', (1, 16))
def test_rows_follow_the_callers_points(q):
    colors = SHELL_COLORS['random']
    perm = np.random.default_rng(1).permutation(len(SHELL))
    data = C.encode(SHELL, colors, q, device='host')
    assert C.encode(SHELL[perm], colors[perm], q, device='host') == data            # the stream does not depend on the row order
    assert np.array_equal(C.decode(data, SHELL[perm], device='host'), C.decode(data, SHELL, device='host')[perm])
    assert np.array_equal(C.reconstruct(SHELL[perm], colors[perm], q), C.reconstruct(SHELL, colors, q)[perm])


def test_the_coder_pair_agrees_with_the_restatement():
    rng = np.random.default_rng(2)
    counts = np.zeros(63, np.int64)
    counts[[0, 1, 2, 5, 20, 21, 40, 62]] = [700, 300, 150, 60, 30, 7, 2, 1]
    n = int(counts.sum())
    coef = np.zeros((n, 3), np.int16)
    coef[:40] = rng.choice([0, 1, -1, 510, -510], (40, 3))
    coef[300:500] = rng.integers(-510, 511, (200, 3))
    coef[900:1000, 0] = rng.choice([0, 0, 0, 1, -1, 2, 255, 256, -256], 100)           # zero runs around and inside
    coef[-1] = (510, -510, 0)
    steps = [s for s in range(62, -1, -1) for _ in range(counts[s])]
    want = R.code_coefficients([(s, tuple(int(v) for v in c)) for s, c in zip(steps, coef)])
    data = ops.color_anchor_encode_coefficients(coef, counts)
    assert data == want
    back, used = ops.color_anchor_decode_coefficients(data, counts, n)
    assert used == len(data) and np.array_equal(back, coef)
    rback, rused = R.decode_coefficients(data, steps)
    assert rused == len(data) and rback == [tuple(r) for r in coef.tolist()]
    with pytest.raises(AssertionError):
        ops.color_anchor_encode_coefficients(np.full((n, 3), 512, np.int16), counts)
    with pytest.raises(AssertionError):
        ops.color_anchor_encode_coefficients(coef[:-1], counts)                           # the counts do not sum to the coefficients


def _ninth_one_payload(top_step):
    """A payload whose first coefficient has nine one-bits in its prefix, from the restatement's encoder."""
    e = R.RefEncoder()
    m = 32 * R.group(top_step, 0)
    e.encode(m, 1)
    e.encode(m + 2, 0)
    for j in range(9):
        e.encode(m + 3 + j, 1)
    for _ in range(40):
        e.encode(m, 0)
    return e.finish()


def test_damaged_streams_raise():
    points, colors = SMALL['line_x']
    data = C.encode(points, colors, 4, device='host')
    magic, version, q, depth, n, *dc = FMT.unpack_from(data)
    payload = data[17:]
    pack = lambda **kw: FMT.pack(*[kw.get(k, v) for k, v in (('magic', magic), ('version', version), ('q', q), ('depth', depth), ('n', n))],
                                 *kw.get('dc', dc)) + payload
    assert pack() == data
    bad = {
        'magic': pack(magic=b'PCOA'), 'version': pack(version=2), 'q0': pack(q=0), 'depth': pack(depth=depth + 1), 'n': pack(n=n + 1),
        'dc_y_low': pack(dc=(-1, 0, 0)), 'dc_y_high': pack(dc=(256, 0, 0)), 'dc_co': pack(dc=(0, 256, 0)), 'dc_cg': pack(dc=(0, 0, -256)),
        'short_header': data[:16], 'no_payload': data[:17], 'cut': data[:-1], 'cut_more': data[:20], 'left_over': data + b'\0',
        'first_byte': data[:17] + b'\1' + data[18:],
        'ninth_one': data[:17] + _ninth_one_payload(max(s for s, c in enumerate(R.coefficients(points, colors, 4)[0]) if c)),
    }
    for name, d in bad.items():
        with pytest.raises(AnchorStreamError):
            C.decode(d, points, device='host')
        assert name
    with pytest.raises(AnchorStreamError):
        C.decode(data, points[:-1], device='host')                 # another N
    with pytest.raises(AnchorStreamError):
        C.decode(data, points * 4, device='host')                  # another D
    assert np.array_equal(C.decode(data, points, device='host'), C.reconstruct(points, colors, 4))


def test_bad_arguments_raise():
    points, colors = SMALL['n3']
    for pts, col, q in ((np.concatenate([points, points[:1]]), np.concatenate([colors, colors[:1]]), 4),      # duplicate positions
                        (points, colors.astype(np.int32), 4), (points, colors.astype(np.float32), 4), (points, colors[:2], 4),
                        (points, colors, 0), (points, colors, 256), (points, colors, 2.5), (points, colors, -1),
                        (points - 1, colors, 4), (points + (1 << 21), colors, 4)):
        with pytest.raises(ValueError):
            C.encode(pts, col, q, device='host')
    with pytest.raises(ValueError):
        C.reconstruct(np.concatenate([points, points[:1]]), np.concatenate([colors, colors[:1]]), 4)
    with pytest.raises(ValueError):
        C.encode(points, colors, 4, device='cpu')
    data = C.encode(points, colors, 4, device='host')
    with pytest.raises(ValueError):
        C.decode(FMT.pack(b'PCCA', 1, 4, 3, 4, 0, 0, 0) + data[17:], np.concatenate([points, points[:1]]), device='host')


def test_size_conditions_on_the_smooth_field():
    """Measured with the host path before they were fixed here: 7.13 bits per point lossless; 6.11, 0.94, 0.18 bits per point and
    a falling luma PSNR at Q = 2, 16, 255."""
    colors = SHELL_COLORS['smooth']
    assert 8 * len(C.encode(SHELL, colors, 1, device='host')) / len(SHELL) < 24
    sizes = [len(C.encode(SHELL, colors, q, device='host')) for q in (2, 16, 255)]
    assert sizes[0] >= sizes[1] >= sizes[2]
    psnr = [psnr_y(colors, C.reconstruct(SHELL, colors, q)) for q in (2, 16, 255)]
    assert psnr[0] >= psnr[1] >= psnr[2]


def test_the_abi_declares_and_exports_the_new_symbols():
    with open(os.path.join(ROOT, 'include', 'pcc_geo.h')) as f:
        header = f.read()
    lib = _lib.lib()
    for name in NEW_EXPORTS:
        assert re.search(r'\b' + name + r'\(', header), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert re.search(r'#define PCC_COLOR_HDR_WORDS\s+%d\b' % _lib.PCC_COLOR_HDR_WORDS, header)
    assert _lib.ABI_VERSION == 4 and lib.pcc_abi_version() == 4


def test_cli_round_trips_through_files(tmp_path):
    points, colors = SHELL[:600], SHELL_COLORS['smooth'][:600]
    src, geo, enc, out = (str(tmp_path / n) for n in ('in.ply', 'geo.ply', 'out.bin', 'out.ply'))
    pc_io.write_df(src, pc_io.pa_to_df(np.concatenate([points.astype(np.float64), colors], axis=1)))
    perm = np.random.default_rng(4).permutation(len(points))
    pc_io.write_df(geo, pc_io.pa_to_df(points[perm]))
    run = lambda *a: subprocess.run([sys.executable, '-m', 'pcc_geo_cnn_v2_amd.anchor_color', *a, '--device', 'host'], cwd=ROOT, capture_output=True,
                                    text=True, timeout=300)
    r = run('encode', src, enc, '--qstep', '8')
    assert r.returncode == 0, r.stderr
    with open(enc, 'rb') as f:
        assert f.read() == C.encode(points, colors, 8, device='host')
    r = run('decode', enc, geo, out)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pc_io.load_pc(out), points[perm])
    assert np.array_equal(pc_io.load_colors(out), C.reconstruct(points, colors, 8)[perm])
