"""CPU: the mesh sampling definition (utils/mesh_sampling.py, include/pcc_geo.h "mesh sampling") against numpy's Philox stream, a
plain-Python restatement and the reference's voxel lines; its statistics; the mesh readers (utils/mesh_io.py); and the ds_* CLIs
end to end on the host path."""
import bisect
import os
import struct
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
from scipy.stats import chisquare

import _mesh_ref as R
from pcc_geo_cnn_v2_amd import ds_mesh_to_pc
from pcc_geo_cnn_v2_amd.utils import mesh_io, mesh_sampling as MS, pc_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- definition -----------------------------------------------------------------------------------------------------------------

def test_philox_known_answer():
    ref = [0x16554d9eca36314c, 0xdb20fe9d672d0fdc, 0xd7e772cee186176b, 0x7e68b68aec7ba23b]
    assert [int(x) for x in MS.philox_rows(0, 0, 1)[0]] == ref
    assert R.philox4x64_10([0, 0, 0, 0], [0, 0]) == ref


@pytest.mark.parametrize('seed', [0, 1, 12345, 2 ** 64 - 1])
def test_raw_bits_are_numpys_philox_stream(seed):
    n = 3000
    rows = MS.philox_rows(seed, 0, n)
    assert np.array_equal(rows, np.random.Philox(key=seed, counter=2 ** 256 - 1).random_raw(4 * n).reshape(n, 4))
    assert np.array_equal(MS.philox_rows(seed, 1000, 7), rows[1000:1007])           # chunks start anywhere
    for s in (0, 1, 2999):
        assert [int(x) for x in rows[s]] == R.philox4x64_10([s, 0, 0, 0], [seed, 0])


def test_umul64hi():
    a = np.random.default_rng(0).integers(0, 2 ** 63, 2000, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    for b in (0, 1, 2 ** 32 + 7, 2 ** 62 + 12345, 2 ** 63 - 1):
        assert [int(x) for x in MS.umul64hi(a, b)] == [(int(y) * b) >> 64 for y in a]


def _scalar_samples(v, f, n, seed):
    """Steps 1-4 one sample at a time in plain Python (float64 scalars, integer weights as Python ints)."""
    areas = []
    for t in f:
        a, b, c = v[t[0]], v[t[1]], v[t[2]]
        e1, e2 = [b[i] - a[i] for i in range(3)], [c[i] - a[i] for i in range(3)]
        cx, cy, cz = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
        areas.append(0.5 * ((cx * cx + cy * cy) + cz * cz) ** 0.5)
    amax = max(areas)
    cum, acc = [], 0
    for a in areas:
        acc += int(np.floor(np.ldexp(a / amax, 32)))
        cum.append(acc)
    out = np.empty((n, 3), np.float32)
    for s in range(n):
        r = R.philox4x64_10([s, 0, 0, 0], [seed, 0])
        i = bisect.bisect_right(cum, (r[0] * cum[-1]) >> 64)
        u = (r[1] >> 11) * 2.0 ** -53
        w = (1.0 - u) * ((r[2] >> 11) * 2.0 ** -53)
        t = f[i]
        out[s] = [((v[t[0]][k] * u) + (v[t[1]][k] * w)) + ((1.0 - (u + w)) * v[t[2]][k]) for k in range(3)]
    return out


@pytest.mark.parametrize('seed', [0, 2 ** 64 - 1])
def test_samples_equal_the_scalar_restatement(seed):
    v, f = R.soup(50, 3, zero=5)
    got = MS.sample_points(*MS.check_mesh(v, f, 400, 64, seed), 400, seed)
    assert got.tobytes() == _scalar_samples(v.tolist(), f.tolist(), 400, seed).tobytes()


@pytest.mark.parametrize('vg', [2, 64, 1024, 2 ** 21])
def test_voxel_stage_equals_the_reference_lines(vg):
    rng = np.random.default_rng(vg)
    for p in (rng.random((20000, 3)).astype(np.float32) * 3 - 1,
              (rng.integers(0, 40, (20000, 3)) * 0.25 + 1e6).astype(np.float32),       # offset cloud, many duplicates
              R.icosphere(2)[0].astype(np.float32)[rng.integers(0, 162, 5000)]):
        got = MS.voxelize_samples(p, vg)
        ref = R.reference_voxels(p, vg)
        assert got.dtype == np.float32 and np.array_equal(got, ref)
        assert got.min() >= 0 and got.max() <= vg - 1


def test_voxel_stage_of_coincident_samples_is_one_point():
    p = np.full((5, 3), 2.5, np.float32)
    assert np.array_equal(MS.voxelize_samples(p, 64), np.zeros((1, 3), np.float32))
    assert np.array_equal(MS.voxelize_samples(p[:1], 64), np.zeros((1, 3), np.float32))


def test_pick_counts_follow_the_weights_and_zero_area_is_never_picked():
    areas = [1.0, 0.5, 0.0, 0.25, 2.0, 1e-3, 0.0, 0.75]
    v, f = R.stacked_triangles(areas)
    n = 400000
    p = MS.sample_points(*MS.check_mesh(v, f, n, 64, 7), n, 7)
    counts = np.bincount(np.rint(p[:, 2]).astype(int), minlength=len(areas))
    assert counts[2] == 0 and counts[6] == 0
    w = np.floor(np.ldexp(np.array(areas) / max(areas), 32))
    live = w > 0
    res = chisquare(counts[live], n * w[live] / w.sum())
    assert res.pvalue > 1e-3, (counts, res)


def test_barycentric_means_are_pyntclouds():
    v = np.eye(3)
    p = MS.sample_points(v, np.array([[0, 1, 2]], np.int32), 200000, 11)     # p = (u, v, 1 - u - v)
    assert np.all(np.abs(p.mean(0) - [0.5, 0.25, 0.25]) < 0.005), p.mean(0)


def test_host_path_is_reproducible_and_seeded():
    v, f = R.icosphere(3)
    a, sa = MS.mesh_to_points(v, f, 50000, 64, 5, return_samples=True)
    b, sb = MS.mesh_to_points(v, f, 50000, 64, 5, return_samples=True)
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()
    assert not np.array_equal(MS.mesh_to_points(v, f, 50000, 64, 6, return_samples=True)[1], sa)
    assert np.array_equal(a, R.reference_voxels(sa, 64))


def test_bad_meshes_are_refused():
    v, f = R.soup(10, 0)
    cases = [
        (np.where(np.arange(30)[:, None] == 4, np.nan, v), f),
        (np.where(np.arange(30)[:, None] == 4, np.inf, v), f),
        (v * 2.0 ** 101, f),
        (v, f + 1),
        (v, f - 1),
        (np.zeros((3, 3)), np.array([[0, 1, 2]])),
        (R.soup(4, 0, zero=4)[0], R.soup(4, 0, zero=4)[1]),
        (v, f[:, :2]),
        (v, np.zeros((0, 3), np.int32)),
        (v, f.astype(np.float64)),
    ]
    for vv, ff in cases:
        with pytest.raises(ValueError):
            MS.check_mesh(vv, ff, 100, 64, 0)
    MS.check_mesh(v * 2.0 ** 99, f, 100, 64, 0)                      # the bound itself is fine
    for n, vg, seed in ((0, 64, 0), (2 ** 31, 64, 0), (10, 0, 0), (10, 2 ** 21 + 1, 0), (10, 64, -1), (10, 64, 2 ** 64)):
        with pytest.raises(ValueError):
            MS.check_mesh(v, f, n, vg, seed)


# ---- readers --------------------------------------------------------------------------------------------------------------------

QUAD_V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1.5]], np.float64)
QUAD_F = [[0, 1, 2, 3], [0, 1, 4]]
QUAD_TRIS = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4]], np.int32)


def _check(path, v=QUAD_V, tris=QUAD_TRIS):
    gv, gf = mesh_io.read_mesh(str(path))
    assert gv.dtype == np.float64 and gf.dtype == np.int32
    assert np.array_equal(gv, v)
    assert np.array_equal(gf, tris)                                          # file order


def test_off_variants(tmp_path):
    body = ['0 0 0', '1 0 0', '1 1 0', '0 1 0', '0 0 1.5', '4 0 1 2 3', '3 0 1 4']
    p = tmp_path / 'a.off'
    p.write_text('OFF\n5 2 0\n' + '\n'.join(body) + '\n')
    _check(p)
    p.write_text('OFF5 2 0\n' + '\n'.join(body) + '\n')                        # ModelNet's glued header
    _check(p)
    p.write_text('# made by hand\nOFF\n# counts next\n\n5 2 0\n' + '\n'.join(body[:5]) + '\n# faces\n'
                 + '4 0 1 2 3 255 0 0\n3 0 1 4 0 255 0   # coloured\n')       # comments, extra per-face values
    _check(p)
    p.write_text('OFF\n5 1 0\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n0 0 1.5\n5 0 1 2 3 4\n')
    _check(p, tris=np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4]], np.int32))    # pentagon fan


def test_mixed_polygons_keep_the_file_order(tmp_path):
    v = '\n'.join(' '.join(map(str, r)) for r in QUAD_V.tolist())
    p = tmp_path / 'a.off'
    p.write_text(f'OFF\n5 4 0\n{v}\n3 0 1 4\n4 0 1 2 3\n3 1 2 4\n5 4 3 2 1 0\n')
    tris = np.array([[0, 1, 4], [0, 1, 2], [0, 2, 3], [1, 2, 4], [4, 3, 2], [4, 2, 1], [4, 1, 0]], np.int32)
    assert np.array_equal(mesh_io.read_mesh(str(p))[1], tris)                # not sorted: exactly this order
    q = tmp_path / 'a.ply'
    faces = [[0, 1, 4], [0, 1, 2, 3], [1, 2, 4], [4, 3, 2, 1, 0]]
    for fmt in ('ascii', 'binary_little_endian', 'binary_big_endian'):
        _ply(q, fmt, faces=faces)
        assert np.array_equal(mesh_io.read_mesh(str(q))[1], tris)


def _ply(path, fmt, vtype='float', ctype='uchar', itype='int', name='vertex_indices', faces=QUAD_F, extra_elem=False, face_extra=False):
    endian = {'binary_little_endian': '<', 'binary_big_endian': '>'}.get(fmt)
    codes = {'float': 'f', 'double': 'd', 'uchar': 'B', 'ushort': 'H', 'int': 'i', 'uint': 'I', 'char': 'b', 'short': 'h'}
    head = ['ply', f'format {fmt} 1.0', 'comment test', f'element vertex {len(QUAD_V)}', f'property {vtype} x',
            f'property {vtype} y', 'property uchar red', f'property {vtype} z', f'element face {len(faces)}',
            f'property list {ctype} {itype} {name}']
    if face_extra:
        head.append('property uchar flags')
    if extra_elem:
        head += ['element edge 1', 'property int vertex1', 'property int vertex2']
    head.append('end_header')
    out = ('\n'.join(head) + '\n').encode('ascii')
    if endian is None:
        rows = [f'{x:g} {y:g} 7 {z:g}' for x, y, z in QUAD_V]
        rows += [' '.join(map(str, [len(fc)] + fc + ([3] if face_extra else []))) for fc in faces]
        rows += ['0 1'] if extra_elem else []
        out += ('\n'.join(rows) + '\n').encode('ascii')
    else:
        for x, y, z in QUAD_V:
            out += struct.pack(endian + codes[vtype] * 2 + 'B' + codes[vtype], x, y, 7, z)
        for fc in faces:
            out += struct.pack(endian + codes[ctype] + codes[itype] * len(fc), len(fc), *fc)
            if face_extra:
                out += struct.pack('B', 3)
        if extra_elem:
            out += struct.pack(endian + 'ii', 0, 1)
    path.write_bytes(out)


@pytest.mark.parametrize('fmt', ['ascii', 'binary_little_endian', 'binary_big_endian'])
def test_ply_variants(tmp_path, fmt):
    p = tmp_path / 'm.ply'
    for kw in (dict(), dict(vtype='double', ctype='uint', itype='uint'), dict(ctype='ushort', itype='short', name='vertex_index'),
               dict(ctype='char', itype='uint', extra_elem=True, face_extra=True)):
        _ply(p, fmt, **kw)
        _check(p)
    tri = [[0, 1, 2], [2, 3, 0], [0, 1, 4]]                                     # uniform counts: the vectorised binary path
    _ply(p, fmt, faces=tri, face_extra=True)
    _check(p, tris=np.array(tri, np.int32))


def test_bad_mesh_files_raise(tmp_path):
    p = tmp_path / 'a.off'
    for text in ('OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n2 0 1\n',              # a face of two vertices
                 'OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 3\n',            # index out of range
                 'OFF\n3 1 0\n0 0 0\n1 0 0\n',                            # truncated
                 'PLY\n3 1 0\n'):
        p.write_text(text)
        with pytest.raises(ValueError):
            mesh_io.read_mesh(str(p))
    q = tmp_path / 'b.ply'
    for kw in (dict(faces=[[0, 1]]), dict(faces=[[0, 1, 9]]), dict(name='other')):
        for fmt in ('ascii', 'binary_little_endian'):
            _ply(q, fmt, **kw)
            with pytest.raises(ValueError):
                mesh_io.read_mesh(str(q))
    pc_io.write_ply(str(q), pd.DataFrame({'x': [0.0], 'y': [1.0], 'z': [2.0]}))       # a cloud is not a mesh
    with pytest.raises(ValueError):
        mesh_io.read_mesh(str(q))


# ---- CLIs -----------------------------------------------------------------------------------------------------------------------

def _write_off(path, v, f):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(f'OFF{len(v)} {len(f)} 0\n')
        fh.write('\n'.join(' '.join(repr(float(x)) for x in r) for r in v) + '\n')
        fh.write('\n'.join('3 ' + ' '.join(str(int(i)) for i in r) for r in f) + '\n')


def _run(*args):
    return subprocess.run([sys.executable, '-m'] + list(args), cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                          text=True, timeout=600)


def test_dataset_clis_end_to_end_on_the_host(tmp_path):
    src, pc, blocks, sel = (str(tmp_path / d) for d in ('meshes', 'pc', 'blocks', 'sel'))
    meshes = {'chair/a.off': R.icosphere(2), 'chair/train/b.off': R.soup(300, 1), 'c.off': R.icosphere(1)}
    for rel, (v, f) in meshes.items():
        _write_off(os.path.join(src, rel), v, f)
    open(os.path.join(src, 'ignored.txt'), 'w').write('x')
    p = _run('pcc_geo_cnn_v2_amd.ds_mesh_to_pc', src, pc, '--vg_size', '32', '--n_samples', '20000', '--seed', '3', '--device', 'host')
    assert p.returncode == 0, p.stderr[-2000:]
    for rel, (v, f) in meshes.items():
        out = os.path.join(pc, rel[:-4] + '.ply')
        assert open(out, 'rb').read().split(b'\n')[1] == b'format binary_little_endian 1.0'
        df = pc_io.read_ply(out)
        assert list(df.columns) == ['x', 'y', 'z'] and all(df[c].dtype == np.float32 for c in 'xyz')
        rv, rf = mesh_io.read_mesh(os.path.join(src, rel))
        ref = MS.mesh_to_points(rv, rf, 20000, 32, ds_mesh_to_pc.file_seed(3, rel))
        assert np.array_equal(df.values, ref)
    assert _run('pcc_geo_cnn_v2_amd.ds_mesh_to_pc', src, pc, '--device', 'host').returncode != 0      # dest exists
    pc2 = str(tmp_path / 'pc2')                                              # `source/` with a trailing slash: the same files
    p = _run('pcc_geo_cnn_v2_amd.ds_mesh_to_pc', src + '/', pc2 + '/', '--vg_size', '32', '--n_samples', '20000', '--seed', '3',
             '--device', 'host')
    assert p.returncode == 0, p.stderr[-2000:]
    for rel in meshes:
        assert open(os.path.join(pc2, rel[:-4] + '.ply'), 'rb').read() == open(os.path.join(pc, rel[:-4] + '.ply'), 'rb').read()

    p = _run('pcc_geo_cnn_v2_amd.ds_pc_octree_blocks', pc, blocks, '--vg_size', '32', '--level', '1')
    assert p.returncode == 0, p.stderr[-2000:]
    got = sorted(os.path.relpath(os.path.join(d, x), blocks) for d, _, fs in os.walk(blocks) for x in fs)
    a = pc_io.read_ply(os.path.join(pc, 'chair', 'a.ply'))
    parts = [pc_io.read_ply(os.path.join(blocks, 'chair', x)) for x in sorted(os.listdir(os.path.join(blocks, 'chair')))
             if x.startswith('a_')]
    assert len(parts) > 1 and sum(len(b) for b in parts) == len(a)
    assert all(list(b.columns) == ['x', 'y', 'z'] and b['x'].dtype == np.float32 and b.values.max() < 16 for b in parts)
    assert 'chair/a_000.ply' in got and any(g.startswith('chair/train/b_') for g in got)
    assert _run('pcc_geo_cnn_v2_amd.ds_pc_octree_blocks', pc + '/', str(tmp_path / 'blocks2'), '--vg_size', '32', '--level',
                '1').returncode == 0
    assert sorted(os.path.relpath(os.path.join(d, x), str(tmp_path / 'blocks2')) for d, _, fs in os.walk(tmp_path / 'blocks2')
                  for x in fs) == got

    p = _run('pcc_geo_cnn_v2_amd.ds_select_largest', blocks, sel, '2')
    assert p.returncode == 0, p.stderr[-2000:]
    links = [os.path.join(d, x) for d, _, fs in os.walk(sel) for x in fs]
    sizes = sorted((os.path.getsize(os.path.join(d, x)) for d, _, fs in os.walk(blocks) for x in fs), reverse=True)
    assert len(links) == 2 and all(os.path.islink(x) for x in links)
    assert sorted(os.path.getsize(x) for x in links) == sorted(sizes[:2])
    for x in links:
        assert os.path.realpath(x) == os.path.realpath(os.path.join(blocks, os.path.relpath(x, sel)))
    sel2 = str(tmp_path / 'sel2')
    assert _run('pcc_geo_cnn_v2_amd.ds_select_largest', blocks + '/', sel2, '2').returncode == 0
    links2 = [os.path.join(d, x) for d, _, fs in os.walk(sel2) for x in fs]
    assert sorted(os.path.relpath(x, sel2) for x in links2) == sorted(os.path.relpath(x, sel) for x in links)
    for x in links2:
        assert os.path.realpath(x) == os.path.realpath(os.path.join(blocks, os.path.relpath(x, sel2)))
