"""GPU: ops.mesh_to_points (include/pcc_geo.h "mesh sampling") against the host definition utils/mesh_sampling.py -- raw samples and
voxels, in order, bit for bit -- repeat-call bits, the ds_mesh_to_pc CLI on both devices, and a converted mesh through the codec CLIs
and the report."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _mesh_ref as R
from pcc_geo_cnn_v2_amd import ops
from pcc_geo_cnn_v2_amd.utils import mesh_sampling as MS, pc_io

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 2 ** 64 - 1)


def _meshes():
    soup = R.soup(20000, 1, zero=500)
    ico = R.icosphere(5)
    return {'soup': soup, 'icosphere': ico, 'offset': (ico[0] + 1e6, ico[1]),
            'single': (np.array([[0.25, -1.0, 3.0], [2.0, 0.5, 3.0], [0.0, 1.0, -4.5]]), np.array([[0, 1, 2]], np.int32))}


MESHES = _meshes()
CASES = [('soup', 1, 64), ('soup', 7, 2), ('soup', 1000, 1024), ('soup', 500000, 64), ('soup', 500000, 2 ** 21), ('soup', 3000000, 1024),
         ('icosphere', 1000, 1), ('icosphere', 500000, 1024), ('icosphere', 3000000, 2 ** 21), ('offset', 500000, 64),
         ('offset', 7, 2 ** 21), ('single', 1, 64), ('single', 1000, 2), ('single', 500000, 1024)]


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('name,n,vg', CASES)
def test_gpu_bits_equal_the_host_path(ctx, name, n, vg, seed):
    v, f = MESHES[name]
    pts, samples = ops.mesh_to_points(ctx, v, f, n, vg, seed, return_samples=True)
    ref_samples = MS.sample_points(*MS.check_mesh(v, f, n, vg, seed), n, seed)
    assert samples.dtype == np.float32 and samples.shape == (n, 3)
    bad = np.nonzero((samples != ref_samples).any(1))[0]
    assert len(bad) == 0, (name, n, vg, seed, len(bad), bad[:3], samples[bad[:3]], ref_samples[bad[:3]])
    assert samples.tobytes() == ref_samples.tobytes()
    ref = MS.voxelize_samples(ref_samples, vg)
    assert pts.dtype == np.float32 and pts.shape == ref.shape, (pts.shape, ref.shape)
    assert pts.tobytes() == ref.tobytes()
    assert pts.min() >= 0 and pts.max() <= vg - 1
    if n < 1000000:
        assert ops.mesh_to_points(ctx, v, f, n, vg, seed).tobytes() == pts.tobytes()      # without the samples


def test_two_calls_give_identical_bits(ctx):
    v, f = MESHES['soup']
    a = ops.mesh_to_points(ctx, v, f, 2000000, 1024, 9, return_samples=True)
    b = ops.mesh_to_points(ctx, v, f, 2000000, 1024, 9, return_samples=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_bad_inputs_are_refused_before_the_gpu(ctx):
    v, f = MESHES['single']
    for args in ((v, f + 1, 10, 64), (v * np.nan, f, 10, 64), (v, f, 0, 64), (v, f, 10, 2 ** 21 + 1), (np.zeros((3, 3)), f, 10, 64)):
        with pytest.raises(ValueError):
            ops.mesh_to_points(ctx, *args)


def _off(path, v, f):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as fh:
        fh.write(f'OFF\n{len(v)} {len(f)} 0\n')
        fh.write('\n'.join(' '.join(repr(float(x)) for x in r) for r in v) + '\n')
        fh.write('\n'.join('3 ' + ' '.join(str(int(i)) for i in r) for r in f) + '\n')


def _run(*args):
    p = subprocess.run([sys.executable, '-m'] + list(args), cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def test_cli_writes_the_same_bytes_on_both_devices(tmp_path):
    src = str(tmp_path / 'meshes')
    _off(os.path.join(src, 'a', 'sphere.off'), *R.icosphere(4))
    _off(os.path.join(src, 'soup.off'), *R.soup(3000, 2, zero=10))
    for dev in ('gpu', 'host'):
        _run('pcc_geo_cnn_v2_amd.ds_mesh_to_pc', src, str(tmp_path / dev), '--vg_size', '256', '--n_samples', '300000', '--seed', '4',
             '--device', dev)
    for rel in ('a/sphere.ply', 'soup.ply'):
        g, h = (open(tmp_path / d / rel, 'rb').read() for d in ('gpu', 'host'))
        assert g == h and len(g) > 1000


def test_converted_mesh_goes_through_the_codec_and_the_report(tmp_path):
    res = 128
    src = str(tmp_path / 'meshes')
    v, f = R.icosphere(4)
    _off(os.path.join(src, 'sphere.off'), v, f)
    pcdir = str(tmp_path / 'pc')
    _run('pcc_geo_cnn_v2_amd.ds_mesh_to_pc', src, pcdir, '--vg_size', str(res), '--n_samples', '500000')
    inp = os.path.join(pcdir, 'sphere.ply')
    pts = pc_io.load_pc(inp)
    assert len(pts) > 10000 and pts.min() == 0 and pts.max() == res - 1
    ck = str(tmp_path / 'ckpt')
    _run('pcc_geo_cnn_v2_amd.init_checkpoint', '--model_config', 'c3p', '--checkpoint_dir', ck)
    out, dec = str(tmp_path / 'o' / 'sphere.ply.bin'), str(tmp_path / 'dec.ply')
    _run('pcc_geo_cnn_v2_amd.compress_octree', '--input_files', inp, '--output_files', out, '--checkpoint_dir', ck, '--model_config',
         'c3p', '--resolution', str(res), '--octree_level', '2', '--opt_metrics', 'd1_mse', '--fixed_threshold')
    _run('pcc_geo_cnn_v2_amd.decompress_octree', '--input_files', out, '--output_files', dec, '--checkpoint_dir', ck,
         '--model_config', 'c3p')
    b = pc_io.load_pc(dec)
    assert len(b) > 0 and b.min() >= 0 and b.max() < res
    rep = str(tmp_path / 'report.json')
    _run('pcc_geo_cnn_v2_amd.ev_report', '--input_pc', inp, '--decoded_pc', dec, '--enc_pc', out, '--resolution', str(res),
         '--output', rep)
    r = json.load(open(rep))
    assert np.isfinite(r['d1_psnr']) and r['d1_mse'] >= 0
