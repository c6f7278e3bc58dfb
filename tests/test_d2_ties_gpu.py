"""GPU: the tie-averaged D2 engine (pcc_cloud_distortion_ties, ops.cloud_distortion(..., ties='mean')) against the brute-force
restatement tests/_ties_ref.py and against the host path within the derived rounding bound, bit-reproducible calls, the reported
pair-capacity overflow, and the default rule (`pick`) unchanged through the new entry point."""
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import _ties_ref as R
from _ops_patch import patch_ops
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ops
from pcc_geo_cnn_v2_amd.utils import pc_io, pc_metric

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()
EXACT = [0, 1, 2, 5, 6]
PLANE = [3, 4, 7, 8]


def _within(got, want, bound, what):
    print(what, 'got', got[PLANE], 'want', want[PLANE], 'diff', np.abs(got - want)[PLANE], 'bound', bound[PLANE])
    assert np.array_equal(got[EXACT], want[EXACT]), (what, got, want)
    assert np.all(np.abs(got - want)[PLANE] <= bound[PLANE]), (what, np.abs(got - want)[PLANE], bound[PLANE])


def _host(a, b, n):
    return pc_metric.cloud_tally_host(a.astype(np.float64), b.astype(np.float64), n, ties='mean')


@pytest.mark.parametrize('name', sorted(CASES))
def test_mean_matches_the_brute_force_and_the_host(ctx, name):
    a, b, n = CASES[name]
    ref = R.tally_ref(a, b, n)
    got, to_b, to_a = ops.cloud_distortion(ctx, a, b, n, return_links=True, ties='mean')
    assert got.dtype == np.float64 and got.shape == (9,)
    _within(got, ref['tally'], R.bounds(ref), (name, 'ref'))
    _within(got, _host(a, b, n), R.bounds(ref), (name, 'host'))
    # the links are the default rule's: the lowest row of each tie set
    q, j, _ = R.tie_sets(b, a)
    assert np.array_equal(to_b, j[np.searchsorted(q, np.arange(len(a)))])
    q, j, _ = R.tie_sets(a, b)
    assert np.array_equal(to_a, j[np.searchsorted(q, np.arange(len(b)))])
    # without normals: the D1 / H1 slots alone
    bare = ops.cloud_distortion(ctx, a, b, ties='mean')
    assert np.array_equal(bare[EXACT], ref['tally'][EXACT]) and not bare[PLANE].any()


def test_large_shell_against_the_brute_force_and_the_host(ctx):
    a, b = R.shell(89, 92), R.shell(88, 92)
    assert len(a) >= 99000 and len(b) >= 97000                             # a 1e5-point shell against its eroded copy
    n = R.radial_normals(a, 92)
    ref = R.tally_ref(a, b, n)
    assert ref['C'] >= 3
    got = ops.cloud_distortion(ctx, a, b, n, ties='mean')
    _within(got, ref['tally'], R.bounds(ref), 'shell89 ref')
    _within(got, _host(a, b, n), R.bounds(ref), 'shell89 host')
    again = ops.cloud_distortion(ctx, a, b, n, ties='mean')
    assert got.tobytes() == again.tobytes()
    # permuted rows: within the bound of the unpermuted result, on the GPU too
    rng = np.random.default_rng(5)
    pa, pb = rng.permutation(len(a)), rng.permutation(len(b))
    _within(ops.cloud_distortion(ctx, a[pa], b[pb], n[pa], ties='mean'), got, R.bounds(ref), 'shell89 permuted')
    # the batch helpers take the rule: one candidate, and an empty one beside it
    tallies = pc_metric.cloud_tallies_gpu(ctx, a, [b, np.zeros((0, 3))], n, ties='mean')
    assert tallies[1] is None and tallies[0].tobytes() == got.tobytes()
    table = pc_metric.cloud_metrics_batch_gpu(ctx, a, [b], 1023, n, ties='mean')[0]
    assert table == pc_metric.metrics_table(len(a), got[:5], 1023)


@pytest.mark.parametrize('name', ['shell', 'duplicates', 'faces_swapped'])
def test_two_calls_give_identical_bits(ctx, name):
    a, b, n = CASES[name]
    t1 = ops.cloud_distortion(ctx, a, b, n, ties='mean')
    t2 = ops.cloud_distortion(ctx, a, b, n, ties='mean')
    assert t1.tobytes() == t2.tobytes()


def test_mean_equals_pick_bit_for_bit_without_ties(ctx):
    a, b, n = R.singleton_case()
    assert R.all_singletons(R.tally_ref(a, b, n))
    mean, pick = ops.cloud_distortion(ctx, a, b, n, ties='mean'), ops.cloud_distortion(ctx, a, b, n)
    assert np.array_equal(mean[EXACT + [7, 8]], pick[EXACT + [7, 8]])      # the per-point terms are the same bits
    assert np.array_equal(mean, pick), (mean, pick)                          # and so are their sums: the same tally order


def test_pair_capacity_overflow_is_reported_not_truncated(ctx):
    a, b, n = CASES['shell']
    pairs = len(R.tie_sets(b, a)[0])
    assert pairs > len(a)
    index = ops.CloudIndex(ctx, a)
    tally, status = ops.cloud_distortion_launch(ctx, index, b, n, ties='mean', max_pairs=pairs)
    assert status.cpu().tolist() == [pairs, 0]
    full = tally.cpu().numpy()
    tally, status = ops.cloud_distortion_launch(ctx, index, b, n, ties='mean', max_pairs=pairs - 1)
    assert status.cpu().tolist() == [pairs, 1]
    short = tally.cpu().numpy()
    assert np.isnan(short[PLANE]).all() and np.array_equal(short[EXACT], full[EXACT])
    with pytest.raises(ops.TiePairOverflow, match=f'needs {pairs} tie pairs') as e:
        ops.cloud_distortion(ctx, a, b, n, ties='mean', max_pairs=len(a))
    assert e.value.pairs == pairs
    assert np.array_equal(ops.cloud_distortion(ctx, a, b, n, ties='mean', max_pairs=e.value.pairs), full)
    assert np.array_equal(ops.cloud_distortion(ctx, a, b, n, ties='mean'), full)           # the default capacity holds them
    with pytest.raises(L.PccError, match='max_pairs'):
        ops.cloud_distortion(ctx, a, b, n, ties='mean', max_pairs=0)


def test_default_capacity_overflow_runs_again_with_the_reported_count(ctx, monkeypatch):
    a, b, n = CASES['single_b']                                            # every original point votes for the one decoded point
    want = ops.cloud_distortion(ctx, a, b, n, ties='mean')
    patch_ops(monkeypatch, 'tie_pair_capacity', lambda n_a: 7)           # a sizing rule this input exceeds
    calls = []
    real = ops.cloud_distortion_launch
    patch_ops(monkeypatch, 'cloud_distortion_launch', lambda *x, **k: calls.append(k.get('max_pairs')) or real(*x, **k))
    assert np.array_equal(ops.cloud_distortion(ctx, a, b, n, ties='mean'), want)
    assert calls == [None, len(a)]
    calls.clear()
    assert np.array_equal(pc_metric.cloud_tallies_gpu(ctx, a, [b], n, ties='mean')[0], want)
    assert calls == [None, len(a)]


@pytest.mark.parametrize('name', ['shell', 'sparse', 'duplicates'])
def test_pick_is_unchanged_through_the_new_entry(ctx, name):
    a, b, n = CASES[name]
    dev = ctx.device
    ia, ib = ops.CloudIndex(ctx, a), ops.CloudIndex(ctx, b)
    nrm = torch.from_numpy(n).to(dev)
    old, new = (torch.empty(9, dtype=torch.float64, device=dev) for _ in range(2))
    links = [torch.empty(k, dtype=torch.int32, device=dev) for k in (len(a), len(b), len(a), len(b))]
    status = torch.full((2,), -1, dtype=torch.int64, device=dev)
    lib = L.lib()
    size = lib.pcc_cloud_distortion_ties_workspace_bytes(len(a), len(b), 0, 0)
    assert size == lib.pcc_cloud_distortion_workspace_bytes(len(a), len(b))
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()
    L.check(lib.pcc_cloud_distortion(ctx.handle, p(ia.buffer), len(a), p(ib.buffer), len(b), p(nrm), p(old), p(links[0]), p(links[1]), p(ws),
                                     ctx.stream), 'pcc_cloud_distortion')
    L.check(lib.pcc_cloud_distortion_ties(ctx.handle, p(ia.buffer), len(a), p(ib.buffer), len(b), p(nrm), 0, 0, p(new), p(status), p(links[2]),
                                          p(links[3]), p(ws), ctx.stream), 'pcc_cloud_distortion_ties')
    assert old.cpu().numpy().tobytes() == new.cpu().numpy().tobytes()
    assert torch.equal(links[0], links[2]) and torch.equal(links[1], links[3]) and status.cpu().tolist() == [0, 0]
    assert np.array_equal(ops.cloud_distortion(ctx, a, b, n, ties='pick'), old.cpu().numpy())
    assert lib.pcc_cloud_distortion_ties(ctx.handle, p(ia.buffer), len(a), p(ib.buffer), len(b), p(nrm), 2, 10, p(new), p(status), None, None,
                                         p(ws), ctx.stream) == L.PCC_ERR_ARG


def test_ev_report_gpu_and_host_agree_under_mean(tmp_path):
    """Each GPU step of the command-line path is a child process under its own time limit."""
    a, b, n = CASES['shell']
    pa, pb, pn, enc = (str(tmp_path / f) for f in ('a.ply', 'b.ply', 'a_n.ply', 'a.bin'))
    rng = np.random.default_rng(9)
    pc_io.write_pc(pa, a.astype(np.float32))
    pc_io.write_pc(pb, b[rng.permutation(len(b))].astype(np.float32))      # the decoded file in another row order
    pc_io.write_df(pn, pd.DataFrame(np.hstack([a, n]).astype(np.float32), columns=['x', 'y', 'z', 'nx', 'ny', 'nz']))
    open(enc, 'wb').write(b'\x00' * 100)
    reports = {}
    for dev in ('host', 'gpu'):
        cmd = ['timeout', '-k', '10', '300', sys.executable, '-m', 'pcc_geo_cnn_v2_amd.ev_report', '--input_pc', pa, '--decoded_pc', pb,
               '--enc_pc', enc, '--input_norm', pn, '--resolution', '64', '--hausdorff', '--d2_ties', 'mean', '--metrics_device', dev,
               '--output', str(tmp_path / f'{dev}.json')]
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True)
        assert done.returncode == 0, done.stderr[-2000:]
        reports[dev] = json.load(open(tmp_path / f'{dev}.json'))
    host, gpu = reports['host'], reports['gpu']
    assert host['d2_ties'] == gpu['d2_ties'] == 'mean' and set(host) == set(gpu)
    ref = R.tally_ref(a, b, np.asarray(pc_io.load_normals(pn), np.float64))
    bound = R.bounds(ref)
    for k in ('d1_mse', 'd1_psnr', 'd1_hausdorff', 'd1_hausdorff_AB', 'd1_hausdorff_BA'):
        assert host[k] == gpu[k], k
    assert abs(host['d2_mse'] - gpu['d2_mse']) <= max(bound[3] / len(a), bound[4] / len(b))
    for k, s in (('d2_hausdorff_AB', 7), ('d2_hausdorff_BA', 8)):
        assert abs(host[k] - gpu[k]) <= bound[s], k
