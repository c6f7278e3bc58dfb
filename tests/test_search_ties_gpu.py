"""GPU: the tie-averaged D2 statistics of the per-block threshold search (ops.d12_threshold_stats_ties, --search_ties mean) against
the host restatement (model_opt.host_threshold_stats(ties='mean')), the brute-force tally of tests/_ties_ref.py and the
reference-produced tie-free fixture.  Every tolerance is the derived rounding bound of tests/_search_ties_ref.py."""
import functools
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _search_ties_ref as S
import _ties_ref as R
from _ops_patch import patch_ops
from pcc_geo_cnn_v2_amd import model_opt, ops
from pcc_geo_cnn_v2_amd.model_syntax import load_compressed_file
from pcc_geo_cnn_v2_amd.utils import pc_io
from pcc_geo_cnn_v2_amd.utils import pc_metric as PM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
THR = np.linspace(0, 1.0, 96)            # two chunks of thresholds (64 at a time)
# the symmetric d2 metrics (the set of the reference-produced fixtures).  The one-directional ones are not part of the decision test: they
# are EXACTLY 0 on several different level sets (every row of A inside B_t, or B_t inside A), a runner-up gap of 0 by construction
METRICS, DELTAS = ['d2_mse', 'd2_sum_max', 'd2_sum_mean'], [np.inf, 2.0]
D2_TABLE = functools.partial(PM.metrics_table, groups=('d2',))


@functools.lru_cache(None)
def _inputs(name):
    """blocks, x_hat, per block: host tallies / guard under 'mean' and the brute-force (ref, slot bounds) of every level set"""
    blocks, x_hat = getattr(S, name)()
    host = [model_opt.host_threshold_stats(b[:, :3], np.clip(x, 0, 1), THR, b[:, 3:], ties='mean') for b, x in zip(blocks, x_hat)]
    brute = [S.brute_tallies(b, x, THR) for b, x in zip(blocks, x_hat)]
    return blocks, x_hat, host, brute


def _gpu(ctx, blocks, x_hat, **kw):
    return model_opt.d12_tallies_gpu(ctx, blocks, torch.from_numpy(np.ascontiguousarray(x_hat)).to(ctx.device), THR, ties='mean', **kw)


ALL_D2 = [m for m in PM.avail_opt_metrics if m.startswith('d2_')]


@pytest.mark.parametrize('name', ['blocks_32', 'blocks_odd'])
def test_tallies_match_the_host_restatement_within_the_derived_bound(ctx, name):
    """Every (block, threshold): D1 / N_B / the number of level sets equal; D2 within the pair's own bound (its C, V, M by brute
    force, the search engines' summation depth); the host restatement and the GPU each within it of the exactly rounded brute force."""
    blocks, x_hat, host, brute = _inputs(name)
    got = _gpu(ctx, blocks, x_hat)
    worst = 0.0
    for i, (blk, (ht, _)) in enumerate(zip(blocks, host)):
        assert len(got[i]) == len(ht) == len(brute[i]), (i, len(got[i]), len(ht))
        assert np.array_equal(got[i][:, :3], ht[:, :3]), i
        for t, (ref, (b_ab, b_ba)) in enumerate(brute[i]):
            assert np.array_equal(ref['tally'][:3], ht[t, :3])
            for slot, bound in ((PM.D2_AB, b_ab), (PM.D2_BA, b_ba)):
                d = abs(got[i][t, slot] - ht[t, slot])
                print(f'{name} block {i} t {t} slot {slot}: gpu {got[i][t, slot]!r} host {ht[t, slot]!r} |diff| {d:.3e} bound {bound:.3e}')
                assert d <= bound, (i, t, slot, d, bound)
                assert abs(got[i][t, slot] - ref['tally'][slot]) <= bound, (i, t, slot)
                worst = max(worst, d / bound if bound else 0.0)
    print(f'{name}: largest |gpu - host| / bound = {worst:.3e}')


@pytest.mark.parametrize('name', ['blocks_32', 'blocks_odd'])
def test_decisions_equal_the_host_restatement(ctx, name):
    """FIRST the precondition, from host data alone (tests/test_search_ties_cpu.py asserts the same without a GPU): on these seeded
    inputs the host restatement's runner-up gap and its distance from the guard exceed 2 beta on every block and symmetric metric
    (beta = the slot bounds carried through the metric formula).  Then the GPU run: for every block and EVERY d2 metric,
    unconditionally, the host's metric at the GPU's choice is within 2 beta of its own minimum; and on the symmetric metrics the
    decisions are EQUAL on all blocks."""
    blocks, x_hat, host, brute = _inputs(name)
    for i, blk in enumerate(blocks):
        bad = S.gap_failures(len(blk), host[i][0], host[i][1], brute[i], 31, METRICS, DELTAS, D2_TABLE, model_opt.ratio_eligible)
        assert not bad, f'precondition: {name} block {i}: (metric, t, gap, guard gap, 2 beta) = {bad}: pick another seed'
    got = _gpu(ctx, blocks, x_hat)
    for i, blk in enumerate(blocks):
        n_a, (ht, guard) = len(blk), host[i]
        beta = S.metric_bounds(n_a, ht, brute[i], ALL_D2, D2_TABLE, 31)
        dec_h = S.decisions(n_a, ht, guard, 31, ALL_D2, DELTAS, D2_TABLE, model_opt.ratio_eligible)
        dec_g = S.decisions(n_a, got[i], guard, 31, ALL_D2, DELTAS, D2_TABLE, model_opt.ratio_eligible)
        for (nm, pool, col, k, gv), (_, pool_g, col_g, k_g, _) in zip(dec_h, dec_g):
            b = float(beta[nm.rsplit('_', 1)[0]][pool].max())
            print(f'{name} block {i} {nm}: host t {pool[k]} gpu t {pool_g[k_g]} excess {col[k_g] - col[k]:.3e} 2beta {2 * b:.3e}')
            assert np.array_equal(pool, pool_g)
            assert col[k_g] - col[k] <= 2 * b, (i, nm, col[k_g] - col[k], 2 * b)
        names_h, best_h = model_opt.select_thresholds_from_stats(n_a, ht, guard, len(THR), 32, METRICS, DELTAS)
        names_g, best_g = model_opt.decide_from_tallies([blk], [got[i]], len(THR), 32, METRICS, DELTAS, gpu_d2=True, ties='mean')
        assert names_g == names_h and best_g[0] == best_h, (i, best_g[0], best_h)


def test_tie_free_fixture_gives_the_references_decisions(ctx):
    """tests/golden/model_opt_d2_tiefree.npz (six blocks without equidistant neighbours, decisions and metric values at every level
    set produced by the reference's own module): under 'mean' the GPU gives all of the reference's decisions, its D1 values exactly
    (to the 1e-12 of the existing host test) and its D2 values within the rounding bound -- float64 normals, so no float32 margin."""
    g = np.load(os.path.join(G, 'model_opt_d2_tiefree.npz'))
    thresholds = np.linspace(0, 1.0, 256)
    mets, deltas = [str(m) for m in g['opt_metrics']], [float(d) for d in g['max_deltas']]
    decided = 0
    for i in range(int(g['n_cases'][0])):
        blk, xh = g[f's{i}_block'], g[f's{i}_x_hat']
        blk64 = blk.astype(np.float64)
        tallies = model_opt.d12_tallies_gpu(ctx, [blk64], torch.from_numpy(xh[None]).to(ctx.device), thresholds, ties='mean')[0]
        keys, want = [str(k) for k in g[f's{i}_keys']], g[f's{i}_vals']
        assert len(tallies) == len(want)
        brute = S.brute_tallies(blk64, xh, thresholds)
        assert all(R.all_singletons(ref) for ref, _ in brute)
        table = PM.metrics_table(len(blk), tallies, 63)
        got = np.array([[table[k][t] for k in keys] for t in range(len(tallies))])
        d1 = [j for j, k in enumerate(keys) if k.startswith('d1_')]
        assert np.allclose(got[:, d1], want[:, d1], rtol=1e-12 if blk.dtype == np.float64 else 1e-6, atol=0)
        for t, (ref, (b_ab, b_ba)) in enumerate(brute):
            assert abs(tallies[t, PM.D2_AB] - ref['tally'][3]) <= b_ab and abs(tallies[t, PM.D2_BA] - ref['tally'][4]) <= b_ba, (i, t)
        if blk.dtype == np.float64:       # the reference's own values: the same float64 inputs, 1e-12 like the tie-free host test
            assert np.allclose(got, want, rtol=1e-12, atol=0), (i, np.nanmax(np.abs(got / want - 1)))
        names, best = model_opt.decide_from_tallies([blk64], [tallies], len(thresholds), 64, mets, deltas, gpu_d2=True, ties='mean')
        assert names == [str(n) for n in g[f's{i}_names']]
        assert best[0] == [int(b) for b in g[f's{i}_best']], (i, best[0], list(g[f's{i}_best']))
        decided += sum(n.startswith('d2_') for n in names)
    assert decided >= 36


def test_row_order_batch_split_and_a_second_call_give_identical_bits(ctx):
    blocks, x_hat, _, _ = _inputs('blocks_32')
    first = _gpu(ctx, blocks, x_hat)
    again = _gpu(ctx, blocks, x_hat)
    rng = np.random.default_rng(3)
    shuffled = _gpu(ctx, [b[rng.permutation(len(b))] for b in blocks], x_hat)
    split = _gpu(ctx, blocks[:1], x_hat[:1]) + _gpu(ctx, blocks[1:], x_hat[1:])
    for a, b, c, d in zip(first, again, shuffled, split):
        assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()


def test_pair_capacity_overflow_is_reported_and_the_default_path_reruns(ctx, monkeypatch):
    blocks, x_hat, _, _ = _inputs('blocks_32')
    full = _gpu(ctx, blocks, x_hat)
    dev = ctx.device
    blks = [model_opt._canonical_rows(b) for b in blocks]
    xyz = torch.from_numpy(np.concatenate([b[:, :3] for b in blks]).astype(np.int32)).to(dev)
    nrm = torch.from_numpy(np.ascontiguousarray(np.concatenate([b[:, 3:] for b in blks]))).to(dev)
    sizes = [len(b) for b in blks]
    bof = torch.from_numpy(np.repeat(np.arange(len(blks), dtype=np.int32), sizes)).to(dev)
    start = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    args = (ctx, torch.from_numpy(x_hat).to(dev), torch.from_numpy(THR.astype(np.float32)).to(dev), xyz, bof, start, nrm)
    s_ab, s_ba, n_b, tcount, d2_ab, d2_ba, (pairs, over) = ops.d12_threshold_stats_ties(*args, max_pairs=1000, return_status=True)
    assert over and pairs > 1000
    assert np.isnan(d2_ab).all() and np.isnan(d2_ba).all()
    for i, t in enumerate(full):
        assert tcount[i] == len(t)
        assert np.array_equal(n_b[i][:len(t)], t[:, PM.N_B]) and np.array_equal(s_ab[i][:len(t)], t[:, PM.D1_AB]) and \
            np.array_equal(s_ba[i][:len(t)], t[:, PM.D1_BA])
    with pytest.raises(ops.SearchTiePairOverflow) as e:
        ops.d12_threshold_stats_ties(*args, max_pairs=1000)
    assert e.value.pairs == pairs
    exact = ops.d12_threshold_stats_ties(*args, max_pairs=pairs, return_status=True)
    assert exact[-1] == (pairs, False)
    # the default path: a default capacity that is too small is followed by one run with the reported count
    patch_ops(monkeypatch, 'search_tie_pair_capacity', lambda *a: 1000)
    rerun = _gpu(ctx, blocks, x_hat)
    for a, b in zip(full, rerun):
        assert a.tobytes() == b.tobytes()
    for i, t in enumerate(full):
        assert np.array_equal(exact[4][i][:len(t)], t[:, PM.D2_AB]) and np.array_equal(exact[5][i][:len(t)], t[:, PM.D2_BA])


def _cloud(res):
    g = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing='ij'), -1).reshape(-1, 3)
    d = np.linalg.norm(g - res / 2 + 0.3, axis=1)
    return g[np.abs(d - res * 0.37) < 0.7].astype(np.float32)


def test_cli_search_ties_mean_writes_the_same_bytes_on_either_engine(tmp_path):
    """compress_octree --search_ties mean on the 128^3 shell: --d2_search gpu and --d2_search kdtree (the host restatement) write
    byte-identical streams, both decode, the JSON carries "search_ties" only under mean, and a run without the flag writes what
    `--search_ties pick` writes (that these are the bytes of before the flag existed rests on the unchanged CLI tests, which run
    without it: tests/test_cli_gpu.py, tests/test_normals_gpu.py)."""
    res, level = 128, 2
    src = str(tmp_path / 'in.ply')
    pc_io.write_df(src, pc_io.pa_to_df(_cloud(res)))
    ck = str(tmp_path / 'ckpt')
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(*a):
        p = subprocess.run([sys.executable, '-m'] + list(a), cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
        assert p.returncode == 0, p.stderr[-3000:]
        return p.stderr

    run('pcc_geo_cnn_v2_amd.init_checkpoint', '--model_config', 'c3p', '--checkpoint_dir', ck, '--cell_level', '4')
    common = ['--checkpoint_dir', ck, '--model_config', 'c3p', '--resolution', str(res), '--octree_level', str(level),
              '--opt_metrics', 'd1_mse', 'd2_mse', '--batch_size', '8', '--estimate_normals']
    outs, logs = {}, {}
    for tag, extra in (('gpu', ['--search_ties', 'mean', '--d2_search', 'gpu']), ('kdtree', ['--search_ties', 'mean', '--d2_search', 'kdtree']),
                       ('mean', ['--search_ties', 'mean']), ('plain', []), ('pick', ['--search_ties', 'pick'])):
        o = [str(tmp_path / tag / f'in.{m}.ply.bin') for m in ('d1', 'd2')]
        logs[tag] = run('pcc_geo_cnn_v2_amd.compress_octree', '--input_files', src, '--output_files', *o, *common, *extra)
        outs[tag] = o
    for k in range(2):
        gpu, kd, mean = (open(outs[t][k], 'rb').read() for t in ('gpu', 'kdtree', 'mean'))
        if gpu != kd:       # name the blocks: (index, threshold of the GPU, threshold of the host restatement)
            tg, tk = ([t for _, t in load_compressed_file(gzip.open(outs[tag][k], 'rb'))[3]] for tag in ('gpu', 'kdtree'))
            differ = [(j, a, b) for j, (a, b) in enumerate(zip(tg, tk)) if a != b]
            raise AssertionError(f'rate point {k}: the GPU and the host restatement chose different thresholds on blocks (block, gpu, host) = '
                                 f'{differ} of {len(tg)}: a runner-up gap within 2 beta there, pick another seed (no differing block: the '
                                 'streams differ elsewhere)')
        assert gpu == mean                                          # mean without --d2_search runs on the GPU
        assert open(outs['plain'][k], 'rb').read() == open(outs['pick'][k], 'rb').read()
        for tag in ('gpu', 'kdtree', 'mean'):
            assert json.load(open(outs[tag][k] + '.enc.metric.json'))['search_ties'] == 'mean'
        for tag in ('plain', 'pick'):
            assert 'search_ties' not in json.load(open(outs[tag][k] + '.enc.metric.json'))
    assert json.load(open(outs['plain'][1] + '.enc.metric.json')) == json.load(open(outs['pick'][1] + '.enc.metric.json'))
    assert 'decisions differ on most blocks' not in logs['gpu'] and 'decisions differ on most blocks' not in logs['mean']
    for a in outs['gpu'] + outs['kdtree']:
        run('pcc_geo_cnn_v2_amd.decompress_octree', '--input_files', a, '--output_files', a + '.dec.ply', '--checkpoint_dir', ck,
            '--model_config', 'c3p')
        assert len(pc_io.load_pc(a + '.dec.ply')) > 0
