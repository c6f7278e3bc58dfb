"""GPU: training summaries -- pcc_tensor_histogram against the numpy restatement (bucket edges, contention inputs, non-finite values,
sizes from 0 to 32 x 64^3), its double sums against math.fsum, pcc_occupancy_scores against numpy, train.summarize on real c3p and
c1 forwards, and the event files a Trainer writes (steps, values, no effect on model.npz / log.jsonl, resumed runs)."""
import json
import math

import numpy as np
import pytest
import torch

from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ops, train
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
from pcc_geo_cnn_v2_amd.utils import tf_summary as T

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max
SIZES = (0, 1, 63, 64, 65, 2 ** 20 + 17, 32 * 64 ** 3)


@pytest.fixture(scope='module')
def pctx():
    return train.training_context(torch.device('cuda', 0))


def _check(pctx, a, what):
    """Device histogram of float32 array `a` against histogram_host and math.fsum; returns the device histogram."""
    a = np.ascontiguousarray(a, np.float32)
    t = torch.from_numpy(a).cuda()
    h = ops.tensor_histogram(pctx, t)
    ref = T.histogram_host(a)
    assert h['counts'].dtype == np.uint64 and h['counts'].shape == (1551,)
    bad = np.flatnonzero(h['counts'] != ref['counts'])
    assert bad.size == 0, f'{what}: counts differ in buckets {bad[:8]}: {h["counts"][bad[:8]]} != {ref["counts"][bad[:8]]}'
    assert (h['num'], h['nonfinite']) == (ref['num'], ref['nonfinite']), what
    assert np.array_equal([h['min'], h['max']], [ref['min'], ref['max']]), (what, h['min'], h['max'], ref['min'], ref['max'])
    v = a[np.isfinite(a)].astype(np.float64)
    n = v.size
    for key, terms in (('sum', v), ('sum_squares', v * v)):          # squares of float32 values are exact in float64
        exact = math.fsum(terms.tolist())
        bound = n * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())   # worst case of any double summation order
        err = abs(h[key] - exact)
        print(f'{what} n={a.size} {key}: err {err:.3g} bound {bound:.3g}')
        assert err <= bound, f'{what}: {key} {h[key]!r} vs {exact!r}: err {err:.3g} > bound {bound:.3g}'
    raw = [ops.tensor_histograms_launch(pctx, [t])[0].cpu().numpy().tobytes() for _ in range(2)]
    assert raw[0] == raw[1], f'{what}: two calls differ'
    return h


def _edge_values():
    """For 200 limits spread from 1e-12 to the largest limit below FLT_MAX, both signs: the float32 values just below, at and just
    above float32(limit); +-0, denormals, +-FLT_MAX."""
    lim = T.default_bucket_limits()
    pos = lim[776:]
    pos = pos[pos < float(FLT_MAX)]
    pick = pos[np.unique(np.linspace(0, len(pos) - 1, 200).round().astype(int))]
    assert len(pick) == 200 and pick[0] == 1e-12 and pick[-1] == pos[-1]
    at = np.concatenate((pick, -pick)).astype(np.float32)
    vals = np.concatenate((np.nextafter(at, np.float32(-np.inf)), at, np.nextafter(at, np.float32(np.inf))))
    tiny = np.float32(1e-45)
    extra = np.array([0.0, -0.0, tiny, -tiny, 1e-40, -1e-40, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny, FLT_MAX, -FLT_MAX],
                     np.float32)
    out = np.concatenate((vals, extra)).astype(np.float32)
    assert np.all(np.isfinite(out))
    return out


def test_histogram_bucket_edges(pctx):
    v = _edge_values()
    h = _check(pctx, v, 'edges')
    assert h['num'] == v.size and h['min'] == -float(FLT_MAX) and h['max'] == float(FLT_MAX)
    # and one value at a time, so that a wrong bucket cannot hide behind another value's count
    hs = ops.tensor_histograms(pctx, [torch.from_numpy(v[i:i + 1].copy()).cuda() for i in range(0, v.size, 7)])
    want = np.searchsorted(T.default_bucket_limits(), v[::7].astype(np.float64), side='right')
    assert [int(np.flatnonzero(x['counts'])[0]) for x in hs] == want.tolist()


def _gen(kind, n, rng):
    if kind == 'binary':
        return (rng.random(n) < .03).astype(np.float32)
    if kind == 'near_binary':
        return np.where(rng.random(n) < .03, np.float32(.999), np.float32(.001)).astype(np.float32)
    if kind.startswith('normal'):
        return (rng.standard_normal(n, dtype=np.float32) * np.float32(float(kind[6:]))).astype(np.float32)
    assert kind == 'nonfinite'
    a = rng.standard_normal(n, dtype=np.float32)
    if n:
        k = max(1, n // 1000)
        for bad in (np.nan, np.inf, -np.inf):
            a[rng.integers(0, n, k)] = bad
    return a


@pytest.mark.parametrize('kind', ['binary', 'near_binary', 'normal1e-6', 'normal1', 'normal1e6', 'nonfinite'])
def test_histogram_matches_host(pctx, kind):
    rng = np.random.default_rng(len(kind))
    for n in SIZES:
        a = _gen(kind, n, rng)
        h = _check(pctx, a, kind)
        if kind == 'nonfinite' and n >= 63:
            assert h['nonfinite'] > 0 and h['num'] + h['nonfinite'] == n
        if n == 0:
            assert h['num'] == 0 and h['sum'] == 0.0 and h['min'] == float(np.finfo(np.float64).max)


def test_histogram_of_an_unaligned_view_has_the_same_bytes(pctx):
    a = np.random.default_rng(5).standard_normal(2 ** 16 + 3).astype(np.float32)
    base = torch.from_numpy(np.concatenate(([np.float32(9)], a))).cuda()
    view = base[1:]                                   # contiguous, 4 bytes off a 16-byte boundary
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    r0 = ops.tensor_histograms_launch(pctx, [view])[0].cpu().numpy().tobytes()
    r1 = ops.tensor_histograms_launch(pctx, [torch.from_numpy(a).cuda()])[0].cpu().numpy().tobytes()
    assert r0 == r1
    _check(pctx, a, 'aligned copy')


def _occupancy_ref(x, xt):
    """src/model_types.py:91-94 on uint8 tensors, wrap-around included."""
    q, qt = (np.rint(np.clip(v, 0, 1)).astype(np.uint8) for v in (x, xt))
    one = np.uint8(1)
    return dict(tp=int(np.count_nonzero(qt * q)), tn=int(np.count_nonzero((qt - one) * (q - one))),
                fp=int(np.count_nonzero(qt * (q - one))), fn=int(np.count_nonzero((qt - one) * q)), num_occupied=int(q.sum(dtype=np.int64)))


def test_occupancy_scores_match_numpy(pctx):
    f = np.float32
    special = np.array([0.5, 1.5, np.nextafter(f(.5), f(0)), np.nextafter(f(.5), f(1)), np.nextafter(f(1.5), f(0)),
                        np.nextafter(f(1.5), f(2)), -1.0, -0.0, 0.0, 1.0, 2.5, 1e30, -1e30, 0.49999, 0.50001, np.nextafter(f(1), f(0)),
                        np.nextafter(f(1), f(2)), np.nextafter(f(0), f(1)), np.nextafter(f(0), f(-1))], f)
    rng = np.random.default_rng(7)
    for n in (len(special) ** 2, 1, 65, 2 ** 20 + 17):
        if n == len(special) ** 2:
            x, xt = (g.reshape(-1).copy() for g in np.meshgrid(special, special, indexing='ij'))
        else:
            x = (rng.random(n) < .05).astype(f)
            xt = rng.uniform(-.5, 1.5, n).astype(f)
            xt[:min(n, len(special))] = special[:min(n, len(special))]
        got, quant = ops.occupancy_scores(pctx, torch.from_numpy(x).cuda(), torch.from_numpy(xt).cuda(), want_quant=True)
        ref = _occupancy_ref(x, xt)
        print('occupancy', n, got)
        assert got == ref
        assert got['tp'] + got['tn'] + got['fp'] + got['fn'] == n and got['num_occupied'] == got['tp'] + got['fn']
        assert np.array_equal(quant.cpu().numpy(), np.rint(np.clip(xt, 0, 1)))
        assert ops.occupancy_scores(pctx, torch.from_numpy(x).cuda(), torch.from_numpy(xt).cuda()) == ref
    e = ops.occupancy_scores(pctx, torch.zeros(0, device='cuda'), torch.zeros(0, device='cuda'))
    assert e == dict(tp=0, tn=0, fp=0, fn=0, num_occupied=0)


def test_exports_name_the_summary_entry_points():
    for name in ('pcc_histogram_limits', 'pcc_tensor_histogram_workspace_bytes', 'pcc_tensor_histogram_slices', 'pcc_tensor_histogram',
                 'pcc_occupancy_scores'):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().pcc_abi_version() == L.ABI_VERSION == 4
    # the number of slices of the double sums depends on n only
    assert [L.lib().pcc_tensor_histogram_slices(n) for n in (0, 1, 4096, 4097, 2 ** 40)] == [1, 1, 1, 2, 1024]


# ---------------------------------------------------------------------------------------------------------------------------------
# train.summarize and the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
SCALARS_V1 = {'loss', 'mbpov/y', 'mbpov/total', 'fl', 'num_occupied_voxels', 'bc/precision', 'bc/recall', 'bc/accuracy',
              'bc/specificity', 'bc/f1_score'}
HIST_V1 = {'y', 'y_tilde', 'x', 'x_tilde', 'x_tilde_quant', 'y_likelihoods', 'log_y_likelihoods'}
HIST_V2 = {'z', 'z_tilde', 'sigma_tilde', 'z_likelihoods', 'log_z_likelihoods'}


def _blocks_dense(n, res, seed):
    """Planes and spherical shells, {0,1} float32 (n, res, res, res)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing='ij'), -1).astype(np.float64)
    out = np.zeros((n, res, res, res), np.float32)
    for i in range(n):
        if i % 2 == 0:
            nrm = rng.normal(size=3)
            nrm /= np.linalg.norm(nrm)
            out[i] = np.abs((g - res / 2) @ nrm - rng.uniform(-res / 6, res / 6)) < .6
        else:
            out[i] = np.abs(np.linalg.norm(g - res / 2 - rng.uniform(-2, 2, 3), axis=-1) - rng.uniform(res / 5, res / 2.5)) < .6
    return out


def _same_histogram(got, a, what):
    ref = T.histogram_host(a)
    assert np.array_equal(got['counts'], ref['counts']), what
    assert (got['num'], got['nonfinite'], got['min'], got['max']) == (ref['num'], 0, ref['min'], ref['max']), what
    v = np.asarray(a, np.float64).reshape(-1)
    for key, terms in (('sum', v), ('sum_squares', v * v)):
        assert abs(got[key] - math.fsum(terms.tolist())) <= v.size * 2.0 ** -53 * math.fsum(np.abs(terms).tolist()), (what, key)


@pytest.mark.parametrize('cfg', ['c3p', 'c1'])
def test_summarize_equals_the_host_restatement(pctx, cfg):
    m = ModelConfigType[cfg].build(seed=3)
    m.compress([1, 1, 16, 16, 16])
    graph = train.TrainGraph(m, pctx)
    v2 = cfg == 'c3p'
    assert graph.v2 == v2
    x = torch.from_numpy(_blocks_dense(2, 16, 4)).cuda()
    gen = torch.Generator(device='cuda')
    gen.manual_seed(5)
    noise = [torch.rand(s, generator=gen, device='cuda') - .5 for s in graph.latent_shapes(tuple(x.shape))]
    with torch.no_grad():
        plain = graph.loss(x, noise, 1e-2)
        out = graph.loss(x, noise, 1e-2, tensors=True)
    assert set(plain) == {'loss', 'fl', 'mbpov'}
    for k in plain:                                   # asking for the tensors changes no number
        assert torch.equal(plain[k], out[k]), k
    s = train.summarize(pctx, out)
    assert set(s) == SCALARS_V1 | HIST_V1 | (HIST_V2 | {'mbpov/z'} if v2 else set())
    host = {k: v.cpu().numpy() for k, v in out['tensors'].items()}
    assert set(host) == (HIST_V1 | (HIST_V2 if v2 else set())) - {'x_tilde_quant'}
    host['x_tilde_quant'] = np.rint(np.clip(host['x_tilde'], 0, 1))
    for k in HIST_V1 | (HIST_V2 if v2 else set()):
        assert isinstance(s[k], dict)
        _same_histogram(s[k], host[k], k)
    assert s['x_tilde_quant']['sum'] == float(host['x_tilde_quant'].sum(dtype=np.float64)) == s['x_tilde_quant']['sum_squares']
    assert s['loss'] == float(out['loss']) and s['fl'] == float(out['fl']) and s['mbpov/total'] == float(out['mbpov'])
    assert s['num_occupied_voxels'] == float(host['x'].sum(dtype=np.float64))
    den = np.float32(-math.log(2)) * np.float32(s['num_occupied_voxels'])
    if v2:
        assert s['mbpov/y'] == float(out['mbpov_y']) and s['mbpov/z'] == float(out['mbpov_z'])
        assert np.float32(s['mbpov/y']) + np.float32(s['mbpov/z']) == np.float32(s['mbpov/total'])
        assert abs(s['mbpov/z'] - host['log_z_likelihoods'].sum(dtype=np.float64) / float(den)) <= 1e-5 * abs(s['mbpov/z'])
    else:
        assert s['mbpov/y'] == s['mbpov/total']
    assert abs(s['mbpov/y'] - host['log_y_likelihoods'].sum(dtype=np.float64) / float(den)) <= 1e-5 * abs(s['mbpov/y'])
    q, qt = host['x'].reshape(-1) > .5, host['x_tilde_quant'].reshape(-1) == 1
    bc = train.binary_classification(int((qt & q).sum()), int((~qt & ~q).sum()), int((qt & ~q).sum()), int((~qt & q).sum()))
    for k, v in bc.items():
        assert s[k] == v or (math.isnan(s[k]) and math.isnan(v)), k


def test_binary_classification_is_float32_and_keeps_nan():
    bc = train.binary_classification(3, 5, 1, 2)
    f = np.float32
    p, r = f(3) / f(4), f(3) / f(5)
    assert bc == {'bc/precision': float(p), 'bc/recall': float(r), 'bc/accuracy': float(f(8) / f(11)),
                  'bc/specificity': float(f(5) / f(6)), 'bc/f1_score': float(f(2) * p * r / (p + r))}
    z = train.binary_classification(0, 10, 0, 0)      # a model collapsed to "all empty" on an empty block
    assert math.isnan(z['bc/precision']) and math.isnan(z['bc/recall']) and math.isnan(z['bc/f1_score'])
    assert z['bc/accuracy'] == 1.0 and z['bc/specificity'] == 1.0


def test_summarize_refuses_non_finite_tensors(pctx):
    x = torch.zeros((1, 4, 4, 4), device='cuda')
    t = {k: torch.ones((1, 4, 4, 4, 1), device='cuda') for k in ('y', 'y_tilde', 'x_tilde', 'y_likelihoods', 'log_y_likelihoods')}
    t['x'] = x
    t['y_tilde'][0, 1, 2, 3, 0] = float('nan')
    one = torch.ones((), device='cuda')
    with pytest.raises(ValueError, match="'y_tilde'"):
        train.summarize(pctx, dict(loss=one, fl=one, mbpov=one, mbpov_y=one, num_occupied_voxels=one, tensors=t))


def _blocks(n, res, seed):
    return [np.argwhere(b > 0) for b in _blocks_dense(n, res, seed)]


def _trainer(ck, data, **kw):
    args = dict(resolution=16, batch_size=2, lmbda=1e-2, validation_interval=3, validation_steps=2, seed=42, log=None)
    args.update(kw)
    return train.Trainer(ModelConfigType['c3p'].build(seed=42), str(ck), data[0], data[1], **args)


def _log_lines(ck):
    return [l for l in open(ck / 'log.jsonl') if 'loss' in l and 'val' not in l]


def test_trainer_writes_event_files_and_changes_nothing_else(tmp_path):
    data = (_blocks(8, 16, 61), _blocks(2, 16, 62))
    _trainer(tmp_path / 'off', data, max_steps=6).run()
    _trainer(tmp_path / 'on', data, max_steps=6, summary_interval=2).run()
    assert not (tmp_path / 'off' / 'train').exists() and not (tmp_path / 'off' / 'val').exists()
    assert (tmp_path / 'off' / 'model.npz').read_bytes() == (tmp_path / 'on' / 'model.npz').read_bytes()
    assert _log_lines(tmp_path / 'off') == _log_lines(tmp_path / 'on') and len(_log_lines(tmp_path / 'on')) == 6
    assert (tmp_path / 'off' / 'log.jsonl').read_bytes() == (tmp_path / 'on' / 'log.jsonl').read_bytes()
    tr, va = str(tmp_path / 'on' / 'train'), str(tmp_path / 'on' / 'val')
    assert len(T.event_files(tr)) == 1 and len(T.event_files(va)) == 1
    events = list(T.read_events(tr))
    assert [e[0] for e in events] == [1, 3, 5]
    recs = {r['step']: r for r in map(json.loads, _log_lines(tmp_path / 'on'))}
    order = train.Batches(data[0], 2, 16, 42)
    counts = [sum(len(data[0][i]) for i in order.next_indices()) for _ in range(6)]
    ulp = lambda v: float(np.spacing(np.float32(abs(v))))
    for step, _, v in events:
        assert set(v) == SCALARS_V1 | HIST_V1 | HIST_V2 | {'mbpov/z'}
        r = recs[step]
        assert v['loss'] == float(np.float32(r['loss'])) and v['fl'] == float(np.float32(r['fl']))
        assert v['mbpov/total'] == float(np.float32(r['mbpov']))
        print('step', step, 'mbpov y z total', v['mbpov/y'], v['mbpov/z'], v['mbpov/total'])
        assert abs(v['mbpov/y'] + v['mbpov/z'] - v['mbpov/total']) <= 2 * ulp(v['mbpov/total'])
        assert v['num_occupied_voxels'] == counts[step - 1]
        assert v['x']['num'] == 2 * 16 ** 3 and v['x']['sum'] == counts[step - 1]
        assert sum(v['y']['bucket']) == v['y']['num'] == sum(v['y_tilde']['bucket']) > 0
    # validations at steps 0, 3 and 6, two batches each, under step + i
    assert [e[0] for e in T.read_events(va)] == [0, 1, 3, 4, 6, 7]
    val = {r['step']: r['val_loss'] for r in map(json.loads, open(tmp_path / 'on' / 'log.jsonl')) if 'val_loss' in r}
    by = dict(T.scalars(va, 'loss'))
    for s in (0, 3, 6):
        assert abs((by[s] + by[s + 1]) / 2 - val[s]) <= 1e-6 * abs(val[s])


def test_cut_and_resumed_run_leaves_two_event_files_and_each_step_once(tmp_path):
    data = (_blocks(8, 16, 31), _blocks(2, 16, 32))
    _trainer(tmp_path / 'full', data, max_steps=8, summary_interval=2).run()
    t = _trainer(tmp_path / 'cut', data, max_steps=8, summary_interval=2)
    step_fn = t.train_step

    def failing(x, **kw):
        if t.step == 5:                   # after the validation (and saves) at step 3
            raise RuntimeError('interrupted')
        return step_fn(x, **kw)
    t.train_step = failing
    with pytest.raises(RuntimeError, match='interrupted'):
        t.run()
    r = _trainer(tmp_path / 'cut', data, max_steps=8, summary_interval=2)
    assert r.step == 3
    r.run()
    assert (tmp_path / 'full' / 'model.npz').read_bytes() == (tmp_path / 'cut' / 'model.npz').read_bytes()
    tr = str(tmp_path / 'cut' / 'train')
    files = T.event_files(tr)
    assert len(files) == 2
    assert [e[0] for e in T.read_events(files[0])] == [1, 3, 5] and [e[0] for e in T.read_events(files[1])] == [5, 7]
    for tag in ('loss', 'mbpov/y', 'bc/accuracy'):
        got = T.scalars(tr, tag)
        assert [s for s, _ in got] == [1, 3, 5, 7]
        assert got == T.scalars(str(tmp_path / 'full' / 'train'), tag)     # the replayed step 5 is the same step
