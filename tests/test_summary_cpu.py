"""CPU: the TensorBoard event files of training summaries -- CRC-32C, TensorFlow's bucket limits (numpy and native), the protobuf
wire format against google.protobuf, the collapsed bucket lists, the reader (truncation, corruption, merging) and the tr_plots and
tr_train command lines."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import _summary_ref as SR
from pcc_geo_cnn_v2_amd.utils import tf_summary as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = sys.float_info.max


def test_crc32c_standard_vectors():
    assert T.crc32c(b'123456789') == 0xE3069283
    assert T.crc32c(bytes(32)) == 0x8A9136AA
    assert T.crc32c(b'\xff' * 32) == 0x62A8AB43
    assert T.masked_crc32c(struct.pack('<Q', 24)) == 0x224B7FA3
    assert T.masked_crc32c(b'some payload') == SR.masked_crc(b'some payload')


def test_bucket_limits():
    lim = T.default_bucket_limits()
    assert lim.dtype == np.float64 and lim.shape == (1551,) and int((lim > 0).sum()) == 775
    assert lim[775] == 0.0 and lim[776] == 1e-12 and lim[777] == 1e-12 * 1.1 and lim[-1] == DBL_MAX
    assert np.all(np.diff(lim) > 0) and np.array_equal(lim[:775], -lim[:775:-1])
    v = np.array([0, 1, 0.5, -0.5, 1e-13, -1e-13, 1e-12, 3.4e38, -3.4e38], np.float32)
    want = [776, 1066, 1059, 492, 776, 775, 776, 1550, 1]
    h = [int(np.flatnonzero(T.histogram_host(v[i:i + 1])['counts'])[0]) for i in range(len(v))]
    assert h == want


def test_native_bucket_limits_equal_numpy_bit_for_bit():
    from pcc_geo_cnn_v2_amd import _lib, ops
    assert np.array_equal(ops.histogram_limits().view(np.uint64), T.default_bucket_limits().view(np.uint64))
    for name in ('pcc_histogram_limits', 'pcc_tensor_histogram', 'pcc_tensor_histogram_workspace_bytes', 'pcc_occupancy_scores'):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert _lib.lib().pcc_abi_version() == 4


def test_histogram_host_fields():
    a = np.array([0.5, -2.0, np.nan, 0.0, np.inf, 3.0, -np.inf], np.float32)
    h = T.histogram_host(a)
    assert h['num'] == 4 and h['nonfinite'] == 3 and h['min'] == -2.0 and h['max'] == 3.0
    assert h['sum'] == 1.5 and h['sum_squares'] == 13.25 and int(h['counts'].sum()) == 4 and h['counts'].dtype == np.uint64
    e = T.histogram_host(np.zeros((0,), np.float32))
    assert e['num'] == 0 and e['min'] == DBL_MAX and e['max'] == -DBL_MAX and e['sum'] == 0.0


def test_encode_histogram_collapses_empty_runs():
    lim = T.default_bucket_limits()
    counts = np.zeros(1551, np.uint64)
    counts[[3, 4, 900]] = [7, 2, 5]
    e = T.encode_histogram(dict(counts=counts, num=14, min=-1.0, max=2.0, sum=3.0, sum_squares=9.0))
    assert e['bucket_limit'] == [lim[2], lim[3], lim[4], lim[899], lim[900], DBL_MAX]
    assert e['bucket'] == [0.0, 7.0, 2.0, 0.0, 5.0, 0.0]
    assert (e['num'], e['min'], e['max'], e['sum'], e['sum_squares']) == (14.0, -1.0, 2.0, 3.0, 9.0)
    e = T.encode_histogram(T.histogram_host(np.zeros((0,), np.float32)))
    assert e['bucket_limit'] == [DBL_MAX] and e['bucket'] == [0.0]
    # a count in the first and in the last bucket: no run before / after
    counts = np.zeros(1551, np.uint64)
    counts[[0, 1550]] = 1
    e = T.encode_histogram(dict(counts=counts, num=2, min=0, max=0, sum=0, sum_squares=0))
    assert e['bucket_limit'] == [lim[0], lim[1549], lim[1550]] and e['bucket'] == [1.0, 0.0, 1.0]


def _sample_values(seed):
    rng = np.random.default_rng(seed)
    return {'loss': 1.25, 'mbpov/total': float(np.float32(0.1)), 'bc/precision': float('nan'),
            'y': T.histogram_host(rng.normal(0, 3, 1000).astype(np.float32)),
            'x': T.histogram_host((rng.random(500) < .1).astype(np.float32))}


def test_event_file_parses_with_google_protobuf(tmp_path):
    vals = [_sample_values(0), _sample_values(1)]
    with T.EventFileWriter(str(tmp_path), wall_time=1700000000.5, hostname='box') as w:
        w.add_summary(vals[0], 1, wall_time=1700000001.0)
        w.add_summary(vals[1], 1 << 40, wall_time=1700000002.0)
    assert os.path.basename(w.path) == 'events.out.tfevents.1700000000.box'
    evs = SR.parse_events(w.path)
    assert len(evs) == 3
    assert evs[0].file_version == 'brain.Event:2' and evs[0].wall_time == 1700000000.5 and len(evs[0].summary.value) == 0
    for e, v, step, wall in zip(evs[1:], vals, (1, 1 << 40), (1700000001.0, 1700000002.0)):
        assert e.step == step and e.wall_time == wall and e.file_version == ''
        assert [x.tag for x in e.summary.value] == list(v)
        for x in e.summary.value:
            want = v[x.tag]
            if isinstance(want, dict):
                assert x.HasField('histo')
                enc = T.encode_histogram(want)
                h = x.histo
                assert (h.min, h.max, h.num, h.sum, h.sum_squares) == (want['min'], want['max'], float(want['num']), want['sum'],
                                                                       want['sum_squares'])
                assert list(h.bucket_limit) == enc['bucket_limit'] and list(h.bucket) == enc['bucket']
                assert sum(h.bucket) == want['num'] and len(h.bucket) < 200
            elif math.isnan(want):
                assert math.isnan(x.simple_value)
            else:
                assert x.simple_value == np.float32(want)


def test_a_new_writer_opens_a_new_file(tmp_path):
    a = T.EventFileWriter(str(tmp_path), wall_time=1700000000, hostname='box')
    b = T.EventFileWriter(str(tmp_path), wall_time=1700000000, hostname='box')
    a.close(), b.close()
    assert a.path != b.path and T.event_files(str(tmp_path)) == [a.path, b.path]


def _write(dirname, steps, fn, **kw):
    with T.EventFileWriter(str(dirname), **kw) as w:
        for s in steps:
            w.add_summary(fn(s), s)
    return w.path


def test_read_events_round_trip(tmp_path):
    vals = _sample_values(2)
    path = _write(tmp_path, [5, 7], lambda s: vals)
    got = list(T.read_events(path))
    assert [g[0] for g in got] == [5, 7] and repr(list(T.read_events(str(tmp_path)))) == repr(got)     # repr: NaN != NaN
    for _, _, v in got:
        assert list(v) == list(vals)
        assert v['loss'] == 1.25 and v['mbpov/total'] == float(np.float32(0.1)) and math.isnan(v['bc/precision'])
        enc = T.encode_histogram(vals['y'])
        assert v['y'] == enc
    assert T.tags(str(tmp_path)) == {'loss': 'scalar', 'mbpov/total': 'scalar', 'bc/precision': 'scalar', 'y': 'histogram',
                                     'x': 'histogram'}


def test_truncated_last_record_ends_quietly(tmp_path):
    path = _write(tmp_path, [1, 2, 3], lambda s: {'loss': float(s)})
    raw = open(path, 'rb').read()
    recs = SR.records(path)
    last = 16 + len(recs[-1])
    for cut in (1, 5, last - 14, last - 1):          # inside the trailing CRC, the payload, the header
        open(path, 'wb').write(raw[:len(raw) - cut])
        assert [(s, v['loss']) for s, _, v in T.read_events(path)] == [(1, 1.0), (2, 2.0)]


def test_flipped_payload_byte_raises(tmp_path):
    path = _write(tmp_path, [1, 2], lambda s: {'loss': float(s)})
    raw = bytearray(open(path, 'rb').read())
    first = 16 + len(SR.records(path)[0])
    raw[first + 12 + 3] ^= 0x10                     # a payload byte of the second record
    open(path, 'wb').write(bytes(raw))
    with pytest.raises(ValueError, match='corrupt'):
        list(T.read_events(path))
    raw[first + 12 + 3] ^= 0x10
    raw[first + 2] ^= 0x01                          # a length byte
    open(path, 'wb').write(bytes(raw))
    with pytest.raises(ValueError, match='corrupt'):
        list(T.read_events(path))


def test_scalars_merge_files_and_the_later_record_wins(tmp_path):
    _write(tmp_path, [1, 3, 5], lambda s: {'loss': float(s), 'y': T.histogram_host(np.ones(3, np.float32))}, wall_time=1700000000,
           hostname='box')
    _write(tmp_path, [3, 5, 7], lambda s: {'loss': 10.0 * s}, wall_time=1700000100, hostname='box')
    assert len(T.event_files(str(tmp_path))) == 2
    assert T.scalars(str(tmp_path), 'loss') == [(1, 1.0), (3, 30.0), (5, 50.0), (7, 70.0)]
    assert T.scalars(str(tmp_path), 'y') == [] and T.scalars(str(tmp_path), 'absent') == []


def _cli(module, *args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, '-m', module] + [str(a) for a in args], cwd=ROOT, env=env, check=True,
                          capture_output=True, text=True, timeout=600)


def test_tr_plots_writes_figures_and_the_numbers(tmp_path):
    import csv
    f = {'runA': lambda s: {'loss': 1.0 / s, 'mbpov/total': 0.5 * s, 'y': T.histogram_host(np.ones(2, np.float32))},
         'runB': lambda s: {'loss': 2.0 / s, 'mbpov/total': 0.25 * s}}
    steps = {'runA': [1, 101, 201], 'runB': [1, 101]}
    for name in f:
        _write(tmp_path / name / 'train', steps[name], f[name])
        _write(tmp_path / name / 'val', [500], lambda s: {'loss': 9.0})
    out = tmp_path / 'plots'
    _cli('pcc_geo_cnn_v2_amd.tr_plots', tmp_path / 'runA', tmp_path / 'runB', '--out', out, '--yscale', 'log')
    assert sorted(os.listdir(out)) == sorted(f'{t}.{e}' for t in ('loss', 'mbpov_total') for e in ('csv', 'pdf', 'png'))
    assert open(out / 'loss.png', 'rb').read(8) == b'\x89PNG\r\n\x1a\n' and open(out / 'loss.pdf', 'rb').read(5) == b'%PDF-'
    for tag, stem in (('loss', 'loss'), ('mbpov/total', 'mbpov_total')):
        rows = list(csv.reader(open(out / f'{stem}.csv')))
        assert rows[0] == ['step', 'runA', 'runB'] and [int(r[0]) for r in rows[1:]] == [1, 101, 201]
        for r in rows[1:]:
            s = int(r[0])
            assert float(r[1]) == float(np.float32(f['runA'](s)[tag]))
            assert (float(r[2]) == float(np.float32(f['runB'](s)[tag]))) if s in steps['runB'] else r[2] == ''
    out2 = tmp_path / 'plots_val'
    _cli('pcc_geo_cnn_v2_amd.tr_plots', tmp_path / 'runA', '--out', out2, '--tags', 'loss', '--split', 'val')
    assert list(csv.reader(open(out2 / 'loss.csv'))) == [['step', 'runA'], ['500', '9.0']]
    assert sorted(os.listdir(out2)) == ['loss.csv', 'loss.pdf', 'loss.png']


def test_tr_train_help_lists_summary_interval():
    r = _cli('pcc_geo_cnn_v2_amd.tr_train', '--help')
    assert '--summary_interval' in r.stdout and '100' in r.stdout
