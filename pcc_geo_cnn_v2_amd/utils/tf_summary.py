"""TensorBoard event files without TensorFlow: histograms with TensorFlow's bucket semantics, a protobuf wire encoder for the four
messages a summary needs, TFRecord framing with masked CRC-32C, and a reader.

What src/tr_train.py:45-47,99-104,128-141 writes through tf.summary.FileWriter and src/ut_tensorboard_plots.py reads back.  No
TensorFlow, tensorboard or protobuf import.  The bucket limits, the field numbers and the framing below are written from the public
formats; no TensorFlow was at hand to compare files with (parity unpinned).

Field numbers (proto3 wire types: double = fixed64, float = fixed32, int64 = varint, string / message / packed = length-delimited):
  Event          wall_time = 1 double, step = 2 int64, file_version = 3 string, summary = 5 message
  Summary        value = 1 repeated message
  Summary.Value  tag = 1 string, simple_value = 2 float, histo = 5 message
  HistogramProto min = 1, max = 2, num = 3, sum = 4, sum_squares = 5 double; bucket_limit = 6, bucket = 7 packed repeated double

TFRecord framing: u64 length | u32 masked_crc32c(length bytes) | data | u32 masked_crc32c(data), little-endian;
mask(c) = ((c >> 15 | c << 17) + 0xa282ead8) mod 2^32; CRC-32C is Castagnoli's (reflected polynomial 0x82F63B78).
"""
import glob
import os
import socket
import struct
import time

import numpy as np

NUM_BUCKETS = 1551
DBL_MAX = float(np.finfo(np.float64).max)
FILE_VERSION = 'brain.Event:2'

_LIMITS = None


def default_bucket_limits():
    """TensorFlow histogram.cc: positive limits by repeated IEEE multiplication (1e-12, x 1.1 while < 1e20), then DBL_MAX; the table
    is [-reversed positives, 0.0, positives]: 1551 float64."""
    global _LIMITS
    if _LIMITS is None:
        pos = []
        v = 1e-12
        while v < 1e20:
            pos.append(v)
            v *= 1.1
        pos.append(DBL_MAX)
        pos = np.array(pos, np.float64)
        _LIMITS = np.concatenate((-pos[::-1], [0.0], pos))
        _LIMITS.setflags(write=False)
    return _LIMITS


def histogram_host(array):
    """The histogram of a float32 array on the host, field for field what pcc_tensor_histogram fills: counts (uint64, bucket =
    upper_bound(limits, float64(v))), num, nonfinite (NaN and +-Inf, excluded from the rest), min, max (DBL_MAX / -DBL_MAX when
    empty), sum, sum_squares (float64; the summation order is numpy's)."""
    a = np.asarray(array, np.float32).reshape(-1)
    fin = np.isfinite(a)
    v = a[fin].astype(np.float64)
    limits = default_bucket_limits()
    counts = np.bincount(np.searchsorted(limits, v, side='right'), minlength=NUM_BUCKETS).astype(np.uint64)
    return dict(counts=counts, num=int(v.size), nonfinite=int(a.size - v.size),
                min=float(v.min()) if v.size else DBL_MAX, max=float(v.max()) if v.size else -DBL_MAX,
                sum=float(v.sum()), sum_squares=float(np.dot(v, v)))


def encode_histogram(h, limits=None):
    """TensorFlow's Histogram::EncodeToProto: (bucket_limit, bucket) lists in which every run of empty buckets is one entry that
    carries the run's LAST limit and a zero count.  Returns a dict with min, max, num, sum, sum_squares, bucket_limit, bucket."""
    limits = default_bucket_limits() if limits is None else limits
    counts = np.asarray(h['counts'])
    out_l, out_c = [], []
    i, n = 0, len(counts)
    while i < n:
        c = float(counts[i])
        if c <= 0:
            while i + 1 < n and counts[i + 1] <= 0:
                i += 1
        out_l.append(float(limits[i]))
        out_c.append(c)
        i += 1
    return dict(min=float(h['min']), max=float(h['max']), num=float(h['num']), sum=float(h['sum']),
                sum_squares=float(h['sum_squares']), bucket_limit=out_l, bucket=out_c)


# ---------------------------------------------------------------------------------------------------------------------------------
# CRC-32C and TFRecord framing
# ---------------------------------------------------------------------------------------------------------------------------------
def _crc_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        t.append(c)
    return t


_CRC = _crc_table()


def crc32c(data):
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def masked_crc32c(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def frame_record(data):
    head = struct.pack('<Q', len(data))
    return head + struct.pack('<I', masked_crc32c(head)) + data + struct.pack('<I', masked_crc32c(data))


# ---------------------------------------------------------------------------------------------------------------------------------
# protobuf wire format
# ---------------------------------------------------------------------------------------------------------------------------------
def _varint(n):
    n &= 0xFFFFFFFFFFFFFFFF             # int64: negatives as ten-byte two's complement
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        if n:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _key(field, wire):
    return _varint(field << 3 | wire)


def _f_double(field, v):
    return _key(field, 1) + struct.pack('<d', v)


def _f_float(field, v):
    return _key(field, 5) + np.float32(v).tobytes()


def _f_bytes(field, b):
    return _key(field, 2) + _varint(len(b)) + b


def _f_packed_doubles(field, vs):
    return _f_bytes(field, np.asarray(vs, '<f8').tobytes()) if len(vs) else b''


def encode_histogram_proto(e):
    """HistogramProto bytes of an encode_histogram() dictionary."""
    return (_f_double(1, e['min']) + _f_double(2, e['max']) + _f_double(3, e['num']) + _f_double(4, e['sum'])
            + _f_double(5, e['sum_squares']) + _f_packed_doubles(6, e['bucket_limit']) + _f_packed_doubles(7, e['bucket']))


def encode_value(tag, value):
    """Summary.Value: a number becomes simple_value (float32, NaN kept), a histogram dictionary (counts, ...) becomes histo."""
    body = _f_bytes(1, tag.encode('utf-8'))
    if isinstance(value, dict):
        e = value if 'bucket' in value else encode_histogram(value)
        return body + _f_bytes(5, encode_histogram_proto(e))
    return body + _f_float(2, value)


def encode_summary(values):
    """Summary of {tag: float | histogram}, in the dictionary's order."""
    return b''.join(_f_bytes(1, encode_value(t, v)) for t, v in values.items())


def encode_event(wall_time, step=0, summary=None, file_version=None):
    out = _f_double(1, wall_time)
    if step:
        out += _key(2, 0) + _varint(int(step))
    if file_version is not None:
        out += _f_bytes(3, file_version.encode('utf-8'))
    if summary is not None:
        out += _f_bytes(5, summary)
    return out


class EventFileWriter:
    """events.out.tfevents.<unix seconds, 10 digits>.<hostname> in `logdir`: every instance opens a new file (as tf.summary.FileWriter
    does at every process start) whose first record is the file version; each event is flushed as it is written."""

    def __init__(self, logdir, wall_time=None, hostname=None):
        os.makedirs(logdir, exist_ok=True)
        now = time.time() if wall_time is None else wall_time
        base = os.path.join(logdir, f'events.out.tfevents.{int(now):010d}.{hostname or socket.gethostname()}')
        path, k = base, 0
        while os.path.exists(path):           # two writers within one second: keep both files, in name order
            k += 1
            path = f'{base}.{k}'
        self.path = path
        self._f = open(path, 'xb')
        self._write(encode_event(now, file_version=FILE_VERSION))

    def _write(self, event):
        self._f.write(frame_record(event))
        self._f.flush()

    def add_summary(self, values, step, wall_time=None):
        """values: {tag: float | histogram dictionary of histogram_host / ops.tensor_histogram}."""
        self._write(encode_event(time.time() if wall_time is None else wall_time, step, encode_summary(values)))

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# reader
# ---------------------------------------------------------------------------------------------------------------------------------
def _read_varint(b, i):
    n, shift = 0, 0
    while True:
        c = b[i]
        i += 1
        n |= (c & 0x7F) << shift
        if not c & 0x80:
            return n, i
        shift += 7


def _fields(b):
    """(field, wire type, value) of a message: varint -> int, fixed64 / fixed32 / length-delimited -> bytes."""
    i = 0
    while i < len(b):
        k, i = _read_varint(b, i)
        f, w = k >> 3, k & 7
        if w == 0:
            v, i = _read_varint(b, i)
        elif w == 1:
            v, i = b[i:i + 8], i + 8
        elif w == 5:
            v, i = b[i:i + 4], i + 4
        elif w == 2:
            n, i = _read_varint(b, i)
            v, i = b[i:i + n], i + n
        else:
            raise ValueError(f'unsupported wire type {w}')
        yield f, w, v


def _decode_histogram(b):
    names = {1: 'min', 2: 'max', 3: 'num', 4: 'sum', 5: 'sum_squares'}
    h = dict(min=0.0, max=0.0, num=0.0, sum=0.0, sum_squares=0.0, bucket_limit=[], bucket=[])
    for f, w, v in _fields(b):
        if f in names and w == 1:
            h[names[f]] = struct.unpack('<d', v)[0]
        elif f in (6, 7):
            vals = np.frombuffer(v, '<f8').tolist() if w == 2 else [struct.unpack('<d', v)[0]]
            h['bucket_limit' if f == 6 else 'bucket'].extend(vals)
    return h


def _decode_event(b):
    step, wall, values = 0, 0.0, {}
    for f, w, v in _fields(b):
        if f == 1 and w == 1:
            wall = struct.unpack('<d', v)[0]
        elif f == 2 and w == 0:
            step = v - (1 << 64) if v >> 63 else v
        elif f == 5 and w == 2:
            for f2, w2, val in _fields(v):
                if f2 != 1 or w2 != 2:
                    continue
                tag, x = None, None
                for f3, w3, v3 in _fields(val):
                    if f3 == 1 and w3 == 2:
                        tag = v3.decode('utf-8')
                    elif f3 == 2 and w3 == 5:
                        x = float(np.frombuffer(v3, '<f4')[0])
                    elif f3 == 5 and w3 == 2:
                        x = _decode_histogram(v3)
                if tag is not None and x is not None:
                    values[tag] = x
    return step, wall, values


def event_files(path_or_dir):
    """The event files of a directory in name order (the name carries the start time), or the one file given."""
    if os.path.isdir(path_or_dir):
        return sorted(glob.glob(os.path.join(glob.escape(path_or_dir), 'events.out.tfevents.*')))
    return [path_or_dir]


def read_records(path):
    """The payloads of one TFRecord file.  Both CRCs are verified (ValueError on a mismatch); a last record cut short -- what a
    killed run leaves -- ends the iteration quietly."""
    with open(path, 'rb') as f:
        while True:
            head = f.read(12)
            if len(head) < 12:
                return
            n, crc = struct.unpack('<QI', head)
            if crc != masked_crc32c(head[:8]):
                raise ValueError(f'{path}: corrupt record length')
            body = f.read(n + 4)
            if len(body) < n + 4:
                return
            if struct.unpack('<I', body[n:])[0] != masked_crc32c(body[:n]):
                raise ValueError(f'{path}: corrupt record payload')
            yield body[:n]


def read_events(path_or_dir):
    """Yields (step, wall_time, {tag: float | histogram dictionary}) of every summary event, file after file in name order."""
    for path in event_files(path_or_dir):
        for rec in read_records(path):
            step, wall, values = _decode_event(rec)
            if values:
                yield step, wall, values


def scalars(logdir, tag):
    """[(step, value)] of a scalar tag over every file of a directory, sorted by step; for a repeated step the later record wins
    (a resumed run replays the steps after its last validation)."""
    out = {}
    for step, _, values in read_events(logdir):
        if tag in values and not isinstance(values[tag], dict):
            out[step] = values[tag]
    return sorted(out.items())


def tags(logdir):
    """{tag: 'scalar' | 'histogram'} over every file of a directory."""
    out = {}
    for _, _, values in read_events(logdir):
        for t, v in values.items():
            out[t] = 'histogram' if isinstance(v, dict) else 'scalar'
    return out
