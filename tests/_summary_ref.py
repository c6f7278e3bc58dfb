"""Independent readers for the summary tests: the four event messages built with google.protobuf from a descriptor written here
(field numbers of the public event.proto / summary.proto), and a TFRecord parser of a few lines of struct."""
import struct

from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

_T = descriptor_pb2.FieldDescriptorProto


def _field(msg, name, number, ftype, label=_T.LABEL_OPTIONAL, type_name=None, packed=None):
    f = msg.field.add()
    f.name, f.number, f.type, f.label = name, number, ftype, label
    if type_name:
        f.type_name = type_name
    if packed is not None:
        f.options.packed = packed
    return f


def _build():
    fd = descriptor_pb2.FileDescriptorProto()
    fd.name, fd.package, fd.syntax = 'summary_ref.proto', 'summary_ref', 'proto3'
    h = fd.message_type.add()
    h.name = 'HistogramProto'
    for i, n in enumerate(('min', 'max', 'num', 'sum', 'sum_squares'), 1):
        _field(h, n, i, _T.TYPE_DOUBLE)
    _field(h, 'bucket_limit', 6, _T.TYPE_DOUBLE, _T.LABEL_REPEATED, packed=True)
    _field(h, 'bucket', 7, _T.TYPE_DOUBLE, _T.LABEL_REPEATED, packed=True)
    s = fd.message_type.add()
    s.name = 'Summary'
    v = s.nested_type.add()
    v.name = 'Value'
    _field(v, 'tag', 1, _T.TYPE_STRING)
    _field(v, 'simple_value', 2, _T.TYPE_FLOAT)
    _field(v, 'histo', 5, _T.TYPE_MESSAGE, type_name='.summary_ref.HistogramProto')
    _field(s, 'value', 1, _T.TYPE_MESSAGE, _T.LABEL_REPEATED, type_name='.summary_ref.Summary.Value')
    e = fd.message_type.add()
    e.name = 'Event'
    _field(e, 'wall_time', 1, _T.TYPE_DOUBLE)
    _field(e, 'step', 2, _T.TYPE_INT64)
    _field(e, 'file_version', 3, _T.TYPE_STRING)
    _field(e, 'summary', 5, _T.TYPE_MESSAGE, type_name='.summary_ref.Summary')
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName('summary_ref.Event'))


Event = _build()


def masked_crc(data):
    """CRC-32C bit by bit (no table), masked as TFRecord does."""
    c = 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    c ^= 0xFFFFFFFF
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def records(path):
    """Payloads of a TFRecord file; asserts the framing and both checksums."""
    raw = open(path, 'rb').read()
    out, i = [], 0
    while i < len(raw):
        n, = struct.unpack_from('<Q', raw, i)
        assert struct.unpack_from('<I', raw, i + 8)[0] == masked_crc(raw[i:i + 8])
        data = raw[i + 12:i + 12 + n]
        assert len(data) == n
        assert struct.unpack_from('<I', raw, i + 12 + n)[0] == masked_crc(data)
        out.append(data)
        i += 16 + n
    assert i == len(raw)
    return out


def parse_events(path):
    evs = []
    for r in records(path):
        e = Event()
        e.ParseFromString(r)
        evs.append(e)
    return evs
