"""CPU-only: the host restatement of the occ1 string format (tests/_occ_ref.py) round-trips, its bucket rule sits where DESIGN.md 4.19
puts it, the words stay below the ideal code length, and the tag / CLI / ABI carry the lossless layer."""
import io
import math
import os
import re

import numpy as np
import pytest

import _occ_ref as O
from pcc_geo_cnn_v2_amd import _lib, model_syntax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(O.cases())
NAMES = ('pcc_occ_stream_cap', 'pcc_occ_workspace_bytes', 'pcc_occ_check_strings', 'pcc_occ_encode_batch', 'pcc_occ_decode_batch')


def test_reference_roundtrips_every_input_and_the_words_stay_below_the_ideal():
    """2 n_words <= ideal_bytes + 4 L + 2 on every input (an observation of the restatement, not a theorem: DESIGN.md 4.19 records the
    worst slack seen), and every string fits the capacity the ABI states."""
    worst = -math.inf
    for name, x, o in CASES:
        info = {}
        s = O.encode(x, o, info=info)
        assert np.array_equal(O.decode(x, s), o), name
        assert len(s) == 1 + 2 * info['used'] + 4 * info['lanes'] + 2 * info['n_words'] <= O.stream_cap(x.size), name
        assert s[0] == int(math.log2(info['lanes'])) and info['n_words'] <= info['m'] <= x.size
        ideal = O.ideal_bytes(x, o)
        slack = 2 * info['n_words'] - ideal
        worst = max(worst, slack)
        if x.size > 4097:
            print(f'{name}: {len(s)} bytes, L {info["lanes"]}, m {info["m"]}, words {2 * info["n_words"]} B, ideal {ideal:.1f} B')
        assert 2 * info['n_words'] <= ideal + 4 * info['lanes'] + 2, name
    print(f'worst 2 n_words - ideal_bytes over {len(CASES)} inputs: {worst:.2f} B')


@pytest.mark.parametrize('lanes', [1, 2, 64])
def test_reference_roundtrips_forced_lane_counts(lanes):
    for name, x, o in CASES:
        if x.size > 4097:
            continue
        s = O.encode(x, o, lanes=lanes)
        assert s[0] == lanes.bit_length() - 1 and np.array_equal(O.decode(x, s), o), name
    assert O.encode(np.zeros(0, np.float32), np.zeros(0, bool), lanes=lanes) == b''
    assert O.decode(np.zeros(0, np.float32), b'').size == 0


def test_all_empty_and_skipped_buckets_cost_no_symbols():
    x = np.random.default_rng(0).random(500).astype(np.float32)
    info = {}
    s = O.encode(x, np.zeros(500, bool), info=info)
    assert info['m'] == 0 and info['lanes'] == 1 and info['n_words'] == 0
    assert s == bytes([0]) + b'\0\0' * info['used'] + (1 << 16).to_bytes(4, 'little')
    # one occupied voxel: only its bucket is coded
    o = np.zeros(500, bool)
    o[17] = True
    O.encode(x, o, info=info)
    assert info['m'] == int((O.buckets(x) == O.buckets(x)[17]).sum())


def test_bucket_rule_at_its_edges():
    f32 = np.float32
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    down = lambda v: np.nextafter(f32(v), f32(-np.inf))
    b = lambda v: int(O.buckets(np.array([v], np.float32))[0])
    assert [b(v) for v in (0.0, -0.0, -1.0, np.nan, -np.inf, down(0.0))] == [0] * 6
    assert b(up(0.0)) == 1 and b(np.float32(1e-30)) == 1
    assert [b(v) for v in (1.0, 2.0, np.inf, up(1.0))] == [31] * 4
    # the largest fp32 below 1: its product is 30 - 1.79e-6, which fp32 rounds to 30 - 2^-19, so 1 + 29: the clamp to 30 is a guard that
    # no fp32 input reaches (a product that rounded to 30 would land on 31, the bucket of x_hat >= 1)
    assert b(down(1.0)) == 30 and f32(down(1.0)) * f32(30.0) == down(30.0)
    for k in range(1, 30):
        for v in (down(f32(k / 30)), f32(k / 30), up(f32(k / 30))):
            want = min(30, 1 + int(f32(v) * f32(30.0)))           # one fp32 multiply, then truncation
            assert b(v) == want and want in (k, k + 1), (k, v)
        assert b(up(f32(k / 30))) == k + 1 and b(down(f32(k / 30))) == k
    assert b(f32(0.5)) == 16 and b(f32(1 / 30) / 2) == 1 and b(f32(29.5 / 30)) == 30


def test_entries_are_rounded_shares_clamped_into_the_coder_range():
    assert O.entry(0, 10) == 0 and O.entry(10, 10) == 65535 and O.entry(1, 1 << 28) == 1
    assert O.entry(1, 2) == 32768 and O.entry(1, 3) == (65536 + 1) // 3 and O.entry(2, 3) == (2 * 65536 + 1) // 3
    assert O.entry((1 << 28) - 1, 1 << 28) == 65535


def test_reference_refuses_damaged_strings():
    for name, x, o in CASES:
        if x.size > 4097 or x.size < 63:
            continue
        s = O.encode(x, o)
        for bad in (s[:-1], s[:-2], s + b'\0\0', bytes([7]) + s[1:], b''):
            with pytest.raises(O.OccCorrupt):
                O.decode(x, bad)
                pytest.fail(name)


def test_tags_name_the_layer_and_the_coder_functions_answer_as_before():
    base = 'pcc_geo_cnn_v2_amd/k7/sw0000/fp32'
    M = model_syntax
    assert M.stream_tag(base, 'range', False) == base and M.stream_tag(base, 'rans', False) == base + '/rans1'
    assert M.stream_tag(base, 'range', True) == base + '/occ1' and M.stream_tag(base, 'rans', True) == base + '/rans1/occ1'
    assert M.split_stream_tag(base) == (base, 'range', ())
    assert M.split_stream_tag(base + '/rans1') == (base, 'rans', ())
    assert M.split_stream_tag(base + '/occ1') == (base, 'range', ('occ1',))
    assert M.split_stream_tag(base + '/rans1/occ1') == (base, 'rans', ('occ1',))
    assert M.split_stream_tag(None) == (None, None, ()) and M.split_stream_tag('other') == ('other', None, ())
    for bad in ('/occ9', '/occ1/rans1', '/rans9/occ1', '/occ1/occ1', '/rans1/occ1/x'):
        with pytest.raises(RuntimeError):
            M.split_stream_tag(base + bad)
    assert M.stream_layers(base + '/rans1/occ1', base) == ('rans', ('occ1',)) and M.stream_layers(base, base) == ('range', ())
    assert M.stream_layers(None, base, override='rans') == ('rans', ())
    with pytest.raises(RuntimeError, match='codec numerics'):
        M.stream_layers('pcc_geo_cnn_v2_amd/k7/sw0008/fp32/occ1', base)
    # the coder-only functions: an occ1 tag is still refused by them (what a build before the layer does with such a file) ...
    for tag in (base + '/occ1', base + '/rans1/occ1'):
        with pytest.raises(RuntimeError, match='occ1'):
            M.split_coder_tag(tag)
        with pytest.raises(RuntimeError, match='occ1'):
            M.stream_coder(tag, base)
    # ... and every assertion of tests/test_rans_cpu.py's tag test still describes them
    assert M.coder_tag(base, 'range') == base and M.coder_tag(base, 'rans') == base + '/rans1'
    assert M.split_coder_tag(base) == (base, 'range')
    assert M.split_coder_tag(base + '/rans1') == (base, 'rans')
    assert M.split_coder_tag(None) == (None, None)
    with pytest.raises(RuntimeError, match='rans9'):
        M.split_coder_tag(base + '/rans9')
    assert M.stream_coder(base + '/rans1', base) == 'rans'
    assert M.stream_coder(base, base, override='rans') == 'range'
    assert M.stream_coder(None, base) == 'range' and M.stream_coder(None, base, override='rans') == 'rans'
    with pytest.raises(RuntimeError, match='codec numerics'):
        M.stream_coder('pcc_geo_cnn_v2_amd/k7/sw0008/fp32/rans1', base)


def test_parsers_carry_the_flags_and_lossless_is_single_process():
    from pcc_geo_cnn_v2_amd import compress_octree, decompress_octree
    common = ['--input_files', 'a', '--output_files', 'b', '--checkpoint_dir', 'c', '--model_config', 'c3p']
    assert compress_octree.build_parser().parse_args(common).lossless is False
    assert compress_octree.build_parser().parse_args(common + ['--lossless']).lossless is True
    assert decompress_octree.build_parser().parse_args(common).base_only is False
    assert decompress_octree.build_parser().parse_args(common + ['--base_only']).base_only is True
    assert 'base' in compress_octree.build_parser().format_help().split('--dec_files')[2].split('--checkpoint_dir')[0]
    parse = compress_octree.build_parser().parse_args
    compress_octree.check_encode_options(parse(common), 1)
    compress_octree.check_encode_options(parse(common), 8)
    assert compress_octree.check_encode_options(parse(common + ['--lossless']), 1).layers == ('occ1',)
    with pytest.raises(AssertionError, match='single-process'):
        compress_octree.check_encode_options(parse(common + ['--lossless']), 2)


def test_model_keyword():
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    assert ModelConfigType['c3p'].build().lossless is False
    assert ModelConfigType['c1'].build(lossless=True).lossless is True


def test_the_abi_names_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'pcc_geo.h')).read()
    for name in NAMES:
        assert name in _lib.EXPORTS, name
        assert re.search(r'\b(size_t|int) ' + name + r'\(', header), name
    lib = _lib.lib()
    assert lib.pcc_abi_version() == _lib.ABI_VERSION
    for n in (0, 1, 64, 64 ** 3):
        assert lib.pcc_occ_stream_cap(n) == O.stream_cap(n)
    assert lib.pcc_occ_workspace_bytes(3, 64) >= 3 * 6 * 64 and lib.pcc_occ_workspace_bytes(0, 64) == 0
    assert len(lib.pcc_occ_encode_batch.argtypes) == 15 and len(lib.pcc_occ_decode_batch.argtypes) == 16


def test_host_check_reads_the_lane_byte_and_the_length_only():
    """pcc_occ_check_strings: parity and L.  `used` and m depend on x_hat, so a string cut by two bytes passes here and fails on the device."""
    import ctypes as C
    lib = _lib.lib()
    name, x, o = next(c for c in CASES if c[0] == 'n4097-half-uniform')
    good = O.encode(x, o)

    def check(strings, n):
        blob = np.frombuffer(b''.join(strings) + b'\0', np.uint8).copy()
        lens = np.array([len(s) for s in strings], np.int32)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        return lib.pcc_occ_check_strings(len(strings), blob.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                                         lens.ctypes.data_as(C.c_void_p), n)
    assert check([good, good], x.size) == 0
    assert check([good[:-2]], x.size) == 0 and check([good + b'\0\0'], x.size) == 0
    for bad in (good[:-1], bytes([7]) + good[1:], b'', good[:3]):
        assert check([good, bad], x.size) == _lib.PCC_ERR_CORRUPT
    assert check([b''], 0) == 0 and check([good], 0) == _lib.PCC_ERR_CORRUPT
    assert check([], 5) == 0


def test_container_roundtrips_three_strings_per_block_and_names_the_flag_when_one_is_too_long():
    rng = np.random.default_rng(0)
    blocks = [((rng.bytes(40), rng.bytes(7), rng.bytes(int(k))), int(rng.integers(0, 256))) for k in (0, 1, 300, 65535)]
    raw = model_syntax.save_compressed_file([1, 255], blocks, 128, 1, strict=True)
    res, level, binstr, got = model_syntax.load_compressed_file(io.BytesIO(raw))
    assert (res, level, binstr.tolist()) == (128, 1, [1, 255]) and raw[5] == 3
    assert [(tuple(s), t) for s, t in got] == blocks
    two = [((a, b), t) for (a, b, _), t in blocks]
    assert model_syntax.save_compressed_file([1, 255], two, 128, 1, strict=True)[5] == 2
    with pytest.raises(AssertionError, match='--lossless'):
        model_syntax.save_compressed_file([1, 255], [((b'a', b'b', bytes(65536)), 3)], 128, 1, strict=True)
