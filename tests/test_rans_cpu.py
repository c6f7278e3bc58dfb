"""CPU-only: the host restatement of the rans1 string format (tests/_rans_ref.py) round-trips, the integer cost never underestimates,
the lane rule's estimate bounds the words, and the numerics tag / CLI parsers carry the entropy coder."""
import math

import numpy as np
import pytest

import _rans_ref as R
from pcc_geo_cnn_v2_amd import model_syntax

LANES = (1, 2, 4, 8, 16, 32, 64)


def gaussian_streams(oracle):
    """the streams of test_range_coder_matches_oracle_bytes_and_roundtrips (tests/test_abi_cpu.py): scale x5 forces escapes"""
    tab = oracle.scale_table()
    cdf, size, off = oracle.gaussian_tables(tab)
    rng = np.random.default_rng(0)
    datas, idxs = [], []
    for s in range(13):
        n = int(rng.integers(0, 6000))
        idx = rng.integers(0, 64, n).astype(np.int32)
        scale = rng.choice([0.3, 1.0, 5.0], n)
        datas.append(np.rint(rng.standard_normal(n) * tab[idx] * scale).astype(np.int32))
        idxs.append(idx)
    datas.append(np.array([2 ** 20, -2 ** 20, 0, 7], np.int32))
    idxs.append(np.array([0, 63, 5, 5], np.int32))
    return (cdf, size, off), datas, idxs


def channel_table(oracle, Cn=8):
    rng = np.random.default_rng(1)
    pmf = rng.random((Cn, 21)).astype(np.float32)
    pmf /= pmf.sum(1, keepdims=True) * 1.01
    cdf = np.zeros((Cn, 23), np.int32)
    for c in range(Cn):
        cdf[c, :23] = oracle.pmf_to_quantized_cdf(np.concatenate([pmf[c], [0.0099]]).astype(np.float32))
    return cdf, np.full(Cn, 23, np.int32), np.full(Cn, -10, np.int32)


def _roundtrip(table, data, index=None, index_mod=0, lanes=0):
    info = {}
    s = R.encode(*table, data, index, index_mod, lanes=lanes, info=info)
    assert np.array_equal(R.decode(*table, s, data.size, index, index_mod), data)
    if data.size:
        assert len(s) <= R.stream_cap(data.size)
        assert s[0] == int(math.log2(info['lanes']))
    return s, info


def test_reference_roundtrips_gaussian_streams_and_the_estimate_bounds_the_words(oracle):
    """2 n_words <= est_bytes for every coded stream: per lane 16 words = 16 + sum of bits - log2(final state) <= sum of bits, and
    cost256 over-estimates the bits."""
    table, datas, idxs = gaussian_streams(oracle)
    for d, i in zip(datas, idxs):
        s, info = _roundtrip(table, d, i)
        if d.size:
            print(f'n {d.size} lanes {info["lanes"]} words {info["n_words"]} est_bytes {info["est_bytes"]} escapes {info["n_escapes"]}')
            assert info['lanes'] == R.lane_rule(info['est_bytes'])
            assert 2 * info['n_words'] <= info['est_bytes']
        else:
            assert s == b''


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65, 127])
def test_reference_roundtrips_every_forced_lane_count(oracle, n):
    table, _, _ = gaussian_streams(oracle)
    rng = np.random.default_rng(n)
    idx = rng.integers(0, 64, n).astype(np.int32)
    data = np.rint(rng.standard_normal(n) * oracle.scale_table()[idx] * rng.choice([0.3, 1.0, 5.0], n)).astype(np.int32)
    seen = set()
    for lanes in (0,) + LANES:
        s, info = _roundtrip(table, data, idx, lanes=lanes)
        seen.add(s)
        if n and lanes:
            assert info['lanes'] == lanes and 2 * info['n_words'] <= info['est_bytes']
    assert len(seen) == (1 if n == 0 else len(LANES))          # (auto picks one of the forced ones)


def test_reference_roundtrips_the_index_mod_mode(oracle):
    table = channel_table(oracle)
    rng = np.random.default_rng(1)
    data = rng.integers(-14, 15, (4 * 4 * 4, 8)).astype(np.int32).reshape(-1)
    for lanes in (0, 1, 8, 64):
        s, info = _roundtrip(table, data, None, 8, lanes=lanes)
        assert 2 * info['n_words'] <= info['est_bytes']
    explicit = R.encode(*table, data, np.arange(data.size, dtype=np.int32) % 8)
    assert explicit == R.encode(*table, data, None, 8)
    assert R.encode(*table, np.zeros(0, np.int32), None, 8) == b''


def test_reference_refuses_damaged_strings(oracle):
    table, datas, idxs = gaussian_streams(oracle)
    d, i = datas[0], idxs[0]
    s = R.encode(*table, d, i, lanes=4)
    for bad in (s[:-1], s[:9], bytes([3]) + s[1:], s[:1] + b'\xff\xff\x7f' + s[2:]):
        with pytest.raises(R.RansCorrupt):
            R.decode(*table, bad, d.size, i)


def test_cost256_never_underestimates():
    for f in range(1, 65536):
        assert R.cost256(f) >= 256 * math.log2(65536 / f), f
    assert R.cost256(1) == 4096 and R.cost256(32768) == 256
    assert [R.lane_rule(e) for e in (0, 127, 128, 255, 256, 8191, 8192, 10 ** 9)] == [1, 1, 1, 1, 2, 32, 64, 64]


def test_tag_helper_splits_the_coder_and_refuses_an_unknown_one():
    base = 'pcc_geo_cnn_v2_amd/k7/sw0000/fp32'
    assert model_syntax.coder_tag(base, 'range') == base and model_syntax.coder_tag(base, 'rans') == base + '/rans1'
    assert model_syntax.split_coder_tag(base) == (base, 'range')
    assert model_syntax.split_coder_tag(base + '/rans1') == (base, 'rans')
    assert model_syntax.split_coder_tag(None) == (None, None)
    with pytest.raises(RuntimeError, match='rans9'):
        model_syntax.split_coder_tag(base + '/rans9')
    assert model_syntax.stream_coder(base + '/rans1', base) == 'rans'
    assert model_syntax.stream_coder(base, base, override='rans') == 'range'         # a tagged stream names its own coder
    assert model_syntax.stream_coder(None, base) == 'range' and model_syntax.stream_coder(None, base, override='rans') == 'rans'
    with pytest.raises(RuntimeError, match='codec numerics'):
        model_syntax.stream_coder('pcc_geo_cnn_v2_amd/k7/sw0008/fp32/rans1', base)   # the rest of the tag is compared as before


def test_both_parsers_accept_the_flag():
    from pcc_geo_cnn_v2_amd import compress_octree, decompress_octree
    common = ['--input_files', 'a', '--output_files', 'b', '--checkpoint_dir', 'c', '--model_config', 'c3p']
    assert compress_octree.build_parser().parse_args(common).entropy_coder == 'range'
    assert compress_octree.build_parser().parse_args(common + ['--entropy_coder', 'rans']).entropy_coder == 'rans'
    assert decompress_octree.build_parser().parse_args(common).entropy_coder is None
    assert decompress_octree.build_parser().parse_args(common + ['--entropy_coder', 'rans']).entropy_coder == 'rans'
    with pytest.raises(SystemExit):
        compress_octree.build_parser().parse_args(common + ['--entropy_coder', 'huffman'])


def test_model_keyword():
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    assert ModelConfigType['c3p'].build().entropy_coder == 'range'
    assert ModelConfigType['c1'].build(entropy_coder='rans').entropy_coder == 'rans'
    with pytest.raises(AssertionError):
        ModelConfigType['c1'].build(entropy_coder='huffman')
