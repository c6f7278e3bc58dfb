"""The latent step without a GPU: the ladder, the stream tag and the step strings, the refusals, and the cost model of
the rate ladder against the real host range coder."""
import io
import os
import re

import numpy as np
import pytest

import _latent_step_ref as R
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import model_syntax as MS
from pcc_geo_cnn_v2_amd import model_types as MT
from pcc_geo_cnn_v2_amd import ops
from pcc_geo_cnn_v2_amd import stream_layers as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 'pcc_geo_cnn_v2_amd/k6/sw0000/fp32'
NEW = ('pcc_quantize_step_pack', 'pcc_index_pack_step', 'pcc_unpack_dequantize_step', 'pcc_rate_ladder')

# The gaps between the real range coder's string and the cost model's sum over the streams of test_cost_model_against_the_host_range_coder,
# measured once (DESIGN.md 4.21 quotes them).  They are properties of these streams, not bounds: the string's excess grows with the bits
# coded on frequency-1 bins of narrow rows.  Largest 8 len - bits: MEASURED_OVER_BITS (32768 symbols of N(0, 2) on the four narrowest rows);
# largest bits - 8 len: MEASURED_UNDER_BITS (no string was shorter than the sum; the closest came within that many bits).  The largest
# ratio (8 len - bits - 24) / bits is MEASURED_OVER_PPM parts per million.  Each absolute gate is the value plus 8 bits: the coder's
# termination depends on the final range state.
MEASURED_OVER_BITS = 278.540
MEASURED_UNDER_BITS = 0.0
MEASURED_OVER_PPM = 938.2
TERMINATION_BITS = 8.0


# ---- the ladder ---------------------------------------------------------------------------------------------------------------------------
def test_latent_step_is_the_formula_exact_in_float32():
    for q in range(64):
        want = (8 + (q & 7)) * 2.0 ** ((q >> 3) - 5)
        got = MS.latent_step(q)
        assert isinstance(got, float) and got == want == R.latent_step(q)
        assert float(np.float32(got)) == got                                      # survives float32 unchanged
    assert MS.latent_step(16) == 1.0 and MS.latent_step(0) == 0.25 and MS.latent_step(63) == 60.0
    assert MS.latent_step(np.int64(24)) == 2.0
    assert all(MS.latent_step(q + 1) > MS.latent_step(q) for q in range(63))
    for bad in (-1, 64, 1.0, True, None, '16'):
        with pytest.raises(AssertionError, match='latent_step'):
            MS.latent_step(bad)


# ---- tag and strings ----------------------------------------------------------------------------------------------------------------------
def test_stream_tag_round_trips_with_the_step_part():
    for coder, mid in (('range', ''), ('rans', '/rans1')):
        tag = MS.stream_tag(BASE, coder, step=True)
        assert tag == f'{BASE}{mid}/qs1'
        assert MS.split_stream_tag(tag) == (BASE, coder, ('qs1',))
        assert MS.stream_layers(tag, BASE) == (coder, ('qs1',))
        # the existing calls and results are unchanged
        assert MS.stream_tag(BASE, coder) == MS.stream_tag(BASE, coder, False, False) == f'{BASE}{mid}'
        assert MS.stream_tag(BASE, coder, True) == f'{BASE}{mid}/occ1' and MS.stream_tag(BASE, coder, count=True) == f'{BASE}{mid}/cnt1'
        assert MS.split_stream_tag(f'{BASE}{mid}') == (BASE, coder, ())
        assert MS.split_stream_tag(f'{BASE}{mid}/occ1') == (BASE, coder, ('occ1',))
        assert MS.split_stream_tag(f'{BASE}{mid}/cnt1') == (BASE, coder, ('cnt1',))
        for layer in ('occ1', 'cnt1'):                                             # the fixed order is parsed, and refused in this build
            with pytest.raises(RuntimeError, match='qs1'):
                MS.split_stream_tag(f'{BASE}{mid}/qs1/{layer}')
            with pytest.raises(RuntimeError, match='qs1'):
                MS.stream_layers(f'{BASE}{mid}/qs1/{layer}', BASE)
    for kw in (dict(lossless=True), dict(count=True)):
        with pytest.raises(AssertionError, match='qs1'):
            MS.stream_tag(BASE, 'range', step=True, **kw)
    assert MS.split_stream_tag(None) == (None, None, ()) and MS.split_stream_tag('other/tag') == ('other/tag', None, ())
    with pytest.raises(RuntimeError):
        MS.split_stream_tag(f'{BASE}/qs2')
    with pytest.raises(RuntimeError):                                              # the step part comes behind the coder part, not before it
        MS.split_stream_tag(f'{BASE}/qs1/rans1')


def _model(config='c3p', **kw):
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    m = ModelConfigType[config].build(batch_size=2, **kw)
    m.x_shape = [1, 1, 64, 64, 64]
    return m


def test_container_round_trip_with_the_step_string_and_malformed_ones():
    rng = np.random.default_rng(3)
    qs = [0, 16, 37, 63]
    blocks = [((rng.bytes(40 + b), rng.bytes(7), MS.step_to_bytes(q)), 100 + b) for b, q in enumerate(qs)]
    raw = MS.save_compressed_file([1, 0, 1], blocks, 128, 1, strict=True)
    res, level, binstr, back = MS.load_compressed_file(io.BytesIO(raw))
    assert (res, level, binstr.tolist()) == (128, 1, [1, 0, 1])
    assert [(tuple(s), t) for s, t in back] == [(tuple(s), t) for s, t in blocks]
    m = _model()
    read = SL.layer_values('qs1', back, m.n_strings)
    assert read == qs and all(type(q) is int for q in read) and np.array(read, np.uint8).tolist() == qs      # (one byte each: uint8 holds them)
    assert [MS.step_from_bytes(MS.step_to_bytes(q), 0) for q in range(64)] == list(range(64))
    for bad, match in [(b'', 'block 2.*0 bytes'), (b'\x10\x10', 'block 2.*2 bytes'), (bytes([64]), 'block 2.*64'), (bytes([255]), 'block 2.*255')]:
        broken = list(back)
        broken[2] = ((back[2][0][0], back[2][0][1], bad), back[2][1])
        with pytest.raises(RuntimeError, match=match):
            SL.layer_values('qs1', broken, m.n_strings)
        with pytest.raises(RuntimeError, match=match):                          # ... which is how the decoder reads them, before a context is made
            m.decompress_block_range(None, broken, [64, 64, 64], layers='step')
    with pytest.raises(RuntimeError, match='block 1.*2 strings'):
        SL.layer_values('qs1', [back[0], (back[1][0][:2], 0)], m.n_strings)
    with pytest.raises(RuntimeError, match='hyperprior'):
        _model('c1').decompress_block_range(None, back, [64, 64, 64], layers='step')
    with pytest.raises(AssertionError, match='latent_step'):
        MS.step_to_bytes(64)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _parse(*extra, config='c3p'):
    from pcc_geo_cnn_v2_amd import compress_octree
    return compress_octree.build_parser().parse_args(
        ['--input_files', '/nonexistent/in.ply', '--output_files', '/nonexistent/out.bin', '--checkpoint_dir', '/nonexistent/ckpt',
         '--model_config', config, '--resolution', '128', '--octree_level', '1', '--opt_metrics', 'd1_mse', *extra])


def test_flags_parse_on_both_clis():
    from pcc_geo_cnn_v2_amd import ev_experiment
    a = _parse()
    assert a.latent_step is None and a.target_bpp is None
    assert _parse('--latent_step', '24').latent_step == 24 and _parse('--target_bpp', '0.75').target_bpp == 0.75
    ev = ['--output_dir', 'o', '--model_dir', 'm', '--model_config', 'c3p', '--pc_name', 'p', '--input_pc', 'i', '--opt_metrics', 'd1_mse',
          '--max_deltas', 'inf']
    e = ev_experiment.build_parser().parse_args(ev)
    assert e.latent_step is None and e.target_bpp is None
    e = ev_experiment.build_parser().parse_args(ev + ['--latent_step', '8'])
    assert e.latent_step == 8
    assert ev_experiment.build_parser().parse_args(ev + ['--target_bpp', '1.5']).target_bpp == 1.5


@pytest.mark.parametrize('flag', [('--latent_step', '24'), ('--target_bpp', '1.0')], ids=['latent_step', 'target_bpp'])
@pytest.mark.parametrize('extra,config,world,match', [
    ((), 'c1', '1', 'hyperprior'), (('--precision', 'fp16'), 'c3p', '1', '--precision fp16'), ((), 'c3p', '2', 'single-process'),
    (('--lossless',), 'c3p', '1', '--lossless'), (('--count_threshold',), 'c3p', '1', '--count_threshold'),
    (('--count_search',), 'c3p', '1', '--count_search')])
def test_cli_refuses_before_the_gpu_is_touched(monkeypatch, flag, extra, config, world, match):
    """compress() itself on parsed arguments: the refusal comes before the input is read, the process group joined or a context made"""
    from pcc_geo_cnn_v2_amd import compress_octree
    monkeypatch.setenv('WORLD_SIZE', world)
    monkeypatch.setattr(ops, 'get_context', lambda *a, **k: pytest.fail('a context was asked for'))
    with pytest.raises(AssertionError, match=f'{flag[0]}.*{match}'):
        compress_octree.compress(_parse(*extra, *flag, config=config))


def test_cli_refuses_the_target_with_rans_or_a_step_and_bad_values(monkeypatch):
    from pcc_geo_cnn_v2_amd import compress_octree
    monkeypatch.setenv('WORLD_SIZE', '1')
    monkeypatch.setattr(ops, 'get_context', lambda *a, **k: pytest.fail('a context was asked for'))
    for extra, match in [(('--target_bpp', '1.0', '--entropy_coder', 'rans'), '--target_bpp.*--entropy_coder rans'),
                         (('--target_bpp', '1.0', '--latent_step', '16'), 'drop --latent_step or --target_bpp'),
                         (('--target_bpp', '0'), '--target_bpp.*above 0'), (('--target_bpp', 'nan'), '--target_bpp.*finite'),
                         (('--latent_step', '64'), r'--latent_step.*\[0, 63\]'), (('--latent_step', '-1'), r'--latent_step.*\[0, 63\]')]:
        with pytest.raises(AssertionError, match=match):
            compress_octree.compress(_parse(*extra))


def test_model_refuses_before_a_context_is_made(monkeypatch):
    from pcc_geo_cnn_v2_amd import sharding
    def steps(latent_step=None, target_bpp=None, **kw):
        return SL.plan_encode(latent_step=latent_step, target_bpp=target_bpp, **kw).steps
    assert steps() is None
    assert steps(None, None, version=1, precision='fp16', world=4, entropy_coder='rans') is None            # off: nothing to refuse
    assert steps(None, None, entry='encode_block_range', version=1, precision='fp16', lossless=True, fixed_threshold=True, entropy_coder='rans') is None
    assert steps(16, n_blocks=3).tolist() == [16, 16, 16] and steps(16, n_blocks=3).dtype == np.uint8
    assert steps([0, 16, 37], n_blocks=3).tolist() == [0, 16, 37]
    assert steps(None, 1.5) is None and steps(16, entropy_coder='rans') is not None
    for kw, match in [(dict(version=1), 'hyperprior'), (dict(precision='fp16'), '--precision fp16'), (dict(world=2), 'single-process'),
                      (dict(lossless=True), '--lossless'), (dict(count_scale=1.0), '--count_threshold'), (dict(count_search=(0.5, 2.0, 3)), '--count_search')]:
        with pytest.raises(AssertionError, match=f'latent_step.*{match}'):
            steps(16, **kw)
        with pytest.raises(AssertionError, match=f'target_bpp.*{match}'):
            steps(None, 1.0, **kw)
    with pytest.raises(AssertionError, match='target_bpp.*--entropy_coder rans'):
        steps(None, 1.0, entropy_coder='rans')
    with pytest.raises(AssertionError, match='--latent_step or --target_bpp'):
        steps(16, 1.0)
    for bad in (64, -1, 1.5, [16, 64], [[16]], []):
        with pytest.raises(AssertionError, match='latent_step'):
            steps(bad, n_blocks=2)
    with pytest.raises(AssertionError, match='3 ladder indexes for 2 blocks'):
        steps([1, 2, 3], n_blocks=2)
    for bad in (0, -1.0, np.inf, np.nan, 'x', True):
        with pytest.raises(AssertionError, match='target_bpp'):
            steps(None, bad)
    # the model's own entry points refuse before a context is made: no GPU here, and sess = None would create the default one
    monkeypatch.setattr(ops, 'get_context', lambda *a, **k: pytest.fail('a context was asked for'))
    blocks = [np.zeros((4, 3), np.float32)]
    for m, match in [(_model('c1'), 'hyperprior'), (_model(precision='fp16'), '--precision fp16'), (_model(lossless=True), '--lossless')]:
        with pytest.raises(AssertionError, match=f'latent_step.*{match}'):
            m.encode_block_range(None, blocks, 128, latent_step=16)
        with pytest.raises(AssertionError, match=f'latent_step.*{match}'):
            m.compress_blocks(None, blocks, [], blocks[0], 128, 1, latent_step=16)
        with pytest.raises(AssertionError, match=f'target_bpp.*{match}'):
            m.compress_blocks(None, blocks, [], blocks[0], 128, 1, target_bpp=1.0)
    m = _model()
    for kw, match in [(dict(count_scale=1.0), '--count_threshold'), (dict(count_search=(0.5, 2.0, 3)), '--count_search')]:
        with pytest.raises(AssertionError, match=f'latent_step.*{match}'):
            m.encode_block_range(None, blocks, 128, latent_step=16, **kw)
        with pytest.raises(AssertionError, match=f'target_bpp.*{match}'):
            m.compress_blocks(None, blocks, [], blocks[0], 128, 1, target_bpp=1.0, **kw)
    with pytest.raises(AssertionError, match='--latent_step or --target_bpp'):
        m.compress_blocks(None, blocks, [], blocks[0], 128, 1, latent_step=16, target_bpp=1.0)
    with pytest.raises(AssertionError, match='2 ladder indexes for 1 blocks'):
        m.encode_block_range(None, blocks, 128, latent_step=[16, 16])
    with pytest.raises(AssertionError, match='target_bpp.*--entropy_coder rans'):
        _model(entropy_coder='rans').compress_blocks(None, blocks, [], blocks[0], 128, 1, target_bpp=1.0)
    monkeypatch.setattr(sharding, 'world_info', lambda: (0, 2))
    with pytest.raises(AssertionError, match='latent_step.*single-process'):
        m.compress_blocks(None, blocks, [], blocks[0], 128, 1, latent_step=16)
    with pytest.raises(AssertionError, match='qs1.*one process'):
        m.decompress_blocks(None, [], [64, 64, 64], layers='step')


def test_rate_point_record_carries_the_step_and_the_target(tmp_path):
    """compress_octree._write_rate_point on the info dict compress_blocks returns under a target: the keys of .enc.metric.json, the tag in
    the gzip header, and the container as the decoder reads it back (no GPU: the strings are made up)"""
    import gzip
    import json
    from pcc_geo_cnn_v2_amd import compress_octree as CO
    rng = np.random.default_rng(4)
    blocks = [np.zeros((5, 3)), np.zeros((7, 3))]
    streams = [((rng.bytes(30), rng.bytes(6), MS.step_to_bytes(21)), 128) for _ in blocks]
    tag = MS.stream_tag(BASE, 'range', step=True)
    info = dict(metrics={'d1_psnr': 40.5, 'd1_mse': 0.25}, numerics_tag=tag, latent_step=21,
                rate_target=dict(target_bpp=0.75, budget_bytes=123.4, predicted_bytes=77, predictions=list(range(64))))
    out = str(tmp_path / 'o' / 'x.ply.bin')
    CO._write_rate_point(out, None, [1], streams, info, _parse('--target_bpp', '0.75'), blocks, [])
    rec = json.load(open(out + '.enc.metric.json'))
    with gzip.open(out, 'rb') as f:
        payload = f.read()
    assert rec['latent_step'] == 21 and rec['latent_step_size'] == MS.latent_step(21) == 1.625 and rec['codec_numerics'] == tag
    assert rec['target_bpp'] == 0.75 and rec['predicted_bytes'] == 77 and rec['container_bytes'] == len(payload)
    assert rec['d1_psnr'] == 40.5 and 'predictions' not in rec
    assert MS.read_gzip_tag(out) == tag and MS.stream_layers(MS.read_gzip_tag(out), BASE) == ('range', ('qs1',))
    assert SL.layer_values('qs1', MS.load_compressed_file(io.BytesIO(payload))[3], _model().n_strings) == [21, 21]
    # a plain step: no target keys; per-block steps: lists; no step: none of the keys
    info2 = dict(metrics={'d1_psnr': 40.5}, numerics_tag=tag, latent_step=[0, 37])
    CO._write_rate_point(out, None, [1], streams, info2, _parse(), blocks, [])
    rec = json.load(open(out + '.enc.metric.json'))
    assert rec['latent_step'] == [0, 37] and rec['latent_step_size'] == [0.25, 6.5] and not {'target_bpp', 'predicted_bytes', 'container_bytes'} & set(rec)
    CO._write_rate_point(out, None, [1], streams, dict(metrics={'d1_psnr': 40.5}, numerics_tag=BASE), _parse(), blocks, [])
    assert set(json.load(open(out + '.enc.metric.json'))) == {'d1_psnr', 'codec_numerics'}


# ---- the cost model -----------------------------------------------------------------------------------------------------------------------
def _gaussian():
    from pcc_geo_cnn_v2_amd.entropy_models import GaussianConditional, scale_table
    return GaussianConditional(scale_table(0.11, 256, 64))              # as CompressionModelV2 builds it


def test_cost_table_is_the_restatement_and_refuses_a_zero_frequency():
    gc = _gaussian()
    cost = ops.cost16_table(gc.quantized_cdf, gc.cdf_length, gc.precision)
    assert cost.dtype == np.uint32 and cost.shape == (64, gc.quantized_cdf.shape[1] - 1)
    assert np.array_equal(cost, R.cost_table(gc.quantized_cdf, gc.cdf_length, gc.precision))
    assert cost[:, 0].min() > 0 and cost.max() <= 16 * 65536                   # a frequency of 1 costs `precision` bits
    one = ops.cost16_table(np.array([[0, 1 << 15, 1 << 16]]), [3])
    assert one.tolist() == [[65536, 65536]]
    with pytest.raises(AssertionError, match='frequency 0'):
        ops.cost16_table(np.array([[0, 1 << 15, 1 << 15, 1 << 16]]), [4])
    with pytest.raises(AssertionError, match='cdf_size'):
        ops.cost16_table(np.array([[0, 1 << 15, 1 << 16]]), [4])


def _streams(gc):
    """(name, symbols, rows): all symbols in range; about 1 % escapes on each side; the narrowest row alone; n = 1; n = 32768"""
    rng = np.random.default_rng(21)
    tab, off, m = gc.scale_table, gc.offset.astype(np.int64), gc.cdf_length.astype(np.int64) - 2

    def draw(n, rows=None):
        rows = rng.integers(0, 64, n) if rows is None else rows
        sym = np.rint(rng.standard_normal(n) * tab[rows]).astype(np.int64)
        return np.clip(sym, off[rows], off[rows] + m[rows] - 1), rows

    out = []
    for n in (1000, 5000):
        sym, rows = draw(n)
        out.append((f'in-range-{n}', sym, rows))
    sym, rows = draw(6000)
    esc = rng.permutation(6000)[:120]
    far = rng.integers(0, 3, 120) * rng.integers(1, 40000, 120) + rng.integers(0, 4, 120)       # near and far escapes: one to five digits
    sym[esc[:60]] = off[rows[esc[:60]]] - 1 - far[:60]
    sym[esc[60:]] = off[rows[esc[60:]]] + m[rows[esc[60:]]] + far[60:]
    out.append(('escapes-1pc-each-side', sym, rows))
    sym, rows = draw(4000, np.zeros(4000, np.int64))
    out.append(('narrowest-row', sym, rows))
    for row in (0, 63):
        sym, rows = draw(1, np.full(1, row))
        out.append((f'n1-row{row}', sym, rows))
    sym, rows = draw(32768)
    out.append(('n32768', sym, rows))
    # low entropy on the narrow rows, 32768 symbols (the latents of one 64^3 block of c3p): most symbols that are not 0 sit on bins of
    # frequency 1, where the coder's truncated interval arithmetic loses most against the ideal cost
    for top, scale in ((4, 0.6), (4, 1.0), (4, 2.0), (8, 0.6), (8, 1.0), (16, 2.0)):
        rows = rng.integers(0, top, 32768)
        sym = np.rint(rng.standard_normal(32768) * scale).astype(np.int64)
        out.append((f'n32768-rows-below-{top}-N(0,{scale})', np.clip(sym, off[rows], off[rows] + m[rows] - 1), rows))
    rows = np.zeros(32768, np.int64)
    out.append(('n32768-frequency-1-only', np.where(rng.integers(0, 2, 32768) == 1, 1, -1).astype(np.int64), rows))
    return out


def test_cost_model_against_the_host_range_coder():
    """8 * len(string) of pcc_range_encode_batch (not code under test) against the sum over the product's own cost table (ops.cost16_table,
    equal to the restatement's), over seeded streams on the table the model builds.  Every gap is printed; the absolute gaps are gated
    at their measured values (top of the file) plus 8 bits, and the margin the rate target adds to its prediction
    (model_types.rate_margin_bits16) covers every stream."""
    gc = _gaussian()
    cost = ops.cost16_table(gc.quantized_cdf, gc.cdf_length, gc.precision)
    assert np.array_equal(cost, R.cost_table(gc.quantized_cdf, gc.cdf_length, gc.precision))
    assert gc.offset[0] == -1 and gc.quantized_cdf[0, 1] - gc.quantized_cdf[0, 0] == 1                   # (symbol -1 of the narrowest row: a frequency-1 bin)
    over = under = ppm = -np.inf
    for name, sym, rows in _streams(gc):
        (string,) = ops.range_encode_batch(gc.table, [sym.astype(np.int32)], [rows.astype(np.int32)])
        (back,) = ops.range_decode_batch(gc.table, [string], [sym.size], [rows.astype(np.int32)])
        assert np.array_equal(back, sym), name
        bits16 = int(R.symbol_bits16(sym, rows, cost, gc.cdf_length, gc.offset, 4).sum())
        bits = bits16 / 65536.0
        gap = 8 * len(string) - bits
        rel = 1e6 * (gap - MT.RATE_MARGIN_FIXED_BITS) / bits if bits > 0 else -np.inf
        print(f'{name}: n {sym.size}, string {8 * len(string)} bits, model {bits:.3f} bits, string - model {gap:+.3f} ({gap / sym.size:.5f} per symbol, '
              f'{rel:.0f} ppm of the bits beyond the fixed {MT.RATE_MARGIN_FIXED_BITS})')
        over, under, ppm = max(over, gap), max(under, -gap), max(ppm, rel)
        assert (8 * len(string) << 16) - bits16 <= MT.rate_margin_bits16(bits16), f'{name}: the margin of the rate target does not cover this stream'
    print(f'largest 8 len - bits {over:.3f}, largest bits - 8 len {under:.3f}, largest ratio beyond the fixed part {ppm:.0f} ppm')
    assert over <= MEASURED_OVER_BITS + TERMINATION_BITS
    assert under <= MEASURED_UNDER_BITS + TERMINATION_BITS
    assert MT.RATE_MARGIN_FIXED_BITS == 16 + TERMINATION_BITS and MT.RATE_MARGIN_PPM >= MEASURED_OVER_PPM
    assert int(MT.rate_margin_bits16(np.int64(0))) == 24 << 16 and int(MT.rate_margin_bits16(np.int64(10 ** 6))) == (24 << 16) + MT.RATE_MARGIN_PPM


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_new_symbols():
    header = open(os.path.join(ROOT, 'include', 'pcc_geo.h')).read()
    lib = L.lib()
    for name in NEW:
        assert re.search(rf'\bint\s+{name}\s*\(', header), f'{name} is not declared in include/pcc_geo.h'
        assert name in L.EXPORTS and hasattr(lib, name)
    assert len(lib.pcc_quantize_step_pack.argtypes) == len(lib.pcc_quantize_pack.argtypes) + 1
    assert len(lib.pcc_index_pack_step.argtypes) == len(lib.pcc_index_pack.argtypes) + 1
    assert len(lib.pcc_unpack_dequantize_step.argtypes) == len(lib.pcc_unpack_dequantize.argtypes) + 1
    assert len(lib.pcc_rate_ladder.argtypes) == 19
    assert L.ABI_VERSION == 4 and lib.pcc_abi_version() == 4
    # argument checks that need no device: a NULL context is refused before anything is launched
    assert lib.pcc_rate_ladder(None, None, None, 1, 8, 8, None, 64, 0, None, 1, None, 2, None, None, 4, 0, None, None) == L.PCC_ERR_ARG
    assert lib.pcc_quantize_step_pack(None, None, None, None, None, 1, 8, 8, 0, 1, None, 2, None, None, None) == L.PCC_ERR_ARG
