"""The two-piece fp16 arithmetic of conv_wino_f16s.hip / conv_tr2m_f16s.hip as a numpy model (tests/_f16s_model.py) against a float64
direct convolution, on inputs with a dynamic range inside a block (tests/_dynamic_range_cases.py).  Needs no GPU: this is the
accuracy half of DESIGN.md section 4.1; tests/test_dynamic_range_gpu.py holds the kernels to the model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dynamic_range_cases as DC      # noqa: E402
import _f16s_model as M                # noqa: E402

ALL = list(range(len(DC.GEOMS)))
_ROWS = {}


def test_split_keeps_22_bits_or_half_a_denormal_step():
    """x = h + l, h = fp16_rn(y), l = fp16_rn(y - h), y = s x: over fp16's normal range, its denormal range and zero
    |y - h - l| <= max(2^-22 |y|, 2^-25), and y - h is exact in fp32 (h is y's leading bits: the difference needs no more bits than y)."""
    rng = np.random.default_rng(0)
    e = rng.integers(-40, 16, 200000)
    y = np.ldexp(rng.uniform(0.5, 1, e.size), e).astype(np.float32) * rng.choice([-1, 1], e.size).astype(np.float32)
    edge = np.array([0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 65504, 65519.9, 1 + 2.0 ** -11,
                     1 + 2.0 ** -11 + 2.0 ** -23, 2.0 ** -13 + 2.0 ** -24 + 2.0 ** -36, 2.0 ** -149, 2.0 ** -126], np.float32)
    y = np.concatenate([y, edge, -edge])
    h, l = M.split_f16(y)
    y64, h64, l64 = y.astype(np.float64), h.astype(np.float64), l.astype(np.float64)
    assert np.isfinite(h).all() and np.isfinite(l).all()
    assert np.array_equal((y - h).astype(np.float64), y64 - h64)                    # exact in fp32
    assert (np.abs(y64 - h64 - l64) <= np.maximum(M.SPLIT_REL * np.abs(y64), M.SPLIT_ABS)).all()
    # the floor is real: some residual below fp16's normal range does lose bits
    assert (np.abs(y64 - h64 - l64) > M.SPLIT_REL * np.abs(y64)).any()


@pytest.mark.parametrize('i', [0, 1, 2, 3, 4, 5, 6, 16, 22, 27, 28, 34], ids=lambda i: DC.IDS[i])
def test_float64_reference_agrees_with_the_oracle(oracle, i):
    """The reference of these tests is a plain numpy convolution in float64; the suite's oracle (C, double accumulation, one rounding to
    fp32) must agree with it to that rounding: |oracle - ref| <= 2^-24 |ref| + 2^-40 T."""
    inp = DC.inputs(i)
    ref, T = DC.reference(i)
    o = (oracle.conv3d_transpose if inp['transposed'] else oracle.conv3d)(inp['x'], inp['w'], inp['bias'], inp['stride'], inp['relu'])
    if inp['res'] is not None:
        o = o.astype(np.float64) + inp['res']
        assert (np.abs(o - ref) <= 2.0 ** -24 * np.abs(ref - inp['res']) + 2.0 ** -40 * T).all()
    else:
        assert (np.abs(o - ref) <= 2.0 ** -24 * np.abs(ref) + 2.0 ** -40 * T).all()


@pytest.mark.parametrize('i', ALL, ids=lambda i: DC.IDS[i])
def test_model_is_within_its_derived_bound_of_the_float64_convolution(i):
    """Per output, |model - exact| <= bound with no fitted constant.  u = 2^-24.  The model differs from the exact convolution only in
    its operands (its sums are float64), and every operand error is known:

      weights   Winograd: U32 = fl32(G g G^T): |U32 - U| <= u / (1 - u) |U32|.  Then the split of su U32 (the scale is exact):
                |U32 - (Uh + Ul) / su| <= rU = max(2^-22 |U32|, 2^-25 / su) (the split property above).  eU = their sum; the march splits the
                fp32 taps themselves: eW = max(2^-22 |w|, 2^-25 / su).
      inputs    Winograd: V32 = fl(fl(a -+ b) -+ fl(c -+ d)), two rounded adds per entry, so
                |V32 - V| <= u (|a| + |b| + |c| + |d|) + u (1 + u) (|a| + .. + |d|) = (2 u + u^2) Vabs,   Vabs = |B^T| |d| |B|;
                then the split of s V32: max(2^-22 |V32|, 2^-25 / s).  eV = their sum.  The march splits s x: eX = max(2^-22 |x|, 2^-25 / s).
      product   |U^ V^ - U V| <= eU |V| + |U^| eV <= eU (|V32| + (2 u + u^2) Vabs) + (|U32| + rU) eV, summed over the z taps and cin in the
                transform domain and pushed through |A^T| .. |A|; the bias, the residual and the power-of-two scales are exact, ReLU
                is 1-Lipschitz.  2^-50 A covers the model's own float64 sums.

    The term 2^-25 / s is the block-relative floor: s = 2^12 / 2^floor(log2 max|x|) (2^14 for the march), so the floor is 2^-37 (2^-39)
    of the block's maximum per operand, whatever the operand's own size.  The fp32-operand model (the exact kernels) obeys the same
    bound without the split terms."""
    ref, T = DC.reference(i)
    inp = DC.inputs(i)
    row = {}
    for name, pieces in (('two-piece', 2), ('fp32', None)):
        m = DC.model(i, pieces)
        err = np.abs(m['value'] - ref)
        assert np.isfinite(m['value']).all() and np.isfinite(m['bound']).all()
        bad = err > m['bound']
        assert not bad.any(), (name, int(bad.sum()), float((err / np.maximum(m['bound'], 1e-300)).max()))
        assert (m['A'] >= np.abs(m['value']) * (1 - 1e-12)).all()
        row[name] = DC.far_ratio(i, m['value'][0])
    _ROWS[i] = row
    print(f"{DC.IDS[i]}: far outputs of block 0, max err / T: two-piece model {row['two-piece']:.2e}, fp32-operand model {row['fp32']:.2e}")


@pytest.mark.parametrize('i', [k for k in ALL if DC.GEOMS[k]['case'] == 'hot_voxel_20'], ids=lambda i: DC.IDS[i])
def test_bound_is_not_vacuous_where_the_floor_rules(i):
    """hot_voxel_20, outputs whose tiles (taps) hold no hot voxel: the floor term is all that matters there, and the model's real error
    reaches at least 1/256 of the bound on some output."""
    ref, _ = DC.reference(i)
    m = DC.model(i)
    far = DC.far_mask(i) & (m['bound'][0] > 0)
    r = (np.abs(m['value'][0] - ref[0])[far] / m['bound'][0][far]).max()
    print(f'{DC.IDS[i]}: max err / bound over the far outputs = {r:.3f}')
    assert 1.0 / 256 <= r <= 1.0


@pytest.mark.parametrize('i', [k for k in ALL if DC.GEOMS[k]['case'] == 'tiny_block'], ids=lambda i: DC.IDS[i])
def test_tiny_block_reaches_the_clamp_of_the_pre_scale(i):
    """tiny_block exists for the clamp: the unclamped exponent must pass the upper limit, and without the clamp su s would leave fp32
    (the epilogue's 1 / (su s) would be 0)."""
    inp = DC.inputs(i)
    m = DC.model(i)
    base = 266 if inp['family'] == 'wino' else 268
    free = M.block_scale_log2(inp['x'][0], m['lsu'], base, clamp=False)
    assert m['ls'][0] < free and m['ls'][0] + m['lsu'] == 120 and free + m['lsu'] >= 128
    assert m['ls'][1] == M.block_scale_log2(inp['x'][1], m['lsu'], base, clamp=False)      # the neighbour is not clamped


def _gate_ratio(i, mutate):
    """the assertion of tests/test_dynamic_range_gpu.py (kernel against model, c = 2) applied to a model with one mistake in it"""
    m, mm = DC.model(i), DC.run_model(DC.inputs(i), 2, mutate)
    bound = 2 * m['n'] * M.U32 * m['A'] + 2.0 ** -23 * np.abs(m['value'])
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.abs(mm['value'][0] - m['value'][0]) / bound[0]
    return np.inf if np.isnan(r).any() else float(r.max())


@pytest.mark.parametrize('family', ['wino', 'tr2m'])
def test_the_gpu_assertion_would_see_a_mistake_in_the_arithmetic(family):
    """One mistake at a time in the MODEL, judged by the kernel-against-model assertion of the GPU test with the kernel's share (<= 1
    of the bound) taken off: a flushed denormal low piece shows on hot_voxel_20, a missing clamp on tiny_block (s su overflows), a
    bias scaled by s only on sparse_bias and tiny_block.  Dropping the l.l term does NOT show and cannot: |l| <= 2^-11 |h| on both
    sides, so the term is at most 2^-22 of the products, below the 2^-24 n of any bound that admits an fp32 accumulation of n terms.
    Its absence costs accuracy against float64 (2^-22 instead of 2^-24-ish per operand pair), which the model's own bound allows for."""
    shape = (2, 5, 16, 32, 16) if family == 'wino' else (2, 5, 16, 16, 32)
    idx = {g['case']: k for k, g in enumerate(DC.GEOMS) if g['family'] == family and g['shape'] == shape}
    seen = {'flush_l/hot_voxel_20': _gate_ratio(idx['hot_voxel_20'], 'flush_l'), 'no_clamp/tiny_block': _gate_ratio(idx['tiny_block'], 'no_clamp'),
            'bias_s_only/sparse_bias': _gate_ratio(idx['sparse_bias'], 'bias_s_only'), 'bias_s_only/tiny_block': _gate_ratio(idx['tiny_block'], 'bias_s_only')}
    print(family, {k: f'{v:.3g}' for k, v in seen.items()})
    for k, v in seen.items():
        assert v > 2.0, (k, v)
    for case in ('gauss', 'hot_voxel_20', 'hot_channel_20'):
        r = _gate_ratio(idx[case], 'drop_ll')
        print(f'{family} drop_ll/{case}: {r:.3g} of the bound')
        assert r < 1.0 / 64      # 2^-22 A against 2 n 2^-24 A, n >= 128 (one tap x 32 channels x 4 products)


def test_print_the_table(capsys):
    """far outputs of block 0 (every output where the case has no hot voxel), max |err| / T with T = sum |terms| of the float64 convolution"""
    lines = ['case                                     two-piece model   fp32-operand model']
    for i in ALL:
        row = _ROWS.get(i)
        if row is None:
            row = {n: DC.far_ratio(i, DC.model(i, p)['value'][0]) for n, p in (('two-piece', 2), ('fp32', None))}
        lines.append(f"{DC.IDS[i]:40s} {row['two-piece']:10.2e}        {row['fp32']:10.2e}")
    with capsys.disabled():
        print('\n' + '\n'.join(lines))
    assert len(lines) == len(ALL) + 1
