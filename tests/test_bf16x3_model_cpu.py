"""The three-piece bf16 arithmetic of conv_split.hip / conv_tr2m_bf16.hip / conv_wino_bf16.hip as a numpy model (tests/_bf16x3_model.py) against a
float64 direct convolution, on the impulse lattices and the dense dynamic-range cases of tests/_impulse_cases.py.  Needs no GPU: this is the
half of DESIGN.md section 4.2 that shows what the assertions of tests/test_bf16x3_gpu.py can and cannot see."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bf16x3_model as B              # noqa: E402
import _f16s_model as F                # noqa: E402
import _impulse_cases as IC            # noqa: E402

C_ACC = 2.0                            # tests/test_bf16x3_gpu.py, tests/test_dynamic_range_gpu.py
GI = list(range(len(IC.GEOMS)))
CASES = [(gi, v) for gi in GI for v in IC.VARIANTS]
CASE_IDS = [f'{IC.IDS[gi]}-{v}' for gi, v in CASES]
# the chain of one Winograd point on these lattices: a 4 x 4 patch holds the lattice positions {0, 3}, {1} or {2} of an axis; B^T sends
# position 0 to point 0 alone, 3 to point 3 alone, 1 and 2 to points 1, 2, 3 / 0, 1, 2, so no point of a patch hears two impulses, and only
# one of the three z taps holds a lattice plane: six piece products per point, + 8 + 3 as _f16s_model.wino_model counts; an output reads 9
# points, with at most 3 (point, impulse) pairs per axis
WINO_N_MAX = 6 + 8 + 3
WINO_PRODUCTS_MAX = 9 * 6


def _bf16_bits_scalar(v):
    """bf16_bits of csrc/kernel_common.h, restated on one float with integer arithmetic"""
    b = struct.unpack('<I', struct.pack('<f', v))[0]
    if (b & 0x7f800000) == 0x7f800000:
        return b >> 16
    return ((b + 0x7fff + ((b >> 16) & 1)) & 0xffffffff) >> 16


def _case_values():
    xs = [IC.SPECIALS]
    for gi in GI:
        xs += [IC.launch_x(gi, l)[IC.launch_x(gi, l) != 0] for l in range(len(IC.plan(gi)))]
        xs.append(IC.layer_inputs(gi, 'full')['w'].ravel())
    return np.concatenate(xs)


def test_split_is_exact_and_follows_the_packers_rule():
    """h + m + l == x exactly, x - h and x - h - m are exact in fp32, every piece is a bf16 value, and bf16_rn is bf16_bits bit for bit: on
    random values over the whole exponent range, on the specials, and on every value of the impulse cases."""
    rng = np.random.default_rng(0)
    e = rng.integers(-100, 100, 200000)
    y = np.ldexp(rng.uniform(0.5, 1, e.size), e).astype(np.float32) * rng.choice([-1, 1], e.size).astype(np.float32)
    y = np.concatenate([y, _case_values(), np.array([0, B.BF16_MAX, -B.BF16_MAX, 2.0 ** -126], np.float32)])
    h, m, l = B.split_bf16x3(y)
    y64, h64, m64, l64 = (a.astype(np.float64) for a in (y, h, m, l))
    assert np.isfinite(h).all()
    assert np.array_equal(h64 + m64 + l64, y64)
    assert np.array_equal((y - h).astype(np.float64), y64 - h64) and np.array_equal(((y - h) - m).astype(np.float64), y64 - h64 - m64)
    for p in (h, m, l):
        assert not (p.view(np.uint32) & np.uint32(0xffff)).any()
    assert (np.abs(m64) <= 2.0 ** -8 * np.abs(h64)).all() and (np.abs(l64) <= 2.0 ** -8 * np.abs(m64)).all()      # half a step of the piece above
    for v in np.concatenate([y[:2000], IC.SPECIALS, np.array([np.inf, -np.inf, np.nan, 3.4e38], np.float32)]):
        got = int(B.bf16_rn(np.array([v], np.float32)).view(np.uint32)[0] >> 16)
        assert got == _bf16_bits_scalar(float(v)), v
    assert B.in_domain(_case_values())
    assert not B.in_domain(np.float32(3.4e38)) and not B.in_domain(np.float32(2.0 ** -120 * (1 + 2.0 ** -20)))


def test_specials_are_what_they_are_named():
    h, m, l = B.split_bf16x3(IC.SPECIALS[0:16:2])              # the positive, unscaled ones
    assert m[0] == 0 and l[0] == 0                              # bf16-representable
    assert m[1] != 0 and l[1] == 0
    assert h[2] == 1 and m[2] == np.float32(2.0 ** -8)          # tie to even: down
    assert h[3] == np.float32(1 + 2.0 ** -6) and m[3] == np.float32(-2.0 ** -8)      # tie to even: up
    assert m[4] == np.float32(2.0 ** -10) and l[4] == np.float32(2.0 ** -18)
    assert m[5] == np.float32(2.0 ** -10 * (1 + 2.0 ** -6)) and l[5] == np.float32(-2.0 ** -18)
    assert h[6] == np.float32(1 + 2.0 ** -7) and m[6] < 0 and h[7] == 2 and m[7] < 0
    for sc in (2.0 ** 60, 2.0 ** -60):                          # the scaled copies split into the scaled pieces
        hs, ms, ls = B.split_bf16x3(IC.SPECIALS[0:16:2] * np.float32(sc))
        assert np.array_equal(hs, h * np.float32(sc)) and np.array_equal(ms, m * np.float32(sc)) and np.array_equal(ls, l * np.float32(sc))


def test_the_row_skipping_sums_are_the_plain_ones():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 3, 4, 5, 8)) * (rng.random((1, 3, 4, 5, 1)) < 0.3)
    wt, wl = rng.standard_normal((3, 3, 3, 6, 8)), rng.standard_normal((3, 3, 3, 8, 6)).astype(np.float32).astype(np.float64)
    assert np.allclose(B._tr2_gather(x, wt), F._tr2_scatter(x, wt), rtol=0, atol=1e-13)
    assert np.allclose(B._s1_gather(x, wl), F.direct_conv(x, wl, False, 1)[0], rtol=0, atol=1e-13)


@pytest.mark.parametrize('gi', GI, ids=IC.IDS)
def test_impulse_lattices_give_single_products_and_reach_every_weight(gi):
    """From the inputs alone: one nonzero channel per nonzero voxel; every coordinate of every axis carries an impulse in some launch; every
    input channel sits, in some launch, on a voxel whose 27 taps all land inside the grid -- so every (tap, ci, co) element of the weights is
    the sole product of at least one output; and from the model: no output of a direct kernel accumulates more than the six piece products of
    one x . w (Winograd: WINO_N_MAX)."""
    g = IC.GEOMS[gi]
    N, D, H, W, C = g['shape']
    stride = g['stride']
    seen = [np.zeros(n, bool) for n in (D, H, W)]
    inner_channels = set()
    for l in range(len(IC.plan(gi))):
        x = IC.launch_x(gi, l)
        nz = x != 0
        assert (nz.sum(axis=-1) <= 1).all() and B.in_domain(x)
        vox = np.argwhere(nz.any(axis=-1)[0])
        assert len(vox) == len(IC.lattice((D, H, W), stride, IC.plan(gi)[l][0])[0])
        for a in range(3):
            seen[a][vox[:, a]] = True
            d = np.diff(np.unique(vox[:, a]))
            assert (d == IC.SPACING[stride]).all()
        hi = np.array([D, H, W]) - 2
        inner = (vox <= hi).all(axis=1) & ((vox >= 1).all(axis=1) if stride == 1 else True)
        inner_channels |= {int(np.flatnonzero(nz[0, z, y, xx])[0]) for z, y, xx in vox[inner]}
        for v in IC.VARIANTS:
            m = IC.model(gi, v, l)
            extra = (m['n'] - m['products']).max()
            if g['family'] == 'wino':
                assert m['n'].max() == WINO_N_MAX and m['products'].max() <= WINO_PRODUCTS_MAX
            else:
                assert m['products'].max() == 6 and extra == (2 if v == 'full' and stride == 1 else 1 if v == 'full' else 0)
    assert all(s.all() for s in seen)
    used = np.concatenate([IC.launch_x(gi, l)[IC.launch_x(gi, l) != 0] for l in range(len(IC.plan(gi)))])
    assert np.isin(IC.SPECIALS, used).all(), 'specials that never reach this geometry: ' + str(IC.SPECIALS[~np.isin(IC.SPECIALS, used)])
    assert inner_channels == set(range(C)), sorted(set(range(C)) - inner_channels)
    assert not (IC.layer_inputs(gi, 'bare')['w'] == 0).any() and B.in_domain(IC.layer_inputs(gi, 'bare')['w'])


@pytest.mark.parametrize('gi,variant', CASES, ids=CASE_IDS)
def test_model_is_within_its_bound_of_the_float64_convolution_on_impulses(gi, variant):
    """|model - exact| <= bound per output: the model differs from the exact convolution by the three dropped terms of every product, whose
    magnitudes the bound sums from the pieces (Winograd: plus the fp32 roundings of U and of the entries of V behind more than one element)."""
    for l in range(len(IC.plan(gi))):
        m, ref = IC.model(gi, variant, l), IC.reference(gi, variant, l)
        assert np.isfinite(m['value']).all() and (np.abs(m['value'] - ref) <= m['bound']).all()
        assert (m['A'] >= np.abs(m['value']) * (1 - 1e-12)).all()
        m32 = IC.model(gi, variant, l, None)
        assert (np.abs(m32['value'] - ref) <= m32['bound']).all()


@pytest.mark.parametrize('i', range(len(IC.DENSE)), ids=IC.DENSE_IDS)
def test_model_is_within_its_bound_of_the_float64_convolution_on_dense_inputs(i):
    ref, _ = IC.dense_reference(i)
    assert B.in_domain(IC.dense_inputs(i)['x'], IC.dense_inputs(i)['w'])
    for pieces in (3, None):
        m = IC.dense_model(i, pieces)
        assert np.isfinite(m['value']).all() and (np.abs(m['value'] - ref) <= m['bound']).all()
    print(f"{IC.DENSE_IDS[i]}: far outputs of block 0, max err / T: three-piece model {IC.dense_far_ratio(i, IC.dense_model(i)['value'][0]):.2e}, "
          f"fp32-operand model {IC.dense_far_ratio(i, IC.dense_model(i, None)['value'][0]):.2e}")


def _ratio(diff, m):
    with np.errstate(invalid='ignore', divide='ignore'):
        b = B.acc_bound(m, C_ACC)
        r = np.where(b > 0, np.abs(diff) / b, np.where(np.abs(diff) > 0, np.inf, 0.0))
    return float(r.max())


# What the kernel-against-model assertion cannot see, and why (u = 2^-24, p = |x . w|):
#   trunc   truncation gives another EXACT split x = h + m + l, with |m| < 2^-7 |h|, |l| < 2^-7 |m| where rounding gives 2^-8: the six kept
#           terms then miss ml + lm + ll < (2^-20 + 2^-28) p where the rounded split misses at most (2^-23 + 2^-32) p, so the two models differ
#           by less than 18.1 u p, and only where both operands have large m AND l pieces -- against the 12 u A + 2 u p >= 14 u p that the bound
#           grants six fp32-accumulated terms at c = 2.  The ceiling is 18.1 / 14 = 1.3; these cases reach 0.6 - 0.75.  A truncating split is a
#           valid three-piece split with 3 bits less in the dropped terms; the bits of tests/golden/family_bits.json pin it, this gate cannot.
#   flush   every nonzero piece of every case is a normal number (the model's domain, asserted above), so there is nothing to flush.
BLIND = {'trunc': 18.1 / 14, 'flush': 0.0}


@pytest.mark.parametrize('gi', GI, ids=IC.IDS)
def test_the_gpu_assertion_would_see_a_lost_piece_on_impulses(gi, capsys):
    """One mistake at a time in the MODEL, judged by the kernel-against-model assertion of tests/test_bf16x3_gpu.py: max |mutated - model| /
    (c n 2^-24 A + 2^-23 |model|) over the launches and variants of the geometry.  Every dropped term and every zeroed piece must exceed 1
    (one-piece defects: several times; hm / mh and the h pieces: thousands and more); BLIND lists what the arithmetic says cannot show, with
    the largest ratio it can reach.  The unmutated model accumulated in fp32 in the documented three steps stays below 1."""
    worst = dict.fromkeys(B.MUTATIONS, 0.0)
    own = 0.0
    for v in IC.VARIANTS:
        for l in range(len(IC.plan(gi))):
            m = IC.model(gi, v, l)
            own = max(own, _ratio(m['value32'].astype(np.float64) - m['value'], m))
            for mu in B.MUTATIONS:
                worst[mu] = max(worst[mu], _ratio(IC.mutated(gi, v, l, mu)['value'] - m['value'], m))
    with capsys.disabled():
        print(f'\n{IC.IDS[gi]}: three-step fp32 {own:.3f}; ' + ', '.join(f'{k} {r:.3g}' for k, r in worst.items()))
    assert own < 1.0
    for mu, r in worst.items():
        if mu in BLIND:
            assert r <= BLIND[mu], (mu, r)
        else:
            assert r > 1.0, (mu, r)


def test_flush_hook_flushes_outside_the_domain():
    """model only, no GPU case: a value whose low piece is a denormal is outside the domain; the hook must change it"""
    x = np.array([2.0 ** -112 * (1 + 2.0 ** -9 + 2.0 ** -18)], np.float32)
    assert not B.in_domain(x)
    h, m, l = B.split_bf16x3(x)
    hf, mf, lf = B.split_bf16x3(x, flush=True)
    assert l[0] != 0 and abs(float(l[0])) < B.MIN_NORMAL and lf[0] == 0 and hf[0] == h[0] and mf[0] == m[0]


def test_print_the_same_table_on_dense_inputs(capsys):
    """Printed only: on dense inputs n is 27 Cin x 6 and the same mistakes sit far below the bound -- why dense inputs alone cannot carry the
    check (gauss and hot_voxel_20 of every dense shape)."""
    lines = []
    for i, g in enumerate(IC.DENSE):
        if g['case'] not in ('gauss', 'hot_voxel_20'):
            continue
        m, inp = IC.dense_model(i), IC.dense_inputs(i)
        rs = {mu: _ratio(IC.dense_run(inp, mutate=mu, lean=True)['value'] - m['value'], m) for mu in ('drop_mm', 'drop_lh', 'zero_x_l', 'zero_w_l', 'drop_hm', 'trunc')}
        lines.append(f'{IC.DENSE_IDS[i]:44s} ' + ', '.join(f'{k} {r:.3g}' for k, r in rs.items()))
    with capsys.disabled():
        print('\n' + '\n'.join(lines))
    assert len(lines) == 2 * len(IC._DENSE_SHAPES)
