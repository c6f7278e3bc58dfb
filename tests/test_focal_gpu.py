"""pcc_focal_loss (csrc/elementwise.hip) and pcc_focal_loss_grad (csrc/train.hip) at the sizes where their grids change shape, with the
clamp bounds, labels that are neither class and out-of-range predictions in the first and the last elements, against a float64
evaluation of tests/_train_ref.focal_loss on the float32 inputs.

The loss is a fixed tree of float additions; its bound is written out below from the kernels' code (A additions on the longest path)
and from the measured float32 error of one term (T).  One test here needs no GPU: it re-measures T on the CPU oracle's terms."""
import numpy as np
import pytest
import torch

import _train_ref as R
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ops

gpu = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24                                                             # unit roundoff of float32

SIZES = (1, 63, 64, 65, 255, 256, 257, 262143, 262144, 262145, 524293)     # 1024 * 256 = 262144: one element per thread of the fixed grid
PARAMS = ((2.0, 0.9), (2.0, 0.75), (1.5, 0.5))
LO, HI = f32(1e-3), f32(.999)
# y_pred of the first and the last dozen elements: 0, 1, the bounds, one ulp inside and one ulp outside each bound, 2, -1 (+ two plain ones)
DOZEN_P = np.array([0, 1, LO, HI, np.nextafter(LO, f32(1)), np.nextafter(HI, f32(0)), np.nextafter(LO, f32(0)), np.nextafter(HI, f32(1)),
                    2.0, -1.0, 0.5, 0.25], np.float32)
HEAD_T = np.array([1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 0.5, 2], np.float32)      # 0.5, 2 and NaN are neither class: the constant term only
TAIL_T = np.array([0, 1, 0, 1, 0, 1, 0, 1, 0, 1, np.nan, 0.5], np.float32)

# T: what one float32 term alpha * powf(1 - pt1, gamma) * logf(pt1) (or its pt0 twin) may differ from its float64 value by, in units of
# 2^-24 of the term.  The ROCm device-library documentation that states powf / logf accuracies is not part of the toolchain this
# project builds with, so T is measured: the CPU oracle's float32 terms (oracle.focal_terms, the arithmetic of pcc_oracle_focal_loss)
# against the float64 terms on exactly the inputs below, largest relative error 486.4 * 2^-24, times 4 (the device functions are
# specified to a few ulp, not correctly rounded).  The error is not powf's or logf's own: log(1 - pt0) at pt0 near 1e-3 amplifies the
# rounding of the float32 subtraction 1 - pt0 by 1 / pt0 (0.5 ulp of 1.0 over |log(0.999)| ~ 1e-3, about 500 * 2^-24), and the float64
# reference does not round there.  test_term_allowance_covers_four_times_the_oracles_worst_term re-measures it.
T_TERM = 1946.0
# Resulting bound: (A + T) * 2^-24 * S = (A + 1946) * 5.96e-8 * S ~ 1.18e-4 * S for every n here (A <= 28), which is looser than the
# 2e-5 * |ref| the project has held so far (S == |ref|: all terms have one sign), so the bound in force is 2e-5 * |ref|.


def additions(n):
    """A: float additions on the longest path from one term to out[0].  k_focal_partial: a thread of the 1024 x 256 grid adds
    term1 + term0 (1) and accumulates ceil(n / 262144) elements (one addition each, the first onto 0), the wave butterfly adds 6 times,
    thread 0 adds the 4 wave sums onto 0 (4); k_focal_final: a thread accumulates 1024 / 256 = 4 partials (4), butterfly (6), 4 wave
    sums (4).  The final negation is exact."""
    return 1 + -(-n // (1024 * 256)) + 6 + 4 + 4 + 6 + 4


_INPUTS = {}


def inputs(n, kind='mixed'):
    """(y_true, y_pred) float32, y_pred uniform on [-0.1, 1.1].
    'mixed': 2 % ones, the dozen at the head and, from n = 24 on, at the tail.
    'ends': every label 0.5 (neither class: about 1e-9 per element) but the first and the last element, which are (1, 0): the largest
    term there is, alpha * 0.999^gamma * log(1e-3).  A kernel that loses either end loses half of the loss or all of it; under 'mixed'
    one element of 524293 is less than the bound."""
    if (n, kind) not in _INPUTS:
        rng = np.random.default_rng(40 + n)
        yt = (rng.random(n) < 0.02).astype(np.float32)
        yp = (rng.random(n) * 1.2 - 0.1).astype(np.float32)
        if kind == 'ends':
            yt[:] = 0.5
            yt[[0, -1]], yp[[0, -1]] = 1.0, 0.0
        else:
            k = min(n, 12)
            yp[:k], yt[:k] = DOZEN_P[:k], HEAD_T[:k]
            if n >= 24:
                yp[-12:], yt[-12:] = DOZEN_P, TAIL_T
        yt.setflags(write=False)
        yp.setflags(write=False)
        _INPUTS[n, kind] = (yt, yp)
    return _INPUTS[n, kind]


def terms64(yt, yp, gamma, alpha):
    """the two terms of src/utils/focal_loss.py per element in float64, on the float32 inputs, with the float32-rounded bounds"""
    t, p = yt.astype(np.float64), yp.astype(np.float64)
    pt1 = np.clip(np.where(t == 1, p, 1.0), float(LO), float(HI))
    pt0 = np.clip(np.where(t == 0, p, 0.0), float(LO), float(HI))
    a, g = float(f32(alpha)), float(f32(gamma))                             # the kernel's float arguments
    return a * (1 - pt1) ** g * np.log(pt1), (1 - a) * pt0 ** g * np.log(1 - pt0)


_REF = {}


def reference(n, gamma, alpha, kind='mixed'):
    """(loss, S) in float64: S = sum(|term1| + |term0|)"""
    key = (n, gamma, alpha, kind)
    if key not in _REF:
        yt, yp = inputs(n, kind)
        t1, t0 = terms64(yt, yp, gamma, alpha)
        loss = -float(np.sum(t1)) - float(np.sum(t0))
        torch_loss = float(R.focal_loss(torch.from_numpy(yt.copy()).double(), torch.from_numpy(yp.copy()).double(), gamma, float(f32(alpha))))
        assert abs(loss - torch_loss) <= 1e-12 * abs(torch_loss)            # the same formula as tests/_train_ref.focal_loss
        _REF[key] = (loss, float(np.sum(np.abs(t1)) + np.sum(np.abs(t0))))
    return _REF[key]


def bound(n, gamma, alpha, kind='mixed'):
    ref, S = reference(n, gamma, alpha, kind)
    return min((additions(n) + T_TERM) * U * S, 2e-5 * abs(ref))           # never looser than the bound held so far


def test_term_allowance_covers_four_times_the_oracles_worst_term(oracle):
    worst = 0.0
    for n in SIZES:
        yt, yp = inputs(n)
        for gamma, alpha in PARAMS:
            got = oracle.focal_terms(yt, yp, gamma, alpha)
            for g, w in zip(got, terms64(yt, yp, gamma, alpha)):
                assert (w < 0).all()                                        # one sign: S == |loss|
                worst = max(worst, float(np.max(np.abs(g.astype(np.float64) - w) / np.abs(w))) / U)
    print(f'largest relative error of a float32 term: {worst:.1f} * 2^-24; T = {T_TERM}')
    assert 1.0 <= worst and 4 * worst <= T_TERM <= 4 * worst * 1.05
    assert [additions(n) for n in (1, 262144, 262145, 524293)] == [26, 26, 27, 28]


def test_inputs_hold_the_specials_at_both_ends():
    yt, yp = inputs(524293)
    assert np.array_equal(yp[:12], DOZEN_P) and np.array_equal(yp[-12:], DOZEN_P)
    assert np.array_equal(yt[:12], HEAD_T) and np.array_equal(yt[-12:], TAIL_T, equal_nan=True)
    assert DOZEN_P[4] > LO > DOZEN_P[6] and DOZEN_P[5] < HI < DOZEN_P[7] and not np.isnan(yp).any()
    assert 0.015 < yt[12:-12].mean() < 0.025 and yp.min() < -0.09 and yp.max() > 1.09
    assert inputs(1)[1][0] == 0 and inputs(1)[0][0] == 1
    for n in SIZES:                                                         # 'ends': either end alone is far more than the bound
        yt, yp = inputs(n, 'ends')
        assert (yt[1:-1] == 0.5).all() and yt[0] == yt[-1] == 1 and yp[0] == yp[-1] == 0
        for gamma, alpha in PARAMS:
            t1, _ = terms64(yt, yp, gamma, alpha)
            assert abs(t1[0]) == abs(t1[-1]) > 3.4 and abs(t1[-1]) > 1e4 * bound(n, gamma, alpha, 'ends')


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@gpu
@pytest.mark.parametrize('kind', ('mixed', 'ends'))
@pytest.mark.parametrize('n', SIZES)
def test_focal_loss_within_the_bound_deterministic_and_blind_to_the_tail(ctx, n, kind):
    yt, yp = inputs(n, kind)
    a, b = _dev(yt), _dev(yp)
    # the same inputs at the head of buffers 1024 elements longer, NaN and inf behind them
    tail = np.where(np.arange(1024) % 2 == 0, np.nan, np.inf).astype(np.float32)
    la, lb = _dev(np.concatenate([yt, tail])), _dev(np.concatenate([yp, tail[::-1]]))
    for gamma, alpha in PARAMS:
        got = ops.focal_loss(ctx, a, b, gamma, alpha)
        ref, S = reference(n, gamma, alpha, kind)
        err, lim = abs(float(got) - ref), bound(n, gamma, alpha, kind)
        print(f'{kind} n={n} gamma={gamma} alpha={alpha}: got {float(got)!r} ref {ref!r} |err| {err:.3e} bound {lim:.3e} '
              f'(A={additions(n)}, (A+T)*2^-24*S={(additions(n) + T_TERM) * U * S:.3e}, 2e-5*|ref|={2e-5 * abs(ref):.3e})')
        assert err <= lim, (kind, n, gamma, alpha, float(got), ref, err, lim)
        bits = got.cpu().numpy().view(np.uint32)
        assert ops.focal_loss(ctx, a, b, gamma, alpha).cpu().numpy().view(np.uint32) == bits                  # fixed reduction order
        assert ops.focal_loss(ctx, la[:n], lb[:n], gamma, alpha).cpu().numpy().view(np.uint32) == bits        # nothing past n is read


def _grad_sizes(ctx):
    return SIZES + (ctx.num_cu * 32 * 256 + 5,)                             # a few elements past one pass of the gradient's largest grid


@gpu
@pytest.mark.parametrize('which', range(len(SIZES) + 1))
def test_focal_gradient_per_element_against_float64_autograd(ctx, which):
    n = _grad_sizes(ctx)[which]
    yt, yp = inputs(n)
    a, b = _dev(yt), _dev(yp)
    SENT = 0xCDCDCDCD
    for gamma, alpha in PARAMS:
        p = torch.from_numpy(yp.copy()).double().requires_grad_()
        R.focal_loss(torch.from_numpy(yt.copy()).double(), p, gamma, float(f32(alpha))).backward()
        ref = p.grad.numpy()
        # tf.clip_by_value's gradient: zero strictly outside [1e-3, 0.999] and for a label that is neither class, passed at the bounds
        live = ((yt == 1) | (yt == 0)) & (yp >= LO) & (yp <= HI)
        assert np.array_equal(ref != 0, live)
        out = torch.full((n + 1024,), SENT - (1 << 32), dtype=torch.int32, device=ctx.device).view(torch.float32)
        L.check(L.lib().pcc_focal_loss_grad(ctx.handle, a.data_ptr(), b.data_ptr(), n, gamma, alpha, None, out.data_ptr(), ctx.stream),
                'pcc_focal_loss_grad')
        host = out.cpu().numpy()
        g = host[:n]
        assert (host[n:].view(np.uint32) == SENT).all()                                        # nothing past n is written
        assert np.array_equal(g != 0, live), np.flatnonzero((g != 0) != live)[:8]              # the pattern at the clamp bounds, exactly
        assert np.allclose(g, ref, rtol=1e-5, atol=1e-6), (n, gamma, alpha, float(np.max(np.abs(g - ref))))
        w = ops.focal_loss_grad(ctx, a, b, None, gamma, alpha).cpu().numpy()
        assert np.array_equal(w.view(np.uint32), g.view(np.uint32))
