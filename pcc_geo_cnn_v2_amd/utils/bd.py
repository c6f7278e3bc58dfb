"""Bjøntegaard delta metrics between two rate-distortion curves -- the role of the reference's src/utils/bd.py.

G. Bjøntegaard, "Calculation of average PSNR differences between RD-curves", VCEG-M33 (2001): put both curves on a
logarithmic rate axis, interpolate each one, integrate both over the interval that the two curves share, and report the
difference of the two mean values.

    bdsnr(set1, set2)   mean of  PSNR_2(log r) - PSNR_1(log r)  over the shared log-rate interval, in dB
    bdrate(set1, set2)  mean of  log r_2(PSNR) - log r_1(PSNR)  over the shared PSNR interval, as (exp(mean) - 1) * 100 %

Both take (n, 2) arrays of (rate, PSNR) rows; set1 is the anchor: bdrate = +100 says that curve 2 needs twice the rate of
curve 1 for the same PSNR, bdsnr = +1 that curve 2 is 1 dB better at the same rate.  ev_compare fills row i, column j of its
matrices with bd*(points of mode j, points of mode i), the reference's argument order.

Preparation, the same for both: duplicate rows are removed, then the rows are ordered along the interpolation axis (rate for
bdsnr, PSNR for bdrate).  Rates enter as natural logarithms.

Interpolation: pchip=True (default) is the monotone piecewise-cubic Hermite interpolant through the points
(scipy.interpolate.PchipInterpolator), pchip=False one cubic polynomial fitted to all points by least squares (numpy.polyfit).

Corner cases (what the reference does, found by running it; tests/golden/bd_cases.json holds examples of each):

* fewer than four points, pchip=False: the cubic is under-determined; numpy.polyfit warns (RankWarning) and returns the
  minimum-norm fit, and a finite number comes out.  It means little.
* fewer than two distinct points, pchip=True: ValueError from PchipInterpolator.  Also ValueError when two distinct points share
  their coordinate on the interpolation axis (same rate for bdsnr, same PSNR for bdrate): that axis must increase strictly.
* empty overlap (the shared interval has its lower end above its upper end): no error and no NaN.  Both integrals run
  backwards over the gap between the curves, where each interpolant extrapolates, and a finite number comes out.  It means
  nothing; ev_compare writes it as it is, as the reference does.
* an interval of length zero (the curves touch in one coordinate): bdsnr returns 0.0, bdrate returns NaN (0 / 0).
* a non-positive rate: ValueError from the logarithm.
* bdrate's mean log-rate difference is clamped at 200 before the exponential.
"""
import math

import numpy as np
from scipy.interpolate import PchipInterpolator


def _curve(points, axis):
    """(rate, PSNR) rows -> (log rate, PSNR) columns of the distinct rows, ordered along column `axis`."""
    rows = np.unique(np.asarray(points), axis=0)
    rows = rows[np.argsort(rows[:, axis])]
    return [math.log(r) for r in rows[:, 0]], [p for p in rows[:, 1]]


def _area(x, y, lo, hi, pchip):
    """Integral over [lo, hi] of the interpolant of y over x."""
    if pchip:
        return PchipInterpolator(x, y).integrate(lo, hi)
    primitive = np.polyint(np.polyfit(x, y, 3))
    return np.polyval(primitive, hi) - np.polyval(primitive, lo)


def bdsnr(set1, set2, pchip=True):
    """Mean PSNR gain of curve 2 over curve 1 at equal rate, in dB (see the module docstring)."""
    x1, y1 = _curve(set1, 0)
    x2, y2 = _curve(set2, 0)
    lo, hi = max(min(x1), min(x2)), min(max(x1), max(x2))
    a1, a2 = _area(x1, y1, lo, hi, pchip), _area(x2, y2, lo, hi, pchip)
    if hi == lo:
        return 0.0
    return (a2 - a1) / (hi - lo)


def bdrate(set1, set2, pchip=True):
    """Mean rate excess of curve 2 over curve 1 at equal PSNR, in percent (see the module docstring)."""
    y1, x1 = _curve(set1, 1)
    y2, x2 = _curve(set2, 1)
    lo, hi = max(min(x1), min(x2)), min(max(x1), max(x2))
    a1, a2 = _area(x1, y1, lo, hi, pchip), _area(x2, y2, lo, hi, pchip)
    mean = (a2 - a1) / (hi - lo)
    if mean > 200:
        mean = 200
    return (math.exp(mean) - 1) * 100
