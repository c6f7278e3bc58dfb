"""Generates tests/golden/bd_cases.json by IMPORTING the reference's own utils/bd.py (possible only where the reference
checkout is at hand).  The fixture is DATA: curve points and the numbers the reference's bdrate / bdsnr returned for them.

Run:  python tests/golden/make_bd_cases.py REFERENCE_DIR        (the directory that holds data.csv and src/)

Curves:
  * the published data.csv, eval set `main`: per cloud and optimisation group one curve per mode, and EVERY ordered pair of
    modes of a condition (the pair of a mode with itself included) is a case;
  * seeded synthetic monotone curves of 1..7 points: full, partial, touching and empty overlap, duplicated rows, two points
    at one rate or one PSNR.
Every case holds, for bdrate and bdsnr with pchip=True and pchip=False, the returned float, the string 'nan' / 'inf' / '-inf',
or {'raises': <exception class name>}.  A pair that cannot be evaluated at all is not written; the script prints the number of
cases it wrote (stored as `count`), and tests/test_bd_cpu.py asserts that it finds that many.
"""
import importlib.util
import json
import math
import os
import sys
import warnings

import numpy as np
import pandas as pd

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'bd_cases.json')
FUNCS = [('bdrate', True), ('bdrate', False), ('bdsnr', True), ('bdsnr', False)]


def load_reference_bd(reference_dir):
    spec = importlib.util.spec_from_file_location('reference_bd', os.path.join(reference_dir, 'src', 'utils', 'bd.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def outcome(fn, a, b, pchip):
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            v = float(fn(a, b, pchip=pchip))
    except Exception as e:      # stored: the test expects the same exception class
        return {'raises': type(e).__name__}
    if math.isnan(v):
        return 'nan'
    if math.isinf(v):
        return 'inf' if v > 0 else '-inf'
    return v


def published_curves(csv_path):
    """-> curves [(name, points)], pairs [(i, j)] for eval set `main`."""
    d = pd.read_csv(csv_path)
    d = d[d.eval_id == 'main']
    curves, pairs = [], []
    for (pc, group), cond in d.groupby(['pc_name', 'opt_group'], sort=True):
        first = len(curves)
        for mode in cond.mode_id.unique():
            rows = cond[cond.mode_id == mode]
            curves.append((f'data.csv/{pc}/{group}/{mode}', rows[['x', 'y']].values.tolist()))
        idx = range(first, len(curves))
        pairs += [(i, j) for i in idx for j in idx]
    return curves, pairs


def synthetic_curves(seed=20211):
    rng = np.random.default_rng(seed)
    curves, pairs = [], []

    def curve(n, lo, hi, base, gain):
        r = np.sort(np.exp(rng.uniform(np.log(lo), np.log(hi), n)))
        p = base + gain * np.log(r / lo) + np.cumsum(rng.uniform(0.05, 0.6, n))
        return np.stack([r, p], 1)

    def add(kind, a, b):
        curves.append((f'synthetic/{kind}/{len(pairs)}/a', np.asarray(a).tolist()))
        curves.append((f'synthetic/{kind}/{len(pairs)}/b', np.asarray(b).tolist()))
        pairs.append((len(curves) - 2, len(curves) - 1))

    for k in range(12):                                   # overlapping curves of 4..7 points
        add('overlap', curve(4 + k % 4, .05, 1.5, 55, 5), curve(4 + (k + 1) % 4, .08, 2., 56, 4.5))
    for k in range(6):                                    # partial overlap
        add('partial', curve(5, .05, .4, 55, 5), curve(5, .2, 2., 60, 5))
    for k in range(6):                                    # duplicated rows, shuffled
        a, b = curve(5, .05, 1.5, 55, 5), curve(4, .05, 1.5, 56, 5)
        a = np.vstack([a, a[rng.integers(0, len(a), 2)]])
        b = np.vstack([b, b[:1]])
        add('duplicates', a[rng.permutation(len(a))], b[rng.permutation(len(b))])
    for n in (1, 2, 3):                                   # fewer than four points
        for m in (n, 5):
            add(f'short{n}x{m}', curve(n, .05, 1.5, 55, 5), curve(m, .05, 1.5, 56, 5))
    for k in range(4):                                    # no overlap in rate and none in PSNR
        add('disjoint', curve(4, .05, .2, 50, 3), curve(4, .5, 2., 70, 3))
    a = curve(4, .1, 1., 55, 5)                           # the curves touch in one point: an interval of length zero
    b = curve(4, 1.5, 3., 70, 5)
    b[0] = a[-1]
    add('touching', a, b)
    a = curve(5, .1, 1., 55, 5)                           # two points at one rate / at one PSNR
    t = a.copy(); t[2, 0] = t[1, 0]
    add('same_rate', t, curve(5, .1, 1., 56, 5))
    t = a.copy(); t[2, 1] = t[1, 1]
    add('same_psnr', t, curve(5, .1, 1., 56, 5))
    a = curve(4, .1, 1., 55, 5); a[0, 0] = 0.             # a rate of zero
    add('zero_rate', a, curve(4, .1, 1., 56, 5))
    add('steep', curve(4, .05, 1.5, 55, 5) * [1, 1], curve(4, .05, 1.5, 55, 5) * [1e-120, 1])      # exponent clamp
    return curves, pairs


def main(reference_dir):
    bd = load_reference_bd(reference_dir)
    c1, p1 = published_curves(os.path.join(reference_dir, 'data.csv'))
    c2, p2 = synthetic_curves()
    curves = c1 + c2
    pairs = p1 + [(i + len(c1), j + len(c1)) for i, j in p2]
    cases = []
    for i, j in pairs:
        a, b = curves[i][1], curves[j][1]
        try:
            res = [outcome(getattr(bd, name), a, b, pchip) for name, pchip in FUNCS]
        except BaseException as e:       # cannot be evaluated: not written, and the count shows it
            print(f'skipped {curves[i][0]} x {curves[j][0]}: {e!r}')
            continue
        cases.append([i, j] + res)
    doc = {'functions': [f'{n}(pchip={p})' for n, p in FUNCS], 'count': len(cases),
           'curves': [{'name': n, 'points': p} for n, p in curves], 'cases': cases}
    with open(OUT, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
    print(f'{len(cases)} cases ({len(p1)} published, {len(p2)} synthetic) over {len(curves)} curves -> {OUT}, '
          f'{os.path.getsize(OUT)} bytes')
    kinds = {}
    for c in cases:
        for r in c[2:]:
            k = 'raises ' + r['raises'] if isinstance(r, dict) else (r if isinstance(r, str) else 'finite')
            kinds[k] = kinds.get(k, 0) + 1
    print(kinds)


if __name__ == '__main__':
    main(sys.argv[1])
