"""Host restatement of the top-k selection rule (include/pcc_geo.h "top-k selection"), in two independent forms, and the
cases the kernel is checked on.

    key(i) = 0 unless x[i] > 0, else the raw bits of the float32 x[i];  P = #{key > 0};  k_eff = clamp(k, 0, P)
    taken  = the k_eff voxels that come first by (key descending, i ascending), emitted in ascending i as (x, y, z) rows, x slowest
"""
import numpy as np

SHAPES = ((4, 4, 4), (8, 8, 8), (16, 8, 24), (64, 64, 64))
SENTINEL = np.float32(3.0e38)          # behind every row of a strided launch: the largest key of all if a kernel ever read it


def keys(x):
    x = np.ascontiguousarray(x, np.float32).ravel()
    with np.errstate(invalid='ignore'):
        positive = x > 0
    return np.where(positive, x.view(np.uint32), np.uint32(0)).astype(np.uint32)


def k_eff_of(key, k):
    return int(min(max(int(k), 0), int(np.count_nonzero(key))))


def taken_lexsort(x, k):
    """form 1: sort by (key descending, index ascending), keep the first k_eff, back to index order"""
    key = keys(x)
    ke = k_eff_of(key, k)
    order = np.lexsort((np.arange(key.size), -key.astype(np.int64)))
    return np.sort(order[:ke])


def taken_kth(x, k):
    """form 2: the k_eff-th largest key T, everything above it, and of the equal ones the first r in index order"""
    key = keys(x)
    ke = k_eff_of(key, k)
    if ke == 0:
        return np.zeros(0, np.int64)
    T = np.partition(key, key.size - ke)[key.size - ke]
    above, equal = key > T, key == T
    r = ke - int(above.sum())
    assert 1 <= r <= int(equal.sum())
    return np.flatnonzero(above | (equal & (np.cumsum(equal) <= r)))


def rows_of(idx, dhw):
    """voxel indexes (C order) -> float32 (x, y, z) rows"""
    return np.stack(np.unravel_index(np.asarray(idx, np.int64), dhw), -1).astype(np.float32).reshape(-1, 3)


def select(x, k, dhw, form=taken_kth):
    idx = form(x, k)
    return rows_of(idx, dhw), len(idx)


def _inputs(n, rng):
    """name -> (scores, tied)"""
    f32 = np.float32
    lo = f32(0.5)
    hi = np.nextafter(lo, f32(1.0))
    relu = np.where(rng.random(n) < 0.03, rng.random(n), 0.0)
    special = (rng.random(n) * 3.0 - 0.5).astype(f32)
    plant = [np.nan, -0.0, 0.0, -1.0, np.inf, np.float32(1e-45), 2.5]
    at = rng.choice(n, len(plant), replace=False)
    special[at] = np.array(plant, f32)
    last = np.zeros(n, f32)
    last[-1] = 0.75
    return {
        'uniform': ((rng.random(n) * 1.25 - 0.25).astype(f32), False),
        'constant': (np.full(n, 0.37, f32), True),                                   # the tie cut crosses every wave and segment boundary
        'adjacent': (np.where(rng.random(n) < 0.5, lo, hi).astype(f32), True),       # the decision falls in the lowest digit
        'pow2': ((2.0 ** rng.integers(-20, 20, n)).astype(f32), True),               # ... in the highest digit
        'levels8': (((rng.integers(0, 8, n) + 1) / 8.0).astype(f32), True),          # mass ties at the cut
        'relu97': (relu.astype(f32), False),
        'nonpositive': (np.where(rng.random(n) < 0.5, -rng.random(n), np.where(rng.random(n) < 0.5, 0.0, -0.0)).astype(f32), False),
        'last-voxel': (last, False),
        'special': (special, False),
    }


def _counts(x, tied):
    key = keys(x)
    n, P = key.size, int(np.count_nonzero(key))
    ks = [0, 1, 2, P // 2, P - 1, P, P + 1, n, n + 5, -3]
    if tied and P:
        ranked = np.sort(key[key > 0])[::-1]
        T = ranked[P // 2]
        first = int(np.count_nonzero(ranked > T))                 # voxels above the tie group that holds the median rank
        ks += [first + 1, first + int(np.count_nonzero(ranked == T))]
    return list(dict.fromkeys(ks))


_CASES = {}


def cases(dhw=None):
    """[(name, scores (n,) float32, k)] of a shape (default: of every shape of SHAPES): every input under every k; built once per shape"""
    if dhw is None:
        return [c for shape in SHAPES for c in cases(shape)]
    dhw = tuple(dhw)
    if dhw not in _CASES:
        n = int(np.prod(dhw))
        rng = np.random.default_rng(1000 + n)
        _CASES[dhw] = [(f'{"x".join(map(str, dhw))}-{name}-k{k}', x, k) for name, (x, tied) in _inputs(n, rng).items() for k in _counts(x, tied)]
    return _CASES[dhw]


def strided(arrs, pad):
    """the rows as one (B, n + pad) float32 array with SENTINEL behind each"""
    n = arrs[0].size
    host = np.full((len(arrs), n + pad), SENTINEL, np.float32)
    for b, a in enumerate(arrs):
        host[b, :n] = a
    return host
