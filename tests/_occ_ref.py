"""Host restatement of the "occ1" string format, written from the format's description alone: plain Python / numpy,
one symbol at a time.  The GPU tests compare the device coder's bytes with these, and each side decodes the other's strings.

One string codes the true occupancy o_i of a block given the decoder's x_hat (fp32, voxel i in C order).
  bucket  b = 0 unless x_hat > 0; b = 31 if x_hat >= 1; else min(30, 1 + int(fp32(x_hat * 30))).
  entries for every bucket with tot[b] > 0, ascending: uint16 0 when on[b] == 0, else clamp((on * 65536 + tot // 2) // tot, 1, 65535).
  symbols the voxels of the buckets with a non-zero entry f, ascending i: bit 1 has freq f and start 65536 - f, bit 0 freq 65536 - f, start 0.
  coder   rans1's (tests/_rans_ref.py) without escapes: state in [2^16, 2^32), initial state 2^16, 16-bit words, symbol j on lane j % L at
          step j // L, one forward word cursor, ascending lanes within a step; L by the lane rule over the coded freqs (m = 0: L = 1).
  bytes   log2 L, the entries, L final states, the words (little-endian); n = 0 is b''."""
import math

import numpy as np

from _rans_ref import LOW, MAX_LANES, cost256, lane_rule

K = 32
TOTAL = 1 << 16


class OccCorrupt(ValueError):
    pass


def buckets(x_hat):
    """bucket of every voxel: int64 array"""
    x = np.ascontiguousarray(x_hat, np.float32).reshape(-1)
    with np.errstate(invalid='ignore', over='ignore'):
        pos = x > 0                                          # False for NaN, -0 and negatives
        scaled = (np.where(pos & (x < 1), x, np.float32(0)) * np.float32(30.0)).astype(np.float32)       # one fp32 multiply
        b = np.minimum(K - 2, 1 + scaled.astype(np.int64))                                               # truncation, then the clamp
    b = np.where(x >= 1, K - 1, b)
    return np.where(pos, b, 0).astype(np.int64)


def entry(on, tot):
    if on == 0:
        return 0
    return min(65535, max(1, (int(on) * TOTAL + int(tot) // 2) // int(tot)))


def calibrate(b, occ):
    """-> (tot[K], on[K], f[K] with f[b] = 0 for an empty or skipped bucket)"""
    tot = np.bincount(b, minlength=K)
    on = np.bincount(b[occ], minlength=K)
    return tot, on, [entry(on[k], tot[k]) if tot[k] else 0 for k in range(K)]


def stream_cap(n):
    return 1 + 2 * K + 4 * MAX_LANES + 2 * n


def _bits(occ):
    return (np.asarray(occ).reshape(-1) != 0)


def coded_symbols(x_hat, occ):
    """-> (tot, f per bucket, freqs, starts of the coded symbols)"""
    b = buckets(x_hat)
    o = _bits(occ)
    assert o.size == b.size
    tot, _, f = calibrate(b, o)
    fv = np.array(f, np.int64)[b]
    sel = fv > 0
    fo, oo = fv[sel], o[sel]
    freqs = np.where(oo, fo, TOTAL - fo)
    starts = np.where(oo, TOTAL - fo, 0)
    return tot, f, freqs.tolist(), starts.tolist()


def ideal_bytes(x_hat, occ):
    _, _, freqs, _ = coded_symbols(x_hat, occ)
    return sum(math.log2(TOTAL / f) for f in freqs) / 8


def encode(x_hat, occ, lanes=0, info=None):
    """-> bytes.  lanes: 0 = the lane rule, else a forced power of two <= 64.  info (a dict) receives lanes / n_words / m / used."""
    n = int(np.asarray(x_hat).size)
    if n == 0:
        return b''
    tot, f, freqs, starts = coded_symbols(x_hat, occ)
    m = len(freqs)
    L = lanes if lanes else lane_rule((sum(cost256(v) for v in freqs) + 2047) >> 11)
    assert L in (1, 2, 4, 8, 16, 32, 64)
    state = [LOW] * L
    steps = (m + L - 1) // L
    emitted = [None] * steps
    for t in range(steps - 1, -1, -1):
        words = []
        for lane in range(L):
            j = t * L + lane
            if j >= m:
                continue
            x, fr, s = state[lane], freqs[j], starts[j]
            if x >= (fr << 16):
                words.append(x & 0xffff)
                x >>= 16
            state[lane] = ((x // fr) << 16) + (x % fr) + s
        emitted[t] = words
    words = [w for t in range(steps) for w in emitted[t]]
    entries = [f[k] for k in range(K) if tot[k]]
    if info is not None:
        info.update(lanes=L, n_words=len(words), m=m, used=len(entries))
    return (bytes([L.bit_length() - 1]) + np.array(entries, '<u2').tobytes() + np.array(state, '<u4').tobytes()
            + np.array(words, '<u2').tobytes())


def decode(x_hat, string):
    """-> bool array of n voxels (flat); raises OccCorrupt"""
    b = buckets(x_hat)
    n = b.size
    if n == 0:
        if len(string):
            raise OccCorrupt('bytes for an empty block')
        return np.zeros(0, bool)
    if len(string) < 1 or string[0] > 6:
        raise OccCorrupt('no lane byte, or log2(lanes) > 6')
    L = 1 << string[0]
    tot = np.bincount(b, minlength=K)
    used = [k for k in range(K) if tot[k]]
    rest = len(string) - 1 - 2 * len(used) - 4 * L
    if rest < 0 or rest % 2:
        raise OccCorrupt('the length does not match the header')
    f = [0] * K
    for k, v in zip(used, np.frombuffer(string, '<u2', len(used), 1).tolist()):
        f[k] = v
    fv = np.array(f, np.int64)[b]
    coded = np.flatnonzero(fv > 0)
    m, n_words = coded.size, rest // 2
    if n_words > m:
        raise OccCorrupt('more words than coded symbols')
    pos = 1 + 2 * len(used)
    state = [int(v) for v in np.frombuffer(string, '<u4', L, pos)]
    words = np.frombuffer(string, '<u2', n_words, pos + 4 * L)
    out = np.zeros(n, bool)
    cursor = 0
    for j, i in enumerate(coded.tolist()):
        lane, fr = j % L, int(fv[i])
        x = state[lane]
        slot = x & 0xffff
        bit = slot >= TOTAL - fr
        freq, start = (fr, TOTAL - fr) if bit else (TOTAL - fr, 0)
        x = freq * (x >> 16) + slot - start
        if x < LOW:
            if cursor >= n_words:
                raise OccCorrupt('ran out of words')
            x = (x << 16) | int(words[cursor])
            cursor += 1
        state[lane] = x
        out[i] = bit
    if cursor != n_words or any(x != LOW for x in state):
        raise OccCorrupt('string does not end where its symbols do')
    return out


# ---- the seeded inputs of the tests (ISSUE: sizes x x_hat models x occupancies) ---------------------------------------------------
SIZES = (1, 63, 64, 65, 125, 4097)
MODELS = ('zero', 'uniform', 'equal', 'falloff')
OCCS = ('empty', 'full', 'single', 'half')


def shell_block(res=64, radius=25.0, thickness=1.0):
    g = np.arange(res, dtype=np.float64) - (res - 1) / 2
    d = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    return np.abs(d - radius) <= thickness / 2, np.abs(d - radius)


def make_occ(kind, n, rng):
    o = np.zeros(n, bool)
    if kind == 'full':
        o[:] = True
    elif kind == 'single':
        o[int(rng.integers(0, n))] = True
    elif kind == 'half':
        o = rng.random(n) < 0.5
    return o


def make_x_hat(model, occ, rng, dist=None):
    """dist: distance of every voxel to the surface (the shell); flat inputs use the distance to the nearest occupied index"""
    n = occ.size
    if model == 'zero':
        return np.zeros(n, np.float32)
    if model == 'uniform':
        return rng.random(n).astype(np.float32)
    if model == 'equal':
        return occ.astype(np.float32)
    if dist is None:
        idx = np.flatnonzero(occ)
        if idx.size == 0:
            dist = np.full(n, 1e9)
        else:
            pos = np.arange(n)
            k = np.clip(np.searchsorted(idx, pos), 0, idx.size - 1)
            dist = np.minimum(np.abs(pos - idx[k]), np.abs(pos - idx[np.maximum(k - 1, 0)])).astype(np.float64)
    x = np.exp(-dist.reshape(-1) / 1.5) + 0.15 * rng.standard_normal(n)
    x[dist.reshape(-1) > 3] = 0
    return np.clip(x, 0, None).astype(np.float32)            # (values above 1 stay: the ReLU output is not clipped here)


def cases(with_shell=True):
    """yields (name, x_hat flat fp32, occ flat bool)"""
    for n in SIZES:
        for oi, ok in enumerate(OCCS):
            for mi, mk in enumerate(MODELS):
                rng = np.random.default_rng(1000 * n + 10 * oi + mi)
                occ = make_occ(ok, n, rng)
                yield f'n{n}-{ok}-{mk}', make_x_hat(mk, occ, rng), occ
    if with_shell:
        occ, dist = shell_block()
        for mi, mk in enumerate(MODELS):
            rng = np.random.default_rng(77 + mi)
            yield f'shell64-{mk}', make_x_hat(mk, occ.reshape(-1), rng, dist), occ.reshape(-1)
