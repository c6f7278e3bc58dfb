"""Host restatement of the "rans1" string format, written from the format's description alone: plain Python /
numpy, one symbol at a time.  The GPU tests compare the device coder's bytes with these, and each side decodes the other's strings.

Format of one string (little-endian): one byte log2(L); the escape count as a LEB128 varint; L final states of 4 bytes; the 16-bit
words in the decoder's read order; the escapes, 4 bytes each, in symbol order.  n = 0 codes as b''.
State in [2^16, 2^32), initial state 2^16, 16-bit renormalisation, 16-bit probabilities.  Symbol i belongs to lane i % L at step
i // L.  The decoder walks the steps upwards; after decoding its symbol a lane whose state fell below 2^16 reads one word from the one
forward cursor, lanes in ascending order within a step."""
import numpy as np

PRECISION = 16
LOW = 1 << 16
MAX_LANES = 64


class RansCorrupt(ValueError):
    pass


def cost256(f):
    """256 * (an upper bound of log2(65536 / f)) in integers: f = 2^k + r -> 256 (16 - k) - ((r << 8) >> k)."""
    f = int(f)
    assert 1 <= f <= 65535
    k = f.bit_length() - 1
    r = f - (1 << k)
    return 256 * (16 - k) - ((r << 8) >> k)


def est_bytes(freqs):
    return (sum(cost256(f) for f in freqs) + 2047) >> 11


def lane_rule(est):
    """the largest power of two L <= 64 with 128 L <= est, at least 1"""
    lanes = 1
    while lanes < MAX_LANES and 128 * (2 * lanes) <= est:
        lanes *= 2
    return lanes


def stream_cap(n):
    return 1 + 10 + 4 * MAX_LANES + 2 * n + 4 * n


def _rows(n, index, index_mod):
    if index is not None:
        rows = np.asarray(index).reshape(-1).astype(np.int64)
        assert rows.size == n
        return rows
    assert index_mod > 0
    return np.arange(n, dtype=np.int64) % index_mod


def symbol_bins(cdf, cdf_size, offset, data, index=None, index_mod=0):
    """per symbol (start, freq) of its bin, and the list of escaped raw values in symbol order"""
    data = np.asarray(data).reshape(-1).astype(np.int64)
    rows = _rows(data.size, index, index_mod)
    starts, freqs, escapes = [], [], []
    for v, r in zip(data.tolist(), rows.tolist()):
        m = int(cdf_size[r]) - 2
        b = v - int(offset[r])
        if not 0 <= b < m:
            b = m
            escapes.append(v)
        lo, hi = int(cdf[r][b]), int(cdf[r][b + 1])
        assert 1 <= hi - lo <= 65535, 'every frequency must lie in [1, 65535]'
        starts.append(lo)
        freqs.append(hi - lo)
    return starts, freqs, escapes


def _varint(v):
    out = bytearray()
    while True:
        if v < 0x80:
            out.append(v)
            return bytes(out)
        out.append((v & 0x7f) | 0x80)
        v >>= 7


def encode(cdf, cdf_size, offset, data, index=None, index_mod=0, lanes=0, info=None):
    """-> bytes.  lanes: 0 = the lane rule, else a forced power of two <= 64.  info (a dict) receives lanes / n_words / est_bytes."""
    n = int(np.asarray(data).size)
    if n == 0:
        return b''
    starts, freqs, escapes = symbol_bins(cdf, cdf_size, offset, data, index, index_mod)
    est = est_bytes(freqs)
    L = lanes if lanes else lane_rule(est)
    assert L in (1, 2, 4, 8, 16, 32, 64)
    state = [LOW] * L
    steps = (n + L - 1) // L
    emitted = [None] * steps
    for t in range(steps - 1, -1, -1):
        words = []
        for lane in range(L):
            i = t * L + lane
            if i >= n:
                continue
            x, f, s = state[lane], freqs[i], starts[i]
            if x >= (f << 16):
                words.append(x & 0xffff)
                x >>= 16
            state[lane] = ((x // f) << 16) + (x % f) + s
        emitted[t] = words
    words = [w for t in range(steps) for w in emitted[t]]
    if info is not None:
        info.update(lanes=L, n_words=len(words), est_bytes=est, n_escapes=len(escapes))
    out = bytes([L.bit_length() - 1]) + _varint(len(escapes))
    out += np.array(state, '<u4').tobytes() + np.array(words, '<u2').tobytes()
    out += (np.array(escapes, np.int64) & 0xffffffff).astype('<u4').tobytes()
    return out


def parse_header(string, n):
    """-> (L, n_escapes, offset of the states, n_words); raises RansCorrupt when the header does not fit the string's length"""
    if len(string) < 2:
        raise RansCorrupt('string shorter than its header')
    lg = string[0]
    if lg > 6:
        raise RansCorrupt(f'log2(lanes) = {lg}')
    L = 1 << lg
    esc, shift, pos = 0, 0, 1
    while True:
        if pos >= len(string) or shift > 63:
            raise RansCorrupt('escape count runs past the string')
        b = string[pos]
        pos += 1
        esc |= (b & 0x7f) << shift
        shift += 7
        if b < 0x80:
            break
    rest = len(string) - pos - 4 * L - 4 * esc
    if esc > n or rest < 0 or rest % 2 or rest // 2 > n:
        raise RansCorrupt('header does not match the length of the string')
    return L, esc, pos, rest // 2


def decode(cdf, cdf_size, offset, string, n, index=None, index_mod=0):
    """-> int32 array of n symbols; raises RansCorrupt"""
    n = int(n)
    if n == 0:
        if len(string):
            raise RansCorrupt('bytes for an empty stream')
        return np.zeros(0, np.int32)
    rows = _rows(n, index, index_mod)
    L, n_esc, pos, n_words = parse_header(string, n)
    state = [int(v) for v in np.frombuffer(string, '<u4', L, pos)]
    words = np.frombuffer(string, '<u2', n_words, pos + 4 * L)
    escapes = np.frombuffer(string, '<i4', n_esc, pos + 4 * L + 2 * n_words)
    out = np.zeros(n, np.int32)
    cursor = ecursor = 0
    for i in range(n):
        lane, r = i % L, int(rows[i])
        row, m = cdf[r], int(cdf_size[r]) - 2
        x = state[lane]
        slot = x & 0xffff
        b = int(np.searchsorted(row[:m + 2], slot, side='right')) - 1
        if not 0 <= b <= m:
            raise RansCorrupt('slot outside the table')
        lo, hi = int(row[b]), int(row[b + 1])
        x = (hi - lo) * (x >> 16) + slot - lo
        if x < LOW:
            if cursor >= n_words:
                raise RansCorrupt('ran out of words')
            x = (x << 16) | int(words[cursor])
            cursor += 1
        state[lane] = x
        if b == m:
            if ecursor >= n_esc:
                raise RansCorrupt('ran out of escapes')
            out[i] = escapes[ecursor]
            ecursor += 1
        else:
            out[i] = b + int(offset[r])
    if cursor != n_words or ecursor != n_esc or any(x != LOW for x in state):
        raise RansCorrupt('string does not end where its symbols do')
    return out
