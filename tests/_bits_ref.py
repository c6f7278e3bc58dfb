"""Deterministic test tensors that depend on no library RNG: the inputs of the recorded-bits tests (tests/golden/family_bits.json).

Every element is a function of (tag, flat index) alone: the 64-bit FNV-1a hash of the tag seeds a splitmix64 step per element, done in
numpy.uint64 arithmetic (wrapping multiplies, shifts, xors: the same bits under every numpy version, unlike numpy.random streams, which
numpy only promises per BitGenerator and never for the distributions on top).  Values are k / 2^12 with integer k in a stated range,
so activations, biases and residuals are exact in fp32 (at most 14 significant bits; fp16 storage rounds them, as it rounds any
tensor), and a float64 oracle reads exactly the numbers the kernel reads.
"""
import numpy as np

_M64 = (1 << 64) - 1
_Q = 4096.0          # 2^12


def tag_seed(tag):
    """64-bit FNV-1a of the tag's UTF-8 bytes (plain Python integers)."""
    h = 0xCBF29CE484222325
    for b in tag.encode('utf-8'):
        h = ((h ^ b) * 0x100000001B3) & _M64
    return h


def splitmix64(seed, n):
    """The first n outputs of splitmix64 started at `seed`, as numpy.uint64: output i mixes seed + (i + 1) * 0x9E3779B97F4A7C15."""
    with np.errstate(over='ignore'):
        z = np.uint64(seed) + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


# kind -> (bits of k, i.e. k in [-2^(bits-1), 2^(bits-1) - 1])
_KBITS = {'act': 14, 'residual': 14, 'bias': 12, 'weight': 13}


def tensor(tag, shape, kind, fan_in=None):
    """float32 array of `shape`, element i (C order) from hash(tag, i):

    'act'       k in [-8192, 8191], value k / 2^12 in [-2, 2); an element is an exact zero where bits 40.. of its hash, mod 10, are
                below 3 (about 30 %, like a ReLU output)
    'residual'  k in [-8192, 8191], value k / 2^12
    'bias'      k in [-2048, 2047], value k / 2^12 in [-0.5, 0.5)
    'weight'    k in [-4096, 4095]; value (k / 2^12) / sqrt(fan_in) computed in float64 and rounded to fp32 once.  fan_in defaults to
                shape[0] * shape[1] * shape[2] * shape[3] (a forward Keras kernel (k, k, k, cin, cout)); a transposed kernel
                (k, k, k, cout, cin) passes fan_in = k^3 * cin.
    """
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    h = splitmix64(tag_seed(tag), n)
    bits = _KBITS[kind]
    k = (h & np.uint64((1 << bits) - 1)).astype(np.int64) - (1 << (bits - 1))
    v = k.astype(np.float64) / _Q
    if kind == 'act':
        v[((h >> np.uint64(40)) % np.uint64(10)) < np.uint64(3)] = 0.0
    elif kind == 'weight':
        if fan_in is None:
            assert len(shape) == 5, 'weight: give fan_in for a shape that is not (k, k, k, cin, cout)'
            fan_in = shape[0] * shape[1] * shape[2] * shape[3]
        v = v / np.sqrt(np.float64(fan_in))
    return v.astype(np.float32).reshape(shape)


def digest(a):
    """blake2b-128 of an array's bytes (C order, the array's own dtype), as hex."""
    import hashlib
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=16).hexdigest()
