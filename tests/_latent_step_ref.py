"""Plain numpy restatement of the latent step: the ladder, the three stepped element-wise kernels (pcc_quantize_step_pack,
pcc_index_pack_step, pcc_unpack_dequantize_step), the cost table and the rate ladder (pcc_rate_ladder; csrc/latent_step.hip).  The yardstick
of tests/test_latent_step_cpu.py and tests/test_latent_step_gpu.py.  Nothing is imported from the package; the un-stepped arithmetic is
tests/_pack_ref.py's.

Arithmetic.  Everything is float32, one rounding per operation: t = v / step and s = sigma / step are numpy's float32 divisions (IEEE,
correctly rounded), deq = float32(sym) * step one multiply, the medians one more add.  Subnormal quotients are outside the contract.
"""
import numpy as np

import _pack_ref as P

F32 = np.float32
STEPS = 64


def latent_step(q):
    """(8 + (q & 7)) * 2^((q >> 3) - 5) in float64 arithmetic on exact values"""
    q = int(q)
    assert 0 <= q < STEPS
    return (8 + (q & 7)) * 2.0 ** ((q >> 3) - 5)


def _per_block(q, shape):
    """float32 step of every element of an (N, ..., C) tensor from one ladder index per block"""
    q = np.asarray(q).reshape(-1)
    assert q.size == shape[0]
    step = np.array([latent_step(v) for v in q], F32)
    return step.reshape((shape[0],) + (1,) * (len(shape) - 1))


def quantize_step(v, q, medians=None, mode=P.FLOOR_HALF):
    """(sym int32, deq float32): the un-stepped quantiser on v / step, then deq = float32(sym) * step + medians"""
    v = np.asarray(v, F32)
    step = _per_block(q, v.shape)
    sym, _ = P.quantize((v / step).astype(F32), medians, mode)
    deq = (sym.astype(F32) * step).astype(F32)
    if medians is not None:
        deq = (deq + np.asarray(medians, F32)).astype(F32)
    return sym, deq


def index_step(sigma, table, q):
    sigma = np.asarray(sigma, F32)
    with np.errstate(invalid='ignore'):
        return P.scale_index((sigma / _per_block(q, sigma.shape)).astype(F32), table)


def dequantize_step(sym, q, medians=None):
    sym = np.asarray(sym, np.int32)
    deq = (sym.astype(F32) * _per_block(q, sym.shape)).astype(F32)
    return deq if medians is None else (deq + np.asarray(medians, F32)).astype(F32)


# ---- the cost model -----------------------------------------------------------------------------------------------------------------------
def cost_table(cdf, cdf_size, precision=16):
    """cost16[row][b] = int(rint(65536 * (precision - log2(cdf[b + 1] - cdf[b])))) in float64; (rows, stride - 1) uint32, absent bins 0"""
    cdf = np.asarray(cdf, np.int64)
    cost = np.zeros((cdf.shape[0], cdf.shape[1] - 1), np.uint32)
    for r in range(cdf.shape[0]):
        for b in range(int(cdf_size[r]) - 1):
            f = int(cdf[r, b + 1] - cdf[r, b])
            assert f > 0
            cost[r, b] = int(np.rint(65536.0 * (precision - np.log2(np.float64(f)))))
    return cost


def symbol_bits16(sym, rows, cost, cdf_size, offset, overflow_width=4):
    """Cost of every symbol in units of 2^-16 bit (int64), the bin and the escape as the host range coder's encode_stream takes them"""
    sym, rows = np.asarray(sym, np.int64).ravel(), np.asarray(rows, np.int64).ravel()
    ow, omax = int(overflow_width), (1 << int(overflow_width)) - 1
    v = sym - np.asarray(offset, np.int64)[rows]
    m = np.asarray(cdf_size, np.int64)[rows] - 2
    inside = (v >= 0) & (v < m)
    bits = np.asarray(cost, np.int64)[rows, np.where(inside, v, m)]
    for i in np.flatnonzero(~inside):
        overflow = int(-2 * v[i] - 1 if v[i] < 0 else 2 * (v[i] - m[i])) & 0xFFFFFFFF
        widths = 0
        while widths * ow < 32 and (overflow >> (widths * ow)) != 0:
            widths += 1
        bits[i] += 65536 * ow * (widths // omax + 1 + widths)
    return bits


def rate_ladder(y, sigma, table, mode, steps, cost, cdf_size, offset, overflow_width=4):
    """int64 (N, J): bits16[n][j] = sum over block n of symbol_bits16 under step steps[j]"""
    y, sigma = np.asarray(y, F32), np.asarray(sigma, F32)
    out = np.zeros((y.shape[0], len(steps)), np.int64)
    for j, q in enumerate(steps):
        qs = np.full(y.shape[0], q)
        sym, _ = quantize_step(y, qs, None, mode)
        rows = index_step(sigma, table, qs)
        for n in range(y.shape[0]):
            out[n, j] = symbol_bits16(sym[n], rows[n], cost, cdf_size, offset, overflow_width).sum()
    return out
