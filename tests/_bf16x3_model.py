"""numpy restatement of the three-piece bf16 conv arithmetic (csrc/conv_split.hip, csrc/conv_tr2m_bf16.hip, csrc/conv_wino_bf16.hip, DESIGN.md
section 4.2).

Every operand x of a product is carried as three bf16 pieces, x = h + m + l with h = bf16_rn(x), m = bf16_rn(x - h), l = bf16_rn(x - h - m);
both differences are exact in fp32 and so is the sum.  bf16_rn rounds to nearest even and truncates inf / nan: this is the host packer's
rule (bf16_bits / bf16_split3 in csrc/kernel_common.h, which builds every weight image) and also what v_cvt_pk_bf16_f32, the instruction that
splits the input side in the kernels, is taken to do.  Six of the nine piece products are kept -- written (weight piece, input piece): hh, mm,
hl, mh, lh, hm -- and ml, lm, ll are dropped.  A product of two bf16 pieces is exact in fp32, so the only thing the kernels add on top of this
model is the fp32 accumulation of the products (three MFMAs per tap: hh + mm, hl + mh, lh + hm), which the model does in float64.  Per output:

    value   the six-term sums in float64, plus bias, ReLU, residual
    n       the number of NONZERO piece products accumulated into the output, plus one for the bias and one for the residual (Winograd:
            the nonzero products of ONE point's chain -- the longest among the nine points the output reads -- plus 8 for A^T . A and 3 for
            the epilogue, as _f16s_model.wino_model counts; `products` holds the sum over all nine)
    A       the sum of the magnitudes of those terms (Winograd: pushed through |A^T| .. |A|)
    bound   a bound on |value - exact convolution|: the exact magnitude of the dropped terms of that output, sum |m_w l_x| + |l_w m_x| +
            |l_w l_x|, computed from the pieces (no worst-case constant); Winograd adds the fp32 roundings of U = G g G^T and V = B^T d B, which
            the kernel commits before it splits (the terms of _f16s_model.wino_model(pieces=None)); 2^-50 A covers the model's float64 sums

`pieces=None` models the exact-fp32 siblings (conv_fwd, conv_tr2, conv_tr2m, conv16_wino): fp32 operands, one product per operand pair.

DOMAIN.  The model is the kernels' contract for finite operands with |x| below the bf16 maximum (so that h is finite) and every nonzero piece
a normal number.  Outside that -- an |x| that rounds to a bf16 infinity, pieces in the denormal range -- the kernels' behaviour is not pinned
by this model or its tests: in_domain() is asserted on every case that reaches a GPU.

`mutate` restates one mistake a kernel or a packer could make: 'drop_<t>' for t in TERMS, 'zero_x_<p>' / 'zero_w_<p>' for a piece p in h, m,
l, 'trunc' (truncate instead of round in both splits), 'flush' (pieces below 2^-126 become zero).  numpy only."""
import numpy as np

import _f16s_model as F

U32 = F.U32
TERMS = ('hh', 'mm', 'hl', 'mh', 'lh', 'hm')            # (weight piece, input piece), in the kernels' order: three MFMAs of two terms each
STEPS = (('hh', 'mm'), ('hl', 'mh'), ('lh', 'hm'))
DROPPED = ('ml', 'lm', 'll')
MUTATIONS = tuple('drop_' + t for t in TERMS) + tuple(f'zero_{o}_{p}' for o in 'xw' for p in 'hml') + ('trunc', 'flush')
BF16_MAX = float(np.array([0x7f7f0000], np.uint32).view(np.float32)[0])
MIN_NORMAL = 2.0 ** -126


def bf16_rn(v, trunc=False):
    """float32 -> the nearest bf16 as float32 (ties to even; inf / nan truncated), bit for bit bf16_bits of csrc/kernel_common.h"""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    special = (b & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
    r = b if trunc else b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))
    return (np.where(special, b, r) & np.uint32(0xffff0000)).view(np.float32)


def split_bf16x3(v, trunc=False, flush=False):
    """v float32 -> (h, m, l) as float32 arrays holding bf16 values; h + m + l == v wherever h is finite"""
    v = np.ascontiguousarray(v, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        h = bf16_rn(v, trunc)
        r1 = v - h
        m = bf16_rn(r1, trunc)
        l = bf16_rn(r1 - m, trunc)
    if flush:
        h, m, l = (np.where(np.abs(p) < np.float32(MIN_NORMAL), np.float32(0), p) for p in (h, m, l))
    return h, m, l


def in_domain(*arrays):
    """every value finite and below the bf16 maximum, every nonzero piece normal"""
    for a in arrays:
        a = np.asarray(a, np.float32)
        if not (np.isfinite(a).all() and (np.abs(a) < BF16_MAX).all()):
            return False
        h, m, l = split_bf16x3(a)
        if not np.array_equal(h.astype(np.float64) + m + l, a.astype(np.float64)):      # a residual below the smallest bf16 denormal
            return False
        for p in (h, m, l):
            if ((p != 0) & (np.abs(p) < MIN_NORMAL)).any():
                return False
    return True


def _pieces(v, mutate, side):
    """{piece: float64 array} of one operand side ('x' | 'w') under the mutation"""
    p = dict(zip('hml', (q.astype(np.float64) for q in split_bf16x3(v, trunc=mutate == 'trunc', flush=mutate == 'flush'))))
    if mutate and mutate.startswith(f'zero_{side}_'):
        p[mutate[-1]] = np.zeros_like(p['h'])
    return p


def _s1_gather(x, wl):
    """out[o] = sum_k in[o + k - 1] . W(k): x (N, D, H, W, Ci), wl logical taps (3, 3, 3, Ci, Co), float64, zero padding"""
    N, D, H, W, C = x.shape
    xp = np.zeros((N, D + 2, H + 2, W + 2, C), np.float64)
    xp[:, 1:-1, 1:-1, 1:-1] = x
    out = np.zeros((N, D, H, W, wl.shape[-1]), np.float64)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                _madd(out, xp[:, kz:kz + D, ky:ky + H, kx:kx + W], wl[kz, ky, kx])
    return out


def _madd(out, a, w):
    """out += a . w over the last axis; voxels of `a` that are all zero (most of an impulse lattice) are skipped"""
    rows = (a != 0).any(axis=-1)
    if rows.all():
        out += np.matmul(a, w)
    elif rows.any():
        out[rows] += np.matmul(a[rows], w)


def _tr2_gather(x, wt):
    """_f16s_model._tr2_scatter (out[2 i + k] += in[i] . w[k], planes past 2 n dropped) with all-zero voxels skipped"""
    N, D, H, W, _ = x.shape
    out = np.zeros((N, 2 * D + 2, 2 * H + 2, 2 * W + 2, wt.shape[3]), np.float64)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                _madd(out[:, kz:kz + 2 * D:2, ky:ky + 2 * H:2, kx:kx + 2 * W:2], x, wt[kz, ky, kx].T)
    return out[:, :2 * D, :2 * H, :2 * W]


def _six(op, xp, wp, mutate=None, lean=False):
    """The kept terms under the bilinear sum `op(x-side array, w-side array)`: (value, A, n of nonzero products, dropped magnitude); lean: the
    value alone, zeros for the rest."""
    kept = [t for t in TERMS if mutate != 'drop_' + t]
    value = A = n = dropped = 0.0
    for q in 'hml':                                          # grouped by input piece: float64 sums of bf16 pieces are exact
        ws = [t[0] for t in kept if t[1] == q]
        if ws:
            value = value + op(xp[q], sum(wp[p] for p in ws))
        if lean:
            continue
        if ws:
            A = A + op(np.abs(xp[q]), sum(np.abs(wp[p]) for p in ws))
            n = n + op((xp[q] != 0).astype(np.float64), sum((wp[p] != 0).astype(np.float64) for p in ws))
        ws = [t[0] for t in DROPPED if t[1] == q]
        if ws:
            dropped = dropped + op(np.abs(xp[q]), sum(np.abs(wp[p]) for p in ws))
    if lean:
        return value, 0 * value, 0 * value, 0 * value
    return value, A, np.rint(n), dropped


def _three_step(op, xp, wp):
    """fp32 accumulation in the documented order on an output behind ONE (cin group, tap): acc = fl(acc + (two terms)), three times"""
    acc = np.float32(0)
    for step in STEPS:
        s = sum(op(xp[t[1]], wp[t[0]]) for t in step)
        acc = (np.asarray(acc, np.float64) + s).astype(np.float32)
    return acc


def _epilogue(S, Sa, n, bound, bias, relu, res):
    if bias is not None:
        S, Sa, n = S + np.asarray(bias, np.float64), Sa + np.abs(np.asarray(bias, np.float64)), n + 1
    if relu:
        S = np.maximum(S, 0)
    if res is not None:
        S, Sa, n = S + np.asarray(res, np.float64), Sa + np.abs(np.asarray(res, np.float64)), n + 1
    return dict(value=S, A=Sa, n=n, bound=bound + 2.0 ** -50 * Sa)


def _epilogue32(acc, bias, relu, res):
    if bias is not None:
        acc = acc + np.asarray(bias, np.float32)
    if relu:
        acc = np.maximum(acc, np.float32(0))
    if res is not None:
        acc = acc + np.asarray(res, np.float32)
    assert acc.dtype == np.float32
    return acc


def _bilinear(x, w, op, bias, relu, res, pieces, mutate, three_step, lean=False):
    if not pieces:
        x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
        S, Sa = op(x64, w64), op(np.abs(x64), np.abs(w64))
        n = np.rint(op((x64 != 0).astype(np.float64), (w64 != 0).astype(np.float64)))
        m = _epilogue(S, Sa, n, 0 * Sa, bias, relu, res)
        m['products'] = n
        return m
    xp, wp = _pieces(x, mutate, 'x'), _pieces(w, mutate, 'w')
    S, Sa, n, dropped = _six(op, xp, wp, mutate, lean)
    m = _epilogue(S, Sa, n, dropped, bias, relu, res)
    m['products'] = n
    if three_step:
        m['value32'] = _epilogue32(_three_step(op, xp, wp), bias, relu, res)
    return m


def direct_model(x, w, transposed, bias=None, relu=False, res=None, pieces=3, mutate=None, three_step=False, lean=False):
    """conv_k3s1_split_kernel / conv_k3s1_split32_kernel (pieces=3) or conv_fwd (pieces=None): x (N, D, H, W, C), Keras weights w"""
    wl = F.logical_taps(w, transposed)
    return _bilinear(x, wl, _s1_gather, bias, relu, res, pieces, mutate, three_step, lean)


def tr2_model(x, w, bias=None, relu=False, pieces=3, mutate=None, three_step=False, lean=False):
    """conv_tr2_split_kernel / conv_tr2m_bf16_kernel (pieces=3) or conv_tr2 / conv_tr2m (pieces=None): x (N, D, H, W, Cin), w (3, 3, 3, Cout, Cin);
    the gather of _f16s_model._tr2_scatter"""
    return _bilinear(x, np.asarray(w, np.float32), _tr2_gather, bias, relu, None, pieces, mutate, three_step, lean)


def wino_model(x, w, transposed, bias=None, relu=False, res=None, pieces=3, mutate=None, three_step=False, lean=False):
    """conv16_wino_bf16_kernel (pieces=3) or conv16_wino_kernel (pieces=None): V = B^T d B in fp32, then split; U = fl32(G g G^T) split on the
    host; the six terms summed over the z taps and cin per Winograd point; A^T . A; epilogue."""
    x = np.asarray(x, np.float32)
    U = F.wino_weights(F.logical_taps(w, transposed))
    V, Va = F.wino_input_transform(x)
    Ua, Vabs = np.abs(U.astype(np.float64)), np.abs(V.astype(np.float64))
    eV32 = (2 * U32 + U32 * U32) * Va                          # two fp32 roundings per entry of V (exact zeros where the adds are exact)
    eV32 = np.where(_wino_exact(x), 0.0, eV32)
    eU32 = U32 / (1 - U32) * Ua                                # one fp32 rounding of U
    b32 = F._zmm(Vabs + eV32, eU32) + F._zmm(eV32, Ua)
    if not pieces:
        V64, U64 = V.astype(np.float64), U.astype(np.float64)
        M, Ma = F._zmm(V64, U64), F._zmm(Vabs, Ua)
        n = np.rint(F._zmm((V64 != 0).astype(np.float64), (U64 != 0).astype(np.float64)))
        dropped = 0 * Ma
    else:
        xp, wp = _pieces(V, mutate, 'x'), _pieces(U, mutate, 'w')
        M, Ma, n, dropped = _six(F._zmm, xp, wp, mutate, lean)
    prod = np.rint(F._out_transform(n, True))                  # |A^T| .. |A| is a 0 / 1 pattern: the products of every point the output reads
    # n as _f16s_model.wino_model counts: the accumulation chain of ONE point (here the longest of the nine the output reads), + 8 + 3.
    # Valid because A is already the |A^T| .. |A| sum: the error of sum_p a_p M_p is at most c u max_p n_p sum_p |a_p| A_p.
    m = _epilogue(F._out_transform(M), F._out_transform(Ma, True), _out_max(n) + 8 + 3 - (bias is not None) - (res is not None),
                  F._out_transform(dropped + b32, True), bias, relu, res)
    m['products'] = prod
    if three_step and pieces:
        m['value32'] = _epilogue32(F._out_transform(_three_step(F._zmm, xp, wp).astype(np.float64)).astype(np.float32), bias, relu, res)
    return m


def _out_max(n):
    """per output, the largest entry of n (N, D, TY, TX, 4, 4, C) among the 3 x 3 points it reads: rows of A^T = points 0..2 / 1..3"""
    N, D, TY, TX, _, _, C = n.shape
    out = np.empty((N, D, TY, 2, TX, 2, C), n.dtype)
    for a in range(2):
        for b in range(2):
            out[:, :, :, a, :, b] = n[:, :, :, :, a:a + 3, b:b + 3].max(axis=(4, 5))
    return out.reshape(N, D, 2 * TY, 2 * TX, C)


def _wino_exact(x):
    """per entry of V: True where at most one of the four patch elements behind each of its two adds is nonzero, so that B^T d B commits no
    rounding (a lone element passes through with a sign)"""
    nz = (F.wino_patches(np.asarray(x, np.float32)) != 0).astype(np.float64)
    t = np.stack(F._bt_abs(*[nz[..., i, :] for i in range(4)]), axis=-2)
    cnt = np.stack(F._bt_abs(*[t[..., i, :, :] for i in range(4)]), axis=-3)
    return cnt <= 1


def run(family, x, w, transposed, bias=None, relu=False, res=None, pieces=3, mutate=None, three_step=False, lean=False):
    """family: 'direct' (k3 stride 1) | 'tr2' (k3 stride 2 transposed) | 'wino'"""
    if family == 'direct':
        return direct_model(x, w, transposed, bias, relu, res, pieces, mutate, three_step, lean)
    if family == 'tr2':
        assert res is None
        return tr2_model(x, w, bias, relu, pieces, mutate, three_step, lean)
    return wino_model(x, w, transposed, bias, relu, res, pieces, mutate, three_step, lean)


def acc_bound(m, c_acc=2.0):
    """what a kernel may differ from the model by: n terms accumulated in fp32 in some fixed order, and the rounding of the result"""
    return c_acc * m['n'] * U32 * m['A'] + 2.0 ** -23 * np.abs(m['value'])
