"""numpy restatement of the two-piece fp16 conv arithmetic (csrc/conv_wino_f16s.hip, csrc/conv_tr2m_f16s.hip).

Every operand x of a product is carried as two fp16 pieces under an exact power-of-two scale, x ~ (h + l) / s with
h = fp16_rn(s x), l = fp16_rn(s x - h) (round to nearest even, denormals kept); all four piece products are kept.  The products of
fp16 pieces are exact in fp32, so the only thing the kernels add on top of this model is the fp32 accumulation of the products, which
the model does in float64.  What the model returns per output:

    value   the result with every product summed in float64
    A       the same computation on the absolute values of every piece product, pushed through |A^T| .. |A| (the Winograd output
            transform), the bias and the residual: the scale an accumulation error is relative to
    n       the number of accumulated terms behind the output
    bound   a derived bound on |value - exact convolution| (operand errors only; tests/test_f16s_model_cpu.py derives it)

`pieces=None` models the exact-fp32 siblings (conv16_wino, conv_tr2m): fp32 operands, no split, no scale.  `mutate` restates one
mistake a kernel could make ('drop_ll', 'flush_l', 'no_clamp', 'bias_s_only'); tests use it to show that the assertions would see it.
numpy only."""
import numpy as np

U32 = 2.0 ** -24            # unit roundoff of fp32
SPLIT_REL = 2.0 ** -22      # two fp16 significands
SPLIT_ABS = 2.0 ** -25      # half a denormal step of fp16
F16_MIN_NORMAL = 2.0 ** -14

G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def split_f16(v, flush=False):
    """v float32 (already scaled) -> (h, l) as float32 arrays holding fp16 values.  v - h is exact in fp32."""
    v = np.asarray(v, np.float32)
    with np.errstate(over='ignore'):
        h = v.astype(np.float16).astype(np.float32)
        l = (v - h).astype(np.float16).astype(np.float32)
    if flush:
        l = np.where(np.abs(l) < F16_MIN_NORMAL, np.float32(0), l)
    return h, l


def weight_scale_log2(w):
    """f16s_weight_scale (csrc/kernel_common.h): su = 2^(14 - e), max |w| = f 2^e with f in [0.5, 1), exponent kept in +-100."""
    a = np.abs(np.asarray(w, np.float32))
    a = a[a <= np.float32(3.0e38)]
    wmax = float(a.max()) if a.size else 0.0
    if wmax == 0.0:
        return 0
    e = int(np.frexp(np.float32(wmax))[1])
    return int(np.clip(14 - e, -100, 100))


def block_scale_log2(x_block, lsu, base, clamp=True):
    """f16s_scale_bits / tr2m_scale_bits: biased exponent of s = base - (bits of max |x| >> 23), base = 266 (Winograd) | 268 (march),
    kept inside [max(7 - lsu, 1), min(247 - lsu, 254)]; an all-zero block takes s = 1.  Returns log2 s."""
    a = np.abs(np.asarray(x_block, np.float32))
    a = a[np.isfinite(a)]
    m = int(np.float32(a.max() if a.size else 0.0).view(np.uint32))
    if m == 0:
        return 0
    se = base - (m >> 23)
    if clamp:
        se = min(max(se, max(7 - lsu, 1)), min(247 - lsu, 254))
    return se - 127


def _bt(a0, a1, a2, a3):
    return a0 - a2, a1 + a2, a2 - a1, a1 - a3


def _bt_abs(a0, a1, a2, a3):
    return a0 + a2, a1 + a2, a2 + a1, a1 + a3


def wino_patches(x):
    """(N, D, H, W, C) -> (N, D, H/2, W/2, 4, 4, C): the 4 x 4 input patch (zero padded) of every 2 x 2 output tile."""
    N, D, H, W, C = x.shape
    xp = np.zeros((N, D, H + 2, W + 2, C), x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    d = np.empty((N, D, H // 2, W // 2, 4, 4, C), x.dtype)
    for dy in range(4):
        for dx in range(4):
            d[:, :, :, :, dy, dx] = xp[:, :, dy:dy + H:2, dx:dx + W:2]
    return d


def wino_input_transform(x):
    """V = B^T d B in fp32, along x first, then y: one rounded add per step.  Returns (V, Vabs), Vabs = |B^T| |d| |B| in float64."""
    d = wino_patches(np.asarray(x, np.float32))
    t = np.stack(_bt(*[d[..., i, :] for i in range(4)]), axis=-2)               # along x (axis 5)
    V = np.stack(_bt(*[t[..., i, :, :] for i in range(4)]), axis=-3)            # along y (axis 4)
    da = np.abs(d).astype(np.float64)
    ta = np.stack(_bt_abs(*[da[..., i, :] for i in range(4)]), axis=-2)
    Va = np.stack(_bt_abs(*[ta[..., i, :, :] for i in range(4)]), axis=-3)
    assert V.dtype == np.float32
    return V, Va


def wino_weights(wlog):
    """U = G g G^T in float64, rounded to fp32.  wlog: logical taps (3, 3, 3, Cin, Cout) -> (3, 4, 4, Cin, Cout)."""
    return np.einsum('pi,qj,zijcd->zpqcd', G, G, np.asarray(wlog, np.float64)).astype(np.float32)


def logical_taps(w, transposed):
    """Keras layout -> W(kz, ky, kx, ci, co) of out[o] = sum W(k) in[o + k - 1] (stride 1; transposed layers: taps flipped)."""
    w = np.asarray(w, np.float32)
    return w if not transposed else np.ascontiguousarray(w[::-1, ::-1, ::-1].transpose(0, 1, 2, 4, 3))


def _zmm(Vz, Uz):
    """sum over the 3 z taps and cin: Vz (N, D, TY, TX, 4, 4, Cin), Uz (3, 4, 4, Cin, Cout) -> (N, D, TY, TX, 4, 4, Cout), float64."""
    N, D = Vz.shape[:2]
    Vp = np.zeros((N, D + 2) + Vz.shape[2:], np.float64)
    Vp[:, 1:-1] = Vz
    Vt = np.moveaxis(Vp, (4, 5), (0, 1))                         # (4, 4, N, D + 2, TY, TX, Cin)
    out = 0
    for kz in range(3):
        a = Vt[:, :, :, kz:kz + D]
        sh = a.shape
        out = out + np.matmul(a.reshape(4, 4, -1, sh[-1]), np.asarray(Uz[kz], np.float64)).reshape(sh[:-1] + (Uz.shape[-1],))
    return np.moveaxis(out, (0, 1), (4, 5))


def _out_transform(M, absolute=False):
    """A^T M A per tile -> (N, D, H, W, Cout)."""
    A = np.abs(AT) if absolute else AT
    S = np.einsum('ap,bq,nzyxpqc->nzyaxbc', A, A, M)
    N, D, TY, _, TX, _, C = S.shape
    return S.reshape(N, D, 2 * TY, 2 * TX, C)


def _epilogue(S, Sabs, Sbound, ls, lsu, bias, relu, res, mutate):
    """The kernels' epilogue on the scaled sums of ONE block: bias rides in the accumulator scaled by su s, ReLU, un-scale, residual."""
    with np.errstate(over='ignore', divide='ignore'):
        sprod = np.ldexp(np.float32(1), lsu) * np.ldexp(np.float32(1), ls)          # fp32, as the kernel forms it
        sinv = np.float32(1.0) / sprod
    bs = np.ldexp(np.float32(1), ls) if mutate == 'bias_s_only' else sprod
    if bias is not None:
        with np.errstate(over='ignore', invalid='ignore'):
            b = (np.asarray(bias, np.float32) * bs).astype(np.float64)
        S = S + b
        Sabs = Sabs + np.abs(np.asarray(bias, np.float64)) * float(sprod)
    if relu:
        S = np.maximum(S, 0)
    with np.errstate(over='ignore', invalid='ignore'):
        v, a, bd = S * float(sinv), Sabs * float(sinv), Sbound * float(sinv)
    if res is not None:
        v = v + np.asarray(res, np.float64)
        a = a + np.abs(np.asarray(res, np.float64))
    return v, a, bd


def wino_model(x, w, transposed, bias=None, relu=False, res=None, pieces=2, mutate=None):
    """conv16_wino_f16s_kernel (pieces=2) or conv16_wino_kernel (pieces=None) on x (N, D, H, W, C), Keras weights w."""
    x = np.asarray(x, np.float32)
    N, D, H, W, C = x.shape
    U = wino_weights(logical_taps(w, transposed))
    V, Va = wino_input_transform(x)
    Ua, Vabs32 = np.abs(U.astype(np.float64)), np.abs(V.astype(np.float64))
    eV32 = (2 * U32 + U32 * U32) * Va                          # two fp32 roundings per entry of V
    eU32 = U32 / (1 - U32) * Ua                                # one fp32 rounding of U
    Vup = Vabs32 + eV32                                        # >= |exact V|
    value = np.empty((N, D, H, W, U.shape[-1]), np.float64)
    A, bound = np.empty_like(value), np.empty_like(value)
    n = 3 * C * (4 if pieces else 1) + 8 + 3
    if not pieces:
        S = _out_transform(_zmm(V, U))
        Sa = _out_transform(_zmm(Vabs32, Ua), True)
        Sb = _out_transform(_zmm(Vup, eU32) + _zmm(eV32, Ua), True)
        for b in range(N):
            value[b], A[b], bound[b] = _epilogue(S[b], Sa[b], Sb[b], 0, 0, bias, relu, None if res is None else res[b], None)
        return dict(value=value, A=A, n=n, bound=bound + 2.0 ** -50 * A)
    lsu = weight_scale_log2(U)
    Uh, Ul = split_f16(U * np.float32(2.0 ** lsu))
    if mutate == 'flush_l':
        Ul = split_f16(U * np.float32(2.0 ** lsu), flush=True)[1]
    Uf, Upa = Uh.astype(np.float64) + Ul, np.abs(Uh).astype(np.float64) + np.abs(Ul)
    rU = np.maximum(SPLIT_REL * Ua, SPLIT_ABS / 2.0 ** lsu)    # split residual of U (operand units)
    eU, Uup = eU32 + rU, Ua + rU
    scales = []
    for b in range(N):
        ls = block_scale_log2(x[b], lsu, 266, clamp=mutate != 'no_clamp')
        scales.append(ls)
        Vs = V[b:b + 1] * np.float32(2.0 ** ls)                # exact: a power of two, no over- or underflow inside the clamp
        Vh, Vl = split_f16(Vs, flush=mutate == 'flush_l')
        M = _zmm(Vh.astype(np.float64) + Vl, Uf)
        if mutate == 'drop_ll':
            M = M - _zmm(Vl, Ul)
        Ma = _zmm(np.abs(Vh).astype(np.float64) + np.abs(Vl), Upa)
        eV = eV32[b:b + 1] + np.maximum(SPLIT_REL * Vabs32[b:b + 1], SPLIT_ABS / 2.0 ** ls)
        Mb = (_zmm(Vup[b:b + 1], eU) + _zmm(eV, Uup)) * 2.0 ** (ls + lsu)
        value[b], A[b], bound[b] = _epilogue(_out_transform(M)[0], _out_transform(Ma, True)[0], _out_transform(Mb, True)[0], ls, lsu,
                                             bias, relu, None if res is None else res[b], mutate)
    return dict(value=value, A=A, n=n, bound=bound + 2.0 ** -50 * A, lsu=lsu, ls=scales)


def _tr2_scatter(xb, wt):
    """Conv3DTranspose k3 stride 2 'same' as the kernels gather it: out[2 i + k] += in[i] . w[k] (k = 0, 1, 2; no flip; planes past
    2 n dropped).  xb (N, D, H, W, Cin) float64, wt (3, 3, 3, Cout, Cin) float64 -> (N, 2D, 2H, 2W, Cout)."""
    N, D, H, W, _ = xb.shape
    out = np.zeros((N, 2 * D + 2, 2 * H + 2, 2 * W + 2, wt.shape[3]), np.float64)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                out[:, kz:kz + 2 * D:2, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += np.matmul(xb, wt[kz, ky, kx].T)
    return out[:, :2 * D, :2 * H, :2 * W]


def tr2_term_count(D, H, W, cin, per_product):
    """terms behind each output of the stride-2 layer: taps of its parity class (2 per even coordinate, 1 per odd) x Cin x pieces + 3"""
    t = [np.where(np.arange(2 * n) % 2 == 0, 2, 1) for n in (D, H, W)]
    taps = t[0][:, None, None] * t[1][None, :, None] * t[2][None, None, :]
    return (taps * cin * per_product + 3)[None, ..., None]


def tr2m_model(x, w, bias=None, relu=False, pieces=2, mutate=None):
    """conv_tr2m_f16s_kernel (pieces=2) or conv_tr2m_kernel (pieces=None): x (N, D, H, W, Cin), w (3, 3, 3, Cout, Cin)."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    N, D, H, W, C = x.shape
    wa, xa = np.abs(w.astype(np.float64)), np.abs(x.astype(np.float64))
    n = tr2_term_count(D, H, W, C, 4 if pieces else 1)
    value = np.empty((N, 2 * D, 2 * H, 2 * W, w.shape[3]), np.float64)
    A, bound = np.empty_like(value), np.empty_like(value)
    if not pieces:
        S, Sa = _tr2_scatter(x.astype(np.float64), w.astype(np.float64)), _tr2_scatter(xa, wa)
        for b in range(N):
            value[b], A[b], bound[b] = _epilogue(S[b], Sa[b], 0 * Sa[b], 0, 0, bias, relu, None, None)
        return dict(value=value, A=A, n=n, bound=bound + 2.0 ** -50 * A)
    lsu = weight_scale_log2(w)
    wh, wl = split_f16(w * np.float32(2.0 ** lsu), flush=mutate == 'flush_l')
    wf, wpa = wh.astype(np.float64) + wl, np.abs(wh).astype(np.float64) + np.abs(wl)
    eW = np.maximum(SPLIT_REL * wa, SPLIT_ABS / 2.0 ** lsu)
    scales = []
    for b in range(N):
        ls = block_scale_log2(x[b], lsu, 268, clamp=mutate != 'no_clamp')
        scales.append(ls)
        xh, xl = split_f16(x[b:b + 1] * np.float32(2.0 ** ls), flush=mutate == 'flush_l')
        S = _tr2_scatter(xh.astype(np.float64) + xl, wf)
        if mutate == 'drop_ll':
            S = S - _tr2_scatter(xl.astype(np.float64), wl.astype(np.float64))
        Sa = _tr2_scatter(np.abs(xh).astype(np.float64) + np.abs(xl), wpa)
        eX = np.maximum(SPLIT_REL * xa[b:b + 1], SPLIT_ABS / 2.0 ** ls)
        Sb = (_tr2_scatter(xa[b:b + 1], eW) + _tr2_scatter(eX, wa + eW)) * 2.0 ** (ls + lsu)
        value[b], A[b], bound[b] = _epilogue(S[0], Sa[0], Sb[0], ls, lsu, bias, relu, None, mutate)
    return dict(value=value, A=A, n=n, bound=bound + 2.0 ** -50 * A, lsu=lsu, ls=scales)


# ---- the float64 reference: a plain direct convolution, independent of everything above
def direct_conv(x, w, transposed, stride, bias=None, relu=False, res=None):
    """(exact value in float64, T = sum of |terms| incl. |bias| and |residual|).  Stride-1 layers gather over the logical taps."""
    x64, xa = np.asarray(x, np.float64), np.abs(np.asarray(x, np.float64))
    if stride == 2:
        # gathered per output parity, not scattered like the model: even coordinate 2 i reads (tap 0, in[i]) and (tap 2, in[i - 1]),
        # odd coordinate 2 i + 1 reads (tap 1, in[i])
        w64 = np.asarray(w, np.float64)
        N, D, H, W, C = x64.shape
        v, t = np.zeros((N, 2 * D, 2 * H, 2 * W, w64.shape[3])), np.zeros((N, 2 * D, 2 * H, 2 * W, w64.shape[3]))
        xp, xpa = np.zeros((N, D + 1, H + 1, W + 1, C)), np.zeros((N, D + 1, H + 1, W + 1, C))
        xp[:, 1:, 1:, 1:], xpa[:, 1:, 1:, 1:] = x64, xa
        taps = {0: ((0, 1), (2, 0)), 1: ((1, 1),)}             # parity -> (tap, offset into the padded input)
        for pz in range(2):
            for py in range(2):
                for px in range(2):
                    for kz, oz in taps[pz]:
                        for ky, oy in taps[py]:
                            for kx, ox in taps[px]:
                                a = (slice(None), slice(oz, oz + D), slice(oy, oy + H), slice(ox, ox + W))
                                o = (slice(None), slice(pz, None, 2), slice(py, None, 2), slice(px, None, 2))
                                v[o] += np.matmul(xp[a], w64[kz, ky, kx].T)
                                t[o] += np.matmul(xpa[a], np.abs(w64[kz, ky, kx]).T)
    else:
        wl = logical_taps(w, transposed).astype(np.float64)
        N, D, H, W, C = x64.shape
        v, t = np.zeros((N, D, H, W, wl.shape[-1])), np.zeros((N, D, H, W, wl.shape[-1]))
        xp, xpa = np.zeros((N, D + 2, H + 2, W + 2, C)), np.zeros((N, D + 2, H + 2, W + 2, C))
        xp[:, 1:-1, 1:-1, 1:-1], xpa[:, 1:-1, 1:-1, 1:-1] = x64, xa
        for kz in range(3):
            for ky in range(3):
                for kx in range(3):
                    v += np.matmul(xp[:, kz:kz + D, ky:ky + H, kx:kx + W], wl[kz, ky, kx])
                    t += np.matmul(xpa[:, kz:kz + D, ky:ky + H, kx:kx + W], np.abs(wl[kz, ky, kx]))
    if bias is not None:
        v, t = v + np.asarray(bias, np.float64), t + np.abs(np.asarray(bias, np.float64))
    if relu:
        v = np.maximum(v, 0)
    if res is not None:
        v, t = v + np.asarray(res, np.float64), t + np.abs(np.asarray(res, np.float64))
    return v, t
