"""The occupancy decision that the last synthesis layer folds into its epilogue (csrc/conv_edge.hip, conv_cout1_mfma_kernel<IN16, T,
true>, pcc_thr_fuse) and the point lists compacted from its bits, driven through the codec graph (ops.codec_encode,
ops.codec_decode_main) and compared with numpy on the host (tests/_thr_ref.py) applied to the x_hat that the same call returned:
counts, point rows and every mask word by equality, at thresholds that equal voxels of their block, at 0, -0, 1, the float below 1 and
the ends of the product's threshold grid, for 16 x 16 columns and for 32 x 32 columns with one, two, four and eight z slabs, in the
fp32 and in the fp16 precision.  The reference is never another GPU kernel; ops.threshold_compact is held to the same reference."""
import ctypes as C

import numpy as np
import pytest
import torch

import _direct_cases as DC
import _thr_ref as TR
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ops
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType

pytestmark = pytest.mark.gpu

GAIN = 2.2            # of tests/test_codec_gpu.py::scaled_weights: x_hat reaches from the ReLU's zeros to far above 1 at every resolution here
OCCUPANCY = 0.05


def scaled_weights(model, gain):
    """tests/test_codec_gpu.py::scaled_weights: Glorot kernels times `gain`, small random biases, the last bias at 0.47."""
    w = model.get_weights()
    rng = np.random.default_rng(7)
    for k in list(w):
        if k.endswith('/kernel'):
            w[k] = (w[k] * gain).astype(np.float32)
        if k.endswith('/bias') and not k.startswith('entropy'):
            w[k] = rng.normal(0, 0.05, w[k].shape).astype(np.float32)
    last = max(int(k.split('/')[1]) for k in w if k.startswith('synthesis/'))
    w[f'synthesis/{last}/bias'] = np.array([0.47], np.float32)
    return w


def _model(ctx, case, precision):
    res, batch = case['res'], case['batch']
    m = ModelConfigType['c3p'].build(batch_size=batch, precision=precision)
    m.compress([1, 1, res, res, res])
    m.set_weights(scaled_weights(m, GAIN))
    mc = m._ctx(ctx)
    return m, mc, m._codec(mc)


def _the_case(ctx, cid, precision):
    """The case on THIS machine's CU count, and the launcher's choice for it restated: fail, never skip, when the machine gives another."""
    (case,) = [c for c in TR.cases(ctx.num_cu) if c['id'] == cid]
    assert case['batch'] >= 1, f'{cid}: {ctx.num_cu} CUs leave no batch'
    sel = TR.last_layer(case, precision, ctx.num_cu)
    assert sel['kernel'] == TR.kernel_name(case, precision) and sel['zsp'] == case['zsp'], \
        f'{cid} ({precision}): with {ctx.num_cu} CUs and batch {case["batch"]} the launcher takes {sel["kernel"]} with {sel["zsp"]} slabs'
    return case, sel


class Scratch:
    """The compaction scratch, prefilled: [plane counts, padded to 4 ints][batch * voxels / 32 mask words][the rest]."""
    def __init__(self, ctx, batch, res):
        self.n = L.lib().pcc_threshold_scratch_ints(batch, res, res, res)
        self.off = (batch * res + 3) // 4 * 4
        self.words = batch * res ** 3 // 32
        fill = TR.PREFILL - (1 << 32) if TR.PREFILL >= 1 << 31 else TR.PREFILL
        self.t = torch.full((self.n,), fill, dtype=torch.int32, device=ctx.device)

    def mask(self):
        return self.t[self.off:self.off + self.words].cpu().numpy().view(np.uint32)

    def behind(self):
        return self.t[self.off + self.words:].cpu().numpy().view(np.uint32)


def _check_side(ctx, mc, what, t, scratch, thr, recipes, clip, fused):
    """Counts, rows and mask words of one call against numpy on the x_hat it returned; ops.threshold_compact against the same rows."""
    xh = t['x_hat'].cpu().numpy()
    B, res = xh.shape[0], xh.shape[1]
    counts = t['counts'].cpu().numpy()
    words = scratch.mask().reshape(B, -1) if fused else None
    sa_xyz, sa_cnt = ops.threshold_compact(mc, t['x_hat'], torch.from_numpy(thr).to(ctx.device), clip=clip)
    sa_cnt = sa_cnt.cpu().numpy()
    for b in range(B):
        v = TR.value(xh[b], clip)
        rows, n, ref_words = TR.reference(xh[b], thr[b], clip)
        tag = f'{what}, block {b}, threshold {thr[b]!r} ({recipes[b]!r})'
        if fused:
            if not np.array_equal(words[b], ref_words):
                got = TR.unpack_words(words[b], v.shape)
                raise AssertionError(TR.explain(what + ': mask words', b, thr[b], recipes[b], v, got, v > thr[b]))
        assert int(counts[b]) == n, f'{tag}: count {int(counts[b])}, numpy counts {n}'
        ref = torch.from_numpy(rows).to(ctx.device)
        for name, xyz in (('fused point list', t['xyz']), ('ops.threshold_compact', sa_xyz)):
            if not torch.equal(xyz[b, :n], ref):
                got = xyz[b, :n].cpu().numpy()
                i = int(np.argwhere((got != rows).any(axis=1))[0, 0])
                z, y, x = (int(c) for c in rows[i])
                raise AssertionError(f'{tag}: {name}: row {i} is {got[i].tolist()}, numpy has {rows[i].tolist()} (value {v[z, y, x]!r})')
        assert int(sa_cnt[b]) == n, f'{tag}: ops.threshold_compact counts {int(sa_cnt[b])}, numpy {n}'
        # what the recipe is there for
        if recipes[b] == 'drawn':
            eq = v == thr[b]
            assert eq.any() and 0 < n < v.size, f'{tag}: the drawn threshold decides nothing'
        elif recipes[b] == -1.0:
            assert n == v.size and (not fused or (words[b] == 0xFFFFFFFF).all()), tag
        elif recipes[b] == float('inf'):
            assert n == 0 and (not fused or not words[b].any()), tag
    if fused:
        assert (words != TR.PREFILL).any(), f'{what}: the last layer did not write the occupancy bits'
        behind = scratch.behind()
        assert (behind == TR.PREFILL).all(), f'{what}: {int((behind != TR.PREFILL).sum())} scratch words behind the mask were written'


def _not_vacuous(cid, precision, xh_enc, xh_dec):
    """The encoder's clipped x_hat has voxels at exactly 0 and exactly 1 in every block; the decoder's x_hat leaves [0, 1] upwards.  It
    cannot leave it downwards: the 16 -> 1 layer ends in a ReLU (model_transforms.py, SynthesisTransform*: activation of the last
    Conv3DTranspose), so the decoder's x_hat is never below 0 whatever the weights -- its lower mass sits at exactly 0, asserted here,
    and the thresholds 0, -0 and -1 decide it."""
    if xh_enc is not None:
        v = TR.value(xh_enc, True)
        for b in range(v.shape[0]):
            assert (v[b] == 0).any() and (v[b] == 1).any(), f'{cid} ({precision}): block {b} of the clipped x_hat has no voxel at exactly 0 / 1'
    assert (xh_dec > 1).any() and (xh_dec == 0).any() and xh_dec.min() >= 0, f'{cid} ({precision}): x_hat in [{xh_dec.min()}, {xh_dec.max()}]'


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
@pytest.mark.parametrize('cid', TR.CASE_IDS)
def test_fused_occupancy_bits_equal_numpy_at_the_boundaries(ctx, cid, precision):
    case, sel = _the_case(ctx, cid, precision)
    res, batch, fused = case['res'], case['batch'], sel['fused']
    m, mc, desc = _model(ctx, case, precision)
    dev = ctx.device
    thr0 = torch.linspace(0.35, 0.65, batch, dtype=torch.float32).to(dev)
    enc0 = None
    if 'enc' in case['sides']:
        x = (torch.rand((batch, res, res, res), generator=torch.Generator().manual_seed(11)) < OCCUPANCY).float().to(dev)
        enc0 = ops.codec_encode(mc, desc, x, thr0, scratch=Scratch(ctx, batch, res).t)
        ysym = enc0['symbols']
    else:
        ysym = torch.randint(-3, 4, (batch, res // 8, res // 8, res // 8, desc.filters), generator=torch.Generator().manual_seed(12),
                             dtype=torch.int32).to(dev)
    dec0 = ops.codec_decode_main(mc, desc, ysym, [res] * 3, thr0, scratch=Scratch(ctx, batch, res).t)
    xh_dec = dec0['x_hat'].cpu().numpy()
    if enc0 is not None:
        assert torch.equal(enc0['x_hat'], dec0['x_hat']), 'encoder and decoder disagree on x_hat'
        _not_vacuous(cid, precision, enc0['x_hat'].cpu().numpy(), xh_dec)
    sets = TR.threshold_sets(xh_dec)
    seen = set()
    for k, (thr, recipes) in enumerate(sets):
        seen |= set(map(str, recipes))
        thr_d = torch.from_numpy(thr).to(dev)
        if enc0 is not None:
            s = Scratch(ctx, batch, res)
            e = ops.codec_encode(mc, desc, x, thr_d, scratch=s.t)
            assert torch.equal(e['x_hat'].view(torch.int32), enc0['x_hat'].view(torch.int32)), 'a second encode gave other x_hat bits'
            _check_side(ctx, mc, f'{cid} ({precision}) encoder, call {k}', e, s, thr, recipes, True, fused)
        s = Scratch(ctx, batch, res)
        d = ops.codec_decode_main(mc, desc, ysym, [res] * 3, thr_d, scratch=s.t)
        assert torch.equal(d['x_hat'].view(torch.int32), dec0['x_hat'].view(torch.int32)), 'a second decode gave other x_hat bits'
        _check_side(ctx, mc, f'{cid} ({precision}) decoder, call {k}', d, s, thr, recipes, False, fused)
    assert seen == set(map(str, TR.RECIPES))


def test_a_cap_below_the_largest_count_truncates_the_list_and_nothing_else(ctx):
    """pcc_codec_decode_main with cap below some counts: the counts stay exact, exactly min(count, cap) rows of a block are written and
    the rows behind them, the other blocks' slots and the guards around the buffer keep their fill."""
    case, sel = _the_case(ctx, 't16-r32', 'fp32')
    res, batch = case['res'], case['batch']
    m, mc, desc = _model(ctx, case, 'fp32')
    dev = ctx.device
    x = (torch.rand((batch, res, res, res), generator=torch.Generator().manual_seed(11)) < OCCUPANCY).float().to(dev)
    thr0 = torch.linspace(0.35, 0.65, batch, dtype=torch.float32).to(dev)
    enc = ops.codec_encode(mc, desc, x, thr0)
    xh = ops.codec_decode_main(mc, desc, enc['symbols'], [res] * 3, thr0)['x_hat'].cpu().numpy()
    thr = np.array([-1.0, TR.drawn(xh[1]), 1.0, float('inf'), TR.drawn(xh[4])], np.float32)
    refs = [TR.reference(xh[b], thr[b], False) for b in range(batch)]
    ns = [n for _, n, _ in refs]
    cap = sorted(ns)[-2] - 7
    assert max(ns) == res ** 3 and sum(1 for n in ns if n > cap) >= 2 and any(0 < n < cap for n in ns) and 0 in ns, (ns, cap)
    guard, fill = 64, -7.0
    out = torch.full((guard + batch * cap * 3 + guard,), fill, dtype=torch.float32, device=dev)
    counts = torch.full((batch,), -1, dtype=torch.int32, device=dev)
    s = Scratch(ctx, batch, res)
    ys = enc['symbols'].contiguous()
    y_hat = torch.empty(ys.shape, dtype=torch.float32, device=dev)
    x_hat = torch.empty((batch, res, res, res), dtype=torch.float32, device=dev)
    ws = mc.workspace(L.lib().pcc_codec_workspace_bytes(C.byref(desc), batch, res, res, res))
    thr_d = torch.from_numpy(thr).to(dev)
    p = ops._ptr
    L.check(L.lib().pcc_codec_decode_main(mc.handle, C.byref(desc), p(ys), batch, res, res, res, p(y_hat), p(x_hat), p(thr_d),
                                          C.c_void_p(out.data_ptr() + 4 * guard), p(counts), cap, p(s.t), p(ws), ws.numel(), mc.conv_flags, None,
                                          mc.stream), 'pcc_codec_decode_main')
    torch.cuda.synchronize()
    assert np.array_equal(x_hat.cpu().numpy().view(np.uint32), xh.view(np.uint32))
    assert counts.cpu().tolist() == ns, 'the counts must stay exact under a cap'
    o = out.cpu().numpy()
    assert (o[:guard] == fill).all() and (o[-guard:] == fill).all(), 'written outside the point buffer'
    slots = o[guard:-guard].reshape(batch, cap, 3)
    for b, (rows, n, _) in enumerate(refs):
        k = min(n, cap)
        assert np.array_equal(slots[b, :k], rows[:k]), f'block {b}: the first {k} rows differ from numpy'
        assert (slots[b, k:] == fill).all(), f'block {b}: rows behind the first {k} were written (count {n}, cap {cap})'
