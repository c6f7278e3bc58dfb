"""GPU: the recorded bits of every conv kernel family, of the training kernels and of the codec stages, and the streams an earlier
commit wrote (tests/golden/family_bits.json, tests/golden/streams_k<family>/; DESIGN.md section 5, "Recorded bits").

A stream can only be decoded by a build whose conv kernels give the same bits for sigma-hat and x-hat (include/pcc_geo.h, "codec
numerics"); the tag k<PCC_KERNEL_FAMILY> in every stream says which bits those are, and somebody has to bump the number by hand when a
kernel's summation order changes.  These tests notice when that was forgotten: every family runs small layers on inputs that depend on
no library RNG (tests/_bits_ref.py), and the output must (1) come from the family the case names, (2) be within the suite's stated
tolerance of the float64-accumulating oracle -- a recorded digest is never the only evidence that the bits are right -- and (3) hash to
the recorded digest.
"""
import os

import numpy as np
import pytest
import torch

import _bits_ref as BR
import _codec_pins as CP
import _family_cases as FC

pytestmark = pytest.mark.gpu

BUMP = ('{what}: the bits differ from tests/golden/family_bits.json (recorded {want}, computed {got}).  If the change of bits is '
        'intended, bump PCC_KERNEL_FAMILY in include/pcc_geo.h and regenerate with tests/golden/make_family_bits.py (DESIGN.md section 5: '
        'streams written under the old number must be refused, not misdecoded).  Otherwise the kernel edit changed bits it claimed not '
        'to change: find the reordered sum.')
REGEN = ('{what}: the bits differ from the "training" section of tests/golden/family_bits.json (recorded {want}, computed {got}).  No '
         'stream depends on the training kernels, so PCC_KERNEL_FAMILY stays: if the change is intended, regenerate with '
         'tests/golden/make_family_bits.py and note in DESIGN.md that checkpoints trained before and after differ in their last bits.')


@pytest.fixture(scope='module')
def golden():
    import json
    with open(FC.GOLDEN) as fh:
        return json.load(fh)


_BITS = {}


def _bits(ctx, case):
    """(family, output buffer) of a case, computed once per session and left unchanged"""
    if case['id'] not in _BITS:
        _BITS[case['id']] = FC.run(ctx, case)
    return _BITS[case['id']]


@pytest.mark.parametrize('cid', [c['id'] for c in FC.CASES])
def test_family_bits(ctx, oracle, golden, cid):
    case = FC.BY_ID[cid]
    fam, buf = _bits(ctx, case)
    assert fam == case['family'], f'{cid} no longer reaches its family: the route gives {fam}'
    acc, clean = FC.accuracy(oracle, case, buf)
    for err, tol, what in acc:
        print(f'{cid}: |gpu - ref| / (1 + max |ref|) = {err:.3g} (tolerance {tol:.0e}, {what})')
    assert clean, f'{cid}: the kernel wrote outside its {case["geo"][5]} channels at offset {case["oco"]} of {case["ocs"]}'
    for err, tol, what in acc:
        assert err <= tol, f'{cid}: {err:.3g} > {tol:.3g} against the {what}'
    want, got = golden['cases'][cid]['digest'], BR.digest(buf)
    assert got == want, BUMP.format(what=f'{cid} ({fam}, N D H W Cin Cout k stride transposed = {case["geo"]})', want=want, got=got)


@pytest.mark.parametrize('left,right', FC.SENSITIVITY, ids=[f'{a}~{b if isinstance(b, str) else "+".join(sorted(b[1]))}' for a, b in FC.SENSITIVITY])
def test_the_digest_sees_another_summation_order(ctx, left, right):
    """Two families (or two settings of a switch) on the same layer and the same inputs: the same sum in another order or from another
    operand split.  Their digests must differ: the digest sees a reordered sum, and the switches switch.  (That both are right is
    test_family_bits' accuracy check of either case.)"""
    a = FC.BY_ID[left]
    b = FC.variant(*right) if isinstance(right, tuple) else FC.BY_ID[right]
    assert a['geo'] == b['geo'] and all(a[k] == b[k] for k in ('bias', 'relu', 'res', 'mode', 'ocs', 'oco'))
    for x, y in zip(FC.inputs(a), FC.inputs(b)):
        assert (x is None and y is None) or np.array_equal(x, y)
    xa, xb = _bits(ctx, a)[1], _bits(ctx, b)[1]
    assert xa.shape == xb.shape and BR.digest(xa) != BR.digest(xb), f'{left} and {b["id"]} give the same bits'


@pytest.fixture(scope='module')
def pctx():
    from pcc_geo_cnn_v2_amd import train
    c = train.training_context(torch.device('cuda', 0))
    yield c
    c.close()


@pytest.mark.parametrize('tid', list(FC.TRAINING))
def test_training_bits(pctx, golden, tid):
    """pcc_conv3d_wgrad on one MFMA and one VALU geometry and the dual-descriptor input gradient of one layer, N = 2, D = 8: within the
    bounds of tests/test_train_gpu.py against float64 autograd, then the recorded bits."""
    want = golden['training'][tid]
    if FC.TRAINING[tid][0] == 'wgrad':
        from test_train_gpu import _check_wgrad
        layer, d, x, dout, dw, db = FC.run_wgrad(pctx, tid)
        _check_wgrad(layer, d, x, dout, dw, db)
        got = dict(dw=BR.digest(dw.cpu().numpy()), db=BR.digest(db.cpu().numpy()))
    else:
        layer, x, dout, dx = FC.run_dgrad(pctx, tid)
        worst = FC.check_dgrad(layer, x, dout, dx)
        assert worst <= 1.0, f'{tid}: max error / bound {worst:.3g}'
        got = dict(dx=BR.digest(dx.cpu().numpy()))
    assert got == want, REGEN.format(what=tid, want=want, got=got)


# ---- codec level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layerwise', [False, True], ids=['one-launch', 'layerwise'])
@pytest.mark.parametrize('cfg,prec,res', CP.COMBOS, ids=[CP.combo_id(*c) for c in CP.COMBOS])
def test_codec_stage_bits(ctx, golden, cfg, prec, res, layerwise):
    """y / z symbols, scale indexes, x-hat, the decoded point rows, the strings of the range coder, of the rANS coder and of the occupancy
    layer, for three blocks under hash weights: a change of the quantiser, pcc_scale_to_index, the CDF builder or one of the coders
    breaks old streams while every encode -> decode round trip of the same build stays green.  CP.stage_digests first asserts that no
    block is empty, that at least 1 % of the y symbols are non-zero, and that encoder-side x-hat equals decoder-side x-hat; the
    one-launch path and PCC_LAYERWISE=1 are held to the same recorded digests."""
    want = golden['codec'][CP.combo_id(cfg, prec, res)]
    got = CP.stage_digests(ctx, cfg, prec, res, layerwise=layerwise)
    bad = {k: (want.get(k), got.get(k)) for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)}
    assert not bad, BUMP.format(what=f'codec stages of {cfg} {prec} @{res}^3' + (' (PCC_LAYERWISE=1)' if layerwise else ''),
                                want={k: v[0] for k, v in bad.items()}, got={k: v[1] for k, v in bad.items()})


@pytest.fixture(scope='module')
def checkpoints(tmp_path_factory):
    made = {}

    def get(cfg):
        if cfg not in made:
            made[cfg] = CP.write_checkpoint(cfg, str(tmp_path_factory.mktemp('ck_' + cfg)))
        return made[cfg]
    return get


@pytest.mark.parametrize('name', list(CP.STREAMS))
def test_committed_stream_decodes_to_its_recorded_points(golden, checkpoints, tmp_path, name):
    """A stream that the commit named in the listing wrote (tests/golden/streams_k<family>/, through the encoder CLI's own entry point)
    decodes with today's decoder CLI and the regenerated weights to exactly the recorded points."""
    from pcc_geo_cnn_v2_amd.utils import pc_io
    family = golden['family']
    entry = CP.load_listing(family)['streams'][name]
    cfg, res, prec, coder, lossless = CP.STREAMS[name]
    assert (entry['model'], entry['resolution'], entry['precision'], entry['coder'], entry['lossless']) == (cfg, 2 * res, prec, coder, lossless)
    out = str(tmp_path / 'dec.ply')
    CP.cli_decode(cfg, prec, checkpoints(cfg), os.path.join(CP.streams_dir(family), entry['file']), out)
    got = CP.rows(pc_io.load_pc(out))
    assert len(got) == entry['points'] and BR.digest(got) == entry['point_digest'], \
        f'{name}: today\'s decoder gives {len(got)} points ({BR.digest(got)}), the stream was recorded with {entry["points"]} ({entry["point_digest"]})'
    if lossless:
        assert np.array_equal(got, CP.rows(CP.cloud_of(res)))


@pytest.mark.parametrize('name', list(CP.STREAMS))
def test_todays_encoder_writes_the_committed_stream(golden, checkpoints, tmp_path, name):
    """The encoder CLI's own entry point on the cloud and flags of the listing writes the committed file again, byte for byte: tag, container,
    every string of every layer (plain, occ1, cnt1 by a scale and by the count search, qs1 by a step and by a rate target)."""
    from pcc_geo_cnn_v2_amd.utils import pc_io
    family = golden['family']
    entry = CP.load_listing(family)['streams'][name]
    cfg, res, prec, coder, lossless = CP.STREAMS[name]
    assert entry.get('flags') == CP.STREAM_FLAGS.get(name)
    src, out = str(tmp_path / 'in.ply'), str(tmp_path / 'out.bin')
    pc_io.write_df(src, pc_io.pa_to_df(CP.cloud_of(res)))
    CP.cli_encode(name, checkpoints(cfg), src, out, str(tmp_path / 'enc.ply'))
    with open(out, 'rb') as a, open(os.path.join(CP.streams_dir(family), entry['file']), 'rb') as b:
        assert a.read() == b.read(), f'{name}: today\'s encoder writes another file than the committed one'


def test_stream_of_another_kernel_family_is_refused(golden, checkpoints, tmp_path):
    """The same payload under the tag of the family before this one: refused with the "codec numerics" error, nothing written.  After
    a bump of PCC_KERNEL_FAMILY the directory of the old family stays in the tree and takes the place of this retagged copy."""
    from pcc_geo_cnn_v2_amd import model_syntax
    family = golden['family']
    entry = CP.load_listing(family)['streams']['c3p_16_fp32_range']
    src = os.path.join(CP.streams_dir(family), entry['file'])
    tag = model_syntax.read_gzip_tag(src)
    assert f'/k{family}/' in tag
    old = str(tmp_path / 'old.bin')
    model_syntax.write_tagged_gzip(old, CP.payload_of(src), tag.replace(f'/k{family}/', f'/k{family - 1}/'))
    out = str(tmp_path / 'old.ply')
    with pytest.raises(RuntimeError, match='codec numerics'):
        CP.cli_decode('c3p', 'fp32', checkpoints('c3p'), old, out)
    assert not os.path.exists(out)
