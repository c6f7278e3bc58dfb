"""Records the bits of every conv kernel family, of the training kernels and of the codec stages, and writes the committed streams.

Run by hand on the GPU, from the repository root, after a deliberate change of a kernel's bits (and the bump of PCC_KERNEL_FAMILY in
include/pcc_geo.h that goes with it):

    python tests/golden/make_family_bits.py --kernels-of <commit whose kernels these are>  [--out DIR]

rewrites tests/golden/family_bits.json and tests/golden/streams_k<family>/ (or DIR/...).  Run it twice, in two fresh processes, with two
--out directories, and diff them before committing: the files carry no time stamp and must be identical.

Nothing is recorded for a case whose output misses its accuracy tolerance against the float64 oracle, whose second launch in this
process gives other bits, or whose kernel family is not the expected one.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import _bits_ref as BR  # noqa: E402
import _codec_pins as CP  # noqa: E402
import _family_cases as FC  # noqa: E402


def sig(v):
    return float(f'{v:.3g}')


def record_cases(ctx, O):
    out, bits = {}, {}
    for case in FC.CASES:
        arrays = FC.inputs(case)
        fam, buf = FC.run(ctx, case, arrays)
        fam2, buf2 = FC.run(ctx, case, arrays)
        assert fam == case['family'], f"{case['id']}: expected {case['family']}, the route gives {fam}"
        assert buf.tobytes() == buf2.tobytes(), f"{case['id']}: a second launch in this process gives other bits"
        acc, clean = FC.accuracy(O, case, buf, arrays)
        assert clean, f"{case['id']}: the kernel wrote outside its channels"
        for err, tol, what in acc:
            assert err <= tol, f"{case['id']}: {err:.3g} > {tol:.3g} of 1 + max |ref| against the {what}"
        bits[case['id']] = BR.digest(buf)
        out[case['id']] = dict(family=fam, shape=list(case['geo']), digest=bits[case['id']], rel_err=[sig(e) for e, _, _ in acc])
        print(f"{case['id']:16s} {bits[case['id']]}  " + '  '.join(f'{e:.2e} (<= {t:.0e})' for e, t, _ in acc), flush=True)
    for left, right in FC.SENSITIVITY:
        if isinstance(right, tuple):
            v = FC.variant(*right)
            other, name = BR.digest(FC.run(ctx, v)[1]), v['id']
        else:
            other, name = bits[right], right
        assert bits[left] != other, f'{left} and {name} compute the same layer with different arithmetic and give the same bits'
    return out


def record_training():
    import torch
    from pcc_geo_cnn_v2_amd import train
    import test_train_gpu as TT
    pctx = train.training_context(torch.device('cuda', 0))
    out = {}
    for tid, (what, g) in FC.TRAINING.items():
        if what == 'wgrad':
            layer, d, x, dout, dw, db = FC.run_wgrad(pctx, tid)
            _, _, _, _, dw2, db2 = FC.run_wgrad(pctx, tid)
            assert torch.equal(dw, dw2) and torch.equal(db, db2), f'{tid}: a second launch gives other bits'
            TT._check_wgrad(layer, d, x, dout, dw, db)
            out[tid] = dict(dw=BR.digest(dw.cpu().numpy()), db=BR.digest(db.cpu().numpy()))
        else:
            layer, x, dout, dx = FC.run_dgrad(pctx, tid)
            assert torch.equal(dx, FC.run_dgrad(pctx, tid)[3]), f'{tid}: a second launch gives other bits'
            worst = FC.check_dgrad(layer, x, dout, dx)
            assert worst <= 1.0, f'{tid}: error / bound {worst:.3g}'
            out[tid] = dict(dx=BR.digest(dx.cpu().numpy()))
        print(tid, out[tid], flush=True)
    pctx.close()
    return out


def record_codec(ctx):
    out = {}
    for cfg, prec, res in CP.COMBOS:
        a = CP.stage_digests(ctx, cfg, prec, res)
        b = CP.stage_digests(ctx, cfg, prec, res, layerwise=True)
        assert a == b, f'{CP.combo_id(cfg, prec, res)}: the one-launch path and PCC_LAYERWISE=1 differ: {a} {b}'
        out[CP.combo_id(cfg, prec, res)] = a
        print(CP.combo_id(cfg, prec, res), a['y_symbols_nonzero'], a['points'], flush=True)
    return out


def record_streams(folder, family):
    from pcc_geo_cnn_v2_amd import model_syntax
    from pcc_geo_cnn_v2_amd.utils import pc_io
    if os.path.isdir(folder):
        shutil.rmtree(folder)
    os.makedirs(folder)
    listing = {}
    with tempfile.TemporaryDirectory() as tmp:
        cks, clouds = {}, {}
        for name, (cfg, res, prec, coder, lossless) in CP.STREAMS.items():
            if cfg not in cks:
                cks[cfg] = CP.write_checkpoint(cfg, os.path.join(tmp, 'ck_' + cfg))
            if res not in clouds:
                clouds[res] = (CP.cloud_of(res), os.path.join(tmp, f'in{res}.ply'))
                pc_io.write_df(clouds[res][1], pc_io.pa_to_df(clouds[res][0]))
            pts, src = clouds[res]
            out, enc_ply, dec_ply = (os.path.join(tmp, name + e) for e in ('.bin', '.enc.ply', '.dec.ply'))
            CP.cli_encode(name, cks[cfg], src, out, enc_ply)
            CP.cli_decode(cfg, prec, cks[cfg], out, dec_ply)
            got = CP.rows(pc_io.load_pc(dec_ply))
            want = CP.rows(pts if lossless else pc_io.load_pc(enc_ply))
            assert len(got) > 0 and np.array_equal(got, want), f'{name}: the decoder does not give the ' + ('input cloud' if lossless else "encoder's cloud")
            tag = model_syntax.read_gzip_tag(out)
            assert tag.startswith(f'pcc_geo_cnn_v2_amd/k{family}/sw0000/'), f'{name}: {tag} (generate without PCC_* switches in the environment)'
            shutil.copyfile(out, os.path.join(folder, name + '.bin'))
            listing[name] = dict(file=name + '.bin', model=cfg, resolution=2 * res, octree_level=CP.LEVEL, precision=prec, coder=coder,
                                 lossless=lossless, tag=tag, bytes=os.path.getsize(out), input_points=len(pts), points=len(got),
                                 point_digest=BR.digest(got), **({'flags': CP.STREAM_FLAGS[name]} if name in CP.STREAM_FLAGS else {}))
            print(name, listing[name]['bytes'], 'bytes', len(got), 'points', tag, flush=True)
    with open(os.path.join(folder, 'streams.json'), 'w') as fh:
        json.dump(dict(family=family, streams=listing), fh, indent=1, sort_keys=True)
        fh.write('\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--kernels-of', required=True, help='the commit whose kernels computed these bits (recorded in the header)')
    ap.add_argument('--out', default=HERE, help='directory that receives family_bits.json and streams_k<family>/')
    ap.add_argument('--skip-streams', action='store_true', help='leave the stream directory alone')
    args = ap.parse_args()
    import torch
    from oracle import oracle as O
    from pcc_geo_cnn_v2_amd import ops
    O.lib()
    ctx = ops.get_context(torch.device('cuda', 0))
    family, switches = ctx.numerics()
    assert family == FC.family_number(), 'the library was built from another include/pcc_geo.h'
    assert switches == 0, f'PCC_* numerics switches are set in the environment (sw{switches:04x}): record the default build'
    os.makedirs(args.out, exist_ok=True)
    doc = dict(
        header=dict(kernel_family=family, kernels_of_commit=args.kernels_of, num_cu=int(ctx.num_cu), rocm=str(torch.version.hip),
                    device=torch.cuda.get_device_properties(0).gcnArchName.split(':')[0],
                    digest='blake2b-128 of the whole output buffer; inputs: tests/_bits_ref.py',
                    note='the bits that the kernels of kernels_of_commit compute'),
        family=family,
        cases=record_cases(ctx, O),
        training=record_training(),
        codec=record_codec(ctx))
    with open(os.path.join(args.out, 'family_bits.json'), 'w') as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write('\n')
    if not args.skip_streams:
        record_streams(os.path.join(args.out, f'streams_k{family}'), family)
    print('recorded', len(doc['cases']), 'cases,', len(doc['training']), 'training pins,', len(doc['codec']), 'codec combinations')


if __name__ == '__main__':
    main()
