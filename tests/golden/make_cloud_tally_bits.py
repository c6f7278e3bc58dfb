"""Records the bits of the whole-cloud distortion tallies and of the D2 threshold searches (tests/_cloud_tally_cases.py).

Run by hand on the GPU, from the repository root, before a change that claims to leave these sums' order alone (on the commit whose
bits are to be kept), or after a deliberate change of that order:

    python tests/golden/make_cloud_tally_bits.py --kernels-of <commit whose kernels these are>  [--out DIR]

rewrites tests/golden/cloud_tally_bits.json (or DIR/...).  Every case is computed twice; the file is not written when any case gives
other bytes the second time (the engines claim bit-reproducible calls).  The file carries no time stamp.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import _cloud_tally_cases as TC  # noqa: E402


def record(ctx, what, names, run):
    out, unstable = {}, []
    for name in names:
        first, second = run(ctx, name), run(ctx, name)
        if first != second:
            unstable.append(f'{what}.{name}')
        out[name] = first
        print(what, name, 'ok' if first == second else 'A SECOND CALL GIVES OTHER BITS', flush=True)
    return out, unstable


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--kernels-of', required=True, help='the commit whose kernels computed these bits (recorded in the header)')
    ap.add_argument('--out', default=HERE, help='directory that receives cloud_tally_bits.json')
    args = ap.parse_args()
    import torch
    from pcc_geo_cnn_v2_amd import ops
    ctx = ops.get_context(torch.device('cuda', 0))
    doc = dict(header=dict(kernels_of_commit=args.kernels_of, num_cu=int(ctx.num_cu), rocm=str(torch.version.hip),
                           device=torch.cuda.get_device_properties(0).gcnArchName.split(':')[0],
                           encoding='tally / status: hex of the float64 / int64 bytes; every other entry: blake2b-128 of the array; '
                                    'inputs: tests/_cloud_tally_cases.py',
                           note='the bits that the kernels of kernels_of_commit compute'))
    unstable = []
    for what, names, run in (('cloud', TC.CLOUD_NAMES, TC.run_cloud), ('color', TC.COLOR_NAMES, TC.run_color),
                             ('search', sorted(TC.SEARCH), TC.run_search)):
        doc[what], bad = record(ctx, what, names, run)
        unstable += bad
    if unstable:
        sys.exit(f'not written: a second call gives other bits for {unstable}')
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'cloud_tally_bits.json'), 'w') as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('recorded', len(doc['cloud']), 'cloud pairs,', len(doc['color']), 'colour pairs,', len(doc['search']), 'search calls')


if __name__ == '__main__':
    main()
