"""Codec-level recorded bits and committed streams (tests/test_family_bits_gpu.py, tests/golden/make_family_bits.py): the models, weights
and inputs of the pins, the digests of every stage, and the CLI calls that write and read the streams of tests/golden/streams_k<family>/.
"""
import gzip
import hashlib
import json
import os

import numpy as np

import _bits_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3
# (model, precision, block edge)
COMBOS = [(cfg, prec, res) for cfg in ('c1', 'c3p') for prec in ('fp32', 'fp16') for res in (16, 32)]


def combo_id(cfg, prec, res):
    return f'{cfg}-{prec}-{res}'


# Kernel gains on top of Glorot-uniform per model and transform, and the bias of the last synthesis layer: chosen on the CPU oracle
# (oracle.compress_block on these blocks) so that a few per cent to a half of the y symbols are non-zero with |symbol| <= 4, most z
# symbols are non-zero and the scale indexes spread over 8 - 46 rows of the table, and x_hat crosses thresholds[128] in a part of every
# block (29 - 12 000 voxels).  scaled_weights' single gain of 2.2 and bias of 0.47 leave c1 almost dead at 16^3 (under 1 % of the symbols
# non-zero), saturate the deeper c3p, and lift x_hat over the threshold in most of the block whatever the symbols are.
GAINS = {'c1': dict(analysis=3.5, synthesis=2.2, last_bias=0.30),
         'c3p': dict(analysis=1.8, synthesis=1.6, hyper_analysis=5.0, hyper_synthesis=2.2, last_bias=0.30)}


def hash_weights(model, cfg, gains=None):
    """Weights shaped as tests/test_codec_gpu.py::scaled_weights shapes them -- Glorot-uniform kernels times a gain, biases within +-0.05,
    the last synthesis bias set so that x_hat hovers around thresholds[128] -- with every number from tests/_bits_ref.py instead of a
    library RNG.  The entropy models keep the model's own defaults."""
    gains = GAINS[cfg] if gains is None else gains
    w = model.get_weights()
    for key in sorted(w):
        if key.startswith(('entropy', 'gaussian')):
            continue
        if key.endswith('/kernel'):
            k = w[key].shape[0]
            limit = np.sqrt(6.0 / (k ** 3 * (w[key].shape[3] + w[key].shape[4])))
            u = BR.tensor('codec/' + key, w[key].shape, 'weight', fan_in=1).astype(np.float64)            # k / 2^12 in [-1, 1)
            w[key] = (u * (gains[key.split('/')[0]] * limit)).astype(np.float32)
        elif key.endswith('/bias'):
            w[key] = (BR.tensor('codec/' + key, w[key].shape, 'bias').astype(np.float64) * 0.1).astype(np.float32)
    last = max(int(k.split('/')[1]) for k in w if k.startswith('synthesis/'))
    w[f'synthesis/{last}/bias'] = np.array([gains['last_bias']], np.float32)
    return w


def build_model(cfg, prec, res, coder='range', batch=B, gains=None):
    from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
    m = ModelConfigType[cfg].build(batch_size=batch, precision=prec, entropy_coder=coder)
    m.compress([1, 1, res, res, res])
    m.set_weights(hash_weights(m, cfg, gains))
    return m


def blocks_of(res, seed=2):
    from test_codec_gpu import make_blocks
    return make_blocks(B, res, seed=seed)


def _strings_digest(strings):
    h = hashlib.blake2b(digest_size=16)
    for s in strings:
        h.update(len(s).to_bytes(4, 'little'))
        h.update(bytes(s))
    return h.hexdigest()


def stage_digests(ctx, cfg, prec, res, layerwise=False):
    """Encode and decode B blocks under both entropy coders (one launch per phase, or layer by layer under PCC_LAYERWISE=1) and return
    the digests of every stage.  Asserts what must hold before a digest means anything: no empty block, a live model (at least 1 % of the
    y symbols non-zero), the two coders agree on everything but the strings, encoder-side x_hat == decoder-side x_hat."""
    import torch
    from pcc_geo_cnn_v2_amd import ops
    old = os.environ.get('PCC_LAYERWISE')
    if layerwise:
        os.environ['PCC_LAYERWISE'] = '1'
    try:
        dhw = (res,) * 3
        blocks = blocks_of(res)
        assert all(len(b) > 0 for b in blocks), 'an empty block'
        out, per_coder = {}, {}
        for coder in ('range', 'rans'):
            m = build_model(cfg, prec, res, coder)
            c = m._ctx(ctx)
            assert (m._codec(c) is None) == layerwise
            x = m._voxelize(c, blocks, dhw)
            thr = m._thr_tensor(c, [128] * B)
            enc = m._encode_batch(c, x, debug=True, thr=thr)
            strings = enc['finish']()
            st = m._decode_phase_a(c, strings, dhw)
            dec = m._decode_phase_b(c, st, dhw, True, thr=thr)
            torch.cuda.synchronize()
            assert torch.equal(enc['x_hat'], dec['x_hat']), f'{coder}: encoder-side x_hat != decoder-side x_hat'
            dbg = enc['debug']
            ysym = np.stack([d['symbols'] for d in dbg])
            live = float(np.count_nonzero(ysym)) / ysym.size
            assert live >= 0.01, f'a dead model: {100 * live:.2f} % of the y symbols are non-zero'
            stages = {'y_symbols': BR.digest(ysym), 'x_hat': BR.digest(enc['x_hat'].cpu().numpy())}
            if 'z_symbols' in dbg[0]:
                stages['z_symbols'] = BR.digest(np.stack([d['z_symbols'] for d in dbg]))
                stages['scale_indexes'] = BR.digest(np.stack([d['indexes'] for d in dbg]))
                for b in range(B):
                    assert np.array_equal(dbg[b]['indexes'], dec['debug'][b]['indexes']), 'scale indexes differ between encoder and decoder'
            counts = dec['counts'].cpu().numpy()
            assert (counts > 0).all(), f'a block decodes to no point: {counts}'
            stages['points'] = BR.digest(np.concatenate([dec['xyz'][b, :int(counts[b])].cpu().numpy() for b in range(B)]))
            per_coder[coder] = stages
            for j in range(len(strings[0])):
                out[f'strings_{coder}_{"yz"[j]}'] = _strings_digest([s[j] for s in strings])
            if coder == 'range':
                occ = ops.occ_encode_fetch(*ops.occ_encode_launch(c, enc['x_hat'], x))
                assert all(len(o) > 0 for o in occ)
                out['strings_occ'] = _strings_digest(occ)
                out['y_symbols_nonzero'] = round(live, 4)
        assert per_coder['range'] == per_coder['rans'], 'the entropy coder changed something besides the strings'
        out.update(per_coder['range'])
        return out
    finally:
        if layerwise:
            if old is None:
                del os.environ['PCC_LAYERWISE']
            else:
                os.environ['PCC_LAYERWISE'] = old


# ---- committed streams ---------------------------------------------------------------------------------------------------------------
# name -> (model, block edge, precision, entropy coder, lossless); the cloud is B blocks in three octants of a (2 edge)^3 box, level 1
STREAMS = {
    'c1_16_fp32_range': ('c1', 16, 'fp32', 'range', False), 'c1_32_fp32_range': ('c1', 32, 'fp32', 'range', False),
    'c1_16_fp16_range': ('c1', 16, 'fp16', 'range', False), 'c1_32_fp16_range': ('c1', 32, 'fp16', 'range', False),
    'c3p_16_fp32_range': ('c3p', 16, 'fp32', 'range', False), 'c3p_32_fp32_range': ('c3p', 32, 'fp32', 'range', False),
    'c3p_16_fp16_range': ('c3p', 16, 'fp16', 'range', False), 'c3p_32_fp16_range': ('c3p', 32, 'fp16', 'range', False),
    'c3p_16_fp32_rans': ('c3p', 16, 'fp32', 'rans', False), 'c1_32_fp32_rans': ('c1', 32, 'fp32', 'rans', False),
    'c3p_32_fp32_range_occ': ('c3p', 32, 'fp32', 'range', True), 'c1_16_fp32_rans_occ': ('c1', 16, 'fp32', 'rans', True),
    'c3p_16_fp32_range_cnt': ('c3p', 16, 'fp32', 'range', False), 'c3p_32_fp32_range_cntsearch': ('c3p', 32, 'fp32', 'range', False),
    'c3p_16_fp32_range_qs21': ('c3p', 16, 'fp32', 'range', False), 'c3p_16_fp32_range_bpp': ('c3p', 16, 'fp32', 'range', False),
}
# name -> the encoder's threshold policy and layer flags where they are not the plain --fixed_threshold; the listing records them.
# --target_bpp 6.0: 769.5 bytes for the 1026 points of the 16^3 cloud; the predictions of the recording build are 848 bytes at q = 12 and
# 729 at q = 13 (2122 at q = 0, 177 from q = 26 on), so the target selects the interior step 13
STREAM_FLAGS = {
    'c3p_16_fp32_range_cnt': ['--count_threshold', '1.0'], 'c3p_32_fp32_range_cntsearch': ['--count_search', '0.5', '2.0', '5'],
    'c3p_16_fp32_range_qs21': ['--fixed_threshold', '--latent_step', '21'], 'c3p_16_fp32_range_bpp': ['--fixed_threshold', '--target_bpp', '6.0'],
}
LEVEL = 1


def streams_dir(family):
    return os.path.join(ROOT, 'tests', 'golden', f'streams_k{family}')


def cloud_of(res):
    """the three blocks of the stage pins (another seed) in octants 0, 1, 2 of a (2 res)^3 box"""
    return np.vstack([b + np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1]) * res for i, b in enumerate(blocks_of(res, seed=3))])


def rows(a):
    a = np.asarray(a, np.float32).reshape(-1, 3)
    return np.ascontiguousarray(a[np.lexsort(a.T[::-1])])


def write_checkpoint(cfg, folder):
    """`model.npz` of the hash weights of `cfg` (they do not depend on the block edge or the precision)"""
    m = build_model(cfg, 'fp32', 16)
    os.makedirs(folder, exist_ok=True)
    np.savez(os.path.join(folder, 'model.npz'), **m.get_weights())
    return folder


def cli_encode(name, ck, src, out, dec_file):
    """the encoder CLI's own entry point on parsed arguments, in this process"""
    from pcc_geo_cnn_v2_amd import compress_octree
    cfg, res, prec, coder, lossless = STREAMS[name]
    compress_octree.compress(compress_octree.build_parser().parse_args(
        ['--input_files', src, '--output_files', out, '--dec_files', dec_file, '--checkpoint_dir', ck, '--model_config', cfg,
         '--resolution', str(2 * res), '--octree_level', str(LEVEL), '--opt_metrics', 'd1_mse', '--batch_size', '2',
         '--precision', prec, '--entropy_coder', coder] + STREAM_FLAGS.get(name, ['--fixed_threshold']) + (['--lossless'] if lossless else [])))


def cli_decode(cfg, prec, ck, inp, out):
    """the decoder CLI's own entry point: the stream names its coder and its layers, the precision is the decoder's"""
    from pcc_geo_cnn_v2_amd import decompress_octree
    decompress_octree.decompress(decompress_octree.build_parser().parse_args(
        ['--input_files', inp, '--output_files', out, '--checkpoint_dir', ck, '--model_config', cfg, '--batch_size', '3', '--precision', prec]))


def payload_of(path):
    with gzip.open(path, 'rb') as fh:
        return fh.read()


def load_listing(family):
    with open(os.path.join(streams_dir(family), 'streams.json')) as fh:
        return json.load(fh)
