"""Trains a model config on point-cloud blocks on the MI355X -- src/tr_train.py's interface.

  python -m pcc_geo_cnn_v2_amd.tr_train 'blocks/**/*.ply' checkpoint_dir --model_config c3p [--resolution 64 --batch_size 32
      --lmbda 1e-4 --alpha 0.9 --gamma 2.0 --max_steps 100000 --warm_start DIR --seed 42 --validation_interval 500
      --validation_steps 10 --summary_interval 0]

Blocks under a directory named `train` train, blocks under `test` validate (src/tr_train.py:26-32).  The checkpoint directory
receives model.npz (what compress_octree / decompress_octree load), train_state.pt (resumed when present), log.jsonl and `done`;
with --summary_interval N > 0 also TensorBoard event files under train/ and val/ (src/tr_train.py:45-47; tr_plots draws them).
"""
import argparse
import glob
import sys

import numpy as np


def build_parser():
    ap = argparse.ArgumentParser(prog='tr_train', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument('train_glob', help='Glob pattern of the training / validation PLY blocks.')
    ap.add_argument('checkpoint_dir', help='Checkpoint directory.')
    ap.add_argument('--model_config', default='c3p', help='Model configuration (c1, c2, c3, c3p).')
    ap.add_argument('--resolution', type=int, default=64, help='Dataset resolution.')
    ap.add_argument('--batch_size', type=int, default=32, help='Batch size for training.')
    ap.add_argument('--lmbda', type=float, default=0.0001, help='Lambda for rate-distortion tradeoff.')
    ap.add_argument('--alpha', type=float, default=0.9, help='Focal loss alpha.')
    ap.add_argument('--gamma', type=float, default=2.0, help='Focal loss gamma.')
    ap.add_argument('--max_steps', type=int, default=100000, help='Train up to this number of steps.')
    ap.add_argument('--warm_start', default=None, help='Checkpoint directory whose model.npz initialises the weights.')
    ap.add_argument('--seed', type=int, default=42, help='Seed of the weights, the data order and the noise.')
    ap.add_argument('--validation_interval', type=int, default=500, help='Steps between validations.')
    ap.add_argument('--validation_steps', type=int, default=10, help='Batches per validation.')
    ap.add_argument('--summary_interval', type=int, default=0,
                    help='Write a TensorBoard summary (scalars and histograms) of every N-th training step to checkpoint_dir/train '
                         'and of every validation batch to checkpoint_dir/val; 0: none.  The reference uses 100.')
    ap.add_argument('--data_format', default='channels_first', help='Accepted and ignored: the layout is NDHWC internally.')
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    from .model_configs import ModelConfigType
    from .train import split_files
    from .utils import pc_io
    files = sorted(glob.glob(a.train_glob, recursive=True))
    assert len(files) > 0, f'no files match {a.train_glob}'
    train_files, val_files = split_files(files)
    assert train_files and val_files, 'blocks must lie under directories named train and test'
    load = lambda fs: [np.asarray(pc_io.load_pc(f))[:, :3] for f in fs]
    model = ModelConfigType[a.model_config].build(seed=a.seed)
    trainer = model.train(None, a.gamma, a.alpha, a.lmbda, checkpoint_dir=a.checkpoint_dir, train_blocks=load(train_files),
                          val_blocks=load(val_files), resolution=a.resolution, batch_size=a.batch_size, max_steps=a.max_steps,
                          seed=a.seed, validation_interval=a.validation_interval, validation_steps=a.validation_steps,
                          warm_start=a.warm_start, summary_interval=a.summary_interval)
    trainer.run()
    return 0


if __name__ == '__main__':
    sys.exit(main())
