"""CPU: bench.py --dump-outputs -- what one step of the timed path yields becomes float32 / float64 .npy files, capped in size."""
import os

import numpy as np


def _chunk(rng, blocks, seed):
    strings = [(bytes(rng.integers(0, 256, 5 + b, dtype=np.uint8)), bytes([seed, b])) for b in range(blocks)]
    cnt_e = np.arange(blocks, dtype=np.int32) + 10 * seed
    pts = [rng.integers(0, 64, (7 * b + seed, 3)).astype(np.float32) for b in range(blocks)]
    return strings, cnt_e, pts


def test_codec_outputs_of_one_step_round_trip_through_the_files(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    items = [_chunk(rng, 3, 1), _chunk(rng, 2, 2)]
    bench.write_outputs(str(tmp_path), bench.codec_outputs(items))
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(got) == {'string_lengths', 'string_bytes', 'encoder_points_per_block', 'decoded_points_per_block', 'decoded_points'}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    strings = [ss for s, _, _ in items for ss in s]
    pts = [p for _, _, ps in items for p in ps]
    assert got['string_lengths'].tolist() == [[len(s) for s in ss] for ss in strings]
    assert bytes(got['string_bytes'].astype(np.uint8)) == b''.join(s for ss in strings for s in ss)
    assert got['encoder_points_per_block'].tolist() == [10, 11, 12, 20, 21]
    assert got['decoded_points_per_block'].tolist() == [len(p) for p in pts]
    assert np.array_equal(got['decoded_points'], np.concatenate(pts)) and got['decoded_points'].dtype == np.float32


def test_write_outputs_samples_the_largest_array_to_fit_the_cap(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 4096)
    big = np.arange(3000, dtype=np.float32).reshape(1000, 3)
    small = np.arange(10, dtype=np.int64)
    for d in ('a', 'b'):
        bench.write_outputs(str(tmp_path / d), {'big': big, 'small': small})
    a, b = (np.load(str(tmp_path / d / 'big.npy')) for d in ('a', 'b'))
    s = np.load(str(tmp_path / 'a' / 'small.npy'))
    assert np.array_equal(a, b)                                       # a fixed sample: the same rows every run
    assert a.nbytes + s.nbytes <= 4096 and len(a) == (4096 - s.nbytes) // 12
    assert np.all(np.diff(a[:, 0]) > 0) and np.all(a[:, 0] % 3 == 0)  # whole rows, in their original order
    assert s.dtype == np.float64 and s.tolist() == list(range(10))
