"""GPU box: per-cloud time of the d2 threshold search under its three rules, in one process, alternating:
   kdtree pick (the default: bound-pruned host KD-trees), gpu pick (--d2_search gpu), gpu mean (--search_ties mean).
Cloud and stand-in decoder output: tools/d2_tie_table.py (a 1024^3 level-4 shell, about 190 blocks of 64^3; what the search sees is
the blurred input occupancy, the bitstream stays the network's).  Timed: the whole compress_blocks call (encode, search, whole-cloud
metrics on the GPU under --d2_ties mean), median of --repeats after one warm-up round.  Also: the share of blocks whose d2_mse
decision differs between gpu mean and kdtree pick (and gpu pick), the D2 PSNR of each mode's d2-optimised stream under d2_ties =
'mean', and the tie-pair counts of the mean search.  Writes profiles/search_ties_bench.json.
    python tools/bench_search_ties.py [--repeats 3] [--kind smooth] [--output profiles/search_ties_bench.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
from pcc_geo_cnn_v2_amd import ops, model_opt
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd.model_configs import ModelConfigType
from pcc_geo_cnn_v2_amd.utils.octree_coding import partition_octree

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--kind', default='smooth', choices=['smooth', 'rough'])
ap.add_argument('--output', default=os.path.join(ROOT, 'profiles', 'search_ties_bench.json'))
args = ap.parse_args()

ctx = ops.get_context(torch.device('cuda', 0))
R, level, res = 1024, 4, 64
model = ModelConfigType['c3p'].build(batch_size=32); model.compress([1, 1, res, res, res])
model.set_weights(bench.synthetic_weights(model))
_orig_encode = model._encode_batch


def _plausible_x_hat(x):
    k = torch.exp(-torch.arange(-2, 3, device=x.device, dtype=torch.float32) ** 2 / (2 * 0.8 ** 2)); k /= k.sum()
    v = x[:, None]
    for ax in range(3):
        shape = [1, 1, 1, 1, 1]; shape[2 + ax] = 5
        pad = [0, 0, 0, 0, 0, 0]; pad[2 * (2 - ax)] = pad[2 * (2 - ax) + 1] = 2
        v = torch.nn.functional.conv3d(torch.nn.functional.pad(v, pad), k.reshape(shape))
    g = torch.Generator(device=x.device).manual_seed(int(x.sum().item()) & 0xffff)
    return (v[:, 0] * 2.2 + 0.03 * torch.randn(x.shape, device=x.device, generator=g)).clamp_(0, 1).contiguous()


def _encode_with_plausible_x_hat(ctx_, x, debug=False, thr=None, slot=0):
    enc = _orig_encode(ctx_, x, debug, thr=thr, slot=slot)
    enc['x_hat'] = _plausible_x_hat(x)
    return enc


model._encode_batch = _encode_with_plausible_x_hat

# tie-pair counts of the mean search: every launch's (status tensor, capacity), read after the run
_launch, launches = ops.d12_threshold_stats_ties_launch, []


def _recording_launch(*a, **kw):
    out = _launch(*a, **kw)
    B, D, H, W = a[1].shape
    launches.append((out[-1], a[3].shape[0] * int(L.lib().pcc_d12_search_ties_chunk(B, D, H, W))))      # (status, rows x thresholds per chunk)
    return out


ops.d12_threshold_stats_ties_launch = ops.search.d12_threshold_stats_ties_launch = _recording_launch      # callers outside and inside the package


def cloud(kind):
    rng = np.random.default_rng(0)
    u = rng.standard_normal((3_000_000 if kind == 'smooth' else 1_500_000, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = 200 if kind == 'smooth' else 200 + 6 * np.sin(9 * u[:, :1]) * np.cos(7 * u[:, 1:2]) + rng.normal(0, 0.6, (len(u), 1))
    pts, first = np.unique(np.round(u * rad + np.array([512, 500, 520])).astype(np.int64), axis=0, return_index=True)
    return np.hstack([pts.astype(np.float64), u[first]])


MODES = {'kdtree_pick': ('kdtree', 'pick'), 'gpu_pick': ('gpu', 'pick'), 'gpu_mean': (None, 'mean')}
c = cloud(args.kind)
blocks, binstr = partition_octree(c, [0, 0, 0], [R] * 3, level)
times, last = {m: [] for m in MODES}, {}
for rep in range(args.repeats + 1):          # round 0 = warm-up of the worker pool and the kernels
    for mode, (engine, ties) in MODES.items():
        model.d2_search, model.search_ties = engine, ties
        launches.clear()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        data, meta, _ = model.compress_blocks(ctx, blocks, binstr, c, R, level, with_normals=True, opt_metrics=['d1_mse', 'd2_mse'],
                                              max_deltas=[np.inf], need_points=False, metrics_device='gpu', d2_ties='mean')
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if rep:
            times[mode].append(dt)
        last[mode] = (data, meta, [(st.cpu().tolist(), n) for st, n in launches])
        print(f'round {rep} {mode}: {dt:.3f} s', flush=True)

thr_of = lambda data: [[t for _, t in d] for d in data]
d2 = {m: thr_of(last[m][0])[-1] for m in MODES}
pairs = last['gpu_mean'][2]
out = dict(cloud=f'{args.kind} shell, {len(c)} points', blocks=len(blocks), repeats=args.repeats,
           timed='compress_blocks wall time per cloud (encode + search + whole-cloud GPU metrics under d2_ties mean), one process, modes alternating',
           seconds_per_cloud={m: dict(median=float(np.median(v)), all=[round(x, 4) for x in v]) for m, v in times.items()},
           d2_mse_decisions_differing_from_kdtree_pick={m: sum(a != b for a, b in zip(d2[m], d2['kdtree_pick'])) / len(blocks) for m in ('gpu_pick', 'gpu_mean')},
           d2_psnr_of_d2_stream_under_d2_ties_mean={m: float(last[m][1][-1]['metrics']['d2_psnr']) for m in MODES},
           d1_psnr_of_d1_stream={m: float(last[m][1][0]['metrics']['d1_psnr']) for m in MODES},
           mean_search_pairs=dict(launches=len(pairs), largest_chunk_pairs_per_launch_max=int(max(s[0] for s, _ in pairs)),
                                  largest_chunk_pairs_per_row_and_threshold=float(max(s[0] / n for s, n in pairs)),      # (a full chunk: an upper bound where a block has fewer level sets)
                                  default_capacity_per_row_and_threshold=4.0,
                                  overflowed_launches=int(sum(s[1] for s, _ in pairs))))
os.makedirs(os.path.dirname(args.output), exist_ok=True)
with open(args.output, 'w') as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
print(json.dumps(out, indent=1, sort_keys=True))
if model._host_search_pool is not None:
    model._host_search_pool.close()
