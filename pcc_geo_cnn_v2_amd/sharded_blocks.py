"""The block loops of the codec under torch.distributed, one process per GPU: every rank codes a contiguous shard of the block list with
its own model and the collectives of sharding.py assemble what a single process returns (the protocol is described there)."""
import os

import numpy as np
from scipy.spatial import cKDTree

from . import sharding
from .model_opt import metric_names
from .model_types import get_normals_if, rank_candidates
from .utils.octree_coding import block_origins, departition_octree
from .utils.pc_metric import cloud_metrics_batch, finish_metrics


def compress_blocks_sharded(model, sess, blocks, binstr, points, resolution, level, with_normals, opt_metrics, max_deltas, fixed_threshold,
                            debug, need_points, tree_future=None):
    """model.compress_blocks over the ranks: rank 0 returns the complete result, the other ranks (None, metadata without point lists,
    local debug list).  tree_future: the KD-tree over the original cloud when the caller is building it meanwhile."""
    rank, world = sharding.world_info()
    lo, hi = sharding.shard_range(len(blocks), rank, world)
    try:
        strings_l, thr_l, xhat_l, names, debug_t_list = model.encode_block_range(
            sess, blocks[lo:hi], resolution, with_normals, opt_metrics, max_deltas, fixed_threshold, debug)
    finally:
        tree_a = tree_future.result() if tree_future is not None else None
    if tree_a is None:
        tree_a = cKDTree(points[:, :3])
    n_str = model.n_strings
    n_m = len(max_deltas) * len(opt_metrics)
    if names is None or not len(blocks[lo:hi]):
        names = metric_names(opt_metrics, max_deltas)
    # What crosses ranks (sharding.py).  Per block one int64 row: string lengths, threshold index and candidate point count per metric.
    # The D1/D2 numbers of every candidate (select_best_per_opt_metric, src/model_types.py:128-176) come from per-rank partial tallies
    # of the pairs a rank OWNS (its decoded point is the nearest one to an original point: MIN over ranks of `d2 * world + rank`).
    origins = block_origins(binstr, [0, 0, 0], [resolution] * 3, level)[lo:hi]
    p1, p1_n = points[:, :3], get_normals_if(points, with_normals)
    cand_global = []
    for m in range(n_m):
        parts = [np.asarray(xhat_l[j][m], np.float64).reshape(-1, 3) + np.asarray(origins[j], np.float64) for j in range(hi - lo)]
        cand_global.append(np.vstack(parts) if parts else np.zeros((0, 3)))
    width = n_str + 2 * n_m
    rows = np.zeros((hi - lo, width), np.int64)
    for j in range(hi - lo):
        rows[j, :n_str] = [len(x) for x in strings_l[j]]
        rows[j, n_str:n_str + n_m] = thr_l[j][:n_m]
        rows[j, n_str + n_m:] = [len(x) for x in xhat_l[j][:n_m]]
    per_rank = sharding.shard_sizes(len(blocks), world)      # known to every rank: no size exchange anywhere below
    first = np.concatenate([[0], np.cumsum(per_rank)])
    my_strings = b''.join(x for ss in strings_l for x in ss)
    if 8 * len(p1) * n_m * world <= int(os.environ.get('PCC_KEY_GATHER_MAX_BYTES', 64 << 20)):
        # TWO collectives per cloud: (1) ONE all_gather of the rows with the MIN keys of all candidates riding as extra
        # rows (sharding.PiggybackGroup: every rank takes the MIN itself), (2) ONE all_gather of bytes: strings + the partial tallies
        grp = sharding.PiggybackGroup(rows, per_rank)
        part_tallies, have = cloud_metrics_batch(p1, cand_global, resolution - 1, p1_n, tree_a, grp, partial=True)
        table = grp.table
        tb = np.ascontiguousarray(part_tallies, np.float64).tobytes()
        payloads = sharding.all_gather_bytes(my_strings + tb, counts=[int(table[first[r]:first[r + 1], :n_str].sum()) + len(tb) for r in range(world)])
        blobs = [p[:len(p) - len(tb)] for p in payloads]
        tallies = np.zeros_like(part_tallies, dtype=np.float64)
        for p in payloads:          # rank order: every rank gets the same doubles
            tallies += np.frombuffer(p[len(p) - len(tb):], np.float64).reshape(part_tallies.shape)
    else:
        # a cloud whose keys (8 B per original point and candidate) are too many to move `world` times: THREE collectives -- (1) ONE
        # all_reduce(MIN) of the keys, (2) ONE all_gather of the rows + T rows with the bit patterns of the partial tallies (summed in
        # rank order), (3) ONE padded uint8 gather of the strings to rank 0
        part_tallies, have = cloud_metrics_batch(p1, cand_global, resolution - 1, p1_n, tree_a, sharding.RankGroup(), partial=True)
        T = -(-part_tallies.size // width)
        send = np.zeros((hi - lo + T, width), np.int64)
        send[:hi - lo] = rows
        send[hi - lo:].reshape(-1)[:part_tallies.size] = np.ascontiguousarray(part_tallies, np.float64).reshape(-1).view(np.int64)
        gathered = sharding.all_gather_rows(send, counts=[n + T for n in per_rank])
        ends = np.cumsum([n + T for n in per_rank])
        table = np.concatenate([gathered[e - n - T:e - T] for e, n in zip(ends, per_rank)], 0)
        tallies = np.zeros_like(part_tallies, dtype=np.float64)
        for e in ends:
            tallies += gathered[e - T:e].reshape(-1)[:part_tallies.size].view(np.float64).reshape(part_tallies.shape)
        blobs = sharding.gather_bytes(my_strings, counts=[int(table[first[r]:first[r + 1], :n_str].sum()) for r in range(world)])
    assert table.shape[0] == len(blocks)
    # the selection is replicated: every rank holds the summed tallies
    cand_metrics = finish_metrics(len(p1), tallies, have, resolution - 1, p1_n is not None)
    metadata = [{'idx': m, 'metrics': met} for _, m, met in rank_candidates(names, cand_metrics)]
    # (4) the reconstruction of the selected candidates on rank 0 (only for --dec_files / --debug)
    if need_points:
        for md in metadata:
            m = md['idx']
            n_pts = table[:, n_str + n_m + m]
            flat = sharding.gather_rows(np.vstack([np.asarray(xhat_l[j][m], np.float32).reshape(-1, 3) for j in range(hi - lo)])
                                        if hi > lo else np.zeros((0, 3), np.float32),
                                        counts=[int(n_pts[first[r]:first[r + 1]].sum()) for r in range(world)])
            if rank == 0:
                off = np.concatenate([[0], np.cumsum(n_pts)])
                md['x_hat_list'] = tuple(flat[off[j]:off[j + 1]] for j in range(len(blocks)))
                md['blocks_depart'] = departition_octree(md['x_hat_list'], binstr, [0, 0, 0], [resolution] * 3, level)
                md['blocks_full'] = np.vstack(md['blocks_depart'])
    if rank != 0:
        return None, metadata, debug_t_list
    # rank 0: split the gathered strings back into per-block tuples, block order == rank order
    strings_list, raw, pos = [], b''.join(blobs), 0
    for j in range(len(blocks)):
        ss = []
        for k in range(n_str):
            ss.append(raw[pos:pos + int(table[j, k])])
            pos += int(table[j, k])
        strings_list.append(tuple(ss))
    assert pos == len(raw)
    data_list = [list(zip(strings_list, [int(t) for t in table[:, n_str + md['idx']]])) for md in metadata]
    return data_list, metadata, debug_t_list


def decompress_blocks_sharded(model, sess, blocks, x_shape, debug=False, layers='all'):
    """model.decompress_blocks over the ranks: contiguous shards; the decoded float32 points go to rank 0 with one (counts, rows)
    gather -- the other ranks return None (rank 0 writes the file, decompress_octree.py:111-113)."""
    rank, world = sharding.world_info()
    lo, hi = sharding.shard_range(len(blocks), rank, world)
    local, dbg = model.decompress_block_range(sess, blocks[lo:hi], x_shape, debug, layers)
    per_rank = sharding.shard_sizes(len(blocks), world)
    first = np.concatenate([[0], np.cumsum(per_rank)])
    counts = sharding.all_gather_rows(np.array([[len(b)] for b in local], np.int64).reshape(-1, 1), counts=per_rank)[:, 0]
    flat = sharding.gather_rows(np.vstack(local).astype(np.float32) if len(local) else np.zeros((0, 3), np.float32),
                                counts=[int(counts[first[r]:first[r + 1]].sum()) for r in range(world)])
    if rank != 0:
        return None, dbg
    off = np.concatenate([[0], np.cumsum(counts)])
    return [flat[off[j]:off[j + 1]] for j in range(len(blocks))], dbg
