"""The per-block threshold search (include/pcc_geo.h: pcc_d1_threshold_stats, pcc_d12_threshold_stats, pcc_d12_threshold_stats_ties)."""
import numpy as np
import torch

from .. import _lib as L
from ._context import _PairOverflow, _ptr, _workspace


def _search_args(x_hat, thr, pts, block_of, block_start=None):
    """The argument contract the three searches share; returns (B, D, H, W) of x_hat."""
    assert x_hat.dtype == torch.float32 and x_hat.is_contiguous() and x_hat.dim() == 4
    assert pts.dtype == torch.int32 and pts.is_contiguous() and block_of.dtype == torch.int32 and block_of.is_contiguous()
    assert thr.dtype == torch.float32 and thr.is_contiguous()
    if block_start is not None:
        assert block_start.dtype == torch.int32 and block_start.is_contiguous() and block_start.numel() == x_hat.shape[0] + 1
    return x_hat.shape


def _search_outputs(x_hat, d2):
    """(s_ab, hsum, hcnt int64 (B,256), tcount int32 (B,)) and, with d2, (d2_ab, d2_ba float64 (B,256)) appended: on x_hat's device."""
    B, dev = x_hat.shape[0], x_hat.device
    out = [torch.empty((B, 256), dtype=torch.int64, device=dev) for _ in range(3)] + [torch.empty((B,), dtype=torch.int32, device=dev)]
    return out + [torch.empty((B, 256), dtype=torch.float64, device=dev) for _ in range(2 if d2 else 0)]


def _search_results(who, s_ab, hsum, hcnt, tcount, *d2):
    """The device outputs of a search as numpy: (s_ab, s_ba, n_b, tcount, *d2) with s_ba, n_b the suffix sums of the level
    histograms over the levels k > t.  tcount[b] == 256 (256 thresholds and a voxel above the last one: a level the engine's uint8
    grid cannot hold, include/pcc_geo.h) raises PccError naming the blocks; its `.results` is the tuple this would have returned,
    whose entries at t < 255 are valid."""
    suffix = lambda h: np.concatenate([np.cumsum(h[:, ::-1], 1)[:, ::-1][:, 1:], np.zeros((h.shape[0], 1), np.int64)], 1)
    s_ba, n_b = suffix(hsum.cpu().numpy()), suffix(hcnt.cpu().numpy())
    res = (s_ab.cpu().numpy(), s_ba, n_b, tcount.cpu().numpy()) + tuple(t.cpu().numpy() for t in d2)
    over = np.flatnonzero(res[3] >= 256)
    if len(over):
        err = L.PccError(f'{who}: block(s) {over.tolist()} hold a voxel above all 256 thresholds (level 256): threshold 255 is not '
                         'computed for them; clip x_hat to a range the last threshold covers, or pass at most 255 thresholds')
        err.blocks, err.results = over.tolist(), res
        raise err
    return res


def d1_threshold_stats(ctx, x_hat, thr, pts, block_of, clip=True):
    """Exact D1 sums for every threshold of every block (see include/pcc_geo.h).  x_hat (B,D,H,W) float32,
    thr (T<=256,) float32, pts (n,3) int32 grouped by block, block_of (n,) int32 -- all on the device.
    Returns int64 numpy arrays s_ab (B,256), s_ba (B,256), n_b (B,256) indexed by threshold, and tcount (B,).  Like the two D2
    searches below it raises PccError when a block holds a voxel above all of 256 thresholds (_search_results)."""
    B, D, H, W = _search_args(x_hat, thr, pts, block_of)
    ws = _workspace(ctx, L.lib().pcc_d1_search_workspace_bytes(B, D, H, W))
    s_ab, hsum, hcnt, tcount = out = _search_outputs(x_hat, d2=False)
    L.check(L.lib().pcc_d1_threshold_stats(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(thr), thr.numel(), int(clip),
                                           _ptr(pts), _ptr(block_of), pts.shape[0], _ptr(ws), _ptr(s_ab), _ptr(hsum),
                                           _ptr(hcnt), _ptr(tcount), ctx.stream), 'pcc_d1_threshold_stats')
    return _search_results('d1_threshold_stats', *out)


def d12_threshold_stats(ctx, x_hat, thr, pts, block_of, block_start, normals, clip=True):
    """d1_threshold_stats plus the D2 sums of every threshold (include/pcc_geo.h: pcc_d12_threshold_stats).  normals (n,3) float32,
    block_start (B+1,) int32 -- on the device.  Returns (s_ab, s_ba, n_b, tcount, d2_ab, d2_ba); d2_* float64 (B,256)."""
    B, D, H, W = _search_args(x_hat, thr, pts, block_of, block_start)
    assert normals.dtype == torch.float32 and normals.is_contiguous() and normals.shape == pts.shape
    ws = _workspace(ctx, L.lib().pcc_d1_search_workspace_bytes(B, D, H, W))
    ws2 = _workspace(ctx, L.lib().pcc_d12_search_workspace_bytes(B, D, H, W, pts.shape[0]))
    s_ab, hsum, hcnt, tcount, d2_ab, d2_ba = out = _search_outputs(x_hat, d2=True)
    L.check(L.lib().pcc_d12_threshold_stats(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(thr), thr.numel(), int(clip), _ptr(pts), _ptr(block_of),
                                            _ptr(block_start), pts.shape[0], _ptr(normals), _ptr(ws), _ptr(ws2), _ptr(s_ab), _ptr(hsum), _ptr(hcnt),
                                            _ptr(tcount), _ptr(d2_ab), _ptr(d2_ba), ctx.stream), 'pcc_d12_threshold_stats')
    return _search_results('d12_threshold_stats', *out)


class SearchTiePairOverflow(_PairOverflow):
    """d12_threshold_stats_ties met more equidistant pairs in one chunk of thresholds than the stated capacity; `.pairs` suffices."""
    _who = 'd12_threshold_stats_ties: a chunk of thresholds'


def search_tie_pair_capacity(B, D, H, W, npts):
    """Default pair capacity of d12_threshold_stats_ties (workspace rule): room for four equidistant voxels per row
    and threshold on average over one chunk of thresholds, 4 npts chunk + 1024, capped at the engine's limit of 2^31 - 1 pairs."""
    return min(4 * int(npts) * int(L.lib().pcc_d12_search_ties_chunk(B, D, H, W)) + 1024, (1 << 31) - 1)


def d12_threshold_stats_ties_launch(ctx, x_hat, thr, pts, block_of, block_start, normals64, clip=True, max_pairs=None):
    """d12_threshold_stats_ties without the host copies: the device tensors (s_ab, hsum, hcnt, tcount, d2_ab, d2_ba, status)."""
    B, D, H, W = _search_args(x_hat, thr, pts, block_of, block_start)
    assert pts.dim() == 2 and pts.shape[1] == 3 and pts.shape[0] > 0 and block_of.numel() == pts.shape[0]
    assert normals64.dtype == torch.float64 and normals64.is_contiguous() and normals64.shape == pts.shape, \
        'd12_threshold_stats_ties: normals must be (n,3) float64'
    lo, hi = pts.min(0).values.cpu(), pts.max(0).values.cpu()
    assert int(lo.min()) >= 0 and bool((hi < torch.tensor([D, H, W])).all()), f'block-local coordinates outside the {(D, H, W)} grid'
    n = pts.shape[0]
    max_pairs = search_tie_pair_capacity(B, D, H, W, n) if max_pairs is None else int(max_pairs)
    if not 1 <= max_pairs <= (1 << 31) - 1:
        raise L.PccError(f'd12_threshold_stats_ties: max_pairs = {max_pairs} outside [1, 2^31)')
    ws = _workspace(ctx, L.lib().pcc_d1_search_workspace_bytes(B, D, H, W))
    ws2 = _workspace(ctx, L.lib().pcc_d12_search_ties_workspace_bytes(B, D, H, W, n, max_pairs))
    s_ab, hsum, hcnt, tcount, d2_ab, d2_ba = out = _search_outputs(x_hat, d2=True)
    status = torch.empty((2,), dtype=torch.int64, device=x_hat.device)
    L.check(L.lib().pcc_d12_threshold_stats_ties(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(thr), thr.numel(), int(clip), _ptr(pts), _ptr(block_of),
                                                 _ptr(block_start), n, _ptr(normals64), max_pairs, _ptr(status), _ptr(ws), _ptr(ws2), _ptr(s_ab),
                                                 _ptr(hsum), _ptr(hcnt), _ptr(tcount), _ptr(d2_ab), _ptr(d2_ba), ctx.stream),
            'pcc_d12_threshold_stats_ties')
    return (*out, status)


def d12_threshold_stats_ties(ctx, x_hat, thr, pts, block_of, block_start, normals64, clip=True, max_pairs=None, return_status=False):
    """d12_threshold_stats under the tie-averaged D2 definition (include/pcc_geo.h: pcc_d12_threshold_stats_ties): D2 of every
    (block, threshold) averages over ALL equidistant nearest points, so it equals the host restatement
    (model_opt.host_threshold_stats(ties='mean')) up to float64 rounding.  normals64 (n,3) float64 -- on the device like the rest.
    The pair list of a chunk of thresholds holds max_pairs pairs (default search_tie_pair_capacity): with the default, a call that
    needs more runs once more with the number the first run reported; an explicit max_pairs that is too small raises
    SearchTiePairOverflow -- or, with return_status=True, returns what the engine wrote (D2 all NaN, D1 valid) with the status.
    Returns (s_ab, s_ba, n_b, tcount, d2_ab, d2_ba) and, with return_status=True, (pairs needed, overflowed) appended."""
    args = (ctx, x_hat, thr, pts, block_of, block_start, normals64, clip)
    out = d12_threshold_stats_ties_launch(*args, max_pairs=max_pairs)
    pairs, over = (int(v) for v in out[-1].cpu())
    if over and not return_status:
        if max_pairs is not None or pairs > (1 << 31) - 1:
            B, D, H, W = x_hat.shape
            raise SearchTiePairOverflow(pairs, search_tie_pair_capacity(B, D, H, W, pts.shape[0]) if max_pairs is None else max_pairs)
        out = d12_threshold_stats_ties_launch(*args, max_pairs=pairs)
        pairs, over = (int(v) for v in out[-1].cpu())
        assert not over, 'd12_threshold_stats_ties: the reported pair capacity did not suffice'
    res = _search_results('d12_threshold_stats_ties', *out[:-1])
    return res + ((pairs, bool(over)),) if return_status else res
