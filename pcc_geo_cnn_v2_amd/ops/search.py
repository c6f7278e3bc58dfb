"""The per-block search statistics (include/pcc_geo.h: pcc_d1_threshold_stats, pcc_d12_threshold_stats, pcc_d12_threshold_stats_ties) and their
count-indexed twins (pcc_rank_levels, pcc_d1_count_stats, pcc_d12_count_stats); with hausdorff=True the four pick entries call their
_hausdorff forms, which return the per-point maxima beside the sums."""
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


def _hausdorff_outputs(x_hat, d2):
    """(h1_ab, h1_max uint32 (B,256)) and, with d2, (h2_ab, h2_max float64 (B,256)): the extra outputs of the _hausdorff entries, which
    zero-fill them.  uint32 travels as int32 storage (every value is at most 3 * 127^2)."""
    B, dev = x_hat.shape[0], x_hat.device
    return [torch.empty((B, 256), dtype=torch.int32, device=dev) for _ in range(2)] + \
        [torch.empty((B, 256), dtype=torch.float64, device=dev) for _ in range(2 if d2 else 0)]


def _suffix_max(h):
    """max over the levels k > t of a per-level table (B,256): where _search_results forms the suffix sums; 0 where no level is above t."""
    return np.concatenate([np.maximum.accumulate(h[:, ::-1], 1)[:, ::-1][:, 1:], np.zeros((h.shape[0], 1), h.dtype)], 1)


def _hausdorff_results(res, h1_ab, h1_max, h2_ab=None, h2_max=None):
    """`res` (the tuple of _search_results) with (h1_ab, h1_ba) int64 and, with D2, (h2_ab, h2_ba) float64 appended: AB per candidate as
    the engine wrote it, BA after the suffix maximum over the levels k > t."""
    out = res + (h1_ab.cpu().numpy().astype(np.int64), _suffix_max(h1_max.cpu().numpy().astype(np.int64)))
    if h2_ab is not None:
        out += (h2_ab.cpu().numpy(), _suffix_max(h2_max.cpu().numpy()))
    return out


def _finish(who, out, hd):
    """_search_results, with the Hausdorff arrays `hd` (None: a plain call) appended -- also to the `.results` of its PccError."""
    if hd is None:
        return _search_results(who, *out)
    try:
        return _hausdorff_results(_search_results(who, *out), *hd)
    except L.PccError as err:
        if hasattr(err, 'results'):
            err.results = _hausdorff_results(err.results, *hd)
        raise


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


def d1_threshold_stats(ctx, x_hat, thr, pts, block_of, clip=True, hausdorff=False):
    """Exact D1 sums for every threshold of every block (see include/pcc_geo.h).  x_hat (B,D,H,W) float32,
    thr (T<=256,) float32, pts (n,3) int32 grouped by block, block_of (n,) int32 -- all on the device.
    Returns int64 numpy arrays s_ab (B,256), s_ba (B,256), n_b (B,256) indexed by threshold, and tcount (B,).  Like the two D2
    searches below it raises PccError when a block holds a voxel above all of 256 thresholds (_search_results).
    hausdorff=True (pcc_d1_threshold_stats_hausdorff): (h1_ab, h1_ba) int64 (B,256) appended -- the largest per-point squared distance
    in each direction, h1_ba after the suffix maximum over the levels; the first four arrays are the plain call's bits."""
    B, D, H, W = _search_args(x_hat, thr, pts, block_of)
    ws = _workspace(ctx, L.lib().pcc_d1_search_workspace_bytes(B, D, H, W))
    s_ab, hsum, hcnt, tcount = out = _search_outputs(x_hat, d2=False)
    if hausdorff:
        hd = _hausdorff_outputs(x_hat, d2=False)
        L.check(L.lib().pcc_d1_threshold_stats_hausdorff(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(thr), thr.numel(), int(clip), _ptr(pts),
                                                         _ptr(block_of), pts.shape[0], _ptr(ws), _ptr(s_ab), _ptr(hsum), _ptr(hcnt), _ptr(tcount),
                                                         _ptr(hd[0]), _ptr(hd[1]), ctx.stream), 'pcc_d1_threshold_stats_hausdorff')
        return _finish('d1_threshold_stats', out, hd)
    L.check(L.lib().pcc_d1_threshold_stats(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(thr), thr.numel(), int(clip),
                                           _ptr(pts), _ptr(block_of), pts.shape[0], _ptr(ws), _ptr(s_ab), _ptr(hsum),
                                           _ptr(hcnt), _ptr(tcount), ctx.stream), 'pcc_d1_threshold_stats')
    return _search_results('d1_threshold_stats', *out)


def d12_threshold_stats(ctx, x_hat, thr, pts, block_of, block_start, normals, clip=True, hausdorff=False):
    """d1_threshold_stats plus the D2 sums of every threshold (include/pcc_geo.h: pcc_d12_threshold_stats).  normals (n,3) float32,
    block_start (B+1,) int32 -- on the device.  Returns (s_ab, s_ba, n_b, tcount, d2_ab, d2_ba); d2_* float64 (B,256).
    hausdorff=True (pcc_d12_threshold_stats_hausdorff): (h1_ab, h1_ba int64, h2_ab, h2_ba float64) appended, the largest of the
    per-point terms whose sums the first six arrays hold (those are the plain call's bits)."""
    B, D, H, W = _search_args(x_hat, thr, pts, block_of, block_start)
    assert normals.dtype == torch.float32 and normals.is_contiguous() and normals.shape == pts.shape
    ws = _workspace(ctx, L.lib().pcc_d1_search_workspace_bytes(B, D, H, W))
    ws2 = _workspace(ctx, L.lib().pcc_d12_search_workspace_bytes(B, D, H, W, pts.shape[0]))
    s_ab, hsum, hcnt, tcount, d2_ab, d2_ba = out = _search_outputs(x_hat, d2=True)
    if hausdorff:
        hd = _hausdorff_outputs(x_hat, d2=True)
        L.check(L.lib().pcc_d12_threshold_stats_hausdorff(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(thr), thr.numel(), int(clip), _ptr(pts),
                                                          _ptr(block_of), _ptr(block_start), pts.shape[0], _ptr(normals), _ptr(ws), _ptr(ws2),
                                                          _ptr(s_ab), _ptr(hsum), _ptr(hcnt), _ptr(tcount), _ptr(d2_ab), _ptr(d2_ba),
                                                          *(_ptr(h) for h in hd), ctx.stream), 'pcc_d12_threshold_stats_hausdorff')
        return _finish('d12_threshold_stats', out, hd)
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


def check_count_rows(counts, B):
    """The candidate rows of the count search: a (B,J) int32 tensor, 1 <= J <= 255, every row non-increasing (block_count is monotone in
    the scale, so the rows of a ladder are).  Anything else is refused here, before the upload: the kernels would still stay inside
    their buffers, but the sets they score would not be the nested top-k family.  `counts` may live on the host or the device."""
    if not (counts.dtype == torch.int32 and counts.dim() == 2 and counts.shape[0] == B and 1 <= counts.shape[1] <= 255):
        raise L.PccError(f'count rows: a ({B}, J) int32 tensor with 1 <= J <= 255, got {tuple(counts.shape)} {counts.dtype}')
    if counts.shape[1] > 1 and bool((counts[:, 1:] > counts[:, :-1]).any()):
        raise L.PccError('count rows: every row must be non-increasing (c[0] >= c[1] >= ...)')
    return int(counts.shape[1])


def _count_rows_device(ctx, counts, B):
    J = check_count_rows(counts, B)
    return counts.to(ctx.device).contiguous(), J


def _rank_workspace(ctx, B, n):
    return _workspace(ctx, lambda: L.lib().pcc_rank_levels_workspace_bytes(B, n),
                      f'rank levels: {B} blocks of {n} voxels are outside the contract (n <= 2^28, B <= 65535, B n < 2^31)')


def rank_levels(ctx, x, counts):
    """The level grid of the count search (include/pcc_geo.h "rank levels"): lev[b][v] = #{j : rank(v) < counts[b][j]} for
    the voxels with a positive score, rank by (score bits descending, voxel index ascending), 0 elsewhere; {lev > j} is the voxel set
    topk_compact emits for k = counts[b][j].  x: (B,D,H,W) float32 on the context's device, each block contiguous, blocks at least D*H*W
    elements apart; counts: (B,J) int32, rows non-increasing (check_count_rows).  Returns (lev (B,D,H,W) uint8, tcount (B,) int32) on the
    device."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.device == ctx.device, 'rank_levels: x is a (B,D,H,W) float32 tensor on the context\'s device'
    B, D, H, W = x.shape
    n = D * H * W
    assert B == 0 or n == 0 or x[0].is_contiguous(), 'rank_levels: the voxels of a block must be contiguous'
    stride = x.stride(0) if B > 1 and n > 0 else n
    assert stride >= n, 'rank_levels: blocks overlap'
    counts, J = _count_rows_device(ctx, counts, B)
    lev = torch.zeros((B, D, H, W), dtype=torch.uint8, device=x.device)
    tcount = torch.zeros((B,), dtype=torch.int32, device=x.device)
    if B == 0 or n == 0:
        return lev, tcount
    ws = _rank_workspace(ctx, B, n)
    L.check(L.lib().pcc_rank_levels(ctx.handle, _ptr(x), stride, B, n, _ptr(counts), J, _ptr(lev), _ptr(tcount), _ptr(ws), ws.numel(), ctx.stream),
            'pcc_rank_levels')
    return lev, tcount


def _count_search_args(ctx, x_hat, counts, pts, block_of, block_start=None):
    assert x_hat.dtype == torch.float32 and x_hat.is_contiguous() and x_hat.dim() == 4
    assert pts.dtype == torch.int32 and pts.is_contiguous() and block_of.dtype == torch.int32 and block_of.is_contiguous()
    if block_start is not None:
        assert block_start.dtype == torch.int32 and block_start.is_contiguous() and block_start.numel() == x_hat.shape[0] + 1
    B, D, H, W = x_hat.shape
    counts, J = _count_rows_device(ctx, counts, B)
    return B, D, H, W, counts, J


def d1_count_stats(ctx, x_hat, counts, pts, block_of, hausdorff=False):
    """d1_threshold_stats with candidate point counts in place of thresholds (include/pcc_geo.h: pcc_d1_count_stats): entry [b][j] of
    s_ab, s_ba, n_b is the exact D1 sum / size of the top-counts[b][j] set of block b -- the voxels topk_compact decodes for that k --
    valid for j < tcount[b]; n_b[b][j] = min(counts[b][j], positive voxels of b).  counts: (B,J) int32, J <= 255, rows non-increasing.
    Nothing is clipped.  Returns the tuple of d1_threshold_stats, (B,256) arrays of which the first J columns are used.
    hausdorff=True (pcc_d1_count_stats_hausdorff): (h1_ab, h1_ba) appended, as d1_threshold_stats does."""
    B, D, H, W, counts, J = _count_search_args(ctx, x_hat, counts, pts, block_of)
    ws = _workspace(ctx, L.lib().pcc_d1_search_workspace_bytes(B, D, H, W))
    rws = _rank_workspace(ctx, B, D * H * W)
    s_ab, hsum, hcnt, tcount = out = _search_outputs(x_hat, d2=False)
    if hausdorff:
        hd = _hausdorff_outputs(x_hat, d2=False)
        L.check(L.lib().pcc_d1_count_stats_hausdorff(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(counts), J, _ptr(pts), _ptr(block_of), pts.shape[0],
                                                     _ptr(ws), _ptr(rws), rws.numel(), _ptr(s_ab), _ptr(hsum), _ptr(hcnt), _ptr(tcount),
                                                     _ptr(hd[0]), _ptr(hd[1]), ctx.stream), 'pcc_d1_count_stats_hausdorff')
        return _finish('d1_count_stats', out, hd)
    L.check(L.lib().pcc_d1_count_stats(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(counts), J, _ptr(pts), _ptr(block_of), pts.shape[0], _ptr(ws),
                                       _ptr(rws), rws.numel(), _ptr(s_ab), _ptr(hsum), _ptr(hcnt), _ptr(tcount), ctx.stream), 'pcc_d1_count_stats')
    return _search_results('d1_count_stats', *out)


def d12_count_stats(ctx, x_hat, counts, pts, block_of, block_start, normals, hausdorff=False):
    """d1_count_stats plus the D2 sums of every candidate count (include/pcc_geo.h: pcc_d12_count_stats), the tie rule of
    d12_threshold_stats.  Returns (s_ab, s_ba, n_b, tcount, d2_ab, d2_ba); hausdorff=True (pcc_d12_count_stats_hausdorff): (h1_ab, h1_ba,
    h2_ab, h2_ba) appended, as d12_threshold_stats does."""
    B, D, H, W, counts, J = _count_search_args(ctx, x_hat, counts, pts, block_of, block_start)
    assert normals.dtype == torch.float32 and normals.is_contiguous() and normals.shape == pts.shape
    ws = _workspace(ctx, L.lib().pcc_d1_search_workspace_bytes(B, D, H, W))
    ws2 = _workspace(ctx, L.lib().pcc_d12_search_workspace_bytes(B, D, H, W, pts.shape[0]))
    rws = _rank_workspace(ctx, B, D * H * W)
    s_ab, hsum, hcnt, tcount, d2_ab, d2_ba = out = _search_outputs(x_hat, d2=True)
    if hausdorff:
        hd = _hausdorff_outputs(x_hat, d2=True)
        L.check(L.lib().pcc_d12_count_stats_hausdorff(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(counts), J, _ptr(pts), _ptr(block_of),
                                                      _ptr(block_start), pts.shape[0], _ptr(normals), _ptr(ws), _ptr(ws2), _ptr(rws), rws.numel(),
                                                      _ptr(s_ab), _ptr(hsum), _ptr(hcnt), _ptr(tcount), _ptr(d2_ab), _ptr(d2_ba),
                                                      *(_ptr(h) for h in hd), ctx.stream), 'pcc_d12_count_stats_hausdorff')
        return _finish('d12_count_stats', out, hd)
    L.check(L.lib().pcc_d12_count_stats(ctx.handle, _ptr(x_hat), B, D, H, W, _ptr(counts), J, _ptr(pts), _ptr(block_of), _ptr(block_start),
                                        pts.shape[0], _ptr(normals), _ptr(ws), _ptr(ws2), _ptr(rws), rws.numel(), _ptr(s_ab), _ptr(hsum),
                                        _ptr(hcnt), _ptr(tcount), _ptr(d2_ab), _ptr(d2_ba), ctx.stream), 'pcc_d12_count_stats')
    return _search_results('d12_count_stats', *out)
