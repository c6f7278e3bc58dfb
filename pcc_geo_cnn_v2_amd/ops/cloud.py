"""Whole-cloud operators (include/pcc_geo.h): point normals, the nearest-neighbour index and the D1 / D2 / colour distortion tallies
over it, colour mapping, mesh sampling and point rendering."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ._context import _PairOverflow, _ptr, _workspace


NORMALS_COORD_LIMIT = 1 << 21        # include/pcc_geo.h "point normals": coordinates are integers in [0, 2^21)


def _voxel_points(points, what='estimate_normals'):
    """The input contract of estimate_normals and the cloud metrics (`what` names the caller in the messages), checked before anything reaches the GPU: an (N,3) cloud of integer coordinates in
    [0, 2^21), 1 <= N < 2^31.  Returns an int32 array (numpy input) or an int32 contiguous device tensor (torch input)."""
    if isinstance(points, torch.Tensor):
        if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] == 0:
            raise L.PccError(f'{what}: points must be (N, 3) with N >= 1, got {tuple(points.shape)}')
        if points.is_floating_point():
            if not bool(torch.isfinite(points).all()) or not bool((points == torch.round(points)).all()):
                raise L.PccError(f'{what}: coordinates must be integers (voxelised cloud); got non-integer values')
        elif points.dtype == torch.bool or points.is_complex():
            raise L.PccError(f'{what}: unsupported dtype {points.dtype}')
        if bool((points < 0).any()) or bool((points >= NORMALS_COORD_LIMIT).any()):
            raise L.PccError(f'{what}: coordinates must lie in [0, {NORMALS_COORD_LIMIT})')
        return points.to(torch.int32).contiguous()
    a = np.asarray(points)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
        raise L.PccError(f'{what}: points must be (N, 3) with N >= 1, got {a.shape}')
    if a.shape[0] >= 1 << 31:
        raise L.PccError(f'{what}: at most 2^31 - 1 points per call')
    if a.dtype.kind == 'f':
        if not np.isfinite(a).all() or not np.array_equal(a, np.round(a)):
            raise L.PccError(f'{what}: coordinates must be integers (voxelised cloud); got non-integer values')
    elif a.dtype.kind not in 'iu':
        raise L.PccError(f'{what}: unsupported dtype {a.dtype}')
    if (a < 0).any() or (a >= NORMALS_COORD_LIMIT).any():
        raise L.PccError(f'{what}: coordinates must lie in [0, {NORMALS_COORD_LIMIT})')
    return np.ascontiguousarray(a, dtype=np.int32)


def estimate_normals(ctx, points, k=16, viewpoint=None, return_knn=False):
    """Point normals of a voxelised cloud (include/pcc_geo.h "point normals"): (N,3) float32 numpy array, oriented away from
    `viewpoint` (3 numbers) or, by default, from the cloud's centroid.  points: (N,3) numpy array or device tensor of integer
    coordinates in [0, 2^21).  return_knn=True also returns the (N, min(k, N)) int32 neighbour rows (nearest first, ties by
    row index).  Deterministic: the same cloud gives the same bits on every call."""
    k = int(k)
    if not 3 <= k <= 64:
        raise L.PccError(f'estimate_normals: k = {k} outside [3, 64]')
    vp = None
    if viewpoint is not None:
        vp = np.asarray(viewpoint, np.float64).reshape(-1)
        if vp.shape != (3,) or not np.isfinite(vp).all():
            raise L.PccError(f'estimate_normals: viewpoint must be 3 finite numbers, got {viewpoint!r}')
    pts_d = _device_points(ctx, points, 'estimate_normals')
    dev = ctx.device
    n = pts_d.shape[0]
    vp_d = None if vp is None else torch.from_numpy(vp).to(dev)
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    knn = torch.empty((n, k), dtype=torch.int32, device=dev) if return_knn else None
    ws = _workspace(ctx, L.lib().pcc_normals_workspace_bytes(n, k))
    L.check(L.lib().pcc_estimate_normals(ctx.handle, _ptr(pts_d), n, k, _ptr(vp_d), _ptr(normals), _ptr(knn), _ptr(ws), ctx.stream),
            'pcc_estimate_normals')
    out = normals.cpu().numpy()
    if return_knn:
        return out, knn[:, :min(k, n)].cpu().numpy()
    return out


CLOUD_TALLY_SLOTS = 9      # include/pcc_geo.h "cloud metrics": N_B, D1_AB, D1_BA, D2_AB, D2_BA, H1_AB, H1_BA, H2_AB, H2_BA


def _to_device(ctx, a):
    """A numpy array or a tensor -> a contiguous tensor on ctx.device."""
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).to(ctx.device).contiguous()


_device_u8 = _to_device       # the name under which the colours used it


def _device_points(ctx, points, what):
    return _to_device(ctx, _voxel_points(points, what))


class CloudIndex:
    """Nearest-neighbour index over a voxelised cloud on the GPU (include/pcc_geo.h "cloud metrics"): Morton-sorted cells, exact
    integer distances, ties to the lowest row.  points: (N,3) numpy array or device tensor of integer coordinates in [0, 2^21),
    1 <= N < 2^31.  Built once, reusable by any number of cloud_nearest / cloud_distortion calls on the same context."""

    def __init__(self, ctx, points):
        pts = _device_points(ctx, points, 'CloudIndex')
        self.n = int(pts.shape[0])
        self.device = ctx.device
        self.buffer = _workspace(ctx, L.lib().pcc_cloud_index_bytes(self.n))
        L.check(L.lib().pcc_cloud_index_build(ctx.handle, _ptr(pts), self.n, _ptr(self.buffer), ctx.stream), 'pcc_cloud_index_build')

    def __len__(self):
        return self.n


def cloud_nearest(ctx, index, queries):
    """For every query point, the row of its nearest point in `index` (ties: the lowest row) and the exact squared distance:
    (int32[nq], int64[nq]) numpy arrays.  queries: (nq,3) integer coordinates in [0, 2^21); nq = 0 gives empty arrays."""
    if len(queries) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64)
    q = _device_points(ctx, queries, 'cloud_nearest')
    nq = int(q.shape[0])
    nn = torch.empty((nq,), dtype=torch.int32, device=ctx.device)
    sq = torch.empty((nq,), dtype=torch.int64, device=ctx.device)
    L.check(L.lib().pcc_cloud_nearest(ctx.handle, _ptr(index.buffer), index.n, _ptr(q), nq, _ptr(nn), _ptr(sq), ctx.stream),
            'pcc_cloud_nearest')
    return nn.cpu().numpy(), sq.cpu().numpy()


def _normals64(a_normals, n):
    """Host-side check of the normals of cloud_distortion; returns them as float64 (numpy) or as a float64 tensor."""
    if a_normals is None:
        return None
    if isinstance(a_normals, torch.Tensor):
        if not a_normals.is_floating_point():
            raise L.PccError(f'cloud_distortion: normals must be floating point, got {a_normals.dtype}')
        nrm = a_normals.to(torch.float64)
    else:
        nrm = np.asarray(a_normals)
        if nrm.dtype.kind != 'f':
            raise L.PccError(f'cloud_distortion: normals must be floating point, got {nrm.dtype}')
        nrm = np.ascontiguousarray(nrm, np.float64)
    if tuple(nrm.shape) != (n, 3):
        raise L.PccError(f'cloud_distortion: normals must be ({n}, 3), got {tuple(nrm.shape)}')
    return nrm


TIE_MODES = {'pick': 0, 'mean': 1}      # include/pcc_geo.h PCC_TIES_*: which of several equidistant nearest points D2 reads
_PAIR_LIMIT = (1 << 31) - 1


def tie_pair_capacity(n_a):
    """Default pair capacity of ties='mean' (DESIGN.md "Tie-averaged D2", workspace rule): room for four equidistant decoded points
    per original point on average, 4 N_A + 1024, capped at the engine's limit of 2^31 - 1 pairs."""
    return min(4 * int(n_a) + 1024, _PAIR_LIMIT)


def _tie_mode(ties):
    if ties not in TIE_MODES:
        raise L.PccError(f'cloud_distortion: ties must be one of {tuple(TIE_MODES)}, got {ties!r}')
    return TIE_MODES[ties]


def cloud_distortion_launch(ctx, index_a, b, a_normals=None, links=False, ties='pick', max_pairs=None):
    """cloud_distortion without the host copy: returns the float64[9] device tally (and the int32 to_b, to_a device tensors with
    links=True), queued on the context's stream.  b: (N_B,3) decoded points, N_B >= 1; a_normals: (N_A,3) or None.  ties='mean'
    (pcc_cloud_distortion_ties) appends the int64[2] device status (pairs needed, 1 = more than max_pairs: the D2 / H2 slots are
    then NaN) to what is returned; max_pairs defaults to tie_pair_capacity(N_A)."""
    mode = _tie_mode(ties)
    b = _voxel_points(b, 'cloud_distortion')
    nrm = _normals64(a_normals, index_a.n)
    dev = ctx.device
    if nrm is not None:
        nrm = _to_device(ctx, nrm)
    if mode:
        max_pairs = tie_pair_capacity(index_a.n) if max_pairs is None else int(max_pairs)
        if not 1 <= max_pairs <= _PAIR_LIMIT:
            raise L.PccError(f'cloud_distortion: max_pairs = {max_pairs} outside [1, 2^31)')
    index_b = CloudIndex(ctx, b)
    tally = torch.empty((CLOUD_TALLY_SLOTS,), dtype=torch.float64, device=dev)
    to_b = torch.empty((index_a.n,), dtype=torch.int32, device=dev) if links else None
    to_a = torch.empty((index_b.n,), dtype=torch.int32, device=dev) if links else None
    if not mode:
        ws = _workspace(ctx, L.lib().pcc_cloud_distortion_workspace_bytes(index_a.n, index_b.n))
        L.check(L.lib().pcc_cloud_distortion(ctx.handle, _ptr(index_a.buffer), index_a.n, _ptr(index_b.buffer), index_b.n, _ptr(nrm),
                                             _ptr(tally), _ptr(to_b), _ptr(to_a), _ptr(ws), ctx.stream), 'pcc_cloud_distortion')
        return (tally, to_b, to_a) if links else tally
    status = torch.empty((2,), dtype=torch.int64, device=dev)
    ws = _workspace(ctx, L.lib().pcc_cloud_distortion_ties_workspace_bytes(index_a.n, index_b.n, mode, max_pairs))
    L.check(L.lib().pcc_cloud_distortion_ties(ctx.handle, _ptr(index_a.buffer), index_a.n, _ptr(index_b.buffer), index_b.n, _ptr(nrm), mode,
                                              max_pairs, _ptr(tally), _ptr(status), _ptr(to_b), _ptr(to_a), _ptr(ws), ctx.stream),
            'pcc_cloud_distortion_ties')
    return (tally, to_b, to_a, status) if links else (tally, status)


class TiePairOverflow(_PairOverflow):
    """ties='mean' met more equidistant pairs than the stated capacity; `.pairs` is the capacity that suffices."""
    _who = "cloud_distortion: ties='mean'"


def cloud_distortion(ctx, a, b, a_normals=None, index_a=None, return_links=False, ties='pick', max_pairs=None):
    """Distortion tally of decoded cloud b against original cloud a on the GPU (include/pcc_geo.h "cloud metrics"): float64[9] =
    N_B, D1_AB, D1_BA, D2_AB, D2_BA, H1_AB, H1_BA, H2_AB, H2_BA (utils/pc_metric.pair_tally's five slots plus the Hausdorff maxima).
    a, b: (N,3) integer coordinates in [0, 2^21), N >= 1; a_normals: (N_A,3) normals of a (None: the D2 / H2 slots are 0);
    index_a: a CloudIndex of a to reuse (a is then not read).  return_links=True also returns to_b (int32[N_A]) and to_a
    (int32[N_B]), the nearest rows across (ties: the lowest row).  Deterministic: the same inputs give the same bits.
    ties='mean': D2 / H2 average over ALL equidistant nearest points (DESIGN.md "Tie-averaged D2"), independent of either cloud's
    row order up to float64 rounding.  Its pair workspace holds max_pairs pairs (default tie_pair_capacity(N_A)); with the default,
    a cloud that needs more is run once more with the exact number the first run reported, an explicit max_pairs that is too small
    raises TiePairOverflow."""
    mode = _tie_mode(ties)
    if index_a is None:                     # every input is checked before the first GPU call
        a = _voxel_points(a, 'cloud_distortion')
        b = _voxel_points(b, 'cloud_distortion')
        _normals64(a_normals, len(a))
        index_a = CloudIndex(ctx, a)
    out = cloud_distortion_launch(ctx, index_a, b, a_normals, links=return_links, ties=ties, max_pairs=max_pairs)
    if mode:
        pairs, over = (int(v) for v in out[-1].cpu())
        if over:
            if max_pairs is not None or pairs > _PAIR_LIMIT:
                raise TiePairOverflow(pairs, tie_pair_capacity(index_a.n) if max_pairs is None else max_pairs)
            out = cloud_distortion_launch(ctx, index_a, b, a_normals, links=return_links, ties=ties, max_pairs=pairs)
        out = out[:-1] if return_links else out[0]
    if return_links:
        return tuple(t.cpu().numpy() for t in out)
    return out.cpu().numpy()


COLOR_TALLY_SLOTS = 6      # include/pcc_geo.h "cloud colours": Y, U, V sums of A->B, then of B->A


def _colors_u8(colors, n, what):
    """Host-side check of an (n,3) colour array (numpy or tensor, integer values in 0..255); returns it as uint8 of the same kind."""
    if isinstance(colors, torch.Tensor):
        if colors.is_floating_point() or colors.is_complex() or colors.dtype == torch.bool:
            raise L.PccError(f'{what}: colours must be integers in 0..255, got {colors.dtype}')
        if tuple(colors.shape) != (n, 3):
            raise L.PccError(f'{what}: colours must be ({n}, 3), got {tuple(colors.shape)}')
        if colors.dtype != torch.uint8 and n and (bool((colors < 0).any()) or bool((colors > 255).any())):
            raise L.PccError(f'{what}: colours must be integers in 0..255')
        return colors.to(torch.uint8).contiguous()
    c = np.asarray(colors)
    if c.dtype.kind not in 'iu':
        raise L.PccError(f'{what}: colours must be integers in 0..255, got {c.dtype}')
    if c.shape != (n, 3):
        raise L.PccError(f'{what}: colours must be ({n}, 3), got {c.shape}')
    if c.dtype != np.uint8 and c.size and (c.min() < 0 or c.max() > 255):
        raise L.PccError(f'{what}: colours must be integers in 0..255')
    return np.ascontiguousarray(c, np.uint8)


def _index_or_points(index, what):
    """A CloudIndex, or points checked by _voxel_points (the index is then built by the caller after every check)."""
    if isinstance(index, CloudIndex):
        return index, index.n
    pts = _voxel_points(index, what)
    return pts, int(pts.shape[0])


def map_colors(ctx, index_a, a_colors, queries, rank=2, return_rows=False):
    """Colour of every query point taken from the original cloud (include/pcc_geo.h "cloud colours"): for each query, the colour of
    its rank-th nearest point of the original cloud, points ordered by (squared distance, row).  rank=2 (the default) is the
    reference's map_color.py (the second of a k = 2 KD-tree query), rank=1 the nearest point (cloud_nearest's row).
    index_a: a CloudIndex of the original cloud or its (N,3) points; a_colors: (N,3) integer colours in 0..255; queries: (nq,3)
    integer coordinates in [0, 2^21), or a CloudIndex of them.  Returns (nq,3) uint8 numpy colours (and the int32 rows with
    return_rows=True); nq = 0 gives empty arrays.  Every input is checked before the first GPU call."""
    if rank not in (1, 2):
        raise L.PccError(f'map_colors: rank = {rank!r}, must be 1 or 2')
    index_a, n = _index_or_points(index_a, 'map_colors')
    if rank > n:
        raise L.PccError(f'map_colors: rank {rank} needs at least {rank} original points, got {n}')
    colors = _colors_u8(a_colors, n, 'map_colors')
    if len(queries) == 0:
        out = np.zeros((0, 3), np.uint8)
        return (out, np.zeros(0, np.int32)) if return_rows else out
    q = _index_or_points(queries, 'map_colors')[0]
    if not isinstance(index_a, CloudIndex):
        index_a = CloudIndex(ctx, index_a)
    index_q = q if isinstance(q, CloudIndex) else CloudIndex(ctx, q)
    nq = index_q.n
    colors_d = _to_device(ctx, colors)          # held in a local: a temporary's block could be handed out again before the launch
    out = torch.empty((nq, 3), dtype=torch.uint8, device=ctx.device)
    rows = torch.empty((nq,), dtype=torch.int32, device=ctx.device) if return_rows else None
    L.check(L.lib().pcc_cloud_map_colors(ctx.handle, _ptr(index_a.buffer), index_a.n, _ptr(colors_d), _ptr(index_q.buffer), nq, rank, _ptr(out),
                                         _ptr(rows), ctx.stream), 'pcc_cloud_map_colors')
    if return_rows:
        return out.cpu().numpy(), rows.cpu().numpy()
    return out.cpu().numpy()


def transfer_colors(ctx, index_a, a_colors, queries, return_votes=False):
    """Least-squares colours of the query (decoded) points from the original cloud (include/pcc_geo.h "cloud colours", DESIGN.md
    §4.9 "Colour transfer"; a simplified MPEG-style recolouring, not TMC13-conformant): every original point votes for all query
    points at its smallest squared distance, a query point takes the mean colour of its voters, or of its own equidistant nearest
    original points when it has none, rounded half up in integers.  Where every original point has one nearest query point these are,
    before rounding, the colours under which the A->B sums of cloud_color_distortion are smallest.  Inputs as map_colors: index_a a CloudIndex of the original cloud or its (N,3) points;
    a_colors (N,3) integers in 0..255; queries (nq,3) integer coordinates in [0, 2^21) (duplicates allowed) or a CloudIndex of
    them.  Returns (nq,3) uint8 numpy colours (and the int32 votes, 0 for a point that fell back, with return_votes=True); nq = 0
    gives empty arrays.  Independent of the row order of either cloud; every input is checked before the first GPU call."""
    index_a, n = _index_or_points(index_a, 'transfer_colors')
    colors = _colors_u8(a_colors, n, 'transfer_colors')
    if len(queries) == 0:
        out = np.zeros((0, 3), np.uint8)
        return (out, np.zeros(0, np.int32)) if return_votes else out
    q = _index_or_points(queries, 'transfer_colors')[0]
    if not isinstance(index_a, CloudIndex):
        index_a = CloudIndex(ctx, index_a)
    index_q = q if isinstance(q, CloudIndex) else CloudIndex(ctx, q)
    nq = index_q.n
    colors_d = _to_device(ctx, colors)          # alive until the launch (see map_colors)
    out = torch.empty((nq, 3), dtype=torch.uint8, device=ctx.device)
    votes = torch.empty((nq,), dtype=torch.int32, device=ctx.device) if return_votes else None
    ws = _workspace(ctx, L.lib().pcc_cloud_transfer_workspace_bytes(index_a.n, nq))
    L.check(L.lib().pcc_cloud_transfer_colors(ctx.handle, _ptr(index_a.buffer), index_a.n, _ptr(colors_d), _ptr(index_q.buffer), nq,
                                              _ptr(out), _ptr(votes), _ptr(ws), ctx.stream), 'pcc_cloud_transfer_colors')
    if return_votes:
        return out.cpu().numpy(), votes.cpu().numpy()
    return out.cpu().numpy()


def cloud_color_distortion(ctx, index_a, a_colors, b_points, b_colors):
    """Colour distortion tally of a decoded coloured cloud B against the original A on the GPU (include/pcc_geo.h "cloud colours"):
    float64[6] = the sums of the squared BT.709 Y, U, V errors over A (against the mean colour of each point's equidistant nearest
    points of B), then over B against A.  index_a: a CloudIndex of A or its (N_A,3) points; colours (N,3) integers in 0..255;
    b_points (N_B,3), N_B >= 1.  utils/pc_metric.color_table turns it into mse / psnr.  Every input is checked before the first GPU
    call; the same inputs give the same bits."""
    index_a, n = _index_or_points(index_a, 'cloud_color_distortion')
    colors_a = _colors_u8(a_colors, n, 'cloud_color_distortion')
    b = _voxel_points(b_points, 'cloud_color_distortion')
    colors_b = _colors_u8(b_colors, int(b.shape[0]), 'cloud_color_distortion')
    if not isinstance(index_a, CloudIndex):
        index_a = CloudIndex(ctx, index_a)
    index_b = CloudIndex(ctx, b)
    dev = ctx.device
    ca_d, cb_d = _to_device(ctx, colors_a), _to_device(ctx, colors_b)     # both alive until the launch (see map_colors)
    tally = torch.empty((COLOR_TALLY_SLOTS,), dtype=torch.float64, device=dev)
    ws = _workspace(ctx, L.lib().pcc_cloud_color_workspace_bytes(index_a.n, index_b.n))
    L.check(L.lib().pcc_cloud_color_distortion(ctx.handle, _ptr(index_a.buffer), index_a.n, _ptr(ca_d), _ptr(index_b.buffer), index_b.n,
                                               _ptr(cb_d), _ptr(tally), _ptr(ws), ctx.stream), 'pcc_cloud_color_distortion')
    return tally.cpu().numpy()


def mesh_to_points(ctx, vertices, faces, n_samples=500000, vg_size=64, seed=0, return_samples=False):
    """A triangle mesh to a voxelised point cloud on the GPU (include/pcc_geo.h "mesh sampling"): the reference's ds_mesh_to_pc
    (area-weighted sampling with pyntcloud's barycentrics, one scalar min / max over all axes, rint onto a vg_size^3 grid, the first
    sample of every voxel), reproducible from `seed` (0 <= seed < 2^64).  vertices (V,3) float64, faces (F,3) integer indices.
    Returns (M,3) float32 voxels in sample order (and the (n,3) float32 raw samples with return_samples=True): the same bits as
    utils/mesh_sampling.mesh_to_points.  Every input is checked on the host before the first GPU call (ValueError)."""
    from ..utils import mesh_sampling
    v, f = mesh_sampling.check_mesh(vertices, faces, n_samples, vg_size, seed)
    n, vg = int(n_samples), int(vg_size)
    dev = ctx.device
    v_d, f_d = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    samples = torch.empty((n, 3), dtype=torch.float32, device=dev) if return_samples else None
    points = torch.empty((n, 3), dtype=torch.float32, device=dev)
    count = torch.empty((1,), dtype=torch.int64, device=dev)
    ws = _workspace(ctx, lambda: L.lib().pcc_mesh_sample_workspace_bytes(f.shape[0], n))
    L.check(L.lib().pcc_mesh_to_points(ctx.handle, _ptr(v_d), v.shape[0], _ptr(f_d), f.shape[0], n, C.c_uint64(int(seed)), vg,
                                       _ptr(samples), _ptr(points), _ptr(count), _ptr(ws), ctx.stream), 'pcc_mesh_to_points')
    m = int(count.item())
    out = points[:m].cpu().numpy()
    return (out, samples.cpu().numpy()) if return_samples else out


def render_points(ctx, points, camera, colors=None, point_size=1, background=(255, 255, 255), return_rows=False):
    """A z-buffered square splat of a point cloud through a pinhole camera on the GPU (include/pcc_geo.h "point rendering").
    points: (n,3) float32, float64 or integer coordinates (any values: points behind the camera or off-screen are dropped);
    camera: a utils.render.Camera; colors: (n,3) integers in 0..255, or None for flat grey (128); point_size: integer side of each
    point's square in [1, 64]; background: RGB.  Returns the (H,W,3) uint8 numpy image (and the (H,W) int32 row of every pixel,
    -1 for the background, with return_rows=True): the same bytes as utils.render.render_host.  Every limit is checked on the
    host before any GPU call (ValueError); n = 0 gives the background without a launch."""
    from ..utils import render
    p, c, s, bg = render.check_render_args(points, colors, camera, point_size, background)
    W, H = camera.width, camera.height
    n = int(p.shape[0])
    if n == 0:
        img = np.broadcast_to(bg, (H, W, 3)).copy()
        return (img, np.full((H, W), -1, np.int32)) if return_rows else img
    dev = ctx.device
    p_d = torch.from_numpy(p).to(dev)
    c_d = None if c is None else torch.from_numpy(c).to(dev)
    img = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    rows = torch.empty((H, W), dtype=torch.int32, device=dev) if return_rows else None
    ws = _workspace(ctx, L.lib().pcc_render_workspace_bytes(W, H))
    E = (C.c_double * 16)(*camera.extrinsic.ravel().tolist())
    K = (C.c_double * 9)(*camera.intrinsic.ravel().tolist())
    bgc = (C.c_uint8 * 3)(*bg.tolist())
    L.check(L.lib().pcc_render_points(ctx.handle, _ptr(p_d), n, _ptr(c_d), E, K, W, H, s, bgc, _ptr(img), _ptr(rows), _ptr(ws),
                                      ctx.stream), 'pcc_render_points')
    if return_rows:
        return img.cpu().numpy(), rows.cpu().numpy()
    return img.cpu().numpy()


def error_map(ctx, index_a, b_points):
    """The squared D1 residual of every decoded point: for each row of b_points, the exact squared distance to its nearest point of
    the original cloud (int64 numpy array; cloud_nearest's distance, so the reference's compute_d1_res_ba whatever the tie rule).
    index_a: a CloudIndex of the original or its (N,3) points; b_points: (nb,3) integer coordinates in [0, 2^21)."""
    index_a, _ = _index_or_points(index_a, 'error_map')
    if len(b_points) == 0:
        return np.zeros(0, np.int64)
    _voxel_points(b_points, 'error_map')
    if not isinstance(index_a, CloudIndex):
        index_a = CloudIndex(ctx, index_a)
    return cloud_nearest(ctx, index_a, b_points)[1]
