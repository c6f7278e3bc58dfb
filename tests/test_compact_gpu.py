"""GPU: pcc_threshold_compact and pcc_voxelize (csrc/elementwise.hip) on the boundary catalogue of tests/_compact_cases.py, against its
numpy restatements (held against the oracle in test_compact_cases_cpu.py).  The kernels are driven through the C ABI so that every
output buffer can be pre-filled with a sentinel: what a call does not own it must leave alone -- the rows from min(count, cap) on, one
extra block of rows behind the last, the ints behind the scratch the call asked for, the floats behind the dense grid."""
import numpy as np
import pytest
import torch

import _compact_cases as K
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ops

pytestmark = pytest.mark.gpu

SENT = 0xCDCDCDCD                      # as a float -4.3e8: no row, no count and no occupancy value looks like it
_SENT_I32 = SENT - (1 << 32)
_DEV = {}


def _filled(n, device):
    return torch.full((int(n),), _SENT_I32, dtype=torch.int32, device=device)


def _on_device(ctx, name):
    """(dhw, blocks, x, thr) of a launch of the catalogue, uploaded once"""
    if name not in _DEV:
        dhw, blocks = K.launch(name)
        x, thr = K.stacked(blocks)
        _DEV[name] = (dhw, blocks, torch.from_numpy(x).to(ctx.device), torch.from_numpy(thr).to(ctx.device))
    return _DEV[name]


def _compact(ctx, x, thr, B, dhw, clip, cap):
    """pcc_threshold_compact into sentinel-filled buffers -> (rc, xyz uint32 (B+1, rows, 3), counts uint32 (B+1,), scratch guard uint32)"""
    D, H, W = dhw
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == B * D * H * W and x.data_ptr() % 4 == 0
    assert thr.dtype == torch.float32 and thr.numel() == B
    rows = max(int(cap), 1)                                               # cap = 0: a one-row dummy per block
    xyz, counts = _filled((B + 1) * rows * 3, ctx.device), _filled(B + 1, ctx.device)
    ns = int(L.lib().pcc_threshold_scratch_ints(B, D, H, W))
    scratch = _filled(ns + 64, ctx.device)
    rc = L.lib().pcc_threshold_compact(ctx.handle, x.data_ptr(), B, D, H, W, thr.data_ptr(), int(clip), xyz.data_ptr(), counts.data_ptr(),
                                       int(cap), scratch.data_ptr(), ctx.stream)
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    return rc, u32(xyz).reshape(B + 1, rows, 3), u32(counts), u32(scratch[ns:])


def _expected(refs, cap, rows):
    """what the buffers hold after a correct call: min(count, cap) rows per block, the sentinel everywhere else"""
    B = len(refs)
    xyz = np.full((B + 1, rows, 3), SENT, np.uint32)
    counts = np.full(B + 1, SENT, np.uint32)
    for b, r in enumerate(refs):
        w = min(len(r), cap)
        xyz[b, :w] = np.ascontiguousarray(r[:w]).view(np.uint32)
        counts[b] = len(r)
    return xyz, counts


def _check(got, refs, cap, names):
    rc, xyz, counts, guard = got
    assert rc == 0, L.lib().pcc_last_error()
    want_xyz, want_counts = _expected(refs, cap, xyz.shape[1])
    B = len(refs)
    bad = np.flatnonzero(counts[:B] != want_counts[:B])
    assert bad.size == 0, [(names[b], int(counts[b]), int(want_counts[b])) for b in bad[:8]]
    for b in range(B):
        if not np.array_equal(xyz[b], want_xyz[b]):
            w = min(int(want_counts[b]), cap)
            row = int(np.flatnonzero((xyz[b] != want_xyz[b]).any(1))[0])
            pytest.fail(f'{names[b]}: row {row} of {w} written rows (cap {cap}) is {xyz[b, row].view(np.float32)} / {xyz[b, row]}, '
                        f'expected {want_xyz[b, row].view(np.float32)} / {want_xyz[b, row]}')
    assert (xyz[B] == SENT).all() and counts[B] == SENT, 'the block behind the last one was written'
    assert (guard == SENT).all(), 'ints behind pcc_threshold_scratch_ints() were written'


@pytest.mark.parametrize('clip', (0, 1))
@pytest.mark.parametrize('name', K.LAUNCHES)
def test_rows_counts_and_untouched_memory(ctx, name, clip):
    dhw, blocks, x, thr = _on_device(ctx, name)
    cap = int(np.prod(dhw))
    _check(_compact(ctx, x, thr, len(blocks), dhw, clip, cap), K.refs(name, clip), cap, [b.name for b in blocks])


@pytest.mark.parametrize('name', K.LAUNCHES)
def test_blocks_are_independent_of_batch_order_and_calls_repeat(ctx, name):
    dhw, blocks, x, thr = _on_device(ctx, name)
    B, cap = len(blocks), int(np.prod(dhw))
    xr, tr = x.flip(0).contiguous(), thr.flip(0).contiguous()
    for clip in (0, 1):
        first = _compact(ctx, x, thr, B, dhw, clip, cap)
        again = _compact(ctx, x, thr, B, dhw, clip, cap)
        assert all(np.array_equal(a, b) for a, b in zip(first[1:], again[1:]))
        rev = _compact(ctx, xr, tr, B, dhw, clip, cap)
        assert rev[0] == first[0] == 0
        assert np.array_equal(rev[2][:B][::-1], first[2][:B]) and np.array_equal(rev[1][:B][::-1], first[1][:B])


@pytest.mark.parametrize('clip', (0, 1))
def test_wrapper_agrees_with_the_direct_call(ctx, clip):
    name = K.shape_id((4, 25, 41))
    dhw, blocks, x, thr = _on_device(ctx, name)
    B, cap = len(blocks), int(np.prod(dhw))
    _, xyz, counts, _ = _compact(ctx, x, thr, B, dhw, clip, cap)
    wx, wc = ops.threshold_compact(ctx, x, thr, clip=bool(clip))
    assert tuple(wx.shape) == (B, cap, 3) and tuple(wc.shape) == (B,)
    wx, wc = wx.cpu().numpy().view(np.uint32), wc.cpu().numpy()
    assert np.array_equal(wc.view(np.uint32), counts[:B])
    for b in range(B):
        assert np.array_equal(wx[b, :wc[b]], xyz[b, :wc[b]]), blocks[b].name


def test_caps_counts_stay_exact_and_only_min_count_cap_rows_are_written(ctx):
    dhw, blocks, caps = K.cap_case()
    x, thr = K.stacked(blocks)
    x, thr = torch.from_numpy(x).to(ctx.device), torch.from_numpy(thr).to(ctx.device)
    refs = K.launch_ref(blocks, 1)
    n = int(np.prod(dhw))
    assert caps[0] == 0 and caps[-1] == n + 5 and len(caps) == 7
    for cap in caps:
        _check(_compact(ctx, x, thr, len(blocks), dhw, 1, cap), refs, cap, [f'{b.name}/cap{cap}' for b in blocks])


def test_batch_limits_65535_blocks_run_and_65536_are_refused(ctx):
    B = 65535
    x = torch.zeros(B + 1, dtype=torch.float32, device=ctx.device)
    x[::2] = 1.0                                                           # alternating hits
    thr = torch.full((B + 1,), 0.5, dtype=torch.float32, device=ctx.device)
    rc, xyz, counts, guard = _compact(ctx, x[:B], thr[:B], B, (1, 1, 1), 0, 1)
    assert rc == 0
    want = (np.arange(B) % 2 == 0)
    assert np.array_equal(counts[:B], want.astype(np.uint32)) and counts[B] == SENT and (guard == SENT).all()
    assert (xyz[:B][want] == 0).all() and (xyz[:B][~want] == SENT).all() and (xyz[B] == SENT).all()
    rc, xyz, counts, guard = _compact(ctx, x, thr, B + 1, (1, 1, 1), 0, 1)
    assert rc == L.PCC_ERR_ARG
    assert (xyz == SENT).all() and (counts == SENT).all() and (guard == SENT).all()      # nothing was launched


def test_view_that_is_not_16_byte_aligned_takes_the_scalar_path(ctx):
    name = K.shape_id((12, 12, 12))
    dhw, blocks, x, thr = _on_device(ctx, name)
    B, cap = len(blocks), int(np.prod(dhw))
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=ctx.device)
    view = buf[1:]
    view.copy_(x.reshape(-1))
    assert x.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    for clip in (0, 1):
        aligned = _compact(ctx, x, thr, B, dhw, clip, cap)
        shifted = _compact(ctx, view, thr, B, dhw, clip, cap)
        _check(shifted, K.refs(name, clip), cap, [b.name for b in blocks])
        assert all(np.array_equal(a, b) for a, b in zip(aligned[1:], shifted[1:]))
        wx, wc = ops.threshold_compact(ctx, view.view(B, *dhw), thr, clip=bool(clip))
        assert np.array_equal(wc.cpu().numpy().view(np.uint32), aligned[2][:B])
        assert np.array_equal(wx.cpu().numpy().view(np.uint32)[0, :int(wc[0])], aligned[1][0, :int(wc[0])])


# ---- voxelise ---------------------------------------------------------------------------------------------------------------------
_VOX_REF = {}


def _vox_ref(c):
    key = (c.name, c.dhw)
    if key not in _VOX_REF:
        _VOX_REF[key] = K.voxelize_ref(c.pts, c.block_of, c.B, *c.dhw)
    return _VOX_REF[key]


def _voxelize(ctx, c):
    """pcc_voxelize into a zeroed grid with 64 sentinel floats behind it in the same allocation -> (rc, dense, guard uint32)"""
    D, H, W = c.dhw
    n = c.B * D * H * W
    buf = torch.zeros(n + 64, dtype=torch.float32, device=ctx.device)
    buf[n:] = _filled(64, ctx.device).view(torch.float32)
    pts = torch.from_numpy(c.pts).to(ctx.device) if len(c.pts) else None
    bof = torch.from_numpy(c.block_of).to(ctx.device) if c.block_of is not None and len(c.pts) else None
    rc = L.lib().pcc_voxelize(ctx.handle, None if pts is None else pts.data_ptr(), None if bof is None else bof.data_ptr(), len(c.pts),
                              c.B, D, H, W, buf.data_ptr(), ctx.stream)
    host = buf.cpu().numpy()
    return rc, host[:n].reshape(c.B, D, H, W), host[n:].view(np.uint32)


def _check_vox(ctx, c):
    from pcc_geo_cnn_v2_amd.model_types import sparse_to_dense
    rc, dense, guard = _voxelize(ctx, c)
    assert rc == 0, (c.name, L.lib().pcc_last_error())
    assert np.array_equal(dense.view(np.uint32), _vox_ref(c).view(np.uint32)), (c.name, c.dhw, np.argwhere(dense != _vox_ref(c))[:4])
    assert (guard == SENT).all(), (c.name, 'floats behind the grid were written')
    if c.in_range:
        bof = np.zeros(len(c.pts), np.int32) if c.block_of is None else c.block_of
        for b in range(c.B):
            want = sparse_to_dense(c.pts[bof == b].astype(np.float64), (1, 1, *c.dhw), 'channels_first')[0, 0]
            assert np.array_equal(dense[b], want), (c.name, c.dhw, b)


@pytest.mark.parametrize('dhw', K.GRIDS, ids=K.shape_id)
def test_voxelize_equals_the_restatement_on_every_case(ctx, dhw):
    cases = K.voxel_cases(dhw)
    assert len(cases) == 11
    for c in cases:
        _check_vox(ctx, c)


def test_voxelize_past_one_pass_of_its_largest_grid(ctx):
    c = K.voxel_grid_pass_case(ctx.num_cu)
    assert len(c.pts) == ctx.num_cu * 8 * 256 + 5
    _check_vox(ctx, c)


def test_voxelize_wrapper_refuses_bad_arguments_before_any_launch(ctx, monkeypatch):
    calls = []
    real = L.lib().pcc_voxelize
    monkeypatch.setattr(L.lib(), 'pcc_voxelize', lambda *a: calls.append(a) or real(*a))
    n = 10
    pts = torch.zeros((n, 3), dtype=torch.int32, device=ctx.device)
    bof = torch.zeros(n, dtype=torch.int32, device=ctx.device)
    bad = {
        'block_of too short': (pts, bof[:n - 1]),
        'block_of too long': (pts, torch.zeros(n + 1, dtype=torch.int32, device=ctx.device)),
        'block_of not contiguous': (pts, torch.zeros(2 * n, dtype=torch.int32, device=ctx.device)[::2]),
        'block_of on the host': (pts, bof.cpu()),
        'block_of int64': (pts, bof.long()),
        'pts (n, 4)': (torch.zeros((n, 4), dtype=torch.int32, device=ctx.device), bof),
        'pts flat': (pts.reshape(-1), bof),
        'pts (3, n)': (torch.zeros((3, n), dtype=torch.int32, device=ctx.device), bof),
        'pts int64': (pts.long(), bof),
        'pts float32': (pts.float(), bof),
    }
    for what, (p, b) in bad.items():
        with pytest.raises(AssertionError):
            ops.voxelize(ctx, p, b, 1, 4, 4, 4)
            pytest.fail(what)
    assert calls == []
    assert float(ops.voxelize(ctx, pts, bof, 1, 4, 4, 4).sum()) == 1.0 and len(calls) == 1
