"""Every instantiation of the direct conv kernels (conv_fwd.hip, conv_tr2.hip, conv_edge.hip, conv_tr2m.hip, conv_generic.hip), of
their fp16-MFMA twins and of the fp16-storage kernels (conv_f16.hip, conv_tr2m_f16.hip, the fp16-input 16 -> 1 layer), launched through
pcc_conv3d on integer operands (tests/_direct_cases.py) and compared with the float64 reference by equality, per output: on these
inputs every correct kernel returns the float64 value bit for bit, whatever its tile, slab, summation order or MFMA chain, and
whether it stores fp32 or fp16.  No tolerance appears in this file."""
import numpy as np
import pytest
import torch

import _direct_cases as DC
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ops

pytestmark = pytest.mark.gpu
FC = DC.FC


def _check(ctx, row, want=None):
    """Steps 1 - 4 of a row; returns the written channels."""
    # 1. the launchers' choice on THIS machine's CU count still names the row's kernel (fail, never skip)
    sel = DC.select(row, DC.flags_of(row), row['switches'], ctx.num_cu)
    assert sel['kernel'] == row['kernel'], f'{row["id"]}: with {ctx.num_cu} CUs the launcher takes {sel["kernel"]}, the row means {row["kernel"]}'
    for key in ('zsplit', 'zsp'):             # ... and the number of z slabs the row means
        assert key not in row or sel[key] == row[key], f'{row["id"]}: with {ctx.num_cu} CUs the launcher takes {key} = {sel[key]}, the row means {row[key]}'
    arrays = DC.inputs(row)
    if want is None:
        want = DC.reference(row)
    # 2. the family, then the launch (run asks pcc_conv_kernel_family under the row's switches before it launches)
    fam, buf = FC.run(ctx, row, arrays)
    assert fam.startswith(row['family']), (row['id'], fam)
    # 3. equality per output, and nothing written outside the layer's channels
    got, clean = FC.written(row, buf)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), DC.explain(row, got, want, sel['tile'])
    assert clean, f'{row["id"]}: channels outside [{row["oco"]}, {row["oco"] + row["geo"][5]}) of the output buffer were written'
    # 4. the same bits again
    fam2, buf2 = FC.run(ctx, row, arrays)
    assert fam2 == fam and np.array_equal(buf2, buf), f'{row["id"]}: a second launch gave other bits'
    return got


@pytest.mark.parametrize('row', DC.ROWS, ids=[r['id'] for r in DC.ROWS])
def test_base_grid_row_is_exact(ctx, oracle, row):
    _check(ctx, row)


def _windowed(ctx, group):
    return [r for r in DC.windowed_rows(ctx.num_cu) if r['group'] == group]


def _pin_torch_oracle(oracle, row):
    """The oneDNN restatement against the float64-accumulating C loops on one block of the row, shortened in z: equal, not close."""
    N, D, H, W, cin, cout, k, s, tr = row['geo']
    slab = dict(row, geo=(1, min(D, 5)) + row['geo'][2:], id=row['id'] + '/slab')
    a, b = DC.reference(slab, use_torch=True), DC.reference(slab, use_torch=False)
    assert np.array_equal(a, b), f'{row["id"]}: oracle/torch_oracle.py and oracle/pcc_oracle.c differ on integer operands'


def test_big_tile_is_exact_and_equals_the_small_tile(ctx, oracle):
    """64 -> 64 k3 stride 1 on (N, 15, 20, 32) with N such that launch_fwd takes the 2 x 8 x 16 tile.  One block of the batch alone
    takes the 2 x 4 x 16 tile: DESIGN.md section 4 promises one summation order per output whatever the batch, so on Gaussian data
    the two launches must agree in every bit."""
    row, twin = _windowed(ctx, 'big')
    _pin_torch_oracle(oracle, row)
    _check(ctx, row)
    _check(ctx, twin)             # the fp16-MFMA twin of the big tile, transposed-flipped, channel-offset output
    N, D, H, W, cin, cout, k, s, tr = row['geo']
    one = dict(row, geo=(1,) + row['geo'][1:])
    assert DC.select(one, DC.flags_of(one), {}, ctx.num_cu)['kernel'] == 'conv_fwd_kernel<64,64,3,1,16,2,4,16,2,4>'
    rng = np.random.default_rng(77)
    w = (rng.standard_normal((3, 3, 3, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    layer = ops.ConvLayer(w, rng.standard_normal(cout).astype(np.float32), 1, False, True)
    g = torch.Generator().manual_seed(78)
    x = torch.randn((N, D, H, W, cin), generator=g).to(ctx.device)
    r = torch.randn((N, D, H, W, cout), generator=g).to(ctx.device)
    batch = ops.conv3d(ctx, x, layer, residual=r, impl=L.PCC_IMPL_MFMA)
    for n in (0, N // 2, N - 1):
        alone = ops.conv3d(ctx, x[n:n + 1].contiguous(), layer, residual=r[n:n + 1].contiguous(), impl=L.PCC_IMPL_MFMA)
        differ = int((alone != batch[n:n + 1]).sum().item())
        assert torch.equal(alone, batch[n:n + 1]), f'block {n}: {differ} of {alone.numel()} outputs differ between the big and the small tile'


@pytest.mark.parametrize('rid', ['pers-loop', 'pers-loop-p16'])
def test_persistent_16_16_walks_more_tiles_than_slots(ctx, oracle, rid):
    """conv16_pers_kernel with more tiles than workgroups: has_next, the LDS buffer swap and the deferred epilogue of the previous
    tile, with partial tiles in z and y."""
    (row,) = [r for r in _windowed(ctx, 'pers') if r['id'] == rid]
    sel = DC.select(row, DC.flags_of(row), row['switches'], ctx.num_cu)
    assert sel['ntiles'] > sel['slots'] and sel['ntiles'] % sel['slots']
    _pin_torch_oracle(oracle, row)
    _check(ctx, row)


@pytest.mark.parametrize('rid', ['tr2g-loop-32-16-w16', 'tr2g-loop-64-32-w16', 'tr2g-loop-64-64-w8'])
def test_tr2g_walks_more_tiles_than_slots(ctx, oracle, rid):
    """conv_tr2g_kernel with more tiles than workgroups: the next tile's first channel group is staged under this tile's last, and
    the weight ring wraps into the next tile."""
    (row,) = [r for r in _windowed(ctx, 'tr2g') if r['id'] == rid]
    sel = DC.select(row, DC.flags_of(row), row['switches'], ctx.num_cu)
    assert sel['ntiles'] > sel['slots'] and sel['ntiles'] % sel['slots']
    _pin_torch_oracle(oracle, row)
    _check(ctx, row)


def test_cout1_mfma_32_wide_columns_one_and_two_slabs(ctx, oracle):
    """conv_cout1_mfma_kernel<false, 32, false> with one z slab, with slabs of 17 and 16 planes, and with four and eight slabs of 16
    planes (the seams of the 64^3 and 128^3 batches); the one-slab layer under cout1_t16 (16 x 16 columns), which the numerics tag
    treats as the same bits."""
    rows = {r['id']: r for r in _windowed(ctx, 'cout1')}
    for rid, zsp in (('cout1m-t32-zsp1', 1), ('cout1m-t32-zsp2', 2), ('cout1m-t32-zsp4', 4), ('cout1m-t32-zsp8', 8)):
        assert rows[rid]['zsp'] == zsp and DC.select(rows[rid], DC.flags_of(rows[rid]), {}, ctx.num_cu)['zsp'] == zsp
    _pin_torch_oracle(oracle, rows['cout1m-t32-zsp2'])
    a = _check(ctx, rows['cout1m-t32-zsp1'])
    b = _check(ctx, rows['cout1m-t16-forced'])
    assert np.array_equal(a, b)
    _check(ctx, rows['cout1m-t32-zsp2'])
    _check(ctx, rows['cout1m-t32-zsp4'])
    _check(ctx, rows['cout1m-t32-zsp8'])


@pytest.mark.parametrize('zsp', [1, 2, 4, 8])
def test_cout1_mfma_32_wide_columns_fp16_input(ctx, oracle, zsp):
    """conv_cout1_mfma_kernel<true, 32, false>: the same four slab counts with an fp16 input tensor (one fp16 MFMA per tap tile)."""
    (row,) = [r for r in _windowed(ctx, 'cout1') if r['id'] == f'cout1m-t32-zsp{zsp}-in16']
    assert row['zsp'] == zsp and row['kernel'] == 'conv_cout1_mfma_kernel<true,32,false>'
    if zsp == 2:
        _pin_torch_oracle(oracle, row)
    _check(ctx, row)


def test_cout1_mfma_with_fp16_input_refuses_a_residual(ctx):
    """The 16 -> 1 kernel reads its residual as fp32.  pcc_conv3d accepts an fp16-input layer only with an fp16 residual
    (PCC_CONV_RES16), so the launcher refuses the combination before anything is launched instead of reading a half-sized tensor as
    fp32."""
    row = dict(DC.BY_ID['cout1m-t16-w24-in16'], res=True)
    out = torch.zeros(1, device=ctx.device)
    with pytest.raises((AssertionError, L.PccError), match='takes no residual'):
        FC.run(ctx, row, DC.inputs(row))
    torch.cuda.synchronize()
    assert float(out.item()) == 0.0
