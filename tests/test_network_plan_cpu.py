"""CPU-only: pcc_network_plan (csrc/network.hip), the one place that decides which tensors of a transform the fp16 mode stores as
fp16 and which layer records block maxima -- against the restatement the layer-by-layer path used to keep (tests/_plan_ref.py), against
answers worked out by hand, and on its own contract (dims, flags, roles, impl, errors).  Integer equality throughout."""
import ctypes as C
import itertools

import pytest

import _plan_ref as R
from pcc_geo_cnn_v2_amd import _lib as L
from pcc_geo_cnn_v2_amd import ops

IN16, OUT16, RES16 = L.PCC_CONV_IN16, L.PCC_CONV_OUT16, L.PCC_CONV_RES16
STORAGE = IN16 | OUT16 | RES16
SYNTHESIS_SIDE = (L.PCC_NET_SYNTHESIS_V1, L.PCC_NET_SYNTHESIS_V2, L.PCC_NET_SYNTHESIS_PROGRESSIVE_V2, L.PCC_NET_HYPER_SYNTHESIS)
ODD_GRIDS = [(8, 8, 24), (8, 8, 12), (8, 24, 8), (33, 32, 32), (32, 32, 34)]


def stack(tid, F):
    """([pcc_conv_desc], [role]) of a transform as pcc_network_layer gives them."""
    descs, roles = [], []
    for i in range(L.lib().pcc_network_num_layers(tid, F)):
        d, role = L.ConvDesc(), C.c_int32()
        assert L.lib().pcc_network_layer(tid, F, i, C.byref(d), C.byref(role)) == 0
        descs.append(d)
        roles.append(role.value)
    return descs, roles


def storage(plan):
    return [p.desc.flags & STORAGE for p in plan]


def grids(tid):
    return [(e, e, e) for e in ((2, 4, 8, 16) if tid in SYNTHESIS_SIDE else (16, 32, 64))] + ODD_GRIDS


def ref_layers(descs, roles):
    """The stack as the Sequential / Residual layer objects grouped it: roles 1, 0, 2 are one 'add' block."""
    convs = [R.Conv(d.Cin, d.Cout, d.k, d.stride, d.transposed, d.flags, d.impl) for d in descs]
    layers, i = [], 0
    while i < len(convs):
        if roles[i] == 1:
            assert roles[i:i + 3] == [1, 0, 2]
            layers.append(R.Block('add', convs[i:i + 3]))
            i += 3
        else:
            assert roles[i] == 0
            layers.append(convs[i])
            i += 1
    return layers


@pytest.mark.parametrize('tid', range(8))
def test_planned_storage_equals_the_layerwise_restatement(tid):
    for F in (32, 64):
        descs, roles = stack(tid, F)
        layers = ref_layers(descs, roles)
        for N, lf, ff, (D, H, W) in itertools.product((1, 3), (0, L.PCC_CONV_F16), (0, L.PCC_CONV_CLIP01), grids(tid)):
            shape = (N, D, H, W, descs[0].Cin)
            plan = ops.network_plan(descs, roles, shape, lf, ff)
            assert storage(plan) == R.storage_bits(lf, layers, shape), (tid, F, shape, lf, ff)
            # dims: the chain of pcc_conv_out_dims; flags: the layer's own, layer_flags, final_flags on the last layer only
            for i, (p, d) in enumerate(zip(plan, descs)):
                assert (p.desc.N, p.desc.D, p.desc.H, p.desc.W) == (N, D, H, W)
                assert (p.desc.Cin, p.desc.Cout, p.desc.k, p.desc.stride, p.desc.transposed, p.desc.impl) == \
                    (d.Cin, d.Cout, d.k, d.stride, d.transposed, d.impl)
                assert p.desc.flags & ~STORAGE == d.flags | lf | (ff if i == len(plan) - 1 else 0)
                od, oh, ow = C.c_int32(), C.c_int32(), C.c_int32()
                assert L.lib().pcc_conv_out_dims(C.byref(p.desc), C.byref(od), C.byref(oh), C.byref(ow)) == 0
                D, H, W = od.value, oh.value, ow.value


KNOWN = [(L.PCC_NET_SYNTHESIS_PROGRESSIVE_V2, 4, [0, 0, 0, 64, 96, 160, 64, 96, 224, 32]),
         (L.PCC_NET_SYNTHESIS_PROGRESSIVE_V2, 2, [0, 0, 0, 0, 0, 0, 64, 96, 224, 32]),
         (L.PCC_NET_ANALYSIS_PROGRESSIVE_V2, 32, [64, 96, 160, 0, 0, 0, 0, 0, 0, 0])]


@pytest.mark.parametrize('tid,edge,want', KNOWN)
def test_known_answers(tid, edge, want):
    """F = 64, N = 1; worked out by hand from the state machine pcc_network_forward ran before the planner."""
    descs, roles = stack(tid, 64)
    shape = (1, edge, edge, edge, descs[0].Cin)
    assert (IN16, OUT16, RES16) == (32, 64, 128)
    assert storage(ops.network_plan(descs, roles, shape, L.PCC_CONV_F16)) == want
    assert R.storage_bits(L.PCC_CONV_F16, ref_layers(descs, roles), shape) == want
    assert storage(ops.network_plan(descs, roles, shape, 0)) == [0] * len(want)


def synthesis_block(C_=32):
    """A SynthesisBlock of width C_ fed with C_ channels: transposed k3 stride 2, then two transposed k3 stride 1."""
    own = L.PCC_CONV_BIAS | L.PCC_CONV_RELU
    return [L.ConvDesc(0, 0, 0, 0, C_, C_, 3, s, 1, own | add, L.PCC_IMPL_AUTO, 0, 0) for s, add in ((2, 0), (1, 0), (1, L.PCC_CONV_ADD))]


def test_roles_and_impl_decide_storage():
    shape = (1, 8, 8, 8, 32)
    blk = synthesis_block()
    assert storage(ops.network_plan(blk, [1, 0, 2], shape, L.PCC_CONV_F16)) == [OUT16, IN16 | OUT16, IN16 | RES16]
    assert storage(ops.network_plan(blk, [0, 0, 0], shape, L.PCC_CONV_F16)) == [0, 0, 0]           # a 'concat' block
    four = blk[:2] + [blk[1]] + blk[2:]
    assert storage(ops.network_plan(four, [1, 0, 0, 2], shape, L.PCC_CONV_F16)) == [0, 0, 0, 0]    # a block of another length
    for i in range(3):          # a caller's impl override on any layer of the block
        over = synthesis_block()
        over[i].impl = L.PCC_IMPL_WINOGRAD
        plan = ops.network_plan(over, [1, 0, 2], shape, L.PCC_CONV_F16)
        assert storage(plan) == [0, 0, 0] and [p.desc.impl for p in plan] == [o.impl for o in over]
    # ... and on the 16 -> 1 layer behind the last block: the block keeps its storage and hands over in fp32
    descs, roles = stack(L.PCC_NET_SYNTHESIS_PROGRESSIVE_V2, 64)
    descs[-1].impl = L.PCC_IMPL_MFMA
    assert storage(ops.network_plan(descs, roles, (1, 4, 4, 4, 64), L.PCC_CONV_F16)) == [0, 0, 0, 64, 96, 160, 64, 96, 160, 0]


def test_block_maxima_requests():
    lib = L.lib()
    descs, roles = stack(L.PCC_NET_SYNTHESIS_PROGRESSIVE_V2, 64)
    n = len(descs)

    def asked(lf, numerics):
        plan, any_amax = (L.LayerPlan * n)(), C.c_int32(-1)
        assert lib.pcc_network_plan((L.ConvDesc * n)(*descs), (C.c_int32 * n)(*roles), n, 2, 8, 8, 8, lf, 0, numerics, plan, C.byref(any_amax)) == 0
        rec = [p.record_amax for p in plan]
        assert set(rec) <= {0, 1} and rec[-1] == 0 and any_amax.value == int(any(rec))
        return rec

    # layer 1 (64 -> 64 k3 stride 1 on the 16^3 grid) takes the two-piece fp16 Winograd kernel: layer 0 records for it
    assert asked(0, 0)[0] == 1
    assert asked(L.PCC_CONV_F16, 0) == [0] * n
    assert asked(0, L.PCC_NUM['no_f16s']) == [0] * n
    assert asked(0, L.PCC_NUM['no_split']) == [0] * n


def test_bad_arguments_are_refused():
    lib = L.lib()
    blk, roles, plan = (L.ConvDesc * 3)(*synthesis_block()), (C.c_int32 * 3)(1, 0, 2), (L.LayerPlan * 3)()
    good = [blk, roles, 3, 1, 8, 8, 8, L.PCC_CONV_F16, 0, 0, plan, None]
    assert lib.pcc_network_plan(*good) == 0
    bad = [{0: None}, {1: None}, {10: None}, {2: 0}, {2: -1}, {3: 0}, {4: 0}, {5: -8}, {6: 0}]
    for change in bad:
        args = [change.get(i, a) for i, a in enumerate(good)]
        lib.pcc_network_plan(*good)
        assert lib.pcc_network_plan(*args) == L.PCC_ERR_ARG, change
        assert b'pcc_network_plan' in lib.pcc_last_error(), change
