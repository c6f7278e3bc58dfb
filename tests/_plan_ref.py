"""The fp16 storage plan as the layer-by-layer path restated it while csrc/network.hip and model_transforms.py each kept a copy:
the bodies of ResidualLayer.fp16_storage and SequentialLayer._final_in16 and the flags their two forward_ndhwc loops set, over plain
layer tuples instead of layer objects.  Test code: the oracle of pcc_network_plan (tests/test_network_plan_cpu.py)."""
import collections
import ctypes as C

from pcc_geo_cnn_v2_amd import _lib as L

Conv = collections.namedtuple('Conv', 'cin cout k stride transposed flags impl')     # flags: the layer's own (BIAS / RELU / ADD)
Block = collections.namedtuple('Block', 'residual_mode layers')                      # a ResidualLayer of Convs

IN16, OUT16, RES16 = L.PCC_CONV_IN16, L.PCC_CONV_OUT16, L.PCC_CONV_RES16


def desc(l, N, D, H, W, flags):
    return L.ConvDesc(N, D, H, W, l.cin, l.cout, l.k, l.stride, int(l.transposed), flags | l.flags, L.PCC_IMPL_AUTO, 0, 0)


def conv_out_shape(l, x_shape):
    N, D, H, W, _ = x_shape
    s = l.stride
    if l.transposed:
        return (N, D * s, H * s, W * s, l.cout)
    o = lambda n: -(-n // s)
    return (N, o(D), o(H), o(W), l.cout)


def fp16_storage(conv_flags, block, x_shape):
    """Inside an AnalysisBlock / SynthesisBlock of width 16, 32 or 64 whose grid is a multiple of 16 the two intermediate tensors live
    in HBM as fp16 -- the stride-2 conv hands over in fp16 (PCC_CONV_OUT16), the two k3 stride-1 convs run on conv_f16.hip
    (PCC_CONV_IN16), the last one adds the fp16 residual and writes fp32."""
    if not (conv_flags & L.PCC_CONV_F16) or block.residual_mode != 'add' or len(block.layers) != 3:
        return False
    if any(c.impl != L.PCC_IMPL_AUTO for c in block.layers):
        return False
    first, mid, last = block.layers
    N, D, H, W, _ = x_shape
    if not (first.k == 3 and first.stride == 2 and first.cout in (16, 32, 64) and H % 2 == 0 and W % 2 == 0):
        return False
    _, oD, oH, oW, _ = conv_out_shape(first, x_shape)
    if oH % 16 or oW % 16:
        return False
    d0 = desc(first, N, D, H, W, L.PCC_CONV_F16)
    if L.lib().pcc_conv_mfma_supported(C.byref(d0)) != 1:          # (a layer on the generic path cannot hand over in fp16)
        return False
    for l in (mid, last):      # pcc_f16_eligible (csrc/conv_f16.hip)
        if not (l.k == 3 and l.stride == 1 and l.cin == l.cout and l.cin in (16, 32, 64) and oH * oW * l.cin * 4 < 2 ** 31):
            return False
        d = desc(l, N, oD, oH, oW, L.PCC_CONV_F16 | L.PCC_CONV_IN16)
        if L.lib().pcc_conv_mfma_supported(C.byref(d)) != 1:
            return False
    return True


def final_in16(conv_flags, block, fin, x_shape):
    """In the fp16 mode the output of the last block stays fp16 when its only consumer is the final 16 -> 1 k3 stride-1 transposed
    conv."""
    if not (isinstance(block, Block) and isinstance(fin, Conv) and fp16_storage(conv_flags, block, x_shape)):
        return False
    if not (fin.transposed and fin.cout == 1 and fin.k == 3 and fin.stride == 1 and fin.impl == L.PCC_IMPL_AUTO
            and block.layers[-1].cout == 16):
        return False
    N, D, H, W, _ = conv_out_shape(block.layers[0], x_shape)
    d = desc(fin, N, D, H, W, L.PCC_CONV_F16 | L.PCC_CONV_IN16)
    return L.lib().pcc_conv_mfma_supported(C.byref(d)) == 1


def storage_bits(conv_flags, layers, x_shape):
    """The PCC_CONV_IN16 / OUT16 / RES16 bits of every conv of a SequentialLayer of Convs and Blocks, conv_layers() order, as its
    forward_ndhwc and ResidualLayer.forward_ndhwc chose them."""
    bits = []
    for i, layer in enumerate(layers):
        if i == len(layers) - 2 and final_in16(conv_flags, layer, layers[-1], x_shape):
            return bits + [OUT16, IN16 | OUT16, IN16 | RES16 | OUT16, IN16]
        if isinstance(layer, Block):
            bits += [OUT16, IN16 | OUT16, IN16 | RES16] if fp16_storage(conv_flags, layer, x_shape) else [0] * len(layer.layers)
            for l in layer.layers:
                x_shape = conv_out_shape(l, x_shape)
        else:
            bits.append(0)
            x_shape = conv_out_shape(layer, x_shape)
    return bits
