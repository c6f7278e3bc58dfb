"""Thin torch-facing wrappers over the C ABI (include/pcc_geo.h), one module per subsystem; every name is used as `ops.<name>`.

PyTorch-ROCm is plumbing only: it owns device memory (tensors) and streams; every operator below is
a hand-written HIP kernel (or the host range coder) inside libpcc_geo_hip.so.
"""
from ._context import (  # noqa: F401
    _ptr, Context, _ContextView, _CONTEXTS, get_context, usable_cores)
from .conv import (  # noqa: F401
    ConvLayer, conv_out_shape, conv3d, NetworkWeights, _FAMILY, network_forward, network_plan, profile_select, profile_read, conv3d_fp16_storage,
    mfma_supported)
from .codec import (  # noqa: F401
    codec_desc, _ITEM, SymbolStaging, symbols_pack, symbols_unpack, _out, quantize_pack, index_pack, unpack_dequantize,
    codec_encode, _packed_io, codec_decode_hyper, codec_decode_main, quantize, dequantize, scale_to_index, threshold_compact, topk_compact, voxelize,
    quantize_step_pack, index_pack_step, unpack_dequantize_step, cost16_table, device_cost_table, rate_ladder)
from .training import (  # noqa: F401
    focal_loss, focal_loss_grad, relu_backward, dual_desc, conv_repack_map, conv_repack_device, conv_wgrad_slices, conv3d_wgrad,
    histogram_limits, _f32_flat, histogram_unpack, tensor_histograms_launch, tensor_histograms, tensor_histogram, occupancy_scores_launch,
    occupancy_scores)
from .search import (  # noqa: F401
    d1_threshold_stats, d12_threshold_stats, SearchTiePairOverflow,
    search_tie_pair_capacity, d12_threshold_stats_ties_launch, d12_threshold_stats_ties, check_count_rows, rank_levels, d1_count_stats,
    d12_count_stats)
from .cloud import (  # noqa: F401
    NORMALS_COORD_LIMIT, _voxel_points, estimate_normals, CLOUD_TALLY_SLOTS, _device_u8, _device_points, CloudIndex, cloud_nearest,
    _normals64, TIE_MODES, _PAIR_LIMIT, tie_pair_capacity, _tie_mode, cloud_distortion_launch, TiePairOverflow, cloud_distortion,
    COLOR_TALLY_SLOTS, _colors_u8, _index_or_points, map_colors, transfer_colors, cloud_color_distortion, mesh_to_points, render_points, error_map)
from .anchors import (  # noqa: F401
    _u8, anchor_code_bits, anchor_decode_bits, anchor_encode_nodes, AnchorDecoder, anchor_tree_launch, anchor_tree,
    anchor_expand, anchor_points, surface_encode_vertices, surface_decode_vertices, _surface_ws, _surface_hdr, surface_leaves,
    surface_edges, surface_vertices, surface_reconstruct, _color_counts, color_anchor_encode_coefficients, color_anchor_decode_coefficients,
    _color_ws, _color_hdr, color_anchor_plan, color_anchor_transform, color_anchor_inverse)
from .coders import (  # noqa: F401
    HostCdfTable, _np_i32, _np_host, _uniform_dtype, _SYM, _ROW, _rows_2d, _row_ptrs, _pp, _sz, range_encode_batch,
    range_decode_batch, pmf_to_quantized_cdf, rans_stream_cap, _rans_counts, _rans_index, rans_encode_launch, rans_encode_fetch,
    rans_encode_batch, rans_check_status, rans_decode_batch, occ_stream_cap, occ_encode_launch, occ_encode_fetch, occ_encode_batch,
    occ_check_status, occ_decode_batch)
