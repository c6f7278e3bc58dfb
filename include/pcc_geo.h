/*
 * pcc_geo.h -- C ABI of libpcc_geo_hip.so, the MI355X (gfx950) implementation of the
 * 64^3-voxel-block encode+decode hot path of mauriceqch/pcc_geo_cnn_v2.
 *
 * The reference has NO native/FFI interface for this path: its operators are TensorFlow-1.15 /
 * tensorflow-compression-1.3 ops invoked from Python.  Each entry point below
 * therefore names the reference call site (file:line under /root/reference) whose third-party op it
 * replaces; INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no torch types; every function returns 0 on success, <0 on error
 *     (pcc_last_error() returns the message of the calling thread's last failure);
 *   - device buffers are owned by the caller (PyTorch-ROCm tensors' data_ptr()); the library
 *     allocates nothing persistent except the context it frees in pcc_ctx_destroy;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls are stream-ordered,
 *     asynchronous, and not re-entrant on one context;
 *   - activations: NDHWC float32, (D,H,W) = (x,y,z) as in src/model_types.py:108-114;
 *     forward kernels (kd,kh,kw,Cin,Cout), transposed kernels (kd,kh,kw,Cout,Cin)  [Keras layouts];
 *   - all convolutions are TF padding='same' (asymmetric, extra element on the high side).
 */
#ifndef PCC_GEO_H
#define PCC_GEO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCC_ABI_VERSION 4

/* ---- errors / context ------------------------------------------------------------------ */
#define PCC_OK 0
#define PCC_ERR_ARG (-1)     /* bad argument / unsupported shape                                   */
#define PCC_ERR_HIP (-2)     /* a HIP runtime call failed                                          */
#define PCC_ERR_NOGPU (-3)   /* no gfx950 device visible                                           */
#define PCC_ERR_SPACE (-4)   /* output buffer too small                                            */
#define PCC_ERR_CORRUPT (-5) /* range decoder ran past a corrupt stream                            */

typedef struct pcc_ctx pcc_ctx;

int pcc_abi_version(void);
const char* pcc_last_error(void);
/* Replaces tf.Session creation (src/compress_octree.py:84-92).  One context per (process, GPU). */
int pcc_ctx_create(int device, pcc_ctx** out);
int pcc_ctx_destroy(pcc_ctx* ctx);
/* Number of compute units of the context's device (256 on MI355X); <0 on error. */
int pcc_ctx_num_cu(pcc_ctx* ctx);

/* ---- codec numerics: which kernel family computes a layer ---------------------------------
 * Encoder and decoder must produce the SAME bits for sigma-hat (it selects the entropy coder's rows: a single flipped scale index
 * desynchronises the range decoder -- the reason for the reference's --debug retries, src/decompress_octree.py:84-101).  Every
 * kernel here is bit-deterministic, but two kernel families (exact-fp32 MFMA, split-bf16 MFMA, Winograd, direct ...) give different
 * round-off.  What selects the family is therefore STATE OF THE CONTEXT, read ONCE from the environment in pcc_ctx_create (the
 * PCC_* variables named below) and changeable only through pcc_ctx_set_numerics -- never per call -- and it is recorded beside
 * every stream the CLIs write (gzip header comment, model_syntax.write_tagged_gzip) together with PCC_KERNEL_FAMILY, which is bumped whenever
 * a default kernel's summation order changes.  The decoder refuses a stream written under another tag. */
#define PCC_KERNEL_FAMILY 6
#define PCC_NUM_NO_SPLIT 0x1         /* PCC_NO_SPLIT=1: every split-bf16 kernel off (exact-fp32 MFMA everywhere)              */
#define PCC_NUM_NO_SPLIT_DIRECT 0x2  /* PCC_NO_SPLIT_DIRECT=1: the direct 32- / 64-channel split kernels off                  */
#define PCC_NUM_NO_SPLIT_TR2 0x4     /* PCC_NO_SPLIT_TR2=1: the stride-2 transposed split kernels off                         */
#define PCC_NUM_NO_WINOGRAD 0x8      /* PCC_NO_WINOGRAD=1: direct kernels instead of Winograd                                 */
#define PCC_NUM_NO_WINOGRAD32 0x10   /* PCC_NO_WINOGRAD32=1                                                                   */
#define PCC_NUM_NO_WINOGRAD64 0x20   /* PCC_NO_WINOGRAD64=1                                                                   */
#define PCC_NUM_WINO_PER_GROUP 0x40  /* PCC_WINO_PER_GROUP=1: one Winograd launch per cin group                               */
#define PCC_NUM_NO_TR2M 0x80         /* PCC_NO_TR2M=1: tiled stride-2 transposed kernels instead of the z march               */
#define PCC_NUM_TR2M 0x100           /* PCC_TR2M=1: the z march wherever it is eligible                                       */
#define PCC_NUM_TR2_OLD 0x200        /* PCC_TR2_OLD=1: per-tile conv_tr2_kernel                                               */
#define PCC_NUM_SPLIT_MFMA16 0x400   /* PCC_SPLIT_MFMA=16: 16x16x32 formulation of the direct split kernel                    */
#define PCC_NUM_SPLIT_MFMA32 0x800   /* PCC_SPLIT_MFMA=32: 32x32x16 formulation                                               */
#define PCC_NUM_SPLIT_TILE8 0x1000   /* PCC_SPLIT_TILE=8                                                                      */
#define PCC_NUM_P16 0x2000           /* PCC_P16=1: one 8-wave workgroup per CU in the direct 16 -> 16 kernel                  */
#define PCC_NUM_NO_F16S 0x4000       /* PCC_NO_F16S=1: the Winograd layers keep three bf16 pieces / exact fp32 (no two-piece fp16 split) */
#define PCC_NUM_COUT1_T16 0x8000     /* PCC_COUT1_T16=1: 16 x 16 columns in the 16 -> 1 last layer (same bits as 32 x 32: tested)  */
/* family = PCC_KERNEL_FAMILY of this build, switches = OR of PCC_NUM_* in effect on this context */
int pcc_ctx_get_numerics(pcc_ctx* ctx, uint32_t* family, uint32_t* switches);
/* Replace the switches (tests, A/B runs).  Not to be called between an encode and the decode of its stream. */
int pcc_ctx_set_numerics(pcc_ctx* ctx, uint32_t switches);

/* ---- 3-D convolution / transposed convolution -------------------------------------------
 * Replaces the TF ops behind keras Conv3D / Conv3DTranspose (+BiasAdd, Relu, AddV2) at
 * src/model_transforms.py:45-47,56-58,67-69,78-80,93,107,121,135,144-146,155-157 and the residual
 * add of ResidualLayer.call (src/model_transforms.py:30-36).
 * out = [clip01]( relu?(conv(in) + bias?) + residual? )                                        */
#define PCC_CONV_BIAS 1
#define PCC_CONV_RELU 2
#define PCC_CONV_ADD 4     /* add `residual` AFTER the activation (ResidualLayer 'add' mode)      */
#define PCC_CONV_CLIP01 8  /* np.clip(x_hat,0,1) fused (src/model_types.py:202), encoder flavour  */
#define PCC_CONV_F16 16    /* fp16 matrix instructions (operands rounded RTN, fp32 accumulate and storage) on the
                              direct MFMA kernels; BASELINE.json configs[4].  Not the default: the reference is fp32 */

/* fp16 STORAGE inside the fp16 mode (mid-network tensors of the c3 / c3p blocks; used by pcc_network_forward with
 * PCC_CONV_F16, accepted here for callers that chain layers themselves).  Buffers are passed through the same pointers.   */
#define PCC_CONV_IN16 32   /* `in` (and `residual`, if any: see RES16) are fp16 NDHWC: k3 stride-1 layers with Cin = Cout in
                              {16, 32, 64} and H, W multiples of 16 (conv_f16.hip, v_mfma_f32_16x16x32_f16), and the 16 -> 1
                              k3 stride-1 transposed layer.  The 64-channel layers keep fp16 partial sums of the first input
                              half in a scratch tensor owned by the context (allocated on first use, N*D*H*W*128 bytes):
                              calls that use it must be ordered on one stream per context                                 */
#define PCC_CONV_OUT16 64  /* `out` is fp16 NDHWC: the IN16 layers and the k3 stride-2 transposed layers                  */
#define PCC_CONV_RES16 128 /* `residual` is fp16 (always together with IN16)                                              */

#define PCC_IMPL_AUTO 0    /* MFMA implicit-GEMM when the shape is covered, else generic          */
#define PCC_IMPL_GENERIC 1 /* direct convolution, any shape (reference-order fp32 FMA chain)      */
#define PCC_IMPL_MFMA 2    /* force the direct MFMA implicit-GEMM path; PCC_ERR_ARG if not covered */
#define PCC_IMPL_WINOGRAD 3 /* force Winograd F(2x2,3x3)+z on MFMA (Cin = Cout in {16,32,64}, k3 s1, W,H % 16 == 0); AUTO
                              picks it when eligible (env PCC_NO_WINOGRAD=1 disables); 16-channel layers take the split-bf16
                              kernel (three bf16 pieces per fp32 operand, fp32-equivalent; env PCC_NO_SPLIT=1: exact-fp32 MFMA)  */
#define PCC_IMPL_SPLIT 4    /* force the direct k3 stride-1 kernel with split-bf16 operands (Cin = Cout in {32,64}, W % 16 == 0);
                              AUTO picks it for launches that fill the CUs (env PCC_NO_SPLIT_DIRECT=1 / PCC_NO_SPLIT=1 disable)    */

typedef struct {
    int32_t N, D, H, W;    /* input batch and spatial size                                       */
    int32_t Cin, Cout;
    int32_t k;             /* cubic kernel size: 3, 5 or 9 on the fast path, any odd k generic    */
    int32_t stride;        /* 1 or 2                                                              */
    int32_t transposed;    /* 0 = Conv3D, 1 = Conv3DTranspose                                     */
    int32_t flags;         /* PCC_CONV_*                                                          */
    int32_t impl;          /* PCC_IMPL_*                                                          */
    int32_t out_cstride;   /* channel stride of `out` (>= Cout); 0 means Cout.  With out_coffset  */
    int32_t out_coffset;   /* it implements ResidualLayer 'concat' mode (model_transforms.py:38). */
} pcc_conv_desc;

/* Output spatial size for a descriptor (ceil(n/s) forward, n*s transposed). */
int pcc_conv_out_dims(const pcc_conv_desc* d, int32_t* OD, int32_t* OH, int32_t* OW);
/* Returns 1 if the MFMA path covers the descriptor, 0 otherwise. */
int pcc_conv_mfma_supported(const pcc_conv_desc* d);
/* Size in floats of the MFMA-fragment-ordered weight image (0 if the MFMA path does not apply). */
size_t pcc_conv_packed_floats(const pcc_conv_desc* d);
/* HOST-side repack of a Keras-layout kernel into MFMA fragment order (done once at model load,
 * replaces saver.restore's variable placement, src/compress_octree.py:90-92). */
int pcc_conv_pack_weights(const pcc_conv_desc* d, const float* w_keras_host, float* packed_host);
/* Name of the kernel family pcc_conv3d takes for this descriptor on this context (w_packed given), e.g. "conv16_wino_f16s (...)":
 * written NUL-terminated into buf (truncated to cap).  Diagnostic: bench.py prints it beside every layer's time.             */
int pcc_conv_kernel_family(pcc_ctx* ctx, const pcc_conv_desc* d, char* buf, int32_t cap);
/* `w` (device, Keras layout) is used by the generic path, `w_packed` (device, may be NULL) by the
 * MFMA path; `bias`/`residual` may be NULL when the matching flag is clear.  `residual` has the
 * shape of `out` with channel stride Cout. */
int pcc_conv3d(pcc_ctx* ctx, const pcc_conv_desc* d, const float* in, const float* w,
               const float* w_packed, const float* bias, const float* residual, float* out,
               void* stream);

/* ---- batched graph: whole transforms and whole graph phases in ONE call ------------------------------------------
 * The layer stacks of src/model_transforms.py:41-158 (one id per member of its TransformType enum, :161-169) run as a
 * sequence of pcc_conv3d launches enqueued by the library on `stream`; the reference runs them as one Keras
 * `layer(tensor)` call inside sess.run (src/model_types.py:289-293,379-388,405-408).  ResidualLayer mode 'add' only
 * (the mode every config uses); 'concat' stays available through pcc_conv3d's out_cstride/out_coffset.               */
#define PCC_NET_ANALYSIS_V1 0               /* model_transforms.py:41-48   */
#define PCC_NET_SYNTHESIS_V1 1              /* :51-59                      */
#define PCC_NET_ANALYSIS_V2 2               /* :84-95                      */
#define PCC_NET_SYNTHESIS_V2 3              /* :98-109                     */
#define PCC_NET_ANALYSIS_PROGRESSIVE_V2 4   /* :112-123                    */
#define PCC_NET_SYNTHESIS_PROGRESSIVE_V2 5  /* :126-137                    */
#define PCC_NET_HYPER_ANALYSIS 6            /* :140-147                    */
#define PCC_NET_HYPER_SYNTHESIS 7           /* :150-158                    */

/* Number of conv layers of a transform (conv_layers() order = Keras construction order), or <0. */
int32_t pcc_network_num_layers(int32_t transform, int32_t filters);
/* Geometry of layer `layer` (Cin, Cout, k, stride, transposed, flags; N/D/H/W left 0) and its role in a residual block:
 * 0 plain, 1 its output is the block's `tensor1`, 2 `tensor1` is added after its activation (model_transforms.py:30-36). */
int pcc_network_layer(int32_t transform, int32_t filters, int32_t layer, pcc_conv_desc* d, int32_t* residual_role);
/* Weight upload -- replaces saver.restore's variable placement (src/compress_octree.py:90-92).  The blob holds, per layer,
 * the Keras-layout kernel, its MFMA/Winograd fragment image and the bias.  It lives in CALLER-owned device memory of
 * pcc_weights_blob_floats() floats; pcc_weights_pack builds the same image on the host.  kernels[i] / biases[i]: host
 * pointers in conv_layers() order (biases[i] ignored for layers without bias).  Synchronous (model-load time).          */
size_t pcc_weights_blob_floats(int32_t transform, int32_t filters);
int pcc_weights_pack(int32_t transform, int32_t filters, const float* const* kernels, const float* const* biases,
                     float* blob_host);
int pcc_weights_upload(pcc_ctx* ctx, int32_t transform, int32_t filters, const float* const* kernels,
                       const float* const* biases, float* blob_device, void* stream);
/* Activations workspace (caller-owned device memory) for an input of N x D x H x W voxels, and the output size.          */
size_t pcc_network_workspace_bytes(int32_t transform, int32_t filters, int32_t N, int32_t D, int32_t H, int32_t W);
int pcc_network_out_dims(int32_t transform, int32_t filters, int32_t D, int32_t H, int32_t W, int32_t* OD, int32_t* OH,
                         int32_t* OW, int32_t* OC);
/* The plan of a stack of conv layers on an N x D x H x W input: host arithmetic, no context, no device.  It is the one place
 * that decides which tensors the fp16 mode stores as fp16 and which layer records the block maxima of its output;
 * pcc_network_forward runs it, and a caller that chains the layers itself through pcc_conv3d asks for it to get the same bits. */
typedef struct {
    pcc_conv_desc desc;    /* what the layer runs with: its input dims; flags = its own | layer_flags | PCC_CONV_IN16 / OUT16 /
                              RES16 as planned | final_flags (last layer); everything else as given                        */
    int32_t record_amax;   /* 1: the next layer runs a two-piece fp16 kernel ("fp16 x 2" in pcc_conv_kernel_family), which scales
                              each block by the max |x| this layer is asked to record with its output                      */
} pcc_layer_plan;
/* layers[i]: geometry (Cin, Cout, k, stride, transposed), own flags (BIAS / RELU / ADD) and impl of layer i as pcc_network_layer
 * gives them (N, D, H, W ignored); roles[i]: its residual role (ibid.).  numerics: the PCC_NUM_* switches (pcc_ctx_get_numerics).
 * fp16 storage needs layer_flags & PCC_CONV_F16, roles 1, 0, 2 and PCC_IMPL_AUTO on a block's three layers.  plan: n entries;
 * *any_amax (may be NULL): whether any record_amax is set.                                                                  */
int pcc_network_plan(const pcc_conv_desc* layers, const int32_t* roles, int32_t n, int32_t N, int32_t D, int32_t H, int32_t W,
                     int32_t layer_flags, int32_t final_flags, uint32_t numerics, pcc_layer_plan* plan, int32_t* any_amax);
/* y = transform(x).  x: (N,D,H,W,Cin) with Cin = 1 for the analysis transforms, `filters` otherwise; y: NDHWC of
 * pcc_network_out_dims.  layer_flags: 0 or PCC_CONV_F16 (every layer); final_flags: 0 or PCC_CONV_CLIP01 (last layer).
 * Results are bit-identical to the same layers issued one by one through pcc_conv3d (with layer_flags = PCC_CONV_F16 the
 * library additionally keeps the mid-block tensors of the residual blocks in fp16: PCC_CONV_IN16 / OUT16 / RES16 above).  */
int pcc_network_forward(pcc_ctx* ctx, int32_t transform, int32_t filters, const float* blob, const float* x, int32_t N,
                        int32_t D, int32_t H, int32_t W, float* y, void* workspace, size_t workspace_bytes,
                        int32_t layer_flags, int32_t final_flags, void* stream);
/* The same call restricted to one family: PCC_ERR_ARG when `transform` is of another family.               */
int pcc_network_forward_analysis(pcc_ctx* ctx, int32_t transform, int32_t filters, const float* blob, const float* x,
                                 int32_t N, int32_t D, int32_t H, int32_t W, float* y, void* workspace,
                                 size_t workspace_bytes, int32_t layer_flags, int32_t final_flags, void* stream);
int pcc_network_forward_synthesis(pcc_ctx* ctx, int32_t transform, int32_t filters, const float* blob, const float* x,
                                  int32_t N, int32_t D, int32_t H, int32_t W, float* y, void* workspace,
                                  size_t workspace_bytes, int32_t layer_flags, int32_t final_flags, void* stream);
int pcc_network_forward_hyper_a(pcc_ctx* ctx, int32_t transform, int32_t filters, const float* blob, const float* x,
                                int32_t N, int32_t D, int32_t H, int32_t W, float* y, void* workspace,
                                size_t workspace_bytes, int32_t layer_flags, int32_t final_flags, void* stream);
int pcc_network_forward_hyper_s(pcc_ctx* ctx, int32_t transform, int32_t filters, const float* blob, const float* x,
                                int32_t N, int32_t D, int32_t H, int32_t W, float* y, void* workspace,
                                size_t workspace_bytes, int32_t layer_flags, int32_t final_flags, void* stream);

/* Graph phases of CompressionModelV1 / V2 (src/model_types.py:283-309, :371-411): the GPU part of compress() and of
 * decompress() in one call each; the range coder (host) sits between them.  Device pointers, NDHWC, caller-owned.        */
typedef struct {
    int32_t version;          /* 1 = CompressionModelV1 (factorized prior on y), 2 = V2 (hyperprior)                     */
    int32_t filters;
    int32_t analysis, synthesis;            /* PCC_NET_* ids; analysis < 0 for a decoder-only model                      */
    const float* w_analysis;                /* weight blobs (pcc_weights_upload); NULL where the transform is absent     */
    const float* w_synthesis;
    const float* w_hyper_analysis;
    const float* w_hyper_synthesis;
    const float* medians;                   /* (filters,) EntropyBottleneck medians                                      */
    const float* scale_table;               /* (scale_levels,) GaussianConditional scale table (V2)                      */
    int32_t scale_levels;
    int32_t round_mode;                     /* PCC_ROUND_*                                                               */
} pcc_codec_desc;
size_t pcc_codec_workspace_bytes(const pcc_codec_desc* c, int32_t N, int32_t D, int32_t H, int32_t W);
/* compress graph on N blocks: x (N,D,H,W) -> y, [z, zsym, z_hat, sigma, idx,] ysym, y_hat, x_hat (N,D,H,W; final_flags =
 * PCC_CONV_CLIP01 applies np.clip(x_hat,0,1), model_types.py:202).  The V2-only tensors may be NULL for version 1.
 * thr != NULL (fixed-threshold policy, model_opt.py:27-31) also extracts the encoder-side point lists in the same call:
 * thr, xyz, counts, cap, scratch as in pcc_threshold_compact with clip = 1.  symbols_ready: NULL or a hipEvent_t the
 * library records on `stream` as soon as zsym / idx / ysym are final, i.e. BEFORE the synthesis transform is enqueued, so
 * that the device->host copy and the host range coder overlap the synthesis.                                               */
/* io (may be NULL): the symbols on their way to / from the host coder, in the coder's stream order and integer width.
 * Encoder: before `symbols_ready` is recorded the library packs zsym, ysym and idx into the caller's device staging buffers
 * (pcc_symbols_pack), so that ONE device->host copy on the caller's side stream is all that runs beside the synthesis
 * transform (round 2 ran the permutation, the narrowing and a max-reduction there as separate kernels, which compete with the
 * one-workgroup-per-CU convolution kernels for CUs).  Decoder: io->zsym / io->ysym are the INPUT of pcc_codec_decode_hyper /
 * _main (what the host->device copy delivered; the library unpacks it into the int32 `zsym` / `ysym` argument, which is then
 * an output), io->idx receives the packed indexes of pcc_codec_decode_hyper.  Pointers of tensors a call does not touch may be
 * NULL.                                                                                                                    */
typedef struct {
    void* zsym;               /* device, stream order, sym_bytes per element (V2)                                       */
    void* ysym;
    void* idx;                /* device, stream order, idx_bytes per element (V2)                                       */
    int32_t* zsym_tile_max;   /* device int32[pcc_symbols_tiles(N, vox_z, F)]: max|symbol| per packed tile; may be NULL  */
    int32_t* ysym_tile_max;   /* device int32[pcc_symbols_tiles(N, vox_y, F)]                                           */
    int32_t sym_bytes;        /* 2 or 4                                                                                 */
    int32_t idx_bytes;        /* 1 or 4                                                                                 */
    int32_t channels_first;   /* stream order: 1 = (C, D,H,W) per block (the reference's default), 0 = (D,H,W, C)       */
} pcc_symbol_io;
int pcc_codec_encode(pcc_ctx* ctx, const pcc_codec_desc* c, const float* x, int32_t N, int32_t D, int32_t H, int32_t W,
                     float* y, float* z, int32_t* zsym, float* z_hat, float* sigma, int32_t* idx, int32_t* ysym,
                     float* y_hat, float* x_hat, const float* thr, float* xyz, int32_t* counts, int64_t cap,
                     int32_t* scratch, void* workspace, size_t workspace_bytes, int32_t layer_flags, int32_t final_flags,
                     const pcc_symbol_io* sink, void* symbols_ready, void* stream);
/* decompress graph, V2 first phase (model_types.py:403-406): zsym -> z_hat -> sigma -> idx.                               */
int pcc_codec_decode_hyper(pcc_ctx* ctx, const pcc_codec_desc* c, int32_t* zsym, int32_t N, int32_t D, int32_t H,
                           int32_t W, float* z_hat, float* sigma, int32_t* idx, void* workspace, size_t workspace_bytes,
                           int32_t layer_flags, const pcc_symbol_io* io, void* stream);
/* decompress graph, main phase (:305-307 / :407-408): ysym -> y_hat -> x_hat and, when thr != NULL, the unclipped
 * thresholding + compaction of :232-234 (arguments as pcc_threshold_compact).                                              */
int pcc_codec_decode_main(pcc_ctx* ctx, const pcc_codec_desc* c, int32_t* ysym, int32_t N, int32_t D, int32_t H,
                          int32_t W, float* y_hat, float* x_hat, const float* thr, float* xyz, int32_t* counts, int64_t cap,
                          int32_t* scratch, void* workspace, size_t workspace_bytes, int32_t layer_flags,
                          const pcc_symbol_io* io, void* stream);

/* Live kernel timing: HIP events recorded on the launch stream around layer `layer` of transform `transform` in every
 * pcc_network_forward / pcc_codec_* call (transform < 0 switches it off); pcc_profile_read waits for the recorded events,
 * returns their durations in milliseconds (at most `cap`) and clears the list.  The events belong to the context.
 * `layer` = index | (stride << 16): with stride > 1 only every stride-th call of the layer is timed (an event record costs the
 * queue a few microseconds: sampling keeps the measurement from slowing what it measures).                               */
int pcc_profile_select(pcc_ctx* ctx, int32_t transform, int32_t layer);
int pcc_profile_read(pcc_ctx* ctx, float* ms, int32_t cap, int32_t* n);

/* ---- entropy-model element-wise kernels -------------------------------------------------
 * Quantisation of tfc.EntropyBottleneck / tfc.GaussianConditional `_quantize`
 * (call sites src/model_types.py:291,382,386): mode 0 = floor(v + (0.5 - median_c)) [tfc 1.3],
 * mode 1 = round-half-even(v - median_c).  Channel of element i is i % C (channels-last).
 * medians/sym/deq may be NULL.  deq = float(sym) + median.                                      */
#define PCC_ROUND_FLOOR_HALF 0
#define PCC_ROUND_HALF_EVEN 1
int pcc_quantize(pcc_ctx* ctx, const float* v, const float* medians, int32_t* sym, float* deq,
                 size_t n, int32_t C, int32_t mode, void* stream);
/* deq[i] = float(sym[i]) + medians[i % C]  (tfc `_dequantize`, decoder side). */
int pcc_dequantize(pcc_ctx* ctx, const int32_t* sym, const float* medians, float* deq, size_t n,
                   int32_t C, void* stream);
/* Scale -> CDF-table index, src/utils/patch_gaussian_conditional.py:57-58,104-116: sigma is
 * lower-bounded at table[0]; idx = (L-1) - #{j < L-1 : sigma <= table[j]}.  Deterministic. */
int pcc_scale_to_index(pcc_ctx* ctx, const float* sigma, const float* table, int32_t L,
                       int32_t* idx, size_t n, void* stream);

/* ---- symbols / CDF-row indexes between the device tensors and the host coder -------------
 * tfc 1.3 codes each block's tensor flattened in ITS memory order (src/model_types.py:180,254,377: data_format
 * 'channels_first' -> (C, D,H,W), channel-major streams); the device tensors are NDHWC int32.  pcc_symbols_pack writes N
 * blocks of (vox, C) int32 in stream order as dst_bytes-wide integers (1: uint8, 2: int16, 4: int32; values are truncated --
 * tile_max, when given, receives max|value| of every 64 x 64 tile (pcc_symbols_tiles entries) so that the host can tell
 * whether the narrow type was enough); pcc_symbols_unpack is the inverse (decoder side).  HBM-bound byte work.            */
size_t pcc_symbols_tiles(int32_t N, int64_t vox, int32_t C);
int pcc_symbols_pack(pcc_ctx* ctx, const int32_t* src, int32_t N, int64_t vox, int32_t C, int32_t channels_first,
                     void* dst, int32_t dst_bytes, int32_t* tile_max, void* stream);
int pcc_symbols_unpack(pcc_ctx* ctx, const void* src, int32_t src_bytes, int32_t N, int64_t vox, int32_t C,
                       int32_t channels_first, int32_t* dst, void* stream);
/* The same two kernels with the element-wise step before / after them folded in: what pcc_codec_encode / _decode_hyper /
 * _decode_main launch (one launch where the stand-alone calls need two).  Each gives, bit for bit, what the stand-alone call
 * followed by pcc_symbols_pack (or pcc_symbols_unpack followed by pcc_dequantize) gives.  N blocks of (vox, C), NDHWC on the
 * device side, dst / src in stream order as above.
 * pcc_quantize_pack: pcc_quantize (v, medians (C) or NULL, mode -> sym int32, deq float32 or NULL; both NDHWC) and the packed,
 *   truncated copy of sym in dst (dst_bytes 1, 2 or 4); tile_max (pcc_symbols_tiles entries, or NULL) receives max|sym| of every
 *   64 x 64 tile, entry (n * ceil(vox/64) + voxel tile) * ceil(C/64) + channel tile.
 * pcc_index_pack: pcc_scale_to_index (sigma, table of L in [1,256] entries -> idx int32 NDHWC) and the packed copy of idx in
 *   dst.  An ascending table (what the reference builds) is searched in log2(L) steps, any other table is counted literally:
 *   the result is the formula of pcc_scale_to_index either way.
 * pcc_unpack_dequantize: pcc_symbols_unpack (src, src_bytes -> sym int32 NDHWC) and deq = float(sym) + medians[c]
 *   (medians (C) or NULL; deq must not be NULL).                                                                            */
int pcc_quantize_pack(pcc_ctx* ctx, const float* v, const float* medians, int32_t* sym, float* deq, int32_t N, int64_t vox,
                      int32_t C, int32_t mode, int32_t channels_first, void* dst, int32_t dst_bytes, int32_t* tile_max,
                      void* stream);
int pcc_index_pack(pcc_ctx* ctx, const float* sigma, const float* table, int32_t L, int32_t* idx, int32_t N, int64_t vox,
                   int32_t C, int32_t channels_first, void* dst, int32_t dst_bytes, void* stream);
int pcc_unpack_dequantize(pcc_ctx* ctx, const void* src, int32_t src_bytes, int32_t N, int64_t vox, int32_t C,
                          int32_t channels_first, int32_t* sym, const float* medians, float* deq, void* stream);

/* ---- latent step: variable rate from one checkpoint ---------------------------------------------------
 * The ladder: step(q) = (8 + (q & 7)) * 2^((q >> 3) - 5) for q in [0, 63] -- 0.25 ... 60, step(16) = 1, every value exact in
 * fp32.  `q` below is a DEVICE array with one ladder index per block (N entries, each <= 63).
 * The three stepped kernels are, bit for bit, their un-stepped twins above applied to a pre-divided input, respectively followed
 * by one multiply; the quotient is the correctly rounded fp32 division (never a reciprocal multiply), and multiply and add are
 * rounded separately (never fused).  Subnormal quotients are outside the contract.
 * pcc_quantize_step_pack: t = v / step(q[n]); sym from t under `mode` and the medians rule of pcc_quantize;
 *   deq = float(sym) * step(q[n]) + medians[c] (medians NULL: + 0); packed copy and tile_max as pcc_quantize_pack.
 * pcc_index_pack_step: s = sigma / step(q[n]), then the formula of pcc_scale_to_index on s (its lower bound at table[0] included).
 * pcc_unpack_dequantize_step: unpack, then deq = float(sym) * step(q[n]) + medians[c].
 * dst of the two pack kernels may be NULL: then no packed copy is written (a coder that reads the int32 tensors on the device).
 * pcc_rate_ladder: bits16[n * J + j] = the exact size of block n's y string under step(steps[j]) in units of 2^-16 bit:
 *   every element adds cost16[row * cost_stride + bin], its symbol as pcc_quantize_step_pack (no medians) and its row as
 *   pcc_index_pack_step compute them; v = sym - offset[row], m = cdf_size[row] - 2; 0 <= v < m: bin v; otherwise bin m plus
 *   65536 * overflow_width * (widths / omax + 1 + widths) for the escape digits of the host range coder (overflow = -2v - 1
 *   for v < 0, else 2 (v - m); widths = its overflow_width-bit digits; omax = 2^overflow_width - 1).  y, sigma: N blocks of
 *   (vox, C) fp32 on the device; table: L scale entries (device); steps: J in [1, 64] ladder indexes on the HOST; cost16
 *   (L rows of cost_stride uint32), offset, cdf_size (L each): device.  groups_per_block: workgroups per block (0: one per
 *   2048 elements); the integer sums do not depend on it.  bits16 is zeroed and filled on `stream`.                        */
int pcc_quantize_step_pack(pcc_ctx* ctx, const float* v, const float* medians, int32_t* sym, float* deq, int32_t N, int64_t vox,
                           int32_t C, int32_t mode, int32_t channels_first, void* dst, int32_t dst_bytes, int32_t* tile_max,
                           const uint8_t* q, void* stream);
int pcc_index_pack_step(pcc_ctx* ctx, const float* sigma, const float* table, int32_t L, int32_t* idx, int32_t N, int64_t vox,
                        int32_t C, int32_t channels_first, void* dst, int32_t dst_bytes, const uint8_t* q, void* stream);
int pcc_unpack_dequantize_step(pcc_ctx* ctx, const void* src, int32_t src_bytes, int32_t N, int64_t vox, int32_t C,
                               int32_t channels_first, int32_t* sym, const float* medians, float* deq, const uint8_t* q,
                               void* stream);
int pcc_rate_ladder(pcc_ctx* ctx, const float* y, const float* sigma, int32_t N, int64_t vox, int32_t C, const float* table,
                    int32_t L, int32_t mode, const uint8_t* steps, int32_t J, const uint32_t* cost16, int32_t cost_stride,
                    const int32_t* offset, const int32_t* cdf_size, int32_t overflow_width, int32_t groups_per_block,
                    int64_t* bits16, void* stream);

/* ---- occupancy thresholding + order-preserving compaction ------------------------------
 * Replaces `np.argwhere(x_hat > thresholds[t]).astype(float32)` (src/model_types.py:209,233-234,
 * src/model_opt.py:12,29).  x: B blocks of D*H*W float32; thr[b] is the float32 threshold of
 * block b (device array); clip!=0 applies np.clip(x,0,1) first (encoder, model_types.py:202).
 * xyz: B * cap * 3 float32, block b's points at xyz + b*cap*3 in C order (x slowest, z fastest),
 * counts[b] = number of points of block b (may exceed cap: then only the first cap are written;
 * rows from min(counts[b], cap) on are left untouched).  thr[b] may be any float: a negative one
 * or -inf takes voxels at or below 0, +inf and NaN take none.  A NaN voxel is never a point,
 * clipped or not (np.clip keeps NaN, and NaN > thr is false).  x needs float alignment only; the
 * 16-byte loads are used when D*H*W % 4 == 0 and x is 16-byte aligned.  B <= 65535.
 * `scratch` must hold pcc_threshold_scratch_ints(B, D, H, W) int32 (the fused occupancy-bit path
 * of the codec graphs shares it, so this is more than the B * ceil(D*H*W/4096) chunk counts).
 * Bit-exact with the numpy expression.                                                          */
int pcc_threshold_compact(pcc_ctx* ctx, const float* x, int32_t B, int32_t D, int32_t H,
                          int32_t W, const float* thr, int32_t clip, float* xyz, int32_t* counts,
                          int64_t cap, int32_t* scratch, void* stream);
size_t pcc_threshold_scratch_ints(int32_t B, int32_t D, int32_t H, int32_t W);

/* ---- top-k selection: count-matched thresholding ------------------------------------------------
 * Block b keeps the k[b] voxels with the highest score instead of those above a threshold.  x: B blocks of n = D*H*W float32, block b at
 * x + b * x_stride (elements, >= n); k: device array of B int32, a negative entry counts as 0.  Per block:
 *   key(i) = 0 unless x[i] > 0 (NaN, -0, +0, negatives), else the 32 raw bits of x[i]; nothing is clipped;
 *   P = #{i : key(i) > 0}, k_eff = clamp(k, 0, P): a voxel with a non-positive score is never emitted;
 *   the k_eff voxels that come first by (key descending, i ascending) are taken: all above the k_eff-th largest key T and, of those
 *   equal to T, the ones with the lowest i.
 * xyz, counts, cap as in pcc_threshold_compact: the taken voxels in ascending i as float32 rows (x slowest), counts[b] = k_eff, which may
 * exceed cap: then only the first cap rows are written.  The result is a function of the block's scores and k alone (integer
 * histograms: no dependence on B, the stride, the position in the batch or the launch geometry).  workspace: device memory of
 * pcc_topk_workspace_bytes(B, n) bytes (0 for an n above 2^28).  B = 0 or n = 0: nothing is launched, counts = 0.  PCC_ERR_ARG: a NULL
 * pointer, a workspace that is too small, n > 2^28, B > 65535.                                                                        */
size_t pcc_topk_workspace_bytes(int32_t B, int64_t n);
int pcc_topk_compact(pcc_ctx* ctx, const float* x, int64_t x_stride, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* k,
                     float* xyz, int32_t* counts, int64_t cap, void* workspace, size_t workspace_bytes, void* stream);

/* sparse_to_dense (src/model_types.py:108-114): scatter ones.  pts: int32 (npts,3) local block
 * coordinates, block_of[i] = destination block; dense must be zero-filled B*D*H*W float32.       */
int pcc_voxelize(pcc_ctx* ctx, const int32_t* pts, const int32_t* block_of, int64_t npts,
                 int32_t B, int32_t D, int32_t H, int32_t W, float* dense, void* stream);

/* ---- adaptive threshold search statistics (src/model_opt.py:21-77, src/utils/pc_metric.py:76-138) ------------
 * Exact D1 sums for EVERY threshold of EVERY block in one call (the reference builds up to 255 KD-trees per block).
 * With level k(v) = #{t : x_hat[v] > thr[t]} the decoded set at threshold t is B_t = {v : k(v) > t}.  Outputs
 * (device, (B,256) uint64 unless noted, zero-filled by the call):
 *   s_ab[b][t]  = sum over the original points a of block b of min_{v in B_t} |a - v|^2        (d1_sum_AB)
 *   hsum[b][k]  = sum over voxels of level k of min_a |v - a|^2;  d1_sum_BA(t) = sum_{k>t} hsum[b][k]
 *   hcnt[b][k]  = number of voxels of level k;                    |B_t|        = sum_{k>t} hcnt[b][k]
 *   tcount[b]   (int32, (B,)) = number of thresholds whose decoded set is non-empty = the largest level of the block.
 * All sums are integers, so the host reproduces the reference's float64 metrics bit for bit.
 * Levels are held as uint8, so the thresholds computed are t < min(tcount[b], 255).  tcount[b] == 256 (nthr == 256 and a voxel above
 * thr[255]: clip == 0 with x_hat above the last threshold, or thresholds that end below 1) reports a level the engine cannot hold:
 * the voxel is counted at level 255 (hsum / hcnt[b][255]), threshold 255 is not computed, s_ab[b][255] and -- in the two D2
 * calls below -- d2_ab / d2_ba[b][255] stay zero and are NOT the statistics of B_255; everything at t < 255, and every other block, is
 * as defined above.  The Python wrappers raise PccError naming such blocks.  With clip != 0 and thresholds up to 1.0 (the
 * encoder's) no float32, infinities and NaN included, has a level above 255.
 * pts: (npts,3) int32 block-local coordinates, block_of: (npts,) int32; thr: nthr <= 256 increasing float32
 * thresholds (device).  clip != 0 applies np.clip(x_hat,0,1) first (the encoder does, model_types.py:202).
 * Blocks up to 128^3.  `workspace`: pcc_d1_search_workspace_bytes(B,D,H,W) bytes of device memory.             */
size_t pcc_d1_search_workspace_bytes(int32_t B, int32_t D, int32_t H, int32_t W);
int pcc_d1_threshold_stats(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W,
                           const float* thr, int32_t nthr, int32_t clip, const int32_t* pts,
                           const int32_t* block_of, int64_t npts, void* workspace, uint64_t* s_ab,
                           uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, void* stream);

/* The same search with the point-to-plane statistics (D2; src/utils/pc_metric.py:109-131: the reference's experiment optimises
 * d1_mse AND d2_mse, src/ev_experiment.yml:47).  D2 needs WHICH point is nearest; where several are equally near the reference
 * takes whatever scipy's KD-tree returns (pc_metric.py:114) -- here the rule is fixed: the candidate with the lowest (x, y, z)
 * in lexicographic order (= lowest row-major voxel index).  A decoded point takes the mean normal of the original points that
 * chose it, summed in ascending point order (pc_metric.py:16-18).  Additional arguments:
 *   normals     : (npts,3) float32, normal of original point i (device)
 *   block_start : (B+1,) int32 offsets of the blocks' points inside pts (points are grouped by block, ascending) (device)
 *   workspace2  : pcc_d12_search_workspace_bytes(B,D,H,W,npts) bytes of device memory (beside `workspace` of the D1 call)
 *   d2_ab, d2_ba: (B,256) float64 (device): d2_sum_AB / d2_sum_BA of threshold t, valid for t < tcount[b]
 * No floating-point atomics: every sum has a fixed order, results are bit-reproducible.                                    */
size_t pcc_d12_search_workspace_bytes(int32_t B, int32_t D, int32_t H, int32_t W, int64_t npts);
int pcc_d12_threshold_stats(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const float* thr,
                            int32_t nthr, int32_t clip, const int32_t* pts, const int32_t* block_of, const int32_t* block_start,
                            int64_t npts, const float* normals, void* workspace, void* workspace2, uint64_t* s_ab, uint64_t* hsum,
                            uint64_t* hcnt, int32_t* tcount, double* d2_ab, double* d2_ba, void* stream);

/* ---- rank levels: the same search over candidate point COUNTS (count-matched thresholding) ------------------------
 * The top-k sets of a block are a nested family like its threshold level sets; here the family is indexed by a row of candidate counts
 * instead of score thresholds.  A block has n = D*H*W float32 scores and a row c[0] >= c[1] >= ... >= c[J-1] of int32, 1 <= J <= 255,
 * a negative entry counts as 0.  Rule (normative):
 *   key(i) and P are those of pcc_topk_compact: the 32 raw bits of x[i] where x[i] > 0, else 0 (NaN, -0, +0, negatives); nothing is
 *   clipped;  rank(i) = the 0-based position of voxel i among the P voxels with key > 0 in the order (key descending, i ascending);
 *   lev(i) = 0 where key(i) = 0, else #{j : rank(i) < c[j]};   tcount = max_i lev(i) = #{j : c[j] >= 1} when P >= 1, else 0.
 * Then {i : lev(i) > j} is exactly the voxel set pcc_topk_compact emits for k = c[j], also for c[j] > P; equal entries give equal sets.
 * For a row that is not non-increasing the formula still is the output (the row is walked whole) and no access leaves the buffers; it
 * just is no nested top-k family.  x: block b at x + b * x_stride (elements, >= n); counts: (B,J) int32 (device); lev: B*n uint8, block b
 * at lev + b*n; tcount: (B,) int32; both written whole by the call.  The result of a block is a function of its scores and its row alone
 * (no dependence on B, the stride, the position in the batch or the launch geometry); no score-valued atomics; every store into lev is
 * under the test index < n.  workspace: pcc_rank_levels_workspace_bytes(B, n) bytes of device memory, 0 for a shape outside the contract.
 * B = 0: nothing is done; n = 0: tcount = 0.  PCC_ERR_ARG: a NULL pointer, n > 2^28, B > 65535, B*n >= 2^31 (one sort of all voxels of
 * the call), J outside [1, 255], a workspace that is too small.                                                                         */
size_t pcc_rank_levels_workspace_bytes(int32_t B, int64_t n);
int pcc_rank_levels(pcc_ctx* ctx, const float* x, int64_t x_stride, int32_t B, int64_t n, const int32_t* counts, int32_t J, uint8_t* lev,
                    int32_t* tcount, void* workspace, size_t workspace_bytes, void* stream);

/* pcc_d1_threshold_stats / pcc_d12_threshold_stats with the level grid of pcc_rank_levels in place of the threshold levels: entry [b][j]
 * of every output is the statistic of the top-counts[b][j] set of block b (sum_{k>j} hcnt[b][k] = min(counts[b][j], P_b)), valid for
 * j < tcount[b].  `thr, nthr, clip` are replaced by `counts` ((B,J) int32, device) and J in [1, 255]; rank_workspace:
 * pcc_rank_levels_workspace_bytes(B, D*H*W) bytes beside the other workspaces.  Everything behind the level grid is the code of the
 * threshold entries, so equal level grids give equal bits.  A level of 256 cannot occur.                                                */
int pcc_d1_count_stats(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* counts, int32_t J,
                       const int32_t* pts, const int32_t* block_of, int64_t npts, void* workspace, void* rank_workspace,
                       size_t rank_workspace_bytes, uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, void* stream);
int pcc_d12_count_stats(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* counts, int32_t J,
                        const int32_t* pts, const int32_t* block_of, const int32_t* block_start, int64_t npts, const float* normals,
                        void* workspace, void* workspace2, void* rank_workspace, size_t rank_workspace_bytes, uint64_t* s_ab,
                        uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, double* d2_ab, double* d2_ba, void* stream);

/* ---- Hausdorff terms of the search -------------------------------------------------------------------------------
 * The four entries above with the per-point MAXIMA beside their sums, through the same kernels: every output they share with the plain
 * entry is the same bits, and the plain entries do no work for the maxima.  With A the original points of block b and B_t the decoded set
 * of candidate t (threshold t, or the top-counts[b][t] set):
 *   h1_ab[b][t]  (uint32)  = max_{a in A} min_{v in B_t} |a - v|^2                       (d1_hausdorff_AB; <= 3 * 127^2)
 *   h1_max[b][k] (uint32)  = max over the voxels v of level k of min_{a in A} |v - a|^2;  d1_hausdorff_BA(t) = max_{k>t} h1_max[b][k]
 *   h2_ab[b][t]  (float64) = the largest of the per-point plane terms whose sum is d2_ab[b][t]            (d2_hausdorff_AB)
 *   h2_max[b][k] (float64) = the largest of the per-voxel plane terms of d2_ba over the voxels of level k;
 *                            d2_hausdorff_BA(t) = max_{k>t} h2_max[b][k]
 * under the tie rule of pcc_d12_threshold_stats (lowest (x, y, z)).  All four are (B,256), device, caller-provided beside the workspaces
 * (whose sizes do not change) and zero-filled by the call on its stream.  Live levels as above: only t < min(tcount[b], 255) are
 * computed, h1_ab / h2_ab[b][t] stay zero elsewhere, a voxel of level 256 is held at level 255.  D1 values are integers and a maximum has
 * no order: h1_* are exact; h2_* are maxima over finite non-negative doubles (integer atomic maxima on their bit patterns, or a tree),
 * hence bit-reproducible like the sums.  There is no tie-averaged (_ties) form.                                                      */
int pcc_d1_threshold_stats_hausdorff(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W,
                                     const float* thr, int32_t nthr, int32_t clip, const int32_t* pts,
                                     const int32_t* block_of, int64_t npts, void* workspace, uint64_t* s_ab,
                                     uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, uint32_t* h1_ab, uint32_t* h1_max, void* stream);
int pcc_d12_threshold_stats_hausdorff(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const float* thr,
                                      int32_t nthr, int32_t clip, const int32_t* pts, const int32_t* block_of, const int32_t* block_start,
                                      int64_t npts, const float* normals, void* workspace, void* workspace2, uint64_t* s_ab, uint64_t* hsum,
                                      uint64_t* hcnt, int32_t* tcount, double* d2_ab, double* d2_ba, uint32_t* h1_ab, uint32_t* h1_max,
                                      double* h2_ab, double* h2_max, void* stream);
int pcc_d1_count_stats_hausdorff(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* counts,
                                 int32_t J, const int32_t* pts, const int32_t* block_of, int64_t npts, void* workspace,
                                 void* rank_workspace, size_t rank_workspace_bytes, uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt,
                                 int32_t* tcount, uint32_t* h1_ab, uint32_t* h1_max, void* stream);
int pcc_d12_count_stats_hausdorff(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const int32_t* counts,
                                  int32_t J, const int32_t* pts, const int32_t* block_of, const int32_t* block_start, int64_t npts,
                                  const float* normals, void* workspace, void* workspace2, void* rank_workspace,
                                  size_t rank_workspace_bytes, uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt, int32_t* tcount,
                                  double* d2_ab, double* d2_ba, uint32_t* h1_ab, uint32_t* h1_max, double* h2_ab, double* h2_max,
                                  void* stream);

/* The same search under the tie-averaged D2 definition (DESIGN.md "Tie-averaged D2", applied per block and threshold with A = the
 * block's rows and B = B_t): T_B(a) = ALL voxels of B_t at the smallest squared distance from row a, T_A(v) = ALL rows at the
 * smallest squared distance from voxel v (rows that share a voxel are separate members).  A voxel b takes the unweighted float64 mean
 * of normals[a] over {a : b in T_B(a)}, summed in increasing row;  d2_ab[b][t] = sum_a mean_{v in T_B(a)} e(a - v, n_B(v)),
 * d2_ba[b][t] = sum_{v in B_t} mean_{a in T_A(v)} e(v - a, normals[a]),  e(g, n) = ((g.x n.x + g.y n.y) + g.z n.z)^2 in float64
 * without contraction.  Nothing depends on which of several equidistant points is met first, so a host restatement gives the same
 * sums up to float64 rounding.  The D1 outputs (s_ab, hsum, hcnt, tcount) are those of pcc_d1_threshold_stats.  Differences to
 * pcc_d12_threshold_stats:
 *   normals     : (npts,3) float64 (device)
 *   max_pairs   : capacity of the pair list of ONE chunk of thresholds, in [1, 2^31): the number of (row, tied voxel) pairs is data
 *                 dependent.  pcc_d12_search_ties_chunk(B,D,H,W) thresholds are processed at a time.
 *   status      : int64[2] (device), written by the call: [0] = the largest pair count of a chunk (the capacity that suffices),
 *                 [1] = 1 when a chunk needed more than max_pairs.  Then no pair was written past the capacity, EVERY d2_ab / d2_ba
 *                 entry is NaN and the D1 outputs are valid: call again with max_pairs >= status[0].  Never a silent truncation.
 *   workspace2  : pcc_d12_search_ties_workspace_bytes(B,D,H,W,npts,max_pairs) bytes (0 = bad arguments), beside `workspace`
 * No floating-point atomics, every sum in a fixed order: two calls give the same bits.                                      */
int32_t pcc_d12_search_ties_chunk(int32_t B, int32_t D, int32_t H, int32_t W);
size_t pcc_d12_search_ties_workspace_bytes(int32_t B, int32_t D, int32_t H, int32_t W, int64_t npts, int64_t max_pairs);
int pcc_d12_threshold_stats_ties(pcc_ctx* ctx, const float* x_hat, int32_t B, int32_t D, int32_t H, int32_t W, const float* thr,
                                 int32_t nthr, int32_t clip, const int32_t* pts, const int32_t* block_of, const int32_t* block_start,
                                 int64_t npts, const double* normals, int64_t max_pairs, int64_t* status, void* workspace,
                                 void* workspace2, uint64_t* s_ab, uint64_t* hsum, uint64_t* hcnt, int32_t* tcount, double* d2_ab,
                                 double* d2_ba, void* stream);

/* ---- point normals (new: the reference reads them from a `--input_normals` file, src/compress_octree.py:142-144) ----------------
 * The normals the D2 metrics need (pcc_d12_threshold_stats, utils/pc_metric.py) estimated from the cloud itself.  Definition:
 *   - pts: (npts,3) int32, every coordinate in [0, 2^21) (the codec's voxelised clouds; other values give unspecified normals,
 *     never an access outside the buffers); duplicates allowed; 1 <= npts < 2^31, 3 <= k <= 64;
 *   - neighbourhood of point i: the k_eff = min(k, npts) points j with the smallest (|p_j - p_i|^2, j), exact integers,
 *     lexicographic (i itself is a candidate like any other);
 *   - M = k_eff * sum q q^T - (sum q)(sum q)^T over the neighbours, q = p_j - p_i, exact in int64;
 *   - normal = unit eigenvector of the smallest eigenvalue of M, solved in double (cyclic Jacobi, fixed sweep count), stored
 *     as float32; M == 0 (all neighbours coincide) gives exactly (0, 0, 1);
 *   - otherwise the sign makes n . (p_i - o) >= 0, o = viewpoint or (viewpoint NULL) the centroid = exact int64 sums / npts;
 *     a product of exactly 0 makes the first non-zero component of n positive.
 * Arguments (device memory, on `stream`): viewpoint 3 doubles or NULL; normals (npts,3) float32; knn NULL or (npts,k) int32:
 * row i = the neighbours of point i in the order above, columns >= k_eff hold -1; workspace: pcc_normals_workspace_bytes(npts,k)
 * bytes.  No host synchronisation, no floating-point atomics: results are bit-reproducible.  pcc_normals_workspace_bytes
 * returns 0 for an npts outside [1, 2^31).                                                                                     */
size_t pcc_normals_workspace_bytes(int64_t npts, int32_t k);
int pcc_estimate_normals(pcc_ctx* ctx, const int32_t* pts, int64_t npts, int32_t k, const double* viewpoint, float* normals,
                         int32_t* knn, void* workspace, void* stream);

/* ---- cloud metrics (new: the whole-cloud D1 / D2 of src/utils/pc_metric.py:76-138 and pc_error's --hausdorff terms) -----------
 * Nearest neighbours across two voxelised clouds and the distortion tally of utils/pc_metric.pair_tally on the GPU.  Definition:
 *   - points: (n,3) int32, every coordinate in [0, 2^21) (other values give unspecified results, never an access outside the
 *     buffers); duplicates allowed; 1 <= n < 2^31;
 *   - nearest indexed point of a query q: the row j with the smallest (|p_j - q|^2, j), exact integers, lexicographic -- ties go
 *     to the LOWEST row (the point-normals rule at k = 1; scipy's cKDTree may pick another of several equidistant points);
 *   - tally (A = original, B = decoded, to_b[i] / to_a[j] the nearest rows across): float64[9] = N_B, D1_AB, D1_BA, D2_AB, D2_BA,
 *     H1_AB, H1_BA, H2_AB, H2_BA.  D1_* = sums of the squared distances, exact in 128-bit integers and rounded once; H1_* = their
 *     maxima.  With a_normals ((na,3) float64, NULL: the D2 / H2 slots are 0): the normal of decoded point j is the mean of
 *     a_normals[i] over {i : to_b[i] == j}, summed in float64 in increasing i and divided by the count, or a_normals[to_a[j]] when
 *     that set is empty (utils/pc_metric.transfer_normals); per point, v = ((g.x*n.x + g.y*n.y) + g.z*n.z)^2 in float64, every
 *     operation rounded (no contraction), g = a_i - b_{to_b[i]} with the decoded point's normal (A->B) or g = b_j - a_{to_a[j]}
 *     with a_normals[to_a[j]] (B->A); D2_* = sums of v in a fixed order that depends on the sizes only, H2_* = maxima of v.
 * Index: pcc_cloud_index_bytes(n) bytes of device memory, written by pcc_cloud_index_build; it keeps a copy of the points and
 * stays valid (and reusable by any number of queries) while the buffer lives.  pcc_cloud_nearest writes nn[i] (int32) and
 * sqdist[i] (int64) for each of the nq query points (either output may be NULL).  pcc_cloud_distortion takes both indices (with
 * their sizes), writes the 9 slots to `tally` (device) and, when non-NULL, to_b (na int32) and to_a (nb int32); workspace:
 * pcc_cloud_distortion_workspace_bytes(na, nb) bytes.  No host synchronisation; floating-point values are summed in a fixed
 * order, so the same inputs give the same bits on every call.  The *_bytes functions return 0 for a size outside [1, 2^31).   */
size_t pcc_cloud_index_bytes(int64_t npts);
int pcc_cloud_index_build(pcc_ctx* ctx, const int32_t* pts, int64_t npts, void* index, void* stream);
int pcc_cloud_nearest(pcc_ctx* ctx, const void* index, int64_t npts, const int32_t* queries, int64_t nq, int32_t* nn, int64_t* sqdist,
                      void* stream);
size_t pcc_cloud_distortion_workspace_bytes(int64_t na, int64_t nb);
int pcc_cloud_distortion(pcc_ctx* ctx, const void* index_a, int64_t na, const void* index_b, int64_t nb, const double* a_normals,
                         double* tally, int32_t* to_b, int32_t* to_a, void* workspace, void* stream);

/* Tie-averaged D2 (new; DESIGN.md "Tie-averaged D2"): pcc_cloud_distortion with a rule for equidistant nearest points.
 * tie_mode PCC_TIES_PICK is pcc_cloud_distortion itself (same kernels, same bits).  PCC_TIES_MEAN, with T_B(a) = ALL rows of B at
 * the smallest squared distance from original point a and T_A(b) the same the other way:
 *   - normal of decoded point b: the unweighted mean of a_normals[a] over votes(b) = {a : b in T_B(a)}, summed in float64 in
 *     increasing a and divided by the count; with no votes, the mean of a_normals[a] over T_A(b);
 *   - per-point terms: t(a) = mean over b in T_B(a) of e(a - b, normal of b), t(b) = mean over a in T_A(b) of e(b - a, a_normals[a]),
 *     e(g, n) = ((g.x*n.x + g.y*n.y) + g.z*n.z)^2 in float64 without contraction; sums inside one tie set run in the index's
 *     visiting order, so the result depends on the row order of either cloud by float64 rounding only;
 *   - D2_* = sums of the terms (the fixed order of pcc_cloud_distortion), H2_* = their maxima; the D1 / H1 slots, to_b and to_a
 *     (the LOWEST tied row) are pcc_cloud_distortion's.  Without a_normals the call is pcc_cloud_distortion.
 * The (b, a) pairs of the votes are materialised: their number, the sum of |T_B(a)| over a, is data-dependent, and the caller
 * states a capacity max_pairs in [1, 2^31) that sizes the workspace.  status (device, int64[2]) receives that number and 1 if it
 * exceeded max_pairs: then no pair was written, the D2 / H2 slots are NaN (D1 / H1 stay valid) and a call with max_pairs >=
 * status[0] succeeds.  Nothing is read back by the call itself: the caller reads status with the tally.  workspace:
 * pcc_cloud_distortion_ties_workspace_bytes(na, nb, tie_mode, max_pairs) bytes (0 for a size or mode outside the contract).    */
#define PCC_TIES_PICK 0
#define PCC_TIES_MEAN 1
size_t pcc_cloud_distortion_ties_workspace_bytes(int64_t na, int64_t nb, int32_t tie_mode, int64_t max_pairs);
int pcc_cloud_distortion_ties(pcc_ctx* ctx, const void* index_a, int64_t na, const void* index_b, int64_t nb, const double* a_normals,
                              int32_t tie_mode, int64_t max_pairs, double* tally, int64_t* status, int32_t* to_b, int32_t* to_a,
                              void* workspace, void* stream);

/* ---- cloud colours (new: the colour step of the reference's evaluation, src/map_color.py, and pc_error's colour terms) ---------
 * Colour transfer and colour distortion across two voxelised clouds on the indices of "cloud metrics" (same point contract).
 * Colours: (n,3) uint8 R, G, B in row order, device memory.  Definition:
 *   - the indexed points of a query q in order: rows j sorted by (|p_j - q|^2, j), exact integers, lexicographic;
 *   - pcc_cloud_map_colors writes, for each query row i, out_colours[i] = colours of the rank-th point of that order and, when
 *     rows is non-NULL, rows[i] = its row (int32).  rank 1 is pcc_cloud_nearest's row; rank 2 is src/map_color.py (the second of a
 *     k = 2 KD-tree query); rank 2 needs npts >= 2.  The queries are given as their own index (pcc_cloud_index_build over the nq
 *     query points): they are answered in its Morton order;
 *   - colour distortion of A (original) and B (decoded): for each point q of A, over ALL points of B at the smallest squared
 *     distance, m = (exact integer colour sums) / count and d = c_q - m in float64; then eY = (0.2126 dR + 0.7152 dG) + 0.0722 dB,
 *     eU = (-0.1146 dR - 0.3854 dG) + 0.5 dB, eV = (0.5 dR - 0.4542 dG) - 0.0458 dB (BT.709), every operation rounded (no
 *     contraction).  tally (device) = float64[6]: the sums of eY^2, eU^2, eV^2 over A (A->B), then the same over B against A
 *     (B->A), summed in a fixed order that depends on the sizes only: the same inputs give the same bits on every call.  Averaging
 *     over the equidistant set makes the tally independent of the row order of either cloud.  workspace:
 *     pcc_cloud_color_workspace_bytes(na, nb) bytes (0 for a size outside [1, 2^31)).  No host synchronisation.          */
int pcc_cloud_map_colors(pcc_ctx* ctx, const void* index, int64_t npts, const uint8_t* colours, const void* query_index, int64_t nq,
                         int32_t rank, uint8_t* out_colours, int32_t* rows, void* stream);
size_t pcc_cloud_color_workspace_bytes(int64_t na, int64_t nb);
int pcc_cloud_color_distortion(pcc_ctx* ctx, const void* index_a, int64_t na, const uint8_t* a_colours, const void* index_b, int64_t nb,
                               const uint8_t* b_colours, double* tally, void* workspace, void* stream);
/* Colour transfer (new; a simplified MPEG-style recolouring, NOT TMC13-conformant): colours for B that make the A->B sums above
 * small (the least-squares ones where every row of A has a single nearest row of B, up to the final rounding).  Every row a of A votes for ALL rows of B at the smallest squared distance from a; row b gathers the exact
 * integer sums S_b[R,G,B] of its voters' colours and their number V_b.  A row with V_b = 0 takes S_b and n from its own tie set in
 * A (all rows of A at the smallest squared distance from b) instead.  out_colours[b][c] = (2 S_b[c] + n) / (2 n) in integer
 * division, n = V_b or the size of that tie set: the mean rounded half up, no floating point.  votes (int32[nb], may be NULL) =
 * V_b, 0 for a row that fell back.  The sums are 64-bit and the counts 32-bit integer atomics: exact for every na < 2^31 and the
 * same bits whatever the order of the votes, the row order of A, or (row for row) of B; duplicate rows of B get the same colour.
 * B is given as its own index (pcc_cloud_index_build over its nb points).  workspace: pcc_cloud_transfer_workspace_bytes(na, nb)
 * bytes (0 for a size outside [1, 2^31)), zeroed by the call on the stream.  No host synchronisation.                          */
size_t pcc_cloud_transfer_workspace_bytes(int64_t na, int64_t nb);
int pcc_cloud_transfer_colors(pcc_ctx* ctx, const void* index_a, int64_t na, const uint8_t* a_colours, const void* index_b, int64_t nb,
                              uint8_t* out_colours, int32_t* votes, void* workspace, void* stream);

/* ---- mesh sampling (new: the reference's dataset step src/ds_mesh_to_pc.py, pyntcloud's mesh_random sampler + voxelisation) -----
 * A triangle mesh to a voxelised point cloud, reproducible from a seed.  Inputs (device): verts (nverts,3) float64, tris (ntris,3)
 * int32; n samples; seed; grid size vg.  Definition (restated in numpy by utils/mesh_sampling.py, which returns the same bits):
 *   1. area_i = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz), c = (v2 - v1) x (v3 - v1) (cx = e1y e2z - e1z e2y, ...), float64, every
 *      operation rounded, no contraction;
 *   2. w_i = floor(ldexp(area_i / A_max, 32)) (uint64), C = their inclusive prefix sums, W = C[ntris-1] < 2^63 (exact: any scan
 *      order gives the same C).  A triangle below 2^-32 of the largest one is never picked;
 *   3. sample s takes the outputs r0..r3 of Philox4x64-10 with counter (s,0,0,0) and key (seed,0) -- row s of numpy's
 *      Philox(key=seed, counter=2**256-1).random_raw(4n).reshape(n,4);
 *   4. triangle = the smallest i with C[i] > umul64hi(r0, W); u = (r1>>11) 2^-53, v = (1-u) ((r2>>11) 2^-53);
 *      p = ((v1 u) + (v2 v)) + ((1-(u+v)) v3) in float64, rounded to float32: the raw samples, written to samples (n,3) when it
 *      is non-NULL;
 *   5. float32, every operation correctly rounded: mn = the min over all 3n coordinates, mx = max - mn,
 *      q = rint(((p - mn) / mx) * (vg-1)); mx == 0 gives q = 0;
 *   6. the first sample of every distinct voxel, in sample order: points (capacity n rows) receives M rows of float32 integers
 *      in [0, vg) (a zero is +0) and *npoints_dev (int64, device) = M.
 * Limits: 1 <= ntris, n < 2^31; 1 <= vg <= 2^21.  The caller checks on the host (the kernels cannot): finite vertices within
 * +-2^100, indices in [0, nverts), a total area above 0.  workspace: pcc_mesh_sample_workspace_bytes(ntris, n) bytes (0 for a size
 * outside the limits), queried while ctx's device is the current one (hipCUB sizes its temporary storage for the current
 * device).  One stream, no host synchronisation; the same inputs give the same bits on every call.                            */
size_t pcc_mesh_sample_workspace_bytes(int64_t ntris, int64_t n);
int pcc_mesh_to_points(pcc_ctx* ctx, const double* verts, int64_t nverts, const int32_t* tris, int64_t ntris, int64_t n, uint64_t seed,
                       int32_t vg, float* samples, float* points, int64_t* npoints_dev, void* workspace, void* stream);

/* ---- point rendering (new: the rendering step of the reference's evaluation, utils/o3d.py pc_to_img without Open3D) ---------
 * A z-buffered square splat of a point cloud through a pinhole camera.  Inputs: points (n,3) float64 and colours (n,3) uint8
 * (device; colours NULL: every point grey 128); extrinsic E (4x4, row-major, world -> camera) and intrinsic K (3x3, row-major,
 * [[fx, k01, cx], [0, fy, cy], [0, 0, 1]]) as host arrays; image W x H; integer point size s; background RGB.  Definition
 * (restated in numpy by utils/render.py, which returns the same bytes), float64, every operation rounded, none contracted:
 *   1. xc = ((e00 x + e01 y) + e02 z) + e03, yc and zc the same with rows 1 and 2 of E;
 *   2. kept only if zc > 0; u = ((fx xc + k01 yc) + cx zc) / zc, v = (fy yc + cy zc) / zc; kept only if |u|, |v| < 2^30
 *      (finite);
 *   3. h = s/2 - 1 (exact), i0 = floor(u - h), j0 = floor(v - h): the point covers the pixels i0 <= i < i0+s, j0 <= j < j0+s
 *      inside the image (s = 1: floor(u + 0.5), pixel centres at integer u);
 *   4. key = bits(float32(zc)) << 32 | row; every pixel takes the smallest key (the nearest point; a depth tie to the lower row);
 *   5. image (H,W,3) uint8: image[j,i] = colours[row], or the background where no point landed; rows (H,W) int32 (nullable): that
 *      row, or -1.
 * Limits: 0 <= n < 2^31; 1 <= W, H <= 16384; 1 <= s <= 64; finite camera values, K rows 1-2 and E's bottom row [0,0,0,1] as
 * above (checked here as well; the Python layer checks them before any GPU call).  workspace: pcc_render_workspace_bytes(W, H)
 * bytes (0 for a size outside the limits).  One stream, no host synchronisation; the same inputs give the same bits on every
 * call, whatever the launch order.                                                                                            */
size_t pcc_render_workspace_bytes(int32_t width, int32_t height);
int pcc_render_points(pcc_ctx* ctx, const double* points, int64_t n, const uint8_t* colours, const double extrinsic[16],
                      const double intrinsic[9], int32_t width, int32_t height, int32_t point_size, const uint8_t background[3],
                      uint8_t* image, int32_t* rows, void* workspace, void* stream);

/* ---- focal loss (src/utils/focal_loss.py:5-12) ------------------------------------------
 * Deterministic two-stage reduction (wavefront DPP/shuffle tree, fixed block order); result is a
 * single float32 written to out[0] (device).  `scratch` must hold pcc_focal_scratch_floats().   */
int pcc_focal_loss(pcc_ctx* ctx, const float* y_true, const float* y_pred, size_t n, float gamma,
                   float alpha, float* out, float* scratch, void* stream);
size_t pcc_focal_scratch_floats(void);

/* ---- training: gradients of the conv layers and of the focal loss ------------------------------
 * Input gradient of a layer: pcc_conv3d on its DUAL descriptor (forward <-> transposed, Cin <-> Cout, same k and stride, the
 * layer's output grid) with the SAME Keras kernel array and no bias / ReLU / ADD: a Conv3DTranspose is the adjoint of the SAME Conv3D
 * on its larger grid.
 * pcc_conv3d_wgrad: dw (device, the layer's Keras layout) and db (device, Cout floats; may be NULL) of the layer `d` (flags ignored)
 * from its input `in` and output gradient `dout` (the gradient of the conv output, after the ReLU mask).  Exact-fp32 MFMA over fixed
 * voxel slices into `workspace` (>= pcc_conv_wgrad_workspace_bytes(d) bytes, 16-byte aligned), then a fixed-order sum of the
 * slices: bitwise identical run to run, no float atomics.                                                                    */
size_t pcc_conv_wgrad_workspace_bytes(const pcc_conv_desc* d);
/* The reduction depth of pcc_conv3d_wgrad on `d`: the number of voxel slices S, and the longest FMA chain of one slice
 * (voxels of its tiles, zero-padded tiles included) -- each dW element's error is below (slice_terms + S) 2^-24 sum|terms|. */
int pcc_conv_wgrad_slices(const pcc_conv_desc* d, int32_t* slices, int64_t* slice_terms);
int pcc_conv3d_wgrad(pcc_ctx* ctx, const pcc_conv_desc* d, const float* in, const float* dout, float* dw, float* db,
                     void* workspace, size_t ws_bytes, void* stream);
/* grad[i] = 0 where !(act[i] > 0), in place */
int pcc_relu_backward(pcc_ctx* ctx, float* grad, const float* act, size_t n, void* stream);
/* grad = scale[0] * d pcc_focal_loss / d y_pred (tf.clip_by_value gradient: zero strictly outside [1e-3, 0.999]).  scale: device
 * float (NULL: 1), so that the upstream gradient never travels to the host. */
int pcc_focal_loss_grad(pcc_ctx* ctx, const float* y_true, const float* y_pred, size_t n, float gamma, float alpha,
                        const float* scale, float* grad, void* stream);
/* Packed weight images rebuilt on the device from a device Keras kernel.  pcc_conv_repack_map (host) writes
 * pcc_conv_packed_floats(d) int32: the Keras index each packed float copies, -1 for a packed zero, -2 for the segments that are not
 * reorders of the taps (Winograd U, bf16 / fp16 pieces).  pcc_conv_repack_weights_device gathers with that map (uploaded by the
 * caller): bit-identical to pcc_conv_pack_weights on the gathered segments, NaN on the others -- a context that computes with the
 * image must have the split, fp16-piece and Winograd families off (pcc_ctx_set_numerics: NO_SPLIT | NO_F16S | NO_WINOGRAD).   */
int pcc_conv_repack_map(const pcc_conv_desc* d, int32_t* map);
int pcc_conv_repack_weights_device(pcc_ctx* ctx, const pcc_conv_desc* d, const int32_t* map, const float* w, float* pk,
                                   void* stream);

/* ---- training summaries (src/model_types.py:65-105) ------------------------------------------------
 * pcc_tensor_histogram: the TensorFlow HistogramProto of a contiguous float32 device tensor in one pass.  Bucket limits are those of
 * TensorFlow's histogram.cc: positive limits v = 1e-12, v *= 1.1 while v < 1e20 (774 values), then DBL_MAX; the table is
 * [-reversed positives, 0.0, positives] (pcc_histogram_limits writes its PCC_HISTOGRAM_BUCKETS doubles, host).  A finite value v
 * counts in bucket upper_bound(limits, (double)v); NaN and +-Inf count in `nonfinite` only.  min / max of an empty histogram are
 * DBL_MAX / -DBL_MAX.  counts are integers; sum and sum_squares are double sums over pcc_tensor_histogram_slices(n) slices added in
 * slice order: the same bytes on every call.  `out` (device, 8-byte aligned) receives one pcc_histogram; `workspace` (device) holds
 * pcc_tensor_histogram_workspace_bytes() bytes.                                                                              */
#define PCC_HISTOGRAM_BUCKETS 1551
typedef struct {
    uint64_t counts[PCC_HISTOGRAM_BUCKETS]; /* offset 0     */
    uint64_t num;                           /* offset 12408: finite values */
    uint64_t nonfinite;                     /* offset 12416 */
    double min, max, sum, sum_squares;      /* offsets 12424, 12432, 12440, 12448; sizeof = 12456 */
} pcc_histogram;
int pcc_histogram_limits(double* limits);
size_t pcc_tensor_histogram_workspace_bytes(void);
int pcc_tensor_histogram_slices(size_t n);
int pcc_tensor_histogram(pcc_ctx* ctx, const float* x, size_t n, pcc_histogram* out, void* workspace, void* stream);
/* pcc_occupancy_scores: the confusion matrix of q(x_tilde) against q(x), q(v) = rint(clip(v, 0, 1)) rounding half to even (0.5 -> 0;
 * NaN -> 0), as src/model_types.py:90-94 counts it; num_occupied = #(q(x) == 1) = tp + fn.  x_tilde_quant (device, n floats, may be
 * NULL) receives q(x_tilde).  `out`: one pcc_occupancy on the device.                                                         */
typedef struct {
    uint64_t tp, tn, fp, fn, num_occupied;  /* offsets 0, 8, 16, 24, 32; sizeof = 40 */
} pcc_occupancy;
int pcc_occupancy_scores(pcc_ctx* ctx, const float* x, const float* x_tilde, size_t n, float* x_tilde_quant, pcc_occupancy* out,
                         void* stream);

/* ---- range coder (HOST) ----------------------------------------------------------------
 * Replaces tfc's C++ ops range_coding_ops.unbounded_index_range_encode/decode
 * (src/utils/patch_gaussian_conditional.py:27-31; src/model_types.py:291-292,382-387,404-407),
 * which the reference also runs on the CPU (patch_gaussian_conditional.py:105-106).
 * Streams are independent (one per block and per string); they are coded on `n_threads` host
 * threads (0 = hardware concurrency).  The workers belong to the CALLING thread (one persistent pool per calling
 * thread, joined when that thread exits): a host that codes from two threads at once -- the encoder of one chunk beside the
 * decoder of another -- owns 2 x n_threads workers and has to size n_threads for that; call from long-lived threads
 * (a short-lived caller pays thread creation and teardown per call sequence).
 *   data[s], index[s] : n[s] int32 symbols / CDF-row indices of stream s (host pointers);
 *   index[s] == NULL  : row = i % index_mod (EntropyBottleneck: per-channel tables);
 *   cdf               : (rows, cdf_stride) int32, row r valid for cdf_size[r] entries;
 *   offset[r]         : smallest in-table value of row r.                                        */
typedef struct {
    const int32_t* cdf;
    const int32_t* cdf_size;
    const int32_t* offset;
    int32_t rows, cdf_stride, precision, overflow_width;
} pcc_cdf_table;

int pcc_range_encode_batch(const pcc_cdf_table* t, int32_t n_streams, const int32_t* const* data,
                           const int32_t* const* index, int32_t index_mod, const size_t* n,
                           uint8_t* const* out, const size_t* cap, size_t* out_len,
                           int32_t n_threads);
int pcc_range_decode_batch(const pcc_cdf_table* t, int32_t n_streams, const uint8_t* const* str,
                           const size_t* str_len, const int32_t* const* index, int32_t index_mod,
                           const size_t* n, int32_t* const* out, int32_t n_threads);
/* The same coders on narrow host arrays (round 3): data_bytes / out_bytes 2 (int16) or 4 (int32) symbols, index_bytes 1 (uint8)
 * or 4 (int32) CDF rows -- the codec moves y symbols as int16 and the 64 Gaussian scale rows as uint8 across PCIe.  Decoding
 * into 16 bits returns PCC_ERR_SPACE when a symbol does not fit (decode again with out_bytes 4).                              */
int pcc_range_encode_batch_n(const pcc_cdf_table* t, int32_t n_streams, const void* const* data, int32_t data_bytes,
                             const void* const* index, int32_t index_bytes, int32_t index_mod, const size_t* n,
                             uint8_t* const* out, const size_t* cap, size_t* out_len, int32_t n_threads);
int pcc_range_decode_batch_n(const pcc_cdf_table* t, int32_t n_streams, const uint8_t* const* str, const size_t* str_len,
                             const void* const* index, int32_t index_bytes, int32_t index_mod, const size_t* n,
                             void* const* out, int32_t out_bytes, int32_t n_threads);
/* tfc `pmf_to_quantized_cdf` (src/utils/patch_gaussian_conditional.py:87-89): pmf[n] -> cdf[n+1]. */
int pcc_pmf_to_quantized_cdf(const float* pmf, int32_t n, int32_t precision, int32_t* cdf);

/* ---- rANS coder (DEVICE): the opt-in "rans1" string format, a second format beside the range coder's ----------
 * An interleaved rANS: 32-bit state in [2^16, 2^32), initial state 2^16, 16-bit words, 16-bit probabilities (any other
 * `precision` of the table: PCC_ERR_ARG; so is a table with a frequency outside [1, 65535] -- then a lane moves at most one word
 * per symbol).  A stream of n symbols uses L in {1, 2, .., 64} lanes, symbol i on lane i % L at step i / L.  Row of symbol i:
 * index[i], or i % index_mod when index is NULL; with m = cdf_size[row] - 2, a value v with 0 <= v - offset[row] < m takes bin
 * v - offset[row], any other takes bin m and its raw int32 goes to the escape list (overflow_width is not used).
 * The decoder walks the steps upwards; after decoding its symbol a lane whose state fell below 2^16 reads one word from a single
 * forward cursor, lanes in ascending order within a step.  String bytes (little-endian): one byte log2(L); the escape count as a
 * LEB128 varint; L final states of 4 bytes; the words; the escapes, 4 bytes each.  n = 0 codes as the empty string.
 * L (lanes = 0): with cost256(f) = 256 (16 - k) - ((r << 8) >> k) for f = 2^k + r and est = (sum of cost256 + 2047) >> 11, the
 * largest power of two <= 64 with 128 L <= est, at least 1.  lanes > 0 forces that L (a power of two <= 64).
 *
 * One wave codes one stream.  Every pointer except `t` (host, as for the range coder; its arrays are uploaded once per context and
 * table and kept) and status_host is a DEVICE pointer:
 *   data / out   : int32 symbols, stream s at s * data_stride (out_stride) elements; index: int32 rows, stream s at s * index_stride
 *                  (0: one row vector shared by all streams); n[s] <= n_max symbols per stream;
 *   channels > 0 : the tensors are (n / channels, channels) in memory and the stream is channel-major: symbol i and its row are
 *                  read (written) at element (i % vox) * channels + i / vox, vox = n / channels -- the codec's NDHWC tensors
 *                  under data_format channels_first, without a permuted copy;
 *   encoder      : string s at out + s * cap with cap >= pcc_rans_stream_cap(n_max) (= 1 + 10 + 4 * 64 + 6 n_max), its length in
 *                  out_len[s]; status[s] != 0: a row outside the table / n[s] not a multiple of `channels` (the string is void);
 *                  workspace of pcc_rans_workspace_bytes(n_streams, n_max) bytes;
 *   decoder      : string s = str[off[s], off[s] + len[s]) inside the str_bytes bytes of `str`.  The kernel tests the header against
 *                  len[s] and clamps every cursor, so a truncated or inconsistent string never reads outside itself; it sets
 *                  status[s] != 0 when the string does not end exactly where its symbols do.  status_host (n_streams ints, may be
 *                  NULL): the call waits for the stream and returns PCC_ERR_CORRUPT / PCC_ERR_ARG from the flags; NULL: the
 *                  flags stay in status[] for the caller to fetch.
 * pcc_rans_check_strings (HOST pointers): the same header test before the upload -- PCC_ERR_CORRUPT.                              */
size_t pcc_rans_stream_cap(int64_t n);
size_t pcc_rans_workspace_bytes(int32_t n_streams, int64_t n_max);
int pcc_rans_check_strings(int32_t n_streams, const uint8_t* str, const int64_t* off, const int32_t* len, const int32_t* n);
int pcc_rans_encode_batch(pcc_ctx* ctx, const pcc_cdf_table* t, int32_t n_streams, const int32_t* data, int64_t data_stride,
                          const int32_t* index, int64_t index_stride, int32_t index_mod, int32_t channels, const int32_t* n,
                          int32_t n_max, int32_t lanes, uint8_t* out, size_t cap, int32_t* out_len, int32_t* status,
                          void* workspace, size_t workspace_bytes, void* stream);
int pcc_rans_decode_batch(pcc_ctx* ctx, const pcc_cdf_table* t, int32_t n_streams, const uint8_t* str, size_t str_bytes,
                          const int64_t* off, const int32_t* len, const int32_t* index, int64_t index_stride, int32_t index_mod,
                          int32_t channels, const int32_t* n, int32_t n_max, int32_t* out, int64_t out_stride, int32_t* status,
                          int32_t* status_host, void* stream);

/* ---- occupancy coder (DEVICE): the "occ1" string format, the lossless layer on top of the y/z strings -----------
 * One string codes the true occupancy of a block of n <= 2^28 voxels given x_hat (fp32, voxel i in C order), which encoder and
 * decoder hold with the same bits.  Bucket of voxel i, K = 32: 0 unless x_hat > 0 (NaN, -0, negatives); 31 if x_hat >= 1; else
 * min(30, 1 + (int)(x_hat * 30.0f)) -- one fp32 multiply, then truncation.  With tot[b] / on[b] the voxels / occupied voxels of
 * bucket b, every bucket with tot[b] > 0 has, in ascending b, one uint16 entry: 0 when on[b] == 0 (its voxels are not coded), else
 * f = clamp((on * 65536 + tot / 2) / tot, 1, 65535) in 64-bit integers.  Coded symbols: the voxels of the buckets with a non-zero
 * entry, in ascending i (m of them); bit 1 has freq f and start 65536 - f, bit 0 has freq 65536 - f and start 0.  Coder: rans1's
 * (above) without escapes -- state in [2^16, 2^32), initial state 2^16, 16-bit words, symbol j on lane j % L at step j / L, the
 * decoder walks the steps upwards with one forward word cursor, ascending lanes within a step; L by the same lane rule over the
 * coded freqs (m = 0: L = 1), lanes > 0 forces it.  String bytes (little-endian): one byte log2 L; the entries; L final states of
 * 4 bytes; the words.  n = 0 codes as the empty string.  A decoder accepts a string only if its length is 1 + 2 used + 4 L +
 * 2 n_words with n_words <= m (used = the buckets with tot > 0), every lane ends in 2^16 and the cursor ends at n_words.
 *
 * One workgroup codes one block.  x_hat, occ, out, out_len, status, str, off, len, occ_out and workspace are DEVICE pointers;
 * status_host is a host pointer.  Block s reads x_hat + s * x_hat_stride and occ + s * occ_stride (elements; the voxeliser's float
 * grid, occupied = != 0).
 *   encoder : string s at out + s * cap with cap >= pcc_occ_stream_cap(n) (= 1 + 2 * 32 + 4 * 64 + 2 n), its length in out_len[s],
 *             status[s] = 0; workspace of pcc_occ_workspace_bytes(n_streams, n) bytes.
 *   decoder : string s = str[off[s], off[s] + len[s]) inside the str_bytes bytes of `str`; occ_out + s * out_stride receives n
 *             floats, 0 or 1, and nothing outside them is written whatever the string says.  Every read of the string is made under
 *             the length test; status[s] != 0 when the string is not accepted (the grid is then undefined).  status_host
 *             (n_streams ints, may be NULL): the call waits for the stream and returns PCC_ERR_CORRUPT / PCC_ERR_ARG from the
 *             flags; NULL: the flags stay in status[] for the caller to fetch.  The same workspace size as the encoder's.
 * pcc_occ_check_strings (HOST pointers) reads the first byte of each string only: log2 L <= 6 and a length that leaves
 * len - 1 - 4 L even, non-negative and at most 2 (32 + n) -- PCC_ERR_CORRUPT.  `used` and m depend on x_hat, so only the device can
 * validate a string fully.                                                                                                      */
size_t pcc_occ_stream_cap(int64_t n);
size_t pcc_occ_workspace_bytes(int32_t n_streams, int64_t n);
int pcc_occ_check_strings(int32_t n_streams, const uint8_t* str, const int64_t* off, const int32_t* len, int64_t n);
int pcc_occ_encode_batch(pcc_ctx* ctx, const float* x_hat, int64_t x_hat_stride, const float* occ, int64_t occ_stride, int32_t n_streams,
                         int64_t n, int32_t lanes, uint8_t* out, size_t cap, int32_t* out_len, int32_t* status, void* workspace,
                         size_t workspace_bytes, void* stream);
int pcc_occ_decode_batch(pcc_ctx* ctx, const float* x_hat, int64_t x_hat_stride, int32_t n_streams, int64_t n, const uint8_t* str,
                         size_t str_bytes, const int64_t* off, const int32_t* len, float* occ_out, int64_t out_stride, int32_t* status,
                         int32_t* status_host, void* workspace, size_t workspace_bytes, void* stream);

/* ---- octree blocking, host (replaces the per-point loop of src/utils/octree_coding.py:82-108) ----------------------
 * Buckets `n` points (row-major doubles, `ncols` >= 3 columns, x y z first) into blocks of edge `block_size`:
 * bucket = Morton code of the block id over `level` bits per axis, x least significant.  order[n] receives the point
 * indices sorted by bucket, input order kept inside a bucket; bucket_count[8^level] the points per bucket.
 * Returns the number of occupied buckets (>= 0) or a negative status.  level <= 7.                                   */
int64_t pcc_octree_bucket(const double* points, int64_t n, int32_t ncols, int32_t block_size, int32_t level,
                                     int64_t* order, int64_t* bucket_count);

/* ---- octree anchor (new: a conventional geometry codec that runs on any cloud; NOT G-PCC, not a TMC13 stream) ----
 * Quantise-and-prune octree coding with neighbour-dependent contexts (pcc_geo_cnn_v2_amd/anchor_octree.py holds the stream header
 * and a numpy path that gives the same bytes).  Definition:
 *   - scale num / den, 0 < num <= den < 2^31; q = (2 p num + den) / (2 den) per coordinate of the integer points (the cell index's
 *     contract: [0, 2^21)), integer division; duplicates merged; depth D = bit_length(max q), at least 1 (the caller computes it:
 *     quantisation is monotone, so max q comes from max p); decoded p = min((2 q den + num) / (2 num), resolution - 1);
 *   - nodes of level l = the distinct key >> 3 (D - l) of the Morton keys (x << 2 | y << 1 | z per bit triple) of the quantised points,
 *     ascending; occupancy byte: bit c set for child c = 4 dx + 2 dy + dz; n6: bit 0 / 1 = the -x / +x face neighbour of the node is
 *     occupied at its own level, 2 / 3 = -y / +y, 4 / 5 = -z / +z, a neighbour outside [0, 2^l) counting as empty;
 *   - the bytes are coded breadth first by an adaptive binary range coder (LZMA's: 11-bit probabilities from 1024, shift 5, 32-bit
 *     range normalised below 2^24, carries through the cache byte, five flush bytes), child 0 first, decision c with model
 *     256 t + m: m = 1, then 2 m + bit (the bits already coded in this byte), t = bit (c >> 2 & 1) of n6 | bit (2 + (c >> 1 & 1))
 *     << 1 | bit (4 + (c & 1)) << 2 (the neighbours across the outer faces of child c's octant).  A byte is never 0: after seven
 *     zeros the eighth decision is not coded.  PCC_ANCHOR_NO_CONTEXT codes with t = 0 (measurement only: such a payload needs the
 *     same flag to decode).
 * Host coder: the *_code_bits / *_decode_bits pair codes raw decisions (model[i] < 2048, bit[i]); pcc_anchor_encode codes n nodes (all
 * levels, in order) into out[cap] and sets *out_len (PCC_ERR_SPACE when it does not fit: 2 n + 16 bytes always do);
 * the decoder keeps its state in pcc_anchor_decoder_bytes caller-owned bytes, reads `data` (which must outlive it) level by level
 * given each level's n6, and returns PCC_ERR_CORRUPT when the payload ends early; a payload is read to its last byte exactly.
 * Device side (one stream, no host synchronisation): pcc_anchor_tree writes, for level l < D, its nodes' occ and n6 bytes at
 * offset pcc_anchor_tree_level_offset(npts, l) = sum over j < l of min(npts, 8^j) of `occ` and `n6` (device, capacity
 * pcc_anchor_tree_capacity(npts, D) bytes each), and hdr (device, int64[PCC_ANCHOR_HDR_WORDS]): hdr[l] = nodes of level l, hdr[D]
 * = distinct quantised points.  pcc_anchor_expand writes the ascending child keys of one decoded level (nchildren = the sum of the
 * popcounts of occ, which the caller knows) and, when n6 is non-NULL, their n6 at child_level.  pcc_anchor_points turns leaf keys
 * into decoded points (n,3) int32.  Every index is checked against its count: wrong counts give wrong bytes, never an access
 * outside the buffers.  The *_bytes / capacity functions return 0 (level_offset: -1) outside the contract.                     */
#define PCC_ANCHOR_NO_CONTEXT 1
#define PCC_ANCHOR_HDR_WORDS 32
int pcc_anchor_code_bits(const uint16_t* model, const uint8_t* bit, int64_t n, uint8_t* out, int64_t cap, int64_t* out_len);
int pcc_anchor_decode_bits(const uint8_t* data, int64_t len, const uint16_t* model, int64_t n, uint8_t* bit);
int pcc_anchor_encode(const uint8_t* occ, const uint8_t* n6, int64_t n, int32_t flags, uint8_t* out, int64_t cap, int64_t* out_len);
size_t pcc_anchor_decoder_bytes(void);
int pcc_anchor_decoder_init(void* state, const uint8_t* data, int64_t len, int32_t flags);
int pcc_anchor_decode_level(void* state, const uint8_t* n6, int64_t n, uint8_t* occ);
int64_t pcc_anchor_decoder_consumed(const void* state);
int64_t pcc_anchor_tree_capacity(int64_t npts, int32_t depth);
int64_t pcc_anchor_tree_level_offset(int64_t npts, int32_t level);
size_t pcc_anchor_tree_workspace_bytes(int64_t npts);
int pcc_anchor_tree(pcc_ctx* ctx, const int32_t* pts, int64_t npts, int64_t num, int64_t den, int32_t depth, int64_t* hdr, uint8_t* occ,
                    uint8_t* n6, void* workspace, void* stream);
size_t pcc_anchor_expand_workspace_bytes(int64_t nparents);
int pcc_anchor_expand(pcc_ctx* ctx, const uint64_t* parents, const uint8_t* occ, int64_t nparents, int32_t child_level, uint64_t* children,
                      int64_t nchildren, uint8_t* n6, void* workspace, void* stream);
int pcc_anchor_points(pcc_ctx* ctx, const uint64_t* keys, int64_t n, int64_t num, int64_t den, int32_t resolution, int32_t* pts, void* stream);

/* ---- surface anchor (new: a triangle-soup class geometry codec; NOT G-PCC, not trisoup-conformant) ----------------
 * pcc_geo_cnn_v2_amd/anchor_surface.py holds the stream header, the normative definition and a numpy path that gives the same bytes.
 * node_log2 = k in [2, 6], W = 2^k.  Leaves: the distinct p >> k, as Morton keys (the octree anchor's order), ascending.  Edge key:
 * morton(corner) << 2 | axis, corner = leaf + {0, 1} in the two other axes; the edge list is the distinct keys of all leaves,
 * ascending.  Vertex of edge (c, a): over the distinct points with p_a >> k = c_a and |p_u - W c_u| <= 1, |p_v - W c_v| <= 1:
 * flag = there is one, t = (2 sum(p_a - W c_a) + n) / (2 n).
 * Device side (one stream, no host synchronisation inside a call; hdr is int64[PCC_SURFACE_HDR_WORDS] on the device, which the
 * caller copies back between calls):
 *   pcc_surface_leaves    points (n,3) int32 -> pkeys[npts] (the distinct points' Morton keys, ascending; hdr[0] of them),
 *                         leaf_keys[npts] (hdr[1] of them);
 *   pcc_surface_edges     leaf keys -> edge_keys[12 nleaves] (hdr[0] of them);
 *   pcc_surface_vertices  distinct point keys + edge list -> flags[nedges], t[nedges] (0 where the flag is 0);
 *   pcc_surface_count     leaves, edge list, flags, t -> pos[nleaves] (first voxel of each leaf), hdr[0] = all voxels emitted;
 *   pcc_surface_reconstruct  the same inputs, pos and total = that hdr[0] -> pts (total,3) int32 of which the first hdr[0] rows are
 *                         the decoded cloud: the voxels of all leaves, duplicates merged, in ascending Morton order, clipped to
 *                         resolution - 1.
 * Every index is checked against its count or capacity.  The *_workspace_bytes functions return 0 outside the contract.
 * Host coder (anchor_coder.cpp): the vertex payload, one run of the octree anchor's binary coder over the edge list: the flag under
 * model 2 a + prev, then behind a set flag the k bits of t, MSB first, under model 8 + m (m = 1, then 2 m + bit).  8 nedges + 16
 * bytes always fit.  The decoder returns PCC_ERR_CORRUPT when the payload ends early and reports the bytes it read.            */
#define PCC_SURFACE_HDR_WORDS 4
int pcc_surface_encode_vertices(const uint64_t* edge_keys, const uint8_t* flags, const uint8_t* t, int64_t nedges, int32_t k, uint8_t* out,
                                int64_t cap, int64_t* out_len);
int pcc_surface_decode_vertices(const uint8_t* data, int64_t len, const uint64_t* edge_keys, int64_t nedges, int32_t k, uint8_t* flags, uint8_t* t,
                                int64_t* nflags, int64_t* consumed);
size_t pcc_surface_leaves_workspace_bytes(int64_t npts);
int pcc_surface_leaves(pcc_ctx* ctx, const int32_t* pts, int64_t npts, int32_t k, int64_t* hdr, uint64_t* pkeys, uint64_t* leaf_keys, void* workspace,
                       void* stream);
size_t pcc_surface_edges_workspace_bytes(int64_t nleaves);
int pcc_surface_edges(pcc_ctx* ctx, const uint64_t* leaf_keys, int64_t nleaves, int64_t* hdr, uint64_t* edge_keys, void* workspace, void* stream);
size_t pcc_surface_vertices_workspace_bytes(int64_t npts);
int pcc_surface_vertices(pcc_ctx* ctx, const uint64_t* pkeys, int64_t npts, int32_t k, const uint64_t* edge_keys, int64_t nedges, uint8_t* flags,
                         uint8_t* t, void* workspace, void* stream);
size_t pcc_surface_count_workspace_bytes(int64_t nleaves);
int pcc_surface_count(pcc_ctx* ctx, const uint64_t* leaf_keys, int64_t nleaves, const uint64_t* edge_keys, const uint8_t* flags, const uint8_t* t,
                      int64_t nedges, int32_t k, uint64_t* pos, int64_t* hdr, void* workspace, void* stream);
size_t pcc_surface_reconstruct_workspace_bytes(int64_t total);
int pcc_surface_reconstruct(pcc_ctx* ctx, const uint64_t* leaf_keys, int64_t nleaves, const uint64_t* edge_keys, const uint8_t* flags,
                            const uint8_t* t, int64_t nedges, int32_t k, int32_t resolution, const uint64_t* pos, int64_t total, int32_t* pts,
                            int64_t* hdr, void* workspace, void* stream);

/* ---- colour anchor (new: an attribute codec for the colours of a voxelised cloud; NOT G-PCC, not RAHT-conformant) ----
 * pcc_geo_cnn_v2_amd/anchor_color.py holds the stream header, the normative definition (integers only) and a numpy path that gives
 * the same bytes.  An integer weighted-Haar lifting over the binary Morton tree of N pairwise distinct points: leaves = the points in
 * ascending key order (the octree anchor's keys over D = depth bits per axis), values = YCoCg-R of their colours.  Leaf i >= 1 owns
 * one coefficient at step s = the highest bit of key[i - 1] ^ key[i]; its node holds the leaves [p0, p1) that agree with key[i] above
 * bit s, wL = i - p0, wR = p1 - i, w = wL + wR.  Forward, s ascending: h = val[i] - val[p0], val[p0] += floor(wR h / w); val[0]
 * ends as the DC.  Quantiser: step = max(1, isqrt(Q Q w / (wL wR))), c = sgn(h) (2 |h| + step) / (2 step).  Inverse, s descending:
 * aL = val[p0] - floor(wR c step / w), val[p0] = aL, val[i] = aL + c step; then RGB, clipped to [0, 255].  Coding order: steps
 * descending, i ascending inside a step, channels Y, Co, Cg.
 * Device side (one stream, no host synchronisation inside a call):
 *   pcc_color_anchor_plan     points (n,3) int32 -> the plan, kept in `workspace` (pcc_color_anchor_workspace_bytes(npts) bytes, 0
 *                             outside the contract) for the two calls below, and hdr (device, int64[PCC_COLOR_HDR_WORDS]): hdr[s] =
 *                             coefficients of step s (s < 64), hdr[64] = adjacent equal keys (duplicate positions: the caller refuses);
 *   pcc_color_anchor_forward  colours (n,3) uint8 RGB in the row order of the planned points -> coef (device, int16[3 (n - 1)]) in
 *                             coding order and hdr[65 .. 67] = the DC triple; hdr[0 .. 64] are left as the plan wrote them;
 *   pcc_color_anchor_inverse  coef (device) and dc (HOST, int32[3], Y in [0, 255], Co, Cg in [-255, 255]) -> colours (n,3) uint8 in
 *                             the row order of the planned points.
 * Every index is checked against its count.  Host coder (anchor_coder.cpp): one run of the octree anchor's binary coder over the
 * coefficients in coding order given the per-step counts (nsteps = 3 D <= 63); g = 2 min(s / 3, 7) + (channel != Y); zero flag under
 * 32 g + z (z = the previous coefficient of the channel was nonzero), sign under 32 g + 2, v = |c| < 512 as n = bit_length(v) - 1
 * ones and a zero under 32 g + 3 + j, then the n low bits, MSB first, under 32 g + 12 + j.  PCC_ERR_SPACE when the bytes do not fit
 * `cap` (48 ncoef + 16 always do).  The decoder returns PCC_ERR_CORRUPT for a ninth one-bit or a payload that ends early and reports
 * the bytes it read.                                                                                                               */
#define PCC_COLOR_HDR_WORDS 72
size_t pcc_color_anchor_workspace_bytes(int64_t npts);
int pcc_color_anchor_plan(pcc_ctx* ctx, const int32_t* pts, int64_t npts, int32_t depth, int64_t* hdr, void* workspace, void* stream);
int pcc_color_anchor_forward(pcc_ctx* ctx, const uint8_t* colors, int64_t npts, int32_t depth, int32_t qstep, int64_t* hdr, int16_t* coef,
                             void* workspace, void* stream);
int pcc_color_anchor_inverse(pcc_ctx* ctx, const int16_t* coef, const int32_t* dc, int64_t npts, int32_t depth, int32_t qstep, uint8_t* colors,
                             void* workspace, void* stream);
int pcc_color_anchor_encode(const int16_t* coef, int64_t ncoef, const int64_t* counts, int32_t nsteps, uint8_t* out, int64_t cap,
                            int64_t* out_len);
int pcc_color_anchor_decode(const uint8_t* data, int64_t len, const int64_t* counts, int32_t nsteps, int16_t* coef, int64_t ncoef,
                            int64_t* consumed);

#ifdef __cplusplus
}
#endif
#endif /* PCC_GEO_H */
