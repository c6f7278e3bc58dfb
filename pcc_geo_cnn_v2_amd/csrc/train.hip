// The element-wise pieces of the training backward pass: ReLU mask, focal-loss gradient and the on-device rebuild of the packed
// weight images (the weights change every step; conv_wgrad.hip holds the weight gradients).  No reductions here.
#include "common.h"

namespace {

constexpr int kThreads = 256;

int blocks_for(size_t n, int num_cu) {
    size_t b = (n + kThreads - 1) / kThreads;
    const size_t cap = (size_t)num_cu * 32;
    return (int)(b > cap ? cap : (b == 0 ? 1 : b));
}

__global__ void __launch_bounds__(kThreads) k_relu_backward(float* __restrict__ g, const float* __restrict__ act, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        if (!(act[i] > 0.f)) g[i] = 0.f;
}

// d/dp of src/utils/focal_loss.py:5-12 with tf.clip_by_value's gradient (zero strictly outside [1e-3, 0.999], passed at the bounds).
// y_true == 1: only pt_1 = clip(p) depends on p; y_true == 0: only pt_0 = clip(p); any other label: neither.
__global__ void __launch_bounds__(kThreads) k_focal_grad(const float* __restrict__ yt, const float* __restrict__ yp, size_t n,
                                                         float gamma, float alpha, const float* __restrict__ scale,
                                                         float* __restrict__ grad) {
    const float sc = scale ? scale[0] : 1.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float t = yt[i], p = yp[i];
        float g = 0.f;
        if ((t == 1.f || t == 0.f) && p >= 1e-3f && p <= .999f) {
            if (t == 1.f)        // -alpha (1-p)^gamma log p
                g = -alpha * (-gamma * powf(1.f - p, gamma - 1.f) * logf(p) + powf(1.f - p, gamma) / p);
            else                 // -(1-alpha) p^gamma log(1-p)
                g = -(1.f - alpha) * (gamma * powf(p, gamma - 1.f) * logf(1.f - p) - powf(p, gamma) / (1.f - p));
        }
        grad[i] = sc * g;
    }
}

__global__ void __launch_bounds__(kThreads) k_repack(const int32_t* __restrict__ map, const float* __restrict__ w, size_t n,
                                                     float* __restrict__ pk) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int32_t m = map[i];
        pk[i] = m >= 0 ? w[m] : (m == -1 ? 0.f : __builtin_nanf(""));
    }
}

}  // namespace

PCC_API int pcc_relu_backward(pcc_ctx* ctx, float* grad, const float* act, size_t n, void* stream) {
    PCC_REQUIRE(ctx && grad && act, "pcc_relu_backward: NULL argument");
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    if (n == 0) return PCC_OK;
    hipLaunchKernelGGL(k_relu_backward, dim3(blocks_for(n, ctx->num_cu)), dim3(kThreads), 0, (hipStream_t)stream, grad, act, n);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_focal_loss_grad(pcc_ctx* ctx, const float* y_true, const float* y_pred, size_t n, float gamma, float alpha,
                                const float* scale, float* grad, void* stream) {
    PCC_REQUIRE(ctx && y_true && y_pred && grad, "pcc_focal_loss_grad: NULL argument");
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    if (n == 0) return PCC_OK;
    hipLaunchKernelGGL(k_focal_grad, dim3(blocks_for(n, ctx->num_cu)), dim3(kThreads), 0, (hipStream_t)stream, y_true, y_pred, n,
                       gamma, alpha, scale, grad);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_conv_repack_weights_device(pcc_ctx* ctx, const pcc_conv_desc* d, const int32_t* map, const float* w, float* pk,
                                           void* stream) {
    PCC_REQUIRE(ctx && d && map && w && pk, "pcc_conv_repack_weights_device: NULL argument");
    const size_t n = pcc_conv_packed_floats(d);
    PCC_REQUIRE(n > 0, "pcc_conv_repack_weights_device: shape not covered by the MFMA path");
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_repack, dim3(blocks_for(n, ctx->num_cu)), dim3(kThreads), 0, (hipStream_t)stream, map, w, n, pk);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
