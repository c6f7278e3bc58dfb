// Point rendering (include/pcc_geo.h "point rendering"): a z-buffered square splat of every point through a
// pinhole camera, the rendering step of the reference's evaluation (its utils/o3d.py pc_to_img, without Open3D or a window).
// The numpy restatement utils/render.py is the definition; tests/test_render_gpu.py pins these kernels to it bit for bit.
//
// One stream, no host synchronisation:
//   1. hipMemsetAsync(0xFF) of the W*H uint64 z-buffer in the workspace;
//   2. k_splat: one thread per point projects it in float64 (every operation rounded: `fp contract(off)`, the ISA of the
//      projection has v_fma_f64 only inside the correctly rounded divisions) and takes the minimum of
//      key = bits(float32(zc)) << 32 | row over the pixels of its square: a plain load first, the atomic only when the key is
//      smaller (the buffer only decreases, so skipping is exact), so a cloud that lands on a few pixels does not queue thousands
//      of device-scope atomics on one address;
//   3. k_resolve: one thread per pixel gathers the colour of the winning row (or the background) and, optionally, the row.
// The result is a minimum over integer keys: it does not depend on dispatch order.
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kEmpty = ~0ull;

// the camera passed by value: rows 0-2 of the extrinsic and the five free intrinsic entries
struct RenderCam {
    double e[12];
    double fx, k01, cx, fy, cy;
};

size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

bool valid_side(int32_t v) { return v >= 1 && v <= 16384; }

__device__ __forceinline__ double row3(const double* r, double x, double y, double z) {
#pragma clang fp contract(off)
    return ((r[0] * x + r[1] * y) + r[2] * z) + r[3];
}

__global__ void __launch_bounds__(kBlock) k_splat(const double* __restrict__ P, long long n, RenderCam cam, int W, int H, int s,
                                                  unsigned long long* __restrict__ zb) {
#pragma clang fp contract(off)
    const double h = 0.5 * (double)s - 1.0;                          // exact
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        const double x = P[3 * r], y = P[3 * r + 1], z = P[3 * r + 2];
        const double xc = row3(cam.e, x, y, z), yc = row3(cam.e + 4, x, y, z), zc = row3(cam.e + 8, x, y, z);
        if (!(zc > 0.0)) continue;
        const double u = ((cam.fx * xc + cam.k01 * yc) + cam.cx * zc) / zc;     // IEEE division (v_div_scale / fmas / fixup)
        const double v = (cam.fy * yc + cam.cy * zc) / zc;
        if (!(fabs(u) < 1073741824.0) || !(fabs(v) < 1073741824.0)) continue;   // also drops NaN and inf
        const long long i0 = (long long)floor(u - h), j0 = (long long)floor(v - h);
        const long long ia = i0 > 0 ? i0 : 0, ib = i0 + s < W ? i0 + s : W;
        const long long ja = j0 > 0 ? j0 : 0, jb = j0 + s < H ? j0 + s : H;
        if (ia >= ib || ja >= jb) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(__double2float_rn(zc)) << 32) | (unsigned long long)r;
        for (long long j = ja; j < jb; ++j)
            for (long long i = ia; i < ib; ++i) {
                unsigned long long* p = zb + (j * W + i);
                if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(p, key);
            }
    }
}

__global__ void __launch_bounds__(kBlock) k_resolve(const unsigned long long* __restrict__ zb, long long npix, const uint8_t* __restrict__ col,
                                                    uint8_t b0, uint8_t b1, uint8_t b2, uint8_t* __restrict__ img, int32_t* __restrict__ rows) {
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const unsigned long long k = zb[p];
        uint8_t c0 = b0, c1 = b1, c2 = b2;
        int32_t row = -1;
        if (k != kEmpty) {
            row = (int32_t)(unsigned)(k & 0xffffffffull);
            if (col) {
                const long long o = 3 * (long long)row;
                c0 = col[o]; c1 = col[o + 1]; c2 = col[o + 2];
            } else {
                c0 = c1 = c2 = 128;
            }
        }
        img[3 * p] = c0; img[3 * p + 1] = c1; img[3 * p + 2] = c2;
        if (rows) rows[p] = row;
    }
}

unsigned grid_for(long long n, unsigned cap) {
    const long long b = (n + kBlock - 1) / kBlock;
    return (unsigned)(b < (long long)cap ? b : cap);
}

}  // namespace

PCC_API size_t pcc_render_workspace_bytes(int32_t width, int32_t height) {
    if (!valid_side(width) || !valid_side(height)) return 0;
    return al256((size_t)width * (size_t)height * 8);
}

PCC_API int pcc_render_points(pcc_ctx* ctx, const double* points, int64_t n, const uint8_t* colours, const double extrinsic[16],
                              const double intrinsic[9], int32_t width, int32_t height, int32_t point_size, const uint8_t background[3],
                              uint8_t* image, int32_t* rows, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && extrinsic && intrinsic && background && image && workspace, "pcc_render_points: NULL argument");
    PCC_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "pcc_render_points: n = %lld outside [0, 2^31)", (long long)n);
    PCC_REQUIRE(n == 0 || points, "pcc_render_points: NULL points");
    PCC_REQUIRE(valid_side(width) && valid_side(height), "pcc_render_points: image %dx%d outside [1, 16384] per side", (int)width, (int)height);
    PCC_REQUIRE(point_size >= 1 && point_size <= 64, "pcc_render_points: point_size = %d outside [1, 64]", (int)point_size);
    for (int k = 0; k < 16; ++k) PCC_REQUIRE(std::isfinite(extrinsic[k]), "pcc_render_points: extrinsic[%d] is not finite", k);
    for (int k = 0; k < 9; ++k) PCC_REQUIRE(std::isfinite(intrinsic[k]), "pcc_render_points: intrinsic[%d] is not finite", k);
    PCC_REQUIRE(extrinsic[12] == 0.0 && extrinsic[13] == 0.0 && extrinsic[14] == 0.0 && extrinsic[15] == 1.0,
                "pcc_render_points: extrinsic bottom row must be [0, 0, 0, 1]");
    PCC_REQUIRE(intrinsic[3] == 0.0 && intrinsic[6] == 0.0 && intrinsic[7] == 0.0 && intrinsic[8] == 1.0,
                "pcc_render_points: intrinsic rows 1 and 2 must be [0, fy, cy] and [0, 0, 1]");
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    RenderCam cam;
    for (int k = 0; k < 12; ++k) cam.e[k] = extrinsic[k];
    cam.fx = intrinsic[0]; cam.k01 = intrinsic[1]; cam.cx = intrinsic[2]; cam.fy = intrinsic[4]; cam.cy = intrinsic[5];
    unsigned long long* zb = (unsigned long long*)workspace;
    const long long npix = (long long)width * height;
    PCC_CHECK_HIP(hipMemsetAsync(zb, 0xFF, (size_t)npix * 8, st));
    if (n > 0)
        hipLaunchKernelGGL(k_splat, dim3(grid_for(n, 1u << 20)), dim3(kBlock), 0, st, points, (long long)n, cam, (int)width, (int)height,
                           (int)point_size, zb);
    hipLaunchKernelGGL(k_resolve, dim3(grid_for(npix, 1u << 20)), dim3(kBlock), 0, st, (const unsigned long long*)zb, npix, colours,
                       background[0], background[1], background[2], image, rows);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
