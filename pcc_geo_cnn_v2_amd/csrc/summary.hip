// Training summaries: the TensorFlow HistogramProto of a float32 tensor in one pass, and the occupancy
// confusion matrix of src/model_types.py:90-99.  Integer counts (LDS-privatised, merged with integer atomics), double sums over
// slices whose number depends on n only and which are added in slice order: the same bytes on every run, no float atomics.
#include "common.h"

#include <cfloat>
#include <mutex>

namespace {

constexpr int kThreads = 256;
constexpr int kPos = PCC_HISTOGRAM_BUCKETS / 2;          // 775 positive limits: 774 of the 1.1 ladder + DBL_MAX
constexpr int kMaxSlices = 1024;
constexpr int kSliceFloats = 4096;                       // a slice covers at least this many elements
constexpr int kBallotRounds = 2;

// TensorFlow's InitDefaultBucketsInner (histogram.cc): the positive limits by repeated IEEE multiplication, then DBL_MAX.
const double* positive_limits() {
    static double pos[kPos];
    static std::once_flag once;
    std::call_once(once, [] {
        int n = 0;
        for (double v = 1e-12; v < 1e20; v *= 1.1) pos[n++] = v;      // 774 values
        pos[n++] = DBL_MAX;
    });
    return pos;
}

struct Partial {          // one per slice (32 bytes)
    double sum, sum_squares;
    float mn, mx;
    unsigned long long nonfinite;
};

// Number of positive limits <= a (kLess: < a) for a finite a >= 0: the index is estimated from log2 and corrected against the table,
// so that it equals the upper_bound answer whatever the estimate's error.  pos[kPos - 1] = DBL_MAX ends both walks.
template <bool kLess>
__device__ __forceinline__ int limits_below(const double* pos, float af) {
    const double a = (double)af;
    if (a < pos[0]) return 0;                                        // zero, denormals, everything under 1e-12
    // pos[j] = 1e-12 * 1.1^j: j ~ (log2 a - log2 1e-12) / log2 1.1
    int c = (int)((__log2f(af) + 39.863137f) * 7.2725408f) + 1;
    c = c < 1 ? 1 : (c > kPos - 1 ? kPos - 1 : c);
    if (kLess) {
        while (c > 0 && pos[c - 1] >= a) --c;
        while (pos[c] < a) ++c;
    } else {
        while (c > 0 && pos[c - 1] > a) --c;
        while (pos[c] <= a) ++c;
    }
    return c;
}

// bucket = upper_bound([-reversed pos, 0, pos], v): a negative v lies before the -pos[k] with pos[k] < |v|
__device__ __forceinline__ int bucket_of(const double* pos, float v) {
    return v >= 0.f ? kPos + 1 + limits_below<false>(pos, v) : kPos - limits_below<true>(pos, -v);
}

// One count into the workgroup's LDS bins.  Tensors of {0,1} (x, x_tilde_quant, a trained x_tilde) send all 64 lanes to one or two
// bins: up to kBallotRounds times the lanes that share the first pending lane's bin are counted by one add of their number; the
// lanes left after that add one by one.  `bin` < 0: nothing to count.
__device__ __forceinline__ void count_bin(unsigned* bins, int bin) {
    bool pending = bin >= 0;
#pragma unroll
    for (int r = 0; r < kBallotRounds; ++r) {
        const unsigned long long live = __ballot(pending);
        if (live == 0) return;
        const int lead = __ffsll((long long)live) - 1;
        const int lead_bin = __shfl(bin, lead);
        const unsigned long long same = __ballot(pending && bin == lead_bin);
        if ((int)(threadIdx.x & 63) == lead) atomicAdd(&bins[lead_bin], (unsigned)__popcll(same));
        if (bin == lead_bin) pending = false;
    }
    if (pending) atomicAdd(&bins[bin], 1u);
}

struct Acc {
    double sum = 0., sq = 0.;
    float mn = FLT_MAX, mx = -FLT_MAX;
    unsigned nonfinite = 0;
};

__device__ __forceinline__ void take(Acc& a, unsigned* bins, const double* pos, float v, bool valid) {
    const bool fin = valid && fabsf(v) <= FLT_MAX;                   // false for NaN and +-Inf
    if (fin) {
        const double d = (double)v;
        a.sum += d;
        a.sq += d * d;
        a.mn = fminf(a.mn, v);
        a.mx = fmaxf(a.mx, v);
    } else if (valid) {
        ++a.nonfinite;
    }
    count_bin(bins, fin ? bucket_of(pos, v) : -1);
}

// grid = S slices.  Quad q (elements 4q .. 4q+3) belongs to thread q % (S * 256) whatever the pointer's alignment, and a thread adds
// its elements in ascending order: the sums are a function of the values and n alone.
template <bool kAligned>
__global__ void __launch_bounds__(kThreads) k_histogram(const float* __restrict__ x, size_t n, const double* __restrict__ limits_pos,
                                                        unsigned long long* __restrict__ counts, Partial* __restrict__ partial) {
    __shared__ double pos[kPos];
    __shared__ unsigned bins[PCC_HISTOGRAM_BUCKETS];
    __shared__ Partial wave_part[kThreads / 64];
    for (int i = threadIdx.x; i < kPos; i += kThreads) pos[i] = limits_pos[i];
    for (int i = threadIdx.x; i < PCC_HISTOGRAM_BUCKETS; i += kThreads) bins[i] = 0;
    __syncthreads();

    Acc a;
    const size_t quads = (n + 3) / 4, stride = (size_t)gridDim.x * kThreads;
    // whole waves stay in the loop together (count_bin's ballots): the bound is rounded up to a wave
    const size_t first = (size_t)blockIdx.x * kThreads + threadIdx.x, wave0 = first - (threadIdx.x & 63);
    for (size_t q = first, w = wave0; w < quads; q += stride, w += stride) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const size_t e = q * 4;
        if (kAligned && e + 4 <= n) {
            const float4 t = *reinterpret_cast<const float4*>(x + e);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e + k < n) v[k] = x[e + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) take(a, bins, pos, v[k], e + k < n);
    }

    // wave tree (fixed order), then the workgroup's four waves in wave order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a.sum += __shfl_xor(a.sum, off);
        a.sq += __shfl_xor(a.sq, off);
        a.mn = fminf(a.mn, __shfl_xor(a.mn, off));
        a.mx = fmaxf(a.mx, __shfl_xor(a.mx, off));
        a.nonfinite += __shfl_xor(a.nonfinite, off);
    }
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = Partial{a.sum, a.sq, a.mn, a.mx, a.nonfinite};
    __syncthreads();
    if (threadIdx.x == 0) {
        Partial p = wave_part[0];
        for (int w = 1; w < kThreads / 64; ++w) {
            p.sum += wave_part[w].sum;
            p.sum_squares += wave_part[w].sum_squares;
            p.mn = fminf(p.mn, wave_part[w].mn);
            p.mx = fmaxf(p.mx, wave_part[w].mx);
            p.nonfinite += wave_part[w].nonfinite;
        }
        partial[blockIdx.x] = p;
    }
    for (int i = threadIdx.x; i < PCC_HISTOGRAM_BUCKETS; i += kThreads)
        if (bins[i]) atomicAdd(&counts[i], (unsigned long long)bins[i]);
}

// one wave: the slice partials in slice order (lane l takes slices l, l + 64, ...; then the fixed wave tree)
__global__ void __launch_bounds__(64) k_histogram_final(const Partial* __restrict__ partial, int slices, size_t n,
                                                        pcc_histogram* __restrict__ out) {
    double sum = 0., sq = 0.;
    float mn = FLT_MAX, mx = -FLT_MAX;
    unsigned long long nf = 0;
    for (int s = threadIdx.x; s < slices; s += 64) {
        const Partial p = partial[s];
        sum += p.sum;
        sq += p.sum_squares;
        mn = fminf(mn, p.mn);
        mx = fmaxf(mx, p.mx);
        nf += p.nonfinite;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sum += __shfl_xor(sum, off);
        sq += __shfl_xor(sq, off);
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
        nf += __shfl_xor(nf, off);
    }
    if (threadIdx.x == 0) {
        const bool any = nf < n;
        out->num = n - nf;
        out->nonfinite = nf;
        out->min = any ? (double)mn : DBL_MAX;           // TensorFlow's Histogram::Clear() values for an empty histogram
        out->max = any ? (double)mx : -DBL_MAX;
        out->sum = sum;
        out->sum_squares = sq;
    }
}

// q(v) = rint(clip(v, 0, 1)) with round-half-to-even is 1 exactly when v > 0.5 (0.5 -> 0, NaN -> 0).
// src/model_types.py:91-94 multiplies uint8 tensors and counts non-zeros: with q - 1 wrapping to 255 for q = 0, q~ * q != 0 is
// (q~, q) = (1, 1), (q~ - 1)(q - 1) != 0 is (0, 0), q~ (q - 1) != 0 is (1, 0) and (q~ - 1) q != 0 is (0, 1) -- the usual confusion
// matrix tp, tn, fp, fn of the reconstruction q~ against the input q.
__global__ void __launch_bounds__(kThreads) k_occupancy(const float* __restrict__ x, const float* __restrict__ xt, size_t n,
                                                        float* __restrict__ quant, unsigned long long* __restrict__ out) {
    __shared__ unsigned tot[5];
    if (threadIdx.x < 5) tot[threadIdx.x] = 0;
    __syncthreads();
    unsigned c[5] = {0, 0, 0, 0, 0};                     // tp tn fp fn occupied
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const bool q = x[i] > .5f, qt = xt[i] > .5f;
        c[0] += qt && q;
        c[1] += !qt && !q;
        c[2] += qt && !q;
        c[3] += !qt && q;
        c[4] += q;
        if (quant) quant[i] = qt ? 1.f : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c[k] += __shfl_xor(c[k], off);
        if ((threadIdx.x & 63) == 0 && c[k]) atomicAdd(&tot[k], c[k]);
    }
    __syncthreads();
    if (threadIdx.x < 5 && tot[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)tot[threadIdx.x]);
}

int slices_of(size_t n) {
    const size_t s = (n + kSliceFloats - 1) / kSliceFloats;
    return (int)(s < 1 ? 1 : (s > (size_t)kMaxSlices ? (size_t)kMaxSlices : s));
}

}  // namespace

PCC_API int pcc_histogram_limits(double* limits) {
    PCC_REQUIRE(limits, "pcc_histogram_limits: NULL argument");
    const double* pos = positive_limits();
    for (int i = 0; i < kPos; ++i) {
        limits[kPos - 1 - i] = -pos[i];
        limits[kPos + 1 + i] = pos[i];
    }
    limits[kPos] = 0.0;
    return PCC_HISTOGRAM_BUCKETS;
}

PCC_API size_t pcc_tensor_histogram_workspace_bytes(void) { return (size_t)kMaxSlices * sizeof(Partial); }

PCC_API int pcc_tensor_histogram_slices(size_t n) { return slices_of(n); }

PCC_API int pcc_tensor_histogram(pcc_ctx* ctx, const float* x, size_t n, pcc_histogram* out, void* workspace, void* stream) {
    PCC_REQUIRE(ctx && out && workspace && (x || n == 0), "pcc_tensor_histogram: NULL argument");
    PCC_REQUIRE(((uintptr_t)out & 7) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)x & 3) == 0,
                "pcc_tensor_histogram: misaligned pointer");
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    if (!ctx->summary_limits) {          // the table goes to the device once per context, as the host computed it
        void* p = nullptr;
        PCC_CHECK_HIP(hipMalloc(&p, kPos * sizeof(double)));
        if (hipMemcpy(p, positive_limits(), kPos * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(p);
            pcc_set_error("pcc_tensor_histogram: uploading the bucket limits failed");
            return PCC_ERR_HIP;
        }
        ctx->summary_limits = p;
    }
    PCC_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(pcc_histogram), st));
    const int S = slices_of(n);
    const double* pos = (const double*)ctx->summary_limits;
    if (((uintptr_t)x & 15) == 0)
        hipLaunchKernelGGL(k_histogram<true>, dim3(S), dim3(kThreads), 0, st, x, n, pos, (unsigned long long*)out->counts, (Partial*)workspace);
    else
        hipLaunchKernelGGL(k_histogram<false>, dim3(S), dim3(kThreads), 0, st, x, n, pos, (unsigned long long*)out->counts, (Partial*)workspace);
    PCC_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_histogram_final, dim3(1), dim3(64), 0, st, (const Partial*)workspace, S, n, out);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_occupancy_scores(pcc_ctx* ctx, const float* x, const float* x_tilde, size_t n, float* x_tilde_quant,
                                 pcc_occupancy* out, void* stream) {
    PCC_REQUIRE(ctx && out && ((x && x_tilde) || n == 0), "pcc_occupancy_scores: NULL argument");
    PCC_REQUIRE(((uintptr_t)out & 7) == 0, "pcc_occupancy_scores: misaligned result");
    PCC_CHECK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    PCC_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(pcc_occupancy), st));
    if (n == 0) return PCC_OK;
    size_t b = (n + kThreads - 1) / kThreads;
    const size_t cap = (size_t)ctx->num_cu * 16;
    hipLaunchKernelGGL(k_occupancy, dim3((unsigned)(b > cap ? cap : b)), dim3(kThreads), 0, st, x, x_tilde, n, x_tilde_quant,
                       (unsigned long long*)out);
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}
