// Device entropy coder of libpcc_geo_hip.so: the "rans1" string format (include/pcc_geo.h "rANS coder (DEVICE)").
//
// An interleaved rANS with a 32-bit state in [2^16, 2^32), 16-bit renormalisation and 16-bit probabilities: every frequency is at
// most 2^16 - 1, so a lane emits (encoder) or reads (decoder) at most ONE word per symbol, and the words of a step can be placed with
// a ballot and a prefix popcount over the renormalising lanes.  One wave codes one stream; a launch codes a batch of streams.
//
//   encoder  pass 1 (all 64 lanes, symbol-parallel): bin of every symbol -> (start << 16 | freq) into the workspace, the integer
//            cost and the escape count; the lane rule picks L
//            pass 2 (L lanes, steps descending): the rANS recurrence; a step's words go to the workspace, filled from its end
//            pass 3 (all 64 lanes): header, final states, words, and the escapes compacted in symbol order
//   decoder  header parsed with every read clamped to the string; steps ascending: bin search (the bin of the value 0 first, then
//            bisection), state update, refill and escape substitution in ballot / prefix order
//
// Every store is a plain C++ store of a vector lane.
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"
#include "rans_common.h"

namespace {

struct DevTable {
    const int32_t* cdf;
    const int32_t* size;
    const int32_t* offset;
    int32_t rows, stride;
};

// where symbol i of a stream lies in memory: as it is, or -- channels > 0: the tensor is (vox, channels) in memory and the stream is
// channel-major -- at (i % vox) * channels + i / vox
struct Layout {
    int32_t channels, vox;
    __device__ __forceinline__ int64_t at(int32_t i) const {
        return channels > 0 ? (int64_t)(i % vox) * channels + i / vox : (int64_t)i;
    }
};

struct Bin { uint32_t start, freq; bool escape; };

// row of symbol i (clamped into the table; a row outside it sets kBadRow)
__device__ __forceinline__ int32_t row_of(const DevTable& t, const int32_t* index, int32_t index_mod, int32_t i, int64_t p, int32_t& flags) {
    int32_t row = index ? index[p] : i % index_mod;
    if ((uint32_t)row >= (uint32_t)t.rows) { flags |= kBadRow; row = 0; }
    return row;
}

__device__ __forceinline__ Bin bin_of(const DevTable& t, int32_t row, int32_t v) {
    const int32_t m = t.size[row] - 2;
    int64_t b = (int64_t)v - t.offset[row];
    const bool esc = b < 0 || b >= m;
    if (esc) b = m;
    const int32_t* c = t.cdf + (int64_t)row * t.stride + b;
    const uint32_t lo = (uint32_t)c[0], hi = (uint32_t)c[1];
    return Bin{lo, hi - lo, esc};
}

__global__ __launch_bounds__(64) void rans_encode_kernel(DevTable t, const int32_t* __restrict__ data, int64_t data_stride,
                                                         const int32_t* __restrict__ index, int64_t index_stride, int32_t index_mod,
                                                         int32_t channels, const int32_t* __restrict__ n_arr, int32_t n_max, int32_t forced,
                                                         uint8_t* __restrict__ out, int64_t cap, int32_t* __restrict__ out_len,
                                                         int32_t* __restrict__ status, uint8_t* __restrict__ ws, int64_t ws_stride) {
    const int s = (int)blockIdx.x, lane = lane_id();
    int32_t n = n_arr[s];
    int32_t flags = 0;
    if (n < 0 || n > n_max || (channels > 0 && n % channels != 0)) { flags = kBadShape; n = 0; }
    if (n == 0) {
        if (lane == 0) { out_len[s] = 0; status[s] = flags; }
        return;
    }
    data += (int64_t)s * data_stride;
    if (index) index += (int64_t)s * index_stride;
    const Layout lay{channels, channels > 0 ? n / channels : 0};
    uint32_t* bins = (uint32_t*)(ws + (int64_t)s * ws_stride);          // n_max packed bins, then n_max words
    uint16_t* words = (uint16_t*)(bins + n_max);
    uint8_t* o = out + (int64_t)s * cap;

    // pass 1
    int64_t cost = 0, n_esc = 0;
    for (int32_t base = 0; base < n; base += 64) {
        const int32_t i = base + lane;
        if (i < n) {
            const int64_t p = lay.at(i);
            const Bin b = bin_of(t, row_of(t, index, index_mod, i, p, flags), data[p]);
            bins[i] = (b.start << 16) | b.freq;
            cost += cost256(b.freq);
            n_esc += b.escape ? 1 : 0;
        }
    }
    cost = wave_sum(cost);
    n_esc = wave_sum(n_esc);
    const int64_t est = (cost + 2047) >> 11;
    const int L = forced ? forced : lane_rule(est);
    __syncthreads();                                                     // (one wave: orders the bins written above before pass 2 reads them)

    // pass 2: steps descending; the words of step t lie before those of step t + 1, ascending lane order inside a step
    const int32_t steps = (n + L - 1) / L;
    uint32_t x = kLow;
    int32_t wcount = 0;                                                  // words so far; they occupy words[n_max - wcount, n_max)
    for (int32_t tstep = steps - 1; tstep >= 0; --tstep) {
        const int32_t i = tstep * L + lane;
        const bool active = lane < L && i < n;
        const uint32_t sf = active ? bins[i] : 1u;
        const uint32_t f = sf & 0xffffu, start = sf >> 16;
        const bool emit = active && x >= (f << 16);
        const uint64_t mask = __ballot(emit);
        const int k = __popcll(mask);
        if (emit) {
            words[n_max - wcount - k + prefix_rank(mask)] = (uint16_t)x;
            x >>= 16;
        }
        wcount += k;
        if (active) x = ((x / f) << 16) + (x % f) + start;
    }
    __syncthreads();

    // pass 3
    int hdr = 1;
    {
        uint64_t v = (uint64_t)n_esc;
        while (true) {
            const uint8_t b = (uint8_t)(v & 0x7f);
            v >>= 7;
            if (lane == 0) o[hdr] = v ? (uint8_t)(b | 0x80) : b;
            ++hdr;
            if (!v) break;
        }
    }
    if (lane == 0) o[0] = (uint8_t)(31 - __clz(L));
    if (lane < L) put32(o + hdr + 4 * lane, x);
    uint8_t* ow = o + hdr + 4 * L;
    for (int32_t j = lane; j < wcount; j += 64) put16(ow + 2 * (int64_t)j, words[n_max - wcount + j]);
    uint8_t* oe = ow + 2 * (int64_t)wcount;
    int64_t ecur = 0;
    if (n_esc > 0) {
        for (int32_t base = 0; base < n; base += 64) {
            const int32_t i = base + lane;
            bool esc = false;
            int32_t v = 0;
            if (i < n) {
                const int64_t p = lay.at(i);
                v = data[p];
                esc = bin_of(t, row_of(t, index, index_mod, i, p, flags), v).escape;
            }
            const uint64_t mask = __ballot(esc);
            if (esc) put32(oe + 4 * (ecur + prefix_rank(mask)), (uint32_t)v);
            ecur += __popcll(mask);
        }
    }
    flags = wave_or(flags);
    if (lane == 0) {
        out_len[s] = (int32_t)(hdr + 4 * L + 2 * (int64_t)wcount + 4 * n_esc);
        status[s] = flags;
    }
}

}  // namespace

// The header of a string against its length: shared by the host check and the decode kernel.  get(q) returns byte q (q < len is the
// caller's to guarantee: every call below is made under that test).
struct RansHeader { int32_t L, hdr; int64_t n_esc, n_words; };
template <class Get>
__host__ __device__ inline bool rans_parse_header(Get get, int64_t len, int64_t n, RansHeader& h) {
    if (len < 2) return false;
    const uint32_t lg = get(0);
    if (lg > 6) return false;
    h.L = 1 << lg;
    uint64_t esc = 0;
    int shift = 0;
    int64_t pos = 1;
    for (;;) {
        if (pos >= len || shift > 63) return false;
        const uint32_t b = get(pos++);
        esc |= (uint64_t)(b & 0x7f) << shift;
        shift += 7;
        if (b < 0x80) break;
    }
    if (esc > (uint64_t)n) return false;
    const int64_t rest = len - pos - 4 * (int64_t)h.L - 4 * (int64_t)esc;
    if (rest < 0 || (rest & 1) || rest / 2 > n) return false;
    h.hdr = (int32_t)pos;
    h.n_esc = (int64_t)esc;
    h.n_words = rest / 2;
    return true;
}

namespace {

__global__ __launch_bounds__(64) void rans_decode_kernel(DevTable t, const uint8_t* __restrict__ str, const int64_t* __restrict__ off_arr,
                                                         const int32_t* __restrict__ len_arr, int64_t str_bytes,
                                                         const int32_t* __restrict__ index, int64_t index_stride, int32_t index_mod,
                                                         int32_t channels, const int32_t* __restrict__ n_arr, int32_t n_max,
                                                         int32_t* __restrict__ out, int64_t out_stride, int32_t* __restrict__ status) {
    const int s = (int)blockIdx.x, lane = lane_id();
    int32_t n = n_arr[s];
    int32_t flags = 0;
    if (n < 0 || n > n_max || (channels > 0 && n % channels != 0)) { flags = kBadShape; n = 0; }
    const int64_t off = off_arr[s];
    int64_t len = len_arr[s];
    if (off < 0 || len < 0 || off > str_bytes || len > str_bytes - off) { flags |= kCorrupt; len = 0; n = 0; }      // the string inside the buffer
    const uint8_t* sp = str + off;
    RansHeader h{};
    if (n > 0 && !rans_parse_header([&](int64_t q) { return (uint32_t)sp[q]; }, len, n, h)) { flags |= kCorrupt; n = 0; }
    if (n == 0) {
        if (len_arr[s] != 0 && flags == 0) flags = kCorrupt;             // bytes for an empty stream
        if (lane == 0) status[s] = flags;
        return;
    }
    // from here on: hdr + 4 L + 2 n_words + 4 n_esc == len, so states, words [0, n_words) and escapes [0, n_esc) lie inside the string
    if (index) index += (int64_t)s * index_stride;
    out += (int64_t)s * out_stride;
    const Layout lay{channels, channels > 0 ? n / channels : 0};
    const int L = h.L;
    const uint8_t* pw = sp + h.hdr + 4 * L;
    const uint8_t* pe = pw + 2 * h.n_words;
    uint32_t x = kLow;
    if (lane < L) x = get16(sp + h.hdr + 4 * lane) | (get16(sp + h.hdr + 4 * lane + 2) << 16);
    int64_t wcur = 0, ecur = 0;
    const int32_t steps = (n + L - 1) / L;
    for (int32_t tstep = 0; tstep < steps; ++tstep) {
        const int32_t i = tstep * L + lane;
        const bool active = lane < L && i < n;
        bool refill = false, esc = false;
        int64_t p = 0;
        int32_t value = 0;
        if (active) {
            p = lay.at(i);
            const int32_t row = row_of(t, index, index_mod, i, p, flags);
            const int32_t m = t.size[row] - 2, offs = t.offset[row];
            const int32_t* c = t.cdf + (int64_t)row * t.stride;
            const uint32_t slot = x & 0xffffu;
            // the bin of the value 0 first (the mode of every prior in use), else bisection for the last b in [0, m] with c[b] <= slot
            int32_t b = -offs;
            if (b < 0 || b >= m || (uint32_t)c[b] > slot || (uint32_t)c[b + 1] <= slot) {
                int32_t lo = 0, hi = m;
                while (lo < hi) {
                    const int32_t mid = (lo + hi + 1) >> 1;
                    if ((uint32_t)c[mid] <= slot) lo = mid; else hi = mid - 1;
                }
                b = lo;
            }
            const uint32_t start = (uint32_t)c[b], f = (uint32_t)c[b + 1] - start;
            if (slot < start || slot - start >= f) flags |= kCorrupt;   // (a table whose last entry is not 2^16)
            x = f * (x >> 16) + slot - start;
            refill = x < kLow;
            esc = b == m;
            value = b + offs;
        }
        const uint64_t rmask = __ballot(refill);
        if (refill) {
            const int64_t w = wcur + prefix_rank(rmask);
            uint32_t word = 0;
            if (w < h.n_words) word = get16(pw + 2 * w); else flags |= kCorrupt;
            x = (x << 16) | word;
        }
        wcur += __popcll(rmask);
        const uint64_t emask = __ballot(esc);
        if (esc) {
            const int64_t e = ecur + prefix_rank(emask);
            if (e < h.n_esc) value = (int32_t)(get16(pe + 4 * e) | (get16(pe + 4 * e + 2) << 16)); else flags |= kCorrupt;
        }
        ecur += __popcll(emask);
        if (active) out[p] = value;
    }
    if (wcur != h.n_words || ecur != h.n_esc || (lane < L && x != kLow)) flags |= kCorrupt;      // the string ends where its symbols do
    flags = wave_or(flags);
    if (lane == 0) status[s] = flags;
}

// ---- CDF tables on the device: uploaded once per (context, table) and kept.  An entry is found by the host addresses and shape of the
// table and confirmed by comparing the host arrays with the copy taken at upload (a table rebuilt at the same addresses is uploaded again).
struct TableEntry {
    pcc_ctx* ctx;
    const int32_t *cdf, *size, *offset;
    int32_t rows, stride;
    std::vector<int32_t> copy;           // cdf, then cdf_size, then offset
    int32_t* dev;
};
std::mutex g_tables_mu;
std::vector<TableEntry> g_tables;

bool table_valid(const pcc_cdf_table* t) {
    for (int r = 0; r < t->rows; ++r) {
        const int32_t sz = t->cdf_size[r];
        if (sz < 2 || sz > t->cdf_stride) return false;
        const int32_t* c = t->cdf + (size_t)r * t->cdf_stride;
        if (c[0] != 0 || c[sz - 1] != (1 << 16)) return false;
        for (int j = 0; j + 1 < sz; ++j) {
            const int64_t f = (int64_t)c[j + 1] - c[j];
            if (f < 1 || f > 65535) return false;
        }
    }
    return true;
}

int device_table(pcc_ctx* ctx, const pcc_cdf_table* t, DevTable* out, const char* who) {
    PCC_REQUIRE(t && t->cdf && t->cdf_size && t->offset && t->rows > 0 && t->cdf_stride >= 2, "%s: bad table", who);
    PCC_REQUIRE(t->precision == 16, "%s: the rANS coder needs 16-bit probabilities (precision %d)", who, t->precision);
    const size_t n_cdf = (size_t)t->rows * t->cdf_stride, n_all = n_cdf + 2 * (size_t)t->rows;
    std::lock_guard<std::mutex> lk(g_tables_mu);
    TableEntry* e = nullptr;
    for (auto& c : g_tables)
        if (c.ctx == ctx && c.cdf == t->cdf && c.size == t->cdf_size && c.offset == t->offset && c.rows == t->rows && c.stride == t->cdf_stride) e = &c;
    const bool same = e && memcmp(e->copy.data(), t->cdf, n_cdf * 4) == 0 && memcmp(e->copy.data() + n_cdf, t->cdf_size, (size_t)t->rows * 4) == 0 &&
                      memcmp(e->copy.data() + n_cdf + t->rows, t->offset, (size_t)t->rows * 4) == 0;
    if (!same) {
        PCC_REQUIRE(table_valid(t), "%s: every row needs cdf[0] = 0, cdf[size - 1] = 2^16 and frequencies in [1, 65535]", who);
        if (!e) {
            g_tables.push_back(TableEntry{ctx, t->cdf, t->cdf_size, t->offset, t->rows, t->cdf_stride, {}, nullptr});
            e = &g_tables.back();
            PCC_CHECK_HIP(hipMalloc((void**)&e->dev, n_all * 4));
        }
        e->copy.resize(n_all);
        memcpy(e->copy.data(), t->cdf, n_cdf * 4);
        memcpy(e->copy.data() + n_cdf, t->cdf_size, (size_t)t->rows * 4);
        memcpy(e->copy.data() + n_cdf + t->rows, t->offset, (size_t)t->rows * 4);
        PCC_CHECK_HIP(hipMemcpy(e->dev, e->copy.data(), n_all * 4, hipMemcpyHostToDevice));       // (waits for the launches that read the old one)
    }
    *out = DevTable{e->dev, e->dev + n_cdf, e->dev + n_cdf + t->rows, t->rows, t->cdf_stride};
    return PCC_OK;
}

inline size_t ws_stride_of(int64_t n_max) { return ((size_t)n_max * 6 + 15) / 16 * 16; }

}  // namespace

void pcc_rans_free(pcc_ctx* ctx) {
    std::lock_guard<std::mutex> lk(g_tables_mu);
    for (size_t i = g_tables.size(); i-- > 0;)
        if (g_tables[i].ctx == ctx) {
            (void)hipFree(g_tables[i].dev);
            g_tables.erase(g_tables.begin() + (long)i);
        }
}

PCC_API size_t pcc_rans_stream_cap(int64_t n) { return n < 0 ? 0 : 1 + 10 + 4 * (size_t)kMaxLanes + 6 * (size_t)n; }

PCC_API size_t pcc_rans_workspace_bytes(int32_t n_streams, int64_t n_max) {
    return n_streams <= 0 || n_max < 0 ? 0 : (size_t)n_streams * ws_stride_of(n_max);
}

PCC_API int pcc_rans_check_strings(int32_t n_streams, const uint8_t* str, const int64_t* off, const int32_t* len, const int32_t* n) {
    PCC_REQUIRE(n_streams >= 0 && (n_streams == 0 || (str && off && len && n)), "pcc_rans_check_strings: bad argument");
    for (int s = 0; s < n_streams; ++s) {
        PCC_REQUIRE(off[s] >= 0 && len[s] >= 0 && n[s] >= 0, "pcc_rans_check_strings: negative offset, length or symbol count");
        const uint8_t* sp = str + off[s];
        RansHeader h{};
        const bool ok = n[s] == 0 ? len[s] == 0 : rans_parse_header([&](int64_t q) { return (uint32_t)sp[q]; }, len[s], n[s], h);
        if (!ok) {
            pcc_set_error("pcc_rans_check_strings: string %d (%d bytes for %d symbols) does not match its header", s, len[s], n[s]);
            return PCC_ERR_CORRUPT;
        }
    }
    return PCC_OK;
}

static int layout_ok(const char* who, const int32_t* index, int32_t index_mod, int32_t channels, int64_t n_max, int32_t lanes) {
    PCC_REQUIRE(index || index_mod > 0, "%s: index NULL needs index_mod > 0", who);
    PCC_REQUIRE(channels >= 0 && n_max >= 0 && n_max <= (int64_t)1 << 28, "%s: channels %d, n_max %lld", who, channels, (long long)n_max);
    PCC_REQUIRE(lanes >= 0 && lanes <= kMaxLanes && (lanes & (lanes - 1)) == 0, "%s: lanes %d (0 or a power of two <= 64)", who, lanes);
    return PCC_OK;
}

PCC_API int pcc_rans_encode_batch(pcc_ctx* ctx, const pcc_cdf_table* t, int32_t n_streams, const int32_t* data, int64_t data_stride,
                                  const int32_t* index, int64_t index_stride, int32_t index_mod, int32_t channels, const int32_t* n,
                                  int32_t n_max, int32_t lanes, uint8_t* out, size_t cap, int32_t* out_len, int32_t* status,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    PCC_REQUIRE(ctx && n_streams >= 0, "pcc_rans_encode_batch: bad argument");
    DevTable dt;
    if (int rc = device_table(ctx, t, &dt, "pcc_rans_encode_batch")) return rc;
    if (int rc = layout_ok("pcc_rans_encode_batch", index, index_mod, channels, n_max, lanes)) return rc;
    if (n_streams == 0) return PCC_OK;
    PCC_REQUIRE(data && n && out && out_len && status && workspace, "pcc_rans_encode_batch: NULL pointer");
    PCC_REQUIRE(n_streams == 1 || data_stride >= n_max, "pcc_rans_encode_batch: data_stride %lld < n_max %d", (long long)data_stride, n_max);
    PCC_REQUIRE(!index || n_streams == 1 || index_stride == 0 || index_stride >= n_max, "pcc_rans_encode_batch: index_stride %lld < n_max %d",
                (long long)index_stride, n_max);
    if (cap < pcc_rans_stream_cap(n_max) || workspace_bytes < pcc_rans_workspace_bytes(n_streams, n_max)) {
        pcc_set_error("pcc_rans_encode_batch: cap %zu < pcc_rans_stream_cap (%zu) or workspace %zu < pcc_rans_workspace_bytes (%zu)", cap,
                      pcc_rans_stream_cap(n_max), workspace_bytes, pcc_rans_workspace_bytes(n_streams, n_max));
        return PCC_ERR_SPACE;
    }
    hipLaunchKernelGGL(rans_encode_kernel, dim3((unsigned)n_streams), dim3(64), 0, (hipStream_t)stream, dt, data, data_stride, index, index_stride,
                       index_mod, channels, n, n_max, lanes, out, (int64_t)cap, out_len, status, (uint8_t*)workspace, (int64_t)ws_stride_of(n_max));
    PCC_CHECK_HIP(hipGetLastError());
    return PCC_OK;
}

PCC_API int pcc_rans_decode_batch(pcc_ctx* ctx, const pcc_cdf_table* t, int32_t n_streams, const uint8_t* str, size_t str_bytes,
                                  const int64_t* off, const int32_t* len, const int32_t* index, int64_t index_stride, int32_t index_mod,
                                  int32_t channels, const int32_t* n, int32_t n_max, int32_t* out, int64_t out_stride, int32_t* status,
                                  int32_t* status_host, void* stream) {
    PCC_REQUIRE(ctx && n_streams >= 0, "pcc_rans_decode_batch: bad argument");
    DevTable dt;
    if (int rc = device_table(ctx, t, &dt, "pcc_rans_decode_batch")) return rc;
    if (int rc = layout_ok("pcc_rans_decode_batch", index, index_mod, channels, n_max, 0)) return rc;
    if (n_streams == 0) return PCC_OK;
    PCC_REQUIRE(str && off && len && n && out && status, "pcc_rans_decode_batch: NULL pointer");
    PCC_REQUIRE(n_streams == 1 || out_stride >= n_max, "pcc_rans_decode_batch: out_stride %lld < n_max %d", (long long)out_stride, n_max);
    PCC_REQUIRE(!index || n_streams == 1 || index_stride == 0 || index_stride >= n_max, "pcc_rans_decode_batch: index_stride %lld < n_max %d",
                (long long)index_stride, n_max);
    hipLaunchKernelGGL(rans_decode_kernel, dim3((unsigned)n_streams), dim3(64), 0, (hipStream_t)stream, dt, str, off, len, (int64_t)str_bytes, index,
                       index_stride, index_mod, channels, n, n_max, out, out_stride, status);
    PCC_CHECK_HIP(hipGetLastError());
    if (status_host) {
        PCC_CHECK_HIP(hipMemcpyAsync(status_host, status, (size_t)n_streams * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
        PCC_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
        for (int s = 0; s < n_streams; ++s) {
            if (status_host[s] & (kBadRow | kBadShape)) {
                pcc_set_error("pcc_rans_decode_batch: stream %d: CDF row out of range or symbol count not a multiple of the channels", s);
                return PCC_ERR_ARG;
            }
            if (status_host[s]) { pcc_set_error("pcc_rans_decode_batch: string %d is corrupt", s); return PCC_ERR_CORRUPT; }
        }
    }
    return PCC_OK;
}
