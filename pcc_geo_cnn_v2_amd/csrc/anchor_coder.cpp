// Adaptive binary range coder of the octree anchor codec (include/pcc_geo.h "octree anchor"), host only.
//
// The coder is the LZMA one: 11-bit probabilities of a zero starting at 1024 and moving by 1/32 of the distance per decision, a
// 32-bit range kept at or above 2^24 by shifting bytes out, a 33-bit `low` whose carry travels through the cache byte and the run of
// 0xff bytes held back behind it.  The encoder ends with five shifts; the decoder starts with five reads, so a stream of N
// normalisations is N + 5 bytes on both sides and a decoder that wants a byte past the end has met a cut or damaged stream.
//
// On top of it, an occupancy byte (never 0) is eight binary decisions, child 0 first.  Decision c uses model 256 * t + m: m = the
// binary-tree node of the bits already coded in this byte (1, then 2m + bit: 255 values), t = three bits of the node's face-neighbour
// mask n6 (bit 0 / 1: the -x / +x neighbour, 2 / 3: -y / +y, 4 / 5: -z / +z) -- the neighbours across the three outer faces of
// child c's octant: bit (c >> 2 & 1) of the x pair, (c >> 1 & 1) of the y pair, (c & 1) of the z pair.  After seven zeros the
// eighth decision is a one and is not coded.  This file shares nothing with range_coder.cpp (table-driven, multi-symbol).
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/pcc_geo.h"

void pcc_set_error(const char* fmt, ...);
#define PCC_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kProbBits = 11, kMoveBits = 5;
constexpr uint32_t kTop = 1u << 24;
constexpr int kModels = 8 * 256;                  // 256 * t + m, m = 1 .. 255 (m = 0 unused)

struct Encoder {
    uint64_t low = 0;
    uint32_t range = 0xffffffffu;
    uint8_t cache = 0;
    int64_t cache_size = 1;
    uint8_t* out;
    int64_t cap, len = 0;
    bool overflow = false;

    Encoder(uint8_t* o, int64_t c) : out(o), cap(c) {}
    void put(uint8_t b) {
        if (len < cap) out[len] = b; else overflow = true;
        ++len;
    }
    void shift_low() {
        if ((uint32_t)low < 0xff000000u || (low >> 32) != 0) {
            const uint8_t carry = (uint8_t)(low >> 32);
            uint8_t b = cache;
            do {
                put((uint8_t)(b + carry));
                b = 0xff;
            } while (--cache_size != 0);
            cache = (uint8_t)(low >> 24);
        }
        ++cache_size;
        low = (low & 0x00ffffffu) << 8;
    }
    void encode(uint16_t& p, int bit) {
        const uint32_t bound = (range >> kProbBits) * p;
        if (bit == 0) {
            range = bound;
            p = (uint16_t)(p + (((1u << kProbBits) - p) >> kMoveBits));
        } else {
            low += bound;
            range -= bound;
            p = (uint16_t)(p - (p >> kMoveBits));
        }
        while (range < kTop) {
            range <<= 8;
            shift_low();
        }
    }
    void finish() {
        for (int i = 0; i < 5; ++i) shift_low();
    }
};

struct Decoder {
    const uint8_t* in = nullptr;
    int64_t len = 0, pos = 0;
    uint32_t range = 0xffffffffu, code = 0;
    bool past_end = false;
    int32_t flags = 0;
    uint16_t probs[kModels];

    uint8_t get() {
        if (pos < len) return in[pos++];
        past_end = true;
        return 0;
    }
    void init(const uint8_t* data, int64_t n, int32_t f) {
        in = data; len = n; pos = 0; range = 0xffffffffu; code = 0; past_end = false; flags = f;
        for (int i = 0; i < kModels; ++i) probs[i] = 1u << (kProbBits - 1);
        uint8_t first = get();
        for (int i = 0; i < 4; ++i) code = code << 8 | get();
        if (first != 0) past_end = true;              // the encoder's first byte is its initial cache byte: always 0
    }
    int decode(uint16_t& p) {
        const uint32_t bound = (range >> kProbBits) * p;
        int bit;
        if (code < bound) {
            range = bound;
            p = (uint16_t)(p + (((1u << kProbBits) - p) >> kMoveBits));
            bit = 0;
        } else {
            code -= bound;
            range -= bound;
            p = (uint16_t)(p - (p >> kMoveBits));
            bit = 1;
        }
        while (range < kTop) {
            range <<= 8;
            code = code << 8 | get();
        }
        return bit;
    }
};

inline int tbits(int n6, int c) { return (n6 >> (c >> 2 & 1) & 1) | (n6 >> (2 + (c >> 1 & 1)) & 1) << 1 | (n6 >> (4 + (c & 1)) & 1) << 2; }

}  // namespace

/* raw decisions: model[i] in [0, 2048), bit[i] in {0, 1} */
PCC_API int pcc_anchor_code_bits(const uint16_t* model, const uint8_t* bit, int64_t n, uint8_t* out, int64_t cap, int64_t* out_len) {
    if (n < 0 || cap < 0 || !out_len || (n > 0 && (!model || !bit))) { pcc_set_error("pcc_anchor_code_bits: bad argument"); return PCC_ERR_ARG; }
    uint16_t probs[kModels];
    for (int i = 0; i < kModels; ++i) probs[i] = 1u << (kProbBits - 1);
    Encoder e(out, cap);
    for (int64_t i = 0; i < n; ++i) {
        if (model[i] >= kModels || bit[i] > 1) { pcc_set_error("pcc_anchor_code_bits: decision %lld out of range", (long long)i); return PCC_ERR_ARG; }
        e.encode(probs[model[i]], bit[i]);
    }
    e.finish();
    *out_len = e.len;
    if (e.overflow) { pcc_set_error("pcc_anchor_code_bits: %lld bytes do not fit %lld", (long long)e.len, (long long)cap); return PCC_ERR_SPACE; }
    return PCC_OK;
}

PCC_API int pcc_anchor_decode_bits(const uint8_t* data, int64_t len, const uint16_t* model, int64_t n, uint8_t* bit) {
    if (n < 0 || len < 0 || (len > 0 && !data) || (n > 0 && (!model || !bit))) { pcc_set_error("pcc_anchor_decode_bits: bad argument"); return PCC_ERR_ARG; }
    Decoder* d = new (std::nothrow) Decoder;
    if (!d) { pcc_set_error("pcc_anchor_decode_bits: out of memory"); return PCC_ERR_SPACE; }
    d->init(data, len, 0);
    int rc = PCC_OK;
    for (int64_t i = 0; i < n && rc == PCC_OK; ++i) {
        if (model[i] >= kModels) { pcc_set_error("pcc_anchor_decode_bits: model %lld out of range", (long long)i); rc = PCC_ERR_ARG; break; }
        bit[i] = (uint8_t)d->decode(d->probs[model[i]]);
        if (d->past_end) { pcc_set_error("pcc_anchor_decode_bits: the stream ends inside decision %lld", (long long)i); rc = PCC_ERR_CORRUPT; }
    }
    if (rc == PCC_OK && d->past_end) { pcc_set_error("pcc_anchor_decode_bits: the stream is cut or does not start with a zero byte"); rc = PCC_ERR_CORRUPT; }
    delete d;
    return rc;
}

/* all occupancy bytes of a tree, breadth first, in one coder run */
PCC_API int pcc_anchor_encode(const uint8_t* occ, const uint8_t* n6, int64_t n, int32_t flags, uint8_t* out, int64_t cap, int64_t* out_len) {
    if (n < 0 || cap < 0 || !out_len || (n > 0 && (!occ || !n6)) || (flags & ~PCC_ANCHOR_NO_CONTEXT)) {
        pcc_set_error("pcc_anchor_encode: bad argument");
        return PCC_ERR_ARG;
    }
    uint16_t probs[kModels];
    for (int i = 0; i < kModels; ++i) probs[i] = 1u << (kProbBits - 1);
    Encoder e(out, cap);
    const bool ctx = !(flags & PCC_ANCHOR_NO_CONTEXT);
    for (int64_t i = 0; i < n; ++i) {
        const int b = occ[i], nb = ctx ? (n6[i] & 63) : 0;
        if (b == 0) { pcc_set_error("pcc_anchor_encode: node %lld has no child", (long long)i); return PCC_ERR_ARG; }
        int m = 1;
        for (int c = 0; c < 8; ++c) {
            if (c == 7 && m == 128) break;            // seven zeros: the eighth is a one
            const int bit = b >> c & 1;
            e.encode(probs[256 * tbits(nb, c) + m], bit);
            m = 2 * m + bit;
        }
    }
    e.finish();
    *out_len = e.len;
    if (e.overflow) { pcc_set_error("pcc_anchor_encode: %lld bytes do not fit %lld", (long long)e.len, (long long)cap); return PCC_ERR_SPACE; }
    return PCC_OK;
}

PCC_API size_t pcc_anchor_decoder_bytes(void) { return sizeof(Decoder); }

/* state: pcc_anchor_decoder_bytes() bytes owned by the caller; data must outlive the last pcc_anchor_decode_level */
PCC_API int pcc_anchor_decoder_init(void* state, const uint8_t* data, int64_t len, int32_t flags) {
    if (!state || len < 0 || (len > 0 && !data) || (flags & ~PCC_ANCHOR_NO_CONTEXT)) { pcc_set_error("pcc_anchor_decoder_init: bad argument"); return PCC_ERR_ARG; }
    Decoder* d = new (state) Decoder;
    d->init(data, len, flags);
    if (d->past_end) { pcc_set_error("pcc_anchor_decoder_init: the payload is shorter than five bytes or does not start with a zero byte"); return PCC_ERR_CORRUPT; }
    return PCC_OK;
}

PCC_API int pcc_anchor_decode_level(void* state, const uint8_t* n6, int64_t n, uint8_t* occ) {
    if (!state || n < 0 || (n > 0 && (!n6 || !occ))) { pcc_set_error("pcc_anchor_decode_level: bad argument"); return PCC_ERR_ARG; }
    Decoder* d = (Decoder*)state;
    const bool ctx = !(d->flags & PCC_ANCHOR_NO_CONTEXT);
    for (int64_t i = 0; i < n; ++i) {
        const int nb = ctx ? (n6[i] & 63) : 0;
        int m = 1;
        for (int c = 0; c < 8; ++c) {
            if (c == 7 && m == 128) { m = 257; break; }
            m = 2 * m + d->decode(d->probs[256 * tbits(nb, c) + m]);
        }
        if (d->past_end) { pcc_set_error("pcc_anchor_decode_level: the stream ends inside node %lld of this level", (long long)i); return PCC_ERR_CORRUPT; }
        // m = 256 + the bits with child 0 first as the HIGHEST bit: reverse them into bit c = child c
        int b = 0;
        for (int c = 0; c < 8; ++c) b |= (m >> (7 - c) & 1) << c;
        occ[i] = (uint8_t)b;
    }
    return PCC_OK;
}

/* bytes of the payload read so far (the whole payload once the last level is decoded) */
PCC_API int64_t pcc_anchor_decoder_consumed(const void* state) { return state ? ((const Decoder*)state)->pos : -1; }

/* ---- vertex payload of the surface anchor (include/pcc_geo.h "surface anchor"): one coder run over the edge list.  Per
 * edge: the flag under model 2 a + prev (a = the edge's axis = key & 3, prev = the previous edge's flag, 0 at the start); behind a set
 * flag the k bits of t, most significant first, under model 8 + m, m = 1 then 2 m + bit.  The decisions depend on decoded bits, so
 * this pair cannot go through pcc_anchor_decode_bits. */
namespace {
constexpr int kSurfaceFlagModels = 8;
bool surface_args_ok(const uint64_t* keys, int64_t n, int32_t k) { return n >= 0 && k >= 2 && k <= 6 && (n == 0 || keys); }
}  // namespace

PCC_API int pcc_surface_encode_vertices(const uint64_t* edge_keys, const uint8_t* flags, const uint8_t* t, int64_t nedges, int32_t k, uint8_t* out,
                                        int64_t cap, int64_t* out_len) {
    if (!surface_args_ok(edge_keys, nedges, k) || cap < 0 || !out_len || (nedges > 0 && (!flags || !t))) {
        pcc_set_error("pcc_surface_encode_vertices: bad argument");
        return PCC_ERR_ARG;
    }
    uint16_t probs[kModels];
    for (int i = 0; i < kModels; ++i) probs[i] = 1u << (kProbBits - 1);
    Encoder e(out, cap);
    int prev = 0;
    for (int64_t i = 0; i < nedges; ++i) {
        const int a = (int)(edge_keys[i] & 3), f = flags[i];
        if (a > 2 || f > 1 || (f && t[i] >= (1 << k))) { pcc_set_error("pcc_surface_encode_vertices: edge %lld out of range", (long long)i); return PCC_ERR_ARG; }
        e.encode(probs[2 * a + prev], f);
        if (f) {
            int m = 1;
            for (int b = k - 1; b >= 0; --b) {
                const int bit = t[i] >> b & 1;
                e.encode(probs[kSurfaceFlagModels + m], bit);
                m = 2 * m + bit;
            }
        }
        prev = f;
    }
    e.finish();
    *out_len = e.len;
    if (e.overflow) { pcc_set_error("pcc_surface_encode_vertices: %lld bytes do not fit %lld", (long long)e.len, (long long)cap); return PCC_ERR_SPACE; }
    return PCC_OK;
}

/* flags[nedges], t[nedges] (0 where the flag is 0); *nflags = the set flags, *consumed = the bytes of data read (the whole payload for a sound one) */
PCC_API int pcc_surface_decode_vertices(const uint8_t* data, int64_t len, const uint64_t* edge_keys, int64_t nedges, int32_t k, uint8_t* flags,
                                        uint8_t* t, int64_t* nflags, int64_t* consumed) {
    if (!surface_args_ok(edge_keys, nedges, k) || len < 0 || (len > 0 && !data) || !nflags || !consumed || (nedges > 0 && (!flags || !t))) {
        pcc_set_error("pcc_surface_decode_vertices: bad argument");
        return PCC_ERR_ARG;
    }
    Decoder* d = new (std::nothrow) Decoder;
    if (!d) { pcc_set_error("pcc_surface_decode_vertices: out of memory"); return PCC_ERR_SPACE; }
    d->init(data, len, 0);
    int rc = PCC_OK, prev = 0;
    int64_t set = 0;
    if (d->past_end) { pcc_set_error("pcc_surface_decode_vertices: the payload is shorter than five bytes or does not start with a zero byte"); rc = PCC_ERR_CORRUPT; }
    for (int64_t i = 0; i < nedges && rc == PCC_OK; ++i) {
        const int a = (int)(edge_keys[i] & 3);
        if (a > 2) { pcc_set_error("pcc_surface_decode_vertices: edge %lld has axis 3", (long long)i); rc = PCC_ERR_ARG; break; }
        const int f = d->decode(d->probs[2 * a + prev]);
        int v = 0;
        if (f) {
            int m = 1;
            for (int b = 0; b < k; ++b) m = 2 * m + d->decode(d->probs[kSurfaceFlagModels + m]);
            v = m - (1 << k);
            ++set;
        }
        if (d->past_end) { pcc_set_error("pcc_surface_decode_vertices: the stream ends inside edge %lld", (long long)i); rc = PCC_ERR_CORRUPT; break; }
        flags[i] = (uint8_t)f;
        t[i] = (uint8_t)v;
        prev = f;
    }
    *nflags = set;
    *consumed = d->pos;
    delete d;
    return rc;
}

/* ---- coefficient payload of the colour anchor (include/pcc_geo.h "colour anchor"): one coder run over the coefficients
 * in coding order -- steps descending (counts[s] coefficients at step s), three channels Y, Co, Cg each.  g = 2 min(s / 3, 7) + (channel
 * != Y).  Zero flag (1 = nonzero) under model 32 g + z, z = the previous coefficient of the same channel was nonzero; behind a set
 * flag the sign (1 = negative) under 32 g + 2, then v = |c| in [1, 512): n = bit_length(v) - 1 one-bits and a zero-bit, prefix bit
 * j under 32 g + 3 + j, then the n low bits of v, most significant first, suffix bit j under 32 g + 12 + j. */
namespace {
constexpr int kColorSteps = 63, kColorMaxPrefix = 8;
bool color_counts_ok(const int64_t* counts, int32_t nsteps, int64_t ncoef) {
    if (nsteps < 0 || nsteps > kColorSteps || ncoef < 0 || (nsteps > 0 && !counts)) return false;
    int64_t sum = 0;
    for (int s = 0; s < nsteps; ++s) {
        if (counts[s] < 0 || counts[s] > ncoef) return false;
        sum += counts[s];
    }
    return sum == ncoef;
}
inline int color_group(int s, int ch) { return 2 * (s / 3 < 7 ? s / 3 : 7) + (ch != 0); }
}  // namespace

/* coef[3 ncoef] int16 in coding order, |c| < 512 */
PCC_API int pcc_color_anchor_encode(const int16_t* coef, int64_t ncoef, const int64_t* counts, int32_t nsteps, uint8_t* out, int64_t cap,
                                    int64_t* out_len) {
    if (!color_counts_ok(counts, nsteps, ncoef) || cap < 0 || !out_len || (ncoef > 0 && !coef) || (cap > 0 && !out)) {
        pcc_set_error("pcc_color_anchor_encode: bad argument");
        return PCC_ERR_ARG;
    }
    uint16_t probs[kModels];
    for (int i = 0; i < kModels; ++i) probs[i] = 1u << (kProbBits - 1);
    Encoder e(out, cap);
    int prev[3] = {0, 0, 0};
    int64_t i = 0;
    for (int s = nsteps - 1; s >= 0; --s)
        for (int64_t k = 0; k < counts[s]; ++k, ++i)
            for (int ch = 0; ch < 3; ++ch) {
                const int c = coef[3 * i + ch], v = c < 0 ? -c : c, m = 32 * color_group(s, ch);
                if (v >= (2 << kColorMaxPrefix)) { pcc_set_error("pcc_color_anchor_encode: coefficient %lld is %d", (long long)i, c); return PCC_ERR_ARG; }
                e.encode(probs[m + prev[ch]], v != 0);
                prev[ch] = v != 0;
                if (!v) continue;
                e.encode(probs[m + 2], c < 0);
                int n = 0;
                while ((v >> (n + 1)) != 0) ++n;
                for (int j = 0; j < n; ++j) e.encode(probs[m + 3 + j], 1);
                e.encode(probs[m + 3 + n], 0);
                for (int j = 0; j < n; ++j) e.encode(probs[m + 12 + j], v >> (n - 1 - j) & 1);
            }
    e.finish();
    *out_len = e.len;
    if (e.overflow) { pcc_set_error("pcc_color_anchor_encode: %lld bytes do not fit %lld", (long long)e.len, (long long)cap); return PCC_ERR_SPACE; }
    return PCC_OK;
}

/* *consumed = the bytes of data read (the whole payload for a sound one) */
PCC_API int pcc_color_anchor_decode(const uint8_t* data, int64_t len, const int64_t* counts, int32_t nsteps, int16_t* coef, int64_t ncoef,
                                    int64_t* consumed) {
    if (!color_counts_ok(counts, nsteps, ncoef) || len < 0 || (len > 0 && !data) || !consumed || (ncoef > 0 && !coef)) {
        pcc_set_error("pcc_color_anchor_decode: bad argument");
        return PCC_ERR_ARG;
    }
    Decoder* d = new (std::nothrow) Decoder;
    if (!d) { pcc_set_error("pcc_color_anchor_decode: out of memory"); return PCC_ERR_SPACE; }
    d->init(data, len, 0);
    int rc = PCC_OK, prev[3] = {0, 0, 0};
    if (d->past_end) { pcc_set_error("pcc_color_anchor_decode: the payload is shorter than five bytes or does not start with a zero byte"); rc = PCC_ERR_CORRUPT; }
    int64_t i = 0;
    for (int s = nsteps - 1; s >= 0 && rc == PCC_OK; --s)
        for (int64_t k = 0; k < counts[s] && rc == PCC_OK; ++k, ++i)
            for (int ch = 0; ch < 3 && rc == PCC_OK; ++ch) {
                const int m = 32 * color_group(s, ch);
                int c = 0;
                const int nz = d->decode(d->probs[m + prev[ch]]);
                prev[ch] = nz;
                if (nz) {
                    const int neg = d->decode(d->probs[m + 2]);
                    int n = 0;
                    while (n <= kColorMaxPrefix && d->decode(d->probs[m + 3 + n])) ++n;
                    if (n > kColorMaxPrefix) {
                        pcc_set_error("pcc_color_anchor_decode: coefficient %lld has a prefix of more than %d ones", (long long)i, kColorMaxPrefix);
                        rc = PCC_ERR_CORRUPT;
                        break;
                    }
                    int v = 1;
                    for (int j = 0; j < n; ++j) v = 2 * v + d->decode(d->probs[m + 12 + j]);
                    c = neg ? -v : v;
                }
                if (d->past_end) { pcc_set_error("pcc_color_anchor_decode: the stream ends inside coefficient %lld", (long long)i); rc = PCC_ERR_CORRUPT; break; }
                coef[3 * i + ch] = (int16_t)c;
            }
    *consumed = d->pos;
    delete d;
    return rc;
}
