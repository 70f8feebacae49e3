// host_compose.h -- the small host-side helpers every api_*.hip unit needs around its launches, defined once: argument tests, launch
// geometry, the workspace and pipeline rules that recur, error propagation, the carving of a chunk's workspace and the strided
// device-to-device copy of the schemes that are composed of two others (eddilithium.h).  Host only; no kernel lives here.
// Everything has internal linkage: the library exports its C ABI, not its plumbing.
#pragma once
#include "host_common.h"
#include <type_traits>

namespace circl {
namespace host {

// every pointer is a multiple of N bytes (a NULL pointer is: the optional arrays of the entry points rely on it)
template <size_t N, class... P> static inline bool aligned(P... p) {
    static_assert(N && !(N & (N - 1)), "a power of two");
    return ((reinterpret_cast<uintptr_t>(static_cast<const void *>(p)) | ...) & (N - 1)) == 0;
}

// the grid of a kernel that gives item (or word) i to thread i of blocks of `block` threads
static inline dim3 lanes_grid(size_t n, unsigned block = 64) { return dim3((unsigned)((n + block - 1) / block)); }

// the workspace rule of a launch that needs none
static const std::function<size_t(size_t)> kNoWs = [](size_t) { return size_t(0); };

// pipeline options of a call whose rows are secret (seeds, private keys, shared secrets): the device staging of every chunk is zeroed
static inline PipeOpts secret_opts(size_t chunk_items) {
    PipeOpts o;
    o.chunk_items = host_chunk_items(chunk_items);
    o.wipe_device = true;
    return o;
}

#define TRY(expr)                            \
    do {                                     \
        const int rc_ = (expr);              \
        if (rc_ != CIRCL_HIP_OK) return rc_; \
    } while (0)

// consecutive 256-byte-aligned regions of a workspace
struct Carve {
    uint8_t *base;
    size_t at = 0;
    uint8_t *take(size_t bytes) {
        uint8_t *p = base + at;
        at += up256(bytes);
        return p;
    }
    uint8_t *rest() const { return base + at; }                      // what no take() has claimed yet ...
    size_t left(size_t ws_bytes) const { return ws_bytes - at; }     // ... and how much of a workspace of ws_bytes that is
};

// Strided device-to-device copy on the copy engine (hipMemcpy2DAsync), byte-granular: columns [src_col, src_col + w) of rows of
// src_pitch -> columns [dst_col, ..) of rows of dst_pitch.  (api_hybrid.hip copies its word-aligned rows with a kernel instead.)
static inline int copy_rows_2d(uint8_t *dst, size_t dst_pitch, size_t dst_col, const uint8_t *src, size_t src_pitch, size_t src_col, size_t w, size_t rows,
                        hipStream_t st) {
    HIP_TRY(hipMemcpy2DAsync(dst + dst_col, dst_pitch, src + src_col, src_pitch, w, rows, hipMemcpyDeviceToDevice, st));
    return CIRCL_HIP_OK;
}

// ---- the staged arrays of a host form, each declared once --------------------------------------------------------------------------
// A unit's Call holds its arrays as the ABI passes them.  Inside shard's callback a Bind takes ONE declaration per array -- the field
// by pointer-to-member and how it is staged -- and from it makes both the HIn / HBlob / HOut record of items [lo, ..) for run_pipeline
// and the way back: on(k) is the copy of the call whose declared fields are the chunk's device pointers and whose item count is the
// chunk's.  A declared array that is absent (a NULL pointer, or take / want false: this operation has no such array) is nullptr in
// that copy, the offsets field of an absent blob included: a host pointer never reaches a launch through a declared field.  Fields
// that are not declared (strides, flags, bytes the launch copies into the kernel arguments) pass through as they are.
template <class Call> struct Bind {
    std::vector<HIn> ins;
    std::vector<HBlob> blobs;
    std::vector<HOut> outs;

    Bind(const Call &c, size_t lo, size_t Call::*n = &Call::n) : c(c), lo(lo), n(n) { static_assert(std::is_trivially_copyable<Call>::value, "on() copies it"); }

    // rows of `row` bytes: + lo * row; shared: ONE row for the whole call, staged with every chunk (HIn::per_call)
    template <class T> void rows(T *Call::*m, size_t row, bool secret, bool shared = false, bool take = true) {
        const uint8_t *p = take ? reinterpret_cast<const uint8_t *>(c.*m) : nullptr;
        if (p) {
            HIn in = {p + (shared ? 0 : lo * row), row, secret};
            in.per_call = shared;
            ins.push_back(in);
        }
        bind(m, kIn, p ? (int)ins.size() - 1 : -1);
    }
    // ragged rows over offsets, each `pad` bytes longer than they say: + pad * lo, off + lo
    void blob(const uint8_t *Call::*m, const uint64_t *Call::*off, bool secret, size_t pad = 0, bool take = true) {
        const bool have = take && c.*m && c.*off;
        if (have) blobs.push_back({c.*m + pad * lo, c.*off + lo, secret, pad});
        bind(m, kBlob, have ? (int)blobs.size() - 1 : -1);
        bind(off, kOff, have ? (int)blobs.size() - 1 : -1);
    }
    // output rows; a wanted one whose host pointer is NULL still gets its device buffer, and nothing is copied back
    void out(uint8_t *Call::*m, size_t row, bool secret, bool want = true) {
        if (want) outs.push_back({c.*m ? c.*m + lo * row : nullptr, row, secret});
        bind(m, kOut, want ? (int)outs.size() - 1 : -1);
    }
    // a ragged output over the offsets of a blob that this call declares too (that declaration binds the offsets field)
    void ragged(uint8_t *Call::*m, const uint64_t *Call::*off, bool secret, size_t pad) {
        outs.push_back({c.*m + pad * lo, 0, secret, c.*off + lo, pad});
        bind(m, kOut, (int)outs.size() - 1);
    }

    Call on(const Chunk &k) const {
        Call d = c;
        for (const Rec &r : recs) {
            const void *p = r.idx < 0 ? nullptr : r.kind == kIn ? k.in[r.idx] : r.kind == kBlob ? k.blob[r.idx] : r.kind == kOff ? (const void *)k.off[r.idx] : k.out[r.idx];
            memcpy(reinterpret_cast<char *>(&d) + r.at, &p, sizeof p);
        }
        d.*n = k.cnt;
        return d;
    }

private:
    enum Kind { kIn, kBlob, kOff, kOut };
    struct Rec { size_t at; Kind kind; int idx; };   // the field's place in the Call, the Chunk vector it is filled from, the index there (-1: absent)
    const Call &c;
    size_t lo;
    size_t Call::*n;
    std::vector<Rec> recs;
    template <class T> void bind(T *Call::*m, Kind kind, int idx) {
        static_assert(sizeof(T *) == sizeof(void *), "every data pointer has one representation");
        recs.push_back({size_t(reinterpret_cast<const char *>(&(c.*m)) - reinterpret_cast<const char *>(&c)), kind, idx});
    }
};

// what an entry point does with its filled Call: the argument contract, nothing for an empty batch, then one launch on the caller's
// device pointers or the host pipeline.  check / launch / host_pipeline are the unit's own, found through the Call's namespace.
template <class Call> static int run_call(const Call &c, bool dev, int device, void *stream) {
    if (int rc = check(c)) return rc;
    if (c.n == 0) return CIRCL_HIP_OK;
    return dev ? launch(c, static_cast<hipStream_t>(stream)) : host_pipeline(c, device);
}

// both forms of one entry point: NAME(params..., n, int device) and NAME_dev(params..., n, void *stream)
#define BOTH_FORMS(NAME, PARAMS, BODY)                                        \
    int NAME(PARAMS, size_t n, int device) {                                  \
        const bool dev_ = false;                                              \
        void *stream = nullptr;                                               \
        BODY                                                                  \
    }                                                                         \
    int NAME##_dev(PARAMS, size_t n, void *stream) {                          \
        const bool dev_ = true;                                               \
        const int device = 0;                                                 \
        BODY                                                                  \
    }
#define P(...) __VA_ARGS__

// host-side check of a key-index vector (the device path trusts its caller: an out-of-range index would read past the table).
// key_idx is not NULL here: what an absent vector means, and which nkeys are valid at all, is the calling entry point's rule.
static inline int check_key_idx(const uint32_t *key_idx, size_t n, size_t nkeys) {
    for (size_t i = 0; i < n; i++)
        if (key_idx[i] >= nkeys) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

}  // namespace host
}  // namespace circl
