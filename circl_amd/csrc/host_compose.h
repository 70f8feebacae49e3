// host_compose.h -- the small host-side helpers every api_*.hip unit needs around its launches, defined once: argument tests, launch
// geometry, the workspace and pipeline rules that recur, error propagation, the carving of a chunk's workspace and the strided
// device-to-device copy of the schemes that are composed of two others (eddilithium.h).  Host only; no kernel lives here.
// Everything has internal linkage: the library exports its C ABI, not its plumbing.
#pragma once
#include "host_common.h"

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

// host-side check of a key-index vector (the device path trusts its caller: an out-of-range index would read past the table).
// key_idx is not NULL here: what an absent vector means, and which nkeys are valid at all, is the calling entry point's rule.
static inline int check_key_idx(const uint32_t *key_idx, size_t n, size_t nkeys) {
    for (size_t i = 0; i < n; i++)
        if (key_idx[i] >= nkeys) return CIRCL_HIP_EPARAM;
    return CIRCL_HIP_OK;
}

}  // namespace host
}  // namespace circl
