// prio3_xof_dev.h -- XofTurboShake128 of draft-irtf-cfrg-vdaf-13 (the reference's vdaf/prio3/internal/prio3/xof.go) and the rejection
// sampler into Field64 (arith/fp64/vector.go RandomSHA3), one stream per lane, over the 12-round permutation of keccak_dev.h.
//
//   stream = TurboSHAKE128(D = 0x01) over  header || seed[32] || binder,   header = LE16(len dst) || dst || 0x20,
//   dst = 0x0c || 0x00 || BE32(algorithm id) || BE16(usage) || ctx
//
// The header is a task parameter: the host builds it once (usage left zero) and it travels to the kernel by value; a stream patches
// the usage in.  Everything that steers the absorb loop -- the lengths, the usage, which binder -- is public and the same in every lane;
// the seed and the nonce are per lane.  The message is gathered a byte at a time into the lane's block buffer (21 words, in LDS on
// the device: word k of lane l at k * stride + l, conflict-free) and XORed into the state from there with constant indices, so the
// state stays in registers; a squeezed block goes out through the same buffer, and the sampler reads its 8-byte words from it with a
// running index.  168 is a multiple of 8: no sample straddles a block.
#pragma once
#include "fp64_dev.h"
#include "keccak_dev.h"

namespace circl {
namespace prio3 {

constexpr int RATE_WORDS = 21, RATE = 8 * RATE_WORDS;
constexpr int SEED = 32, NONCE = 16, MAX_CTX = 255, MAX_TRIES = 10;
constexpr int HEADER_MAX = 2 + 8 + MAX_CTX + 1;
constexpr int USAGE_AT = 2 + 6;   // BE16(usage) inside the header

enum Usage : uint32_t { MEAS_SHARE = 1, PROOF_SHARE = 2, PROVE_RAND = 4, QUERY_RAND = 5 };

struct Header {
    uint8_t b[HEADER_MAX + 6];   // (a multiple of 8 bytes)
    uint32_t len;
};

// what a header holds for algorithm id `kind` and context ctx[ctx_len], ctx_len <= MAX_CTX
static inline Header make_header(uint32_t kind, const uint8_t *ctx, size_t ctx_len) {
    Header h = {};
    const uint32_t dst = 8 + (uint32_t)ctx_len;
    uint8_t *p = h.b;
    *p++ = (uint8_t)dst; *p++ = (uint8_t)(dst >> 8);
    *p++ = 12; *p++ = 0;
    *p++ = (uint8_t)(kind >> 24); *p++ = (uint8_t)(kind >> 16); *p++ = (uint8_t)(kind >> 8); *p++ = (uint8_t)kind;
    *p++ = 0; *p++ = 0;
    for (size_t i = 0; i < ctx_len; i++) *p++ = ctx[i];
    *p++ = SEED;
    h.len = (uint32_t)(p - h.b);
    return h;
}

// element j of a lane's array: lane-interleaved on the device (stride = lanes), dense on the host
struct Strided {
    uint64_t *p;
    size_t stride;
    CIRCL_HD uint64_t &operator[](size_t j) const { return p[j * stride]; }
    CIRCL_HD Strided from(size_t j) const { return Strided{p + j * stride, stride}; }
};

// one stream's input: header (usage patched) || seed || nb binder bytes (b0, b1) || tail[NONCE] (nullptr: none)
struct Msg {
    const Header *h;
    uint32_t usage;
    const uint8_t *seed;
    uint32_t nb;
    uint8_t b0, b1;
    const uint8_t *tail;
    CIRCL_HD uint32_t len() const { return h->len + SEED + nb + (tail ? NONCE : 0); }
    // byte `pos` of the padded message: the message, then the domain byte 0x01, then zeros
    CIRCL_HD uint8_t at(uint32_t pos) const {
        if (pos < h->len) return pos == USAGE_AT + 1 ? (uint8_t)usage : h->b[pos];
        pos -= h->len;
        if (pos < (uint32_t)SEED) return seed[pos];
        pos -= SEED;
        if (pos < nb) return pos == 0 ? b0 : b1;
        pos -= nb;
        if (tail && pos < (uint32_t)NONCE) return tail[pos];
        return pos == (tail ? (uint32_t)NONCE : 0u) ? 0x01 : 0x00;
    }
};

struct Xof {
    KeccakState s;
    Strided blk;    // RATE_WORDS words of this lane
    uint32_t next;  // the next unread word of blk

    CIRCL_HD explicit Xof(Strided blk) : blk(blk), next(RATE_WORDS) {}

    CIRCL_HD void xor_in() {
        detail::static_for<0, RATE_WORDS>([&](auto ic) {
            constexpr int k = decltype(ic)::v;
            const uint64_t w = blk[k];
            s.lo[k] ^= (uint32_t)w;
            s.hi[k] ^= (uint32_t)(w >> 32);
        });
    }
    CIRCL_HD void dump() {
        detail::static_for<0, RATE_WORDS>([&](auto ic) {
            constexpr int k = decltype(ic)::v;
            blk[k] = ((uint64_t)s.hi[k] << 32) | s.lo[k];
        });
        next = 0;
    }
    // absorbs the whole message; the first block of output is ready afterwards
    CIRCL_HD void init(const Msg &m) {
        keccak_zero(s);
        const uint32_t len = m.len(), nblk = len / RATE + 1;
#pragma unroll 1
        for (uint32_t b = 0; b < nblk; b++) {
            const uint32_t base = b * RATE, stop = len + 1 - base < (uint32_t)RATE ? len + 1 - base : (uint32_t)RATE;
#pragma unroll 1
            for (uint32_t k = 0; k < (uint32_t)RATE_WORDS; k++) {
                uint64_t w = 0;
                if (8 * k < stop)
                    for (uint32_t j = 0; j < 8; j++) w |= (uint64_t)m.at(base + 8 * k + j) << (8 * j);
                blk[k] = w;
            }
            xor_in();
            if (b == nblk - 1) s.hi[RATE_WORDS - 1] ^= 0x80000000u;
            keccak_f1600(s, 12);
        }
        dump();
    }
    CIRCL_HD uint64_t next_word() {
        if (next == (uint32_t)RATE_WORDS) {
            keccak_f1600(s, 12);
            dump();
        }
        return blk[next++];
    }
};

// The sampler: the next element of a stream of 8-byte little-endian words, the first of at most MAX_TRIES words that is < p.
// false (and x = 0) when all of them were refused.  Src has next_word().
template <class Src> CIRCL_HD bool sample(Src &src, uint64_t &x) {
    for (int t = 0; t < MAX_TRIES; t++) {
        x = src.next_word();
        if (fp64::canonical(x)) return true;
    }
    x = 0;
    return false;
}

}  // namespace prio3
}  // namespace circl
