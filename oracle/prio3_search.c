/* oracle/prio3_search.c -- TEST INFRASTRUCTURE ONLY (CPU oracle).
 *
 * Search for a seed (or nonce) whose XofTurboShake128 stream makes Prio3's rejection sampler refuse: a 64-bit little-endian word
 * >= p = 2^64 - 2^32 + 1, that is, a word whose top 32 bits are all ones and whose low 32 bits are not all zero (2^-32 per word).
 *
 *   message   = pre || candidate || suf                      (one block: shorter than the rate of 168 bytes)
 *   candidate = LE64(counter) || 0x5c ... 0x5c                (candlen bytes), counter = start, start + 1, ...
 *   stream    = TurboSHAKE128(message, D = 0x01)              (the 12-round permutation)
 *
 * Words 0 .. nwords - 1 of the stream are looked at; with edge != 0 only the last word of each squeezed block (index = 20 mod 21).
 * The answer is the smallest counter in [start, start + trials) with such a word, whatever the number of threads: the range is cut
 * into rounds of threads * SLICE counters, every thread scans its slice of the round to its first hit, and the first round with a hit
 * ends the search.
 *
 * The permutation here is the same function as orc_keccak_f1600(a, 12) with the rho / pi walk tabulated so that the compiler
 * unrolls it; the search refuses to run if the two disagree on a test state.  Little-endian hosts only (the message bytes are copied
 * straight into the state words), like the rest of the oracle's build (x86-64-v3).
 */
#include "oracle.h"
#include "keccak.h"
#include <pthread.h>
#include <string.h>

#define RATE 168
#define RATE_WORDS 21
#define SLICE (1u << 16)

static uint64_t RC12[12];
static int PI_TO[24], RHO[24];   /* step t of the walk moves lane PI_FROM (the previous PI_TO, lane 1 at t = 0) to PI_TO[t], rotated by RHO[t] */

static void tables(void) {
    uint8_t lfsr = 1;
    for (int r = 0; r < 24; r++) {
        uint64_t c = 0;
        for (int j = 0; j < 7; j++) {
            if (lfsr & 1) c ^= 1ULL << ((1u << j) - 1);
            lfsr = (uint8_t)((lfsr << 1) ^ ((lfsr & 0x80) ? 0x71 : 0));
        }
        if (r >= 12) RC12[r - 12] = c;
    }
    int x = 1, y = 0;
    for (int t = 0; t < 24; t++) {
        int nx = y, ny = (2 * x + 3 * y) % 5;
        PI_TO[t] = nx + 5 * ny;
        RHO[t] = ((t + 1) * (t + 2) / 2) % 64;
        x = nx; y = ny;
    }
}

#define ROL(v, n) (((v) << (n)) | ((v) >> (64 - (n))))

/* The tables' values, written out so that every index and rotation is a constant (checked against tables() before a search). */
static const int K_PI[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
static const int K_RHO[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};

static inline __attribute__((always_inline)) void p12(uint64_t a[25]) {
    for (int r = 0; r < 12; r++) {
        uint64_t c[5], t, u;
#pragma GCC unroll 5
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma GCC unroll 5
        for (int x = 0; x < 5; x++) {
            t = c[(x + 4) % 5] ^ ROL(c[(x + 1) % 5], 1);
#pragma GCC unroll 5
            for (int y = 0; y < 25; y += 5) a[x + y] ^= t;
        }
        t = a[1];
#pragma GCC unroll 24
        for (int i = 0; i < 24; i++) {
            u = a[K_PI[i]];
            a[K_PI[i]] = ROL(t, K_RHO[i]);
            t = u;
        }
#pragma GCC unroll 5
        for (int y = 0; y < 25; y += 5) {
#pragma GCC unroll 5
            for (int x = 0; x < 5; x++) c[x] = a[x + y];
#pragma GCC unroll 5
            for (int x = 0; x < 5; x++) a[x + y] = c[x] ^ (~c[(x + 1) % 5] & c[(x + 2) % 5]);
        }
        a[0] ^= RC12[r];
    }
}

static int self_check(void) {
    tables();
    for (int t = 0; t < 24; t++)
        if (K_PI[t] != PI_TO[t] || K_RHO[t] != RHO[t]) return -1;
    uint64_t a[25], b[25];
    for (int i = 0; i < 25; i++) a[i] = b[i] = 0x9e3779b97f4a7c15ULL * (uint64_t)(i + 1) ^ ((uint64_t)i << 57);
    for (int k = 0; k < 3; k++) {
        p12(a);
        orc_keccak_f1600(b, 12);
        if (memcmp(a, b, sizeof a)) return -1;
    }
    return 0;
}

typedef struct {
    const uint8_t *block;   /* the padded message with a zero counter */
    size_t at;              /* where the counter goes */
    unsigned nblocks, lastw, edge;
    uint64_t from, count;   /* this thread's slice */
    int hit;
    uint64_t counter, perms;
    unsigned index;
} job_t;

static inline int refused(uint64_t w) { return (w >> 32) == 0xffffffffu && (uint32_t)w != 0; }

static void *scan(void *arg) {
    job_t *j = (job_t *)arg;
    union { uint64_t a[25]; uint8_t b[200]; } s;
    j->hit = 0;
    j->perms = 0;
    for (uint64_t c = j->from; c < j->from + j->count; c++) {
        memset(s.b + RATE, 0, 200 - RATE);
        memcpy(s.b, j->block, RATE);
        memcpy(s.b + j->at, &c, 8);
        for (unsigned b = 0; b < j->nblocks; b++) {
            p12(s.a);
            j->perms++;
            const unsigned nw = b + 1 == j->nblocks ? j->lastw : RATE_WORDS;
            for (unsigned k = j->edge ? RATE_WORDS - 1 : 0; k < nw; k++)
                if (refused(s.a[k])) {
                    j->hit = 1;
                    j->counter = c;
                    j->index = b * RATE_WORDS + k;
                    return 0;
                }
        }
    }
    return 0;
}

/* 1: found (*counter, *index = the first refused word of that stream among those looked at); 0: none in the range; < 0: bad
 * arguments or a failed self-check.  *perms = permutations run, by all threads. */
int orc_prio3_search(const uint8_t *pre, size_t prelen, const uint8_t *suf, size_t suflen, size_t candlen,
                     uint64_t start, uint64_t trials, unsigned nwords, int edge, int threads,
                     uint64_t *counter, unsigned *index, uint64_t *perms) {
    if (candlen < 8 || prelen + candlen + suflen >= RATE || nwords == 0 || threads < 1 || threads > 16) return -1;
    if (self_check()) return -2;
    uint8_t block[RATE] = {0};
    memcpy(block, pre, prelen);
    memset(block + prelen, 0x5c, candlen);
    memset(block + prelen, 0, 8);
    memcpy(block + prelen + candlen, suf, suflen);
    block[prelen + candlen + suflen] ^= 0x01;
    block[RATE - 1] ^= 0x80;
    job_t jobs[16];
    pthread_t th[16];
    *perms = 0;
    for (uint64_t done = 0; done < trials;) {
        int used = 0;
        for (int t = 0; t < threads && done < trials; t++, used++) {
            const uint64_t n = trials - done < SLICE ? trials - done : SLICE;
            jobs[t] = (job_t){.block = block, .at = prelen, .nblocks = (nwords + RATE_WORDS - 1) / RATE_WORDS,
                              .lastw = nwords - (nwords - 1) / RATE_WORDS * RATE_WORDS, .edge = (unsigned)edge, .from = start + done, .count = n};
            done += n;
        }
        int started = 0;
        for (; started < used; started++)
            if (pthread_create(&th[started], 0, scan, &jobs[started])) break;
        for (int t = started; t < used; t++) scan(&jobs[t]);
        for (int t = 0; t < started; t++) pthread_join(th[t], 0);
        for (int t = 0; t < used; t++) *perms += jobs[t].perms;
        for (int t = 0; t < used; t++)
            if (jobs[t].hit) {
                *counter = jobs[t].counter;
                *index = jobs[t].index;
                return 1;
            }
    }
    return 0;
}
