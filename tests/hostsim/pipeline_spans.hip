// pipeline_spans.hip -- host_common.h span_start / span_bytes (the bytes and the address of a chunk of a ragged, padded array) as a
// stand-alone host program: over shards x chunk sizes x both pads, every byte of a heap block of exactly the blob's size is covered
// once, and the rebased chunk pointer + absolute offset + pad * chunk-local index is the item's address.  Run under ASan / UBSan
// by tests/test_pipeline_spans.py.
#include "host_common.h"
#include <cassert>
#include <cstdlib>
using namespace circl::host;
int main() {
    const size_t n = 300;
    for (size_t pad : {size_t(0), size_t(16)}) {
        std::vector<uint64_t> off(n + 1, 0);
        for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + ((i == 255 || i == 256) ? 0 : i % 37);
        const size_t total = off[n] + pad * n;
        uint8_t *blob = (uint8_t *)malloc(total ? total : 1);
        memset(blob, 0, total);
        for (size_t shards : {size_t(1), size_t(3)})
            for (size_t chunk : {size_t(256), size_t(7), n}) {
                memset(blob, 0, total);
                for (size_t d = 0; d < shards; d++) {
                    const size_t slo = n * d / shards, scnt = n * (d + 1) / shards - slo;
                    HOut o{blob + pad * slo, 0, false, off.data() + slo, pad};
                    HBlob b{blob + pad * slo, off.data() + slo, false, pad};
                    for (size_t lo = 0; lo < scnt; lo += chunk) {
                        const size_t cnt = std::min(chunk, scnt - lo);
                        assert(o.at(lo) == b.at(lo) && o.bytes(lo, cnt) == b.bytes(lo, cnt));
                        uint8_t *p = o.at(lo);
                        for (size_t j = 0; j < o.bytes(lo, cnt); j++) p[j]++;
                        // the rebased chunk pointer + absolute offset + pad * chunk-local index = the item's address
                        uint8_t *rebased = p - o.off[lo];
                        for (size_t i = 0; i < cnt; i++) assert(rebased + o.off[lo + i] + pad * i == blob + off[slo + lo + i] + pad * (slo + lo + i));
                    }
                }
                for (size_t j = 0; j < total; j++) assert(blob[j] == 1);
            }
        free(blob);
    }
    HOut rows{nullptr, 16};
    assert(rows.bytes(5, 7) == 112 && span_start(nullptr, 16, 0, 5) == 80);
    puts("spans ok");
    return 0;
}
