// pipeline_bind.hip -- host_compose.h Bind (one declaration per staged array of a host form) as a stand-alone host program: over a toy
// Call with every kind of field, at lo = 0 and lo = 100, the HIn / HBlob / HOut records follow the staging rules (+ lo * row, a shared
// row per call, + pad * lo and off + lo, a wanted output without a host pointer), and on() puts each chunk pointer into the field it
// was declared for, nullptr into every declared field that is absent, and leaves the rest alone.  Run under ASan / UBSan by
// tests/test_pipeline_bind.py.
#include "host_compose.h"
#include <cassert>
using namespace circl::host;

struct Toy {
    int op = 7;
    const uint8_t *key = nullptr, *rows = nullptr, *null_rows = nullptr, *untaken_rows = nullptr;
    const uint64_t *seq = nullptr;
    uint8_t *proofs = nullptr;   // an output of one operation, read as rows by another
    const uint8_t *pt = nullptr, *ct = nullptr, *null_blob = nullptr, *untaken_blob = nullptr;
    const uint64_t *pt_off = nullptr, *ct_off = nullptr, *null_blob_off = nullptr, *untaken_blob_off = nullptr;
    uint8_t *out = nullptr, *ok = nullptr, *unwanted = nullptr, *rag = nullptr;
    const uint8_t *dst = nullptr;   // not declared: host bytes that the launch reads itself
    size_t stride = 24, n = 0;
};

template <class T> T *fake(uintptr_t v) { return reinterpret_cast<T *>(v); }   // never dereferenced

int main() {
    const size_t n = 300;
    std::vector<uint8_t> bytes(64 * n, 1);
    std::vector<uint64_t> off(n + 1, 0), seq(n, 0);
    for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + i % 37;
    uint8_t *const h = bytes.data();
    Toy c;
    c.key = h; c.rows = h + 1; c.untaken_rows = h + 2; c.seq = seq.data(); c.proofs = h + 3;
    c.pt = h + 4; c.ct = h + 5; c.untaken_blob = h + 6;
    c.pt_off = c.ct_off = c.null_blob_off = c.untaken_blob_off = off.data();   // an absent blob's offsets are host memory all the same
    c.out = h + 7; c.unwanted = h + 8; c.rag = h + 9;
    c.dst = h + 10; c.n = n;
    for (size_t lo : {size_t(0), size_t(100)}) {
        Bind<Toy> b(c, lo);
        b.rows(&Toy::key, 20, true, true);
        b.rows(&Toy::rows, 24, false);
        b.rows(&Toy::null_rows, 32, true);
        b.rows(&Toy::untaken_rows, 32, true, false, false);
        b.rows(&Toy::seq, 8, false);
        b.rows(&Toy::proofs, 64, true);
        b.blob(&Toy::pt, &Toy::pt_off, true);
        b.blob(&Toy::null_blob, &Toy::null_blob_off, true);
        b.blob(&Toy::ct, &Toy::ct_off, false, 16);
        b.blob(&Toy::untaken_blob, &Toy::untaken_blob_off, false, 0, false);
        b.out(&Toy::out, 32, true);
        b.out(&Toy::unwanted, 32, false, false);
        b.out(&Toy::ok, 1, false);
        b.ragged(&Toy::rag, &Toy::pt_off, true, 16);

        // the records: pointer, row, secret, per_call / pad, off
        auto in = [&](size_t j, const void *p, size_t row, bool secret, bool per_call) {
            const HIn &x = b.ins[j];
            return x.p == p && x.row == row && x.secret == secret && x.per_call == per_call && !x.optional;
        };
        assert(b.ins.size() == 4);
        assert(in(0, c.key, 20, true, true));                       // shared: no lo offset, one row per call
        assert(in(1, c.rows + lo * 24, 24, false, false));
        assert(in(2, seq.data() + lo, 8, false, false));            // + lo * 8 bytes of a uint64_t array
        assert(in(3, c.proofs + lo * 64, 64, true, false));
        auto blob = [&](size_t j, const uint8_t *p, bool secret, size_t pad) {
            const HBlob &x = b.blobs[j];
            return x.blob == p && x.off == off.data() + lo && x.secret == secret && x.pad == pad;
        };
        assert(b.blobs.size() == 2);
        assert(blob(0, c.pt, true, 0));
        assert(blob(1, c.ct + 16 * lo, false, 16));
        auto out = [&](size_t j, uint8_t *p, size_t row, bool secret, const uint64_t *o, size_t pad) {
            const HOut &x = b.outs[j];
            return x.p == p && x.row == row && x.secret == secret && x.off == o && x.pad == pad;
        };
        assert(b.outs.size() == 3);
        assert(out(0, c.out + lo * 32, 32, true, nullptr, 0));
        assert(out(1, nullptr, 1, false, nullptr, 0));              // wanted, no host pointer: a device buffer, nothing copied back
        assert(out(2, c.rag + 16 * lo, 0, true, off.data() + lo, 16));

        // a chunk of sentinel pointers
        Chunk k = {};
        for (size_t j = 0; j < b.ins.size(); j++) k.in.push_back(fake<uint8_t>(0x1000 + 0x10 * j));
        for (size_t j = 0; j < b.blobs.size(); j++) k.blob.push_back(fake<const uint8_t>(0x2000 + 0x10 * j)), k.off.push_back(fake<const uint64_t>(0x3000 + 0x10 * j));
        for (size_t j = 0; j < b.outs.size(); j++) k.out.push_back(fake<uint8_t>(0x4000 + 0x10 * j));
        k.cnt = 44;
        const Toy d = b.on(k);
        // each declared field got its own sentinel
        assert(d.key == k.in[0] && d.rows == k.in[1] && d.seq == fake<const uint64_t>(0x1020) && d.proofs == k.in[3]);
        assert(d.pt == k.blob[0] && d.pt_off == k.off[0] && d.ct == k.blob[1] && d.ct_off == k.off[1]);
        assert(d.out == k.out[0] && d.ok == k.out[1] && d.rag == k.out[2]);
        // every absent declared field is nullptr, the offsets of an absent blob included
        assert(!d.null_rows && !d.untaken_rows && !d.null_blob && !d.null_blob_off && !d.untaken_blob && !d.untaken_blob_off && !d.unwanted);
        // what was not declared passed through, and the item count is the chunk's
        assert(d.op == 7 && d.dst == c.dst && d.stride == 24 && d.n == 44);
        // the call itself is untouched
        assert(c.key == h && c.untaken_rows == h + 2 && c.null_blob_off == off.data() && c.unwanted == h + 8 && c.n == n);
    }
    puts("bind ok");
    return 0;
}
