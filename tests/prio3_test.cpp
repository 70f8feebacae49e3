// tests/prio3_test.cpp -- the C++ mirror include/circl/prio3.hpp on the GPU: one Prio3Count and one Prio3Sum flow of four reports under
// three aggregators (Shard, PrepInit per aggregator, PrepSharesToPrep, AggregateUpdate, Unshard), one report of each out of range.  The
// expected leader shares come from the caller (tests/test_gpu_prio3_mirror.py computes them with the checker tests/prio3.py) as hex
// arguments: argv[1 + 4 k + i] = report i of flow k (Count, Sum); "-" where the report is out of range.
#include <cstdio>
#include <cstring>
#include <string>

#include "circl/prio3.hpp"

using namespace circl;
using prio3::Bytes;
using prio3::List;

static Bytes unhex(const char *s) {
    Bytes b;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) b.push_back((uint8_t)std::stoi(std::string(s + i, 2), nullptr, 16));
    return b;
}
// the byte pattern both sides of the test agree on
static Bytes pattern(size_t len, int a, int b) {
    Bytes r(len);
    for (size_t j = 0; j < len; j++) r[j] = (uint8_t)(7 * j + 13 * a + b);
    return r;
}
static int fail(const char *what) {
    printf("FAIL %s\n", what);
    return 1;
}

template <class V> static int flow(V &v, const std::vector<uint64_t> &meas, uint64_t want, char **hex) {
    const size_t n = meas.size();
    const int shares = v.Params().Shares;
    List rands, nonces;
    for (size_t i = 0; i < n; i++) {
        rands.push_back(pattern(v.Params().RandSize, (int)i, 1));
        nonces.push_back(pattern(prio3::NonceSize, (int)i, 2));
    }
    const Bytes vk = pattern(prio3::VerifyKeySize, 0, 3);
    List leader = v.Shard(meas, rands);
    for (size_t i = 0; i < n; i++) {
        const bool bad = !strcmp(hex[i], "-");
        if (v.LastOk()[i] != !bad || leader[i] != (bad ? Bytes() : unhex(hex[i]))) return fail("Shard");
        if (bad) leader[i] = Bytes(v.Params().LeaderShareSize, 0);   // zeros in its place: PrepSharesToPrep must refuse it
    }
    List preps(n), aggs, outs[8];
    for (int j = 0; j < shares; j++) {
        List in = leader;
        if (j)
            for (size_t i = 0; i < n; i++) in[i] = Bytes(rands[i].begin() + 32 * (j - 1), rands[i].begin() + 32 * j);
        const List p = v.PrepInit(vk, nonces, j, in, &outs[j]);
        for (size_t i = 0; i < n; i++) {
            if (!v.LastOk()[i]) return fail("PrepInit");
            preps[i].insert(preps[i].end(), p[i].begin(), p[i].end());
        }
    }
    const std::vector<uint8_t> verdict = v.PrepSharesToPrep(preps);
    for (size_t i = 0; i < n; i++)
        if (verdict[i] != (strcmp(hex[i], "-") != 0)) return fail("PrepSharesToPrep");
    for (int j = 0; j < shares; j++) {
        Bytes agg = v.AggregateInit();
        v.AggregateUpdate(agg, outs[j], verdict);
        aggs.push_back(agg);
    }
    if (v.Unshard(aggs, n) != want) return fail("Unshard");
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 9) return fail("usage: prio3_test <8 hex leader shares or ->");
    try {
        prio3::Sum bad(3, 0, Bytes());
        return fail("a Sum with max_measurement 0 was accepted");
    } catch (const prio3::ErrParams &) {
    }
    try {
        prio3::Count bad(1, Bytes());
        return fail("one share was accepted");
    } catch (const prio3::ErrParams &) {
    }
    const Bytes ctx = pattern(16, 0, 5);
    prio3::Count c(3, ctx);
    if (c.Params().LeaderShareSize != 48 || c.Params().PrepShareSize != 32 || c.Params().RandSize != 96) return fail("Count.Params");
    if (int rc = flow(c, {1, 0, 2, 1}, 2, argv + 1)) return rc;
    prio3::Sum s(3, 1000, ctx);
    if (s.Params().LeaderShareSize != 8 * (20 + 64) || s.Params().PrepShareSize != 24) return fail("Sum.Params");
    if (int rc = flow(s, {1000, 1001, 0, 337}, 1337, argv + 5)) return rc;
    try {
        prio3::Sum big(2, uint64_t(1) << 62, ctx);
        big.Unshard({Bytes(8, 0), Bytes(8, 0)}, 8);
        return fail("an aggregate bound that wraps was accepted");
    } catch (const prio3::ErrAggregateBound &) {
    }
    printf("OK\n");
    return 0;
}
