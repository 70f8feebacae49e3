// circl/prio3.hpp -- C++ mirror of the reference's vdaf/prio3/count and vdaf/prio3/sum (Prio3Count, Prio3Sum; draft-irtf-cfrg-vdaf-13
// section 7) over batches of reports, behind circl_hip_prio3_*.  Header-only over the C ABI (link libcirclhip.so).
//
//   prio3::Count c(shares, context);                 count.New(numShares, context)
//   prio3::Sum s(shares, max_measurement, context);  sum.New(numShares, maxMeasurement, context)
//   v.Params()                                       the lengths of one report's pieces, in bytes
//   v.Shard(measurements, rands) -> leader shares    Shard per report; rands[i]: 32 x shares bytes, helper j's input share is bytes
//                                                    32 (j - 1) .. 32 j of it.  LastOk()[i] = 0 and an empty share where it fails
//   v.PrepInit(verify_key, nonces, agg_id, input_shares, &out_shares) -> prep shares
//                                                    PrepInit per report (the leader shares for agg_id 0, else the 32-byte seeds); the out
//                                                    share is the prepare state: PrepNext is the identity for these two types
//   v.PrepSharesToPrep(prep_shares) -> verdicts      prep_shares[i]: the aggregators' prep shares of report i, concatenated in order
//   v.AggregateUpdate(agg_share, out_shares, mask)   adds the out shares whose mask byte is not zero (an empty mask: all)
//   v.Unshard(agg_shares, num_measurements)          the aggregate result; ErrAggregateBound as the reference's
// The names are the reference's; every call takes a batch.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../circl_hip.h"
#include "kem.hpp"

namespace circl {
namespace prio3 {

using kem::Bytes;
using List = std::vector<Bytes>;

constexpr size_t SeedSize = 32, NonceSize = 16, VerifyKeySize = 32, ElementSize = 8;

struct ErrParams : kem::Error {
    ErrParams() : kem::Error("prio3: invalid type, number of shares or context") {}
};
struct ErrBatchSize : kem::Error {
    ErrBatchSize() : kem::Error("prio3: a list or an item of another length than the batch wants") {}
};
struct ErrAggregateBound : kem::Error {
    ErrAggregateBound() : kem::Error("prio3: aggregate shares or their bound are not representable in Fp64") {}
};

struct Parameters {
    size_t LeaderShareSize, HelperShareSize, PrepShareSize, OutShareSize, AggShareSize, RandSize;
    int Shares;
};

class Prio3 {
public:
    Parameters Params() const {
        return {circl_hip_prio3_leader_share_size(kind_, max_), SeedSize, circl_hip_prio3_prep_share_size(kind_), ElementSize, ElementSize,
                circl_hip_prio3_rand_size(shares_), shares_};
    }
    const std::vector<uint8_t> &LastOk() const { return ok_; }

    List Shard(const std::vector<uint64_t> &measurements, const List &rands) {
        const size_t n = measurements.size(), ls = Params().LeaderShareSize;
        const Bytes rr = rows(rands, n, Params().RandSize);
        Bytes leader(n * ls);
        ok_.assign(n, 0);
        check(circl_hip_prio3_shard(kind_, max_, shares_, ctx_.data(), ctx_.size(), measurements.data(), rr.data(), leader.data(), ok_.data(), n, device_));
        return split(leader, n, ls, true);
    }
    List PrepInit(const Bytes &verify_key, const List &nonces, int agg_id, const List &input_shares, List *out_shares) {
        const size_t n = nonces.size(), ps = Params().PrepShareSize;
        if (verify_key.size() != VerifyKeySize) throw ErrBatchSize();
        const Bytes nn = rows(nonces, n, NonceSize), sh = rows(input_shares, n, agg_id == 0 ? Params().LeaderShareSize : SeedSize);
        Bytes prep(n * ps), out(n * ElementSize);
        ok_.assign(n, 0);
        check(circl_hip_prio3_prep_init(kind_, max_, shares_, ctx_.data(), ctx_.size(), agg_id, verify_key.data(), nn.data(), sh.data(), prep.data(), out.data(),
                                        ok_.data(), n, device_));
        if (out_shares) *out_shares = split(out, n, ElementSize, true);
        return split(prep, n, ps, true);
    }
    std::vector<uint8_t> PrepSharesToPrep(const List &prep_shares) {
        const size_t n = prep_shares.size();
        const Bytes ps = rows(prep_shares, n, (size_t)shares_ * Params().PrepShareSize);
        ok_.assign(n, 0);
        check(circl_hip_prio3_prep_finish(kind_, max_, shares_, ctx_.data(), ctx_.size(), ps.data(), ok_.data(), n, device_));
        return ok_;
    }
    Bytes AggregateInit() const { return Bytes(ElementSize, 0); }
    void AggregateUpdate(Bytes &agg_share, const List &out_shares, const std::vector<uint8_t> &mask = {}) const {
        const size_t n = out_shares.size();
        if (agg_share.size() != ElementSize || (!mask.empty() && mask.size() != n)) throw ErrBatchSize();
        const Bytes out = rows(out_shares, n, ElementSize);
        check(circl_hip_prio3_aggregate(kind_, max_, shares_, ctx_.data(), ctx_.size(), out.data(), mask.empty() ? nullptr : mask.data(), agg_share.data(), n, device_));
    }
    uint64_t Unshard(const List &agg_shares, uint64_t num_measurements) const {
        const Bytes a = rows(agg_shares, (size_t)shares_, ElementSize);
        uint64_t r = 0;
        if (circl_hip_prio3_unshard(kind_, max_, shares_, ctx_.data(), ctx_.size(), a.data(), num_measurements, &r) != CIRCL_HIP_OK) throw ErrAggregateBound();
        return r;
    }

protected:
    Prio3(int kind, uint64_t max_measurement, int shares, const Bytes &context, int device)
        : kind_(kind), max_(max_measurement), shares_(shares), ctx_(context), device_(device) {
        if (!circl_hip_prio3_leader_share_size(kind, max_measurement) || !circl_hip_prio3_rand_size(shares) || context.size() > 255) throw ErrParams();
    }

private:
    static void check(int rc) {
        if (rc != CIRCL_HIP_OK) throw kem::ErrDevice(std::string("error ") + std::to_string(rc) + " " + circl_hip_last_error());
    }
    static Bytes rows(const List &items, size_t n, size_t row) {
        if (items.size() != n) throw ErrBatchSize();
        Bytes b;
        b.reserve(n * row + 1);
        for (const Bytes &x : items) {
            if (x.size() != row) throw ErrBatchSize();
            b.insert(b.end(), x.begin(), x.end());
        }
        b.push_back(0);   // (data() of an empty batch is still a pointer)
        return b;
    }
    // rows of `row` bytes; with ok: an empty item where the report failed
    List split(const Bytes &b, size_t n, size_t row, bool by_ok) const {
        List out(n);
        for (size_t i = 0; i < n; i++)
            if (!by_ok || ok_[i]) out[i].assign(b.begin() + i * row, b.begin() + (i + 1) * row);
        return out;
    }
    int kind_;
    uint64_t max_;
    int shares_;
    Bytes ctx_;
    int device_;
    std::vector<uint8_t> ok_;
};

struct Count : Prio3 {
    Count(int shares, const Bytes &context, int device = 0) : Prio3(CIRCL_HIP_PRIO3_COUNT, 0, shares, context, device) {}
};
struct Sum : Prio3 {
    Sum(int shares, uint64_t max_measurement, const Bytes &context, int device = 0) : Prio3(CIRCL_HIP_PRIO3_SUM, max_measurement, shares, context, device) {}
};

}  // namespace prio3
}  // namespace circl
