// The hits a range search leaves in its handle (vlq_ivfflat_range_search, vlq_flat_range_search) until the next range search,
// reset or destroy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vlq_detail {

// RangeSearchResult::distances / labels of the last range search: blocks of exactly 4 * total and 8 * total bytes
struct RangeHits {
    float* D = nullptr;
    int64_t* I = nullptr;
    int64_t total = 0;
    RangeHits() = default;
    RangeHits(const RangeHits&) = delete;
    RangeHits& operator=(const RangeHits&) = delete;
    ~RangeHits() { drop(); }
    void drop() {
        if (D) (void)hipFree(D);
        if (I) (void)hipFree(I);
        D = nullptr; I = nullptr; total = 0;
    }
};

}  // namespace vlq_detail
