// The check every list loader makes of the caller's offsets (lists_load, lists.hip): a pure host function, so that it can be
// stated and tested without a device (tests/cpp/test_list_offsets.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/vlq_ivfpq.h"      // the error codes

namespace vlq {

constexpr int64_t kNoLenLimit = 0;
constexpr int64_t kIvfLenLimit = int64_t(1) << 31;      // the IVF scans index a list's entries with 32 bits

// off[0 .. nlist]: starts at 0, never drops, and no list holds len_limit entries or more (kNoLenLimit: any length).
// Returns VLQ_OK, or the error code with its text in msg; `noun` is the offsets' name in the caller's signature.
inline int check_list_offsets(const int64_t* off, int64_t nlist, const char* noun, int64_t len_limit, char* msg, size_t cap) {
    if (off[0] != 0) { snprintf(msg, cap, "%s[0] != 0", noun); return VLQ_ERR_INVALID; }
    for (int64_t i = 0; i < nlist; i++) {
        if (off[i + 1] < off[i]) { snprintf(msg, cap, "%s not monotone at %ld", noun, (long)i); return VLQ_ERR_INVALID; }
        if (len_limit != kNoLenLimit && off[i + 1] - off[i] >= len_limit) {
            snprintf(msg, cap, "list %ld longer than 2^31", (long)i);
            return VLQ_ERR_UNSUPPORTED;
        }
    }
    return VLQ_OK;
}

}  // namespace vlq
