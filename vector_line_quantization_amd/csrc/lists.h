// Device-resident inverted lists (ListStore, handle.h): one flat array per field (codes, optional side bytes -- lambda bytes /
// refine codes --, ids), list i at [off[i], off[i] + len[i]) with capacity off[i+1] - off[i].  Lists loaded
// with set_lists are packed (capacity == length); lists grown by add() get 25 % slack when
// the layout has to be rebuilt, so appending is amortised O(batch) and never leaves the
// device: counts, prefix sums, the overflow test and the new layout are computed there, the host
// sees one flag and two totals per call.  Replaces the per-list growable device vectors of the reference
// (gpu/impl/IVFBase.cuh:109-143, gpu/impl/InvertedListAppend.cu:122-247).
#pragma once
#include "handle.h"
#include "list_offsets.h"

namespace vlq {

// The store of a new handle: every list empty and without capacity (lists_clear).
int lists_init(ListStore& ls, int64_t nlist, int code_size, int side_size, hipStream_t s);
// Replace the lists by packed ones: offsets [nlist+1] (host or device memory; checked by check_list_offsets, list_offsets.h,
// with `noun` and `len_limit`), codes / ids [offsets[nlist]] rows, side likewise or nullptr (the side field is then left
// unwritten).  Synchronises s before the arrays are re-reserved -- that frees blocks the stream may still be reading -- and
// again at the end.  *ntotal = offsets[nlist] once the offsets have passed.
int lists_load(ListStore& ls, const void* codes, const void* side, const int64_t* ids, const int64_t* offsets, const char* noun,
               int64_t len_limit, hipStream_t s, int64_t* ntotal);
// every list empty, no capacity left behind (the next add lays the lists out afresh); synchronises
int lists_clear(ListStore& ls, hipStream_t s);
// the readers of list i (0 <= i < nlist, the caller's check) behind everything queued on s; null outputs are skipped
int lists_length(ListStore& ls, int64_t i, int64_t* len, hipStream_t s);
int lists_read(ListStore& ls, int64_t i, void* codes_out, void* side_out, int64_t* ids_out, hipStream_t s);

// Append n encoded vectors: vector i goes to the end of list assign[i] (assign[i] < 0: dropped,
// IndexIVFPQ.cpp:238-243), vectors of one list keep their input order (:236-248).  All
// pointers are device pointers; id of vector i = xids ? xids[i] : id_base + i (:244).
// assign32 != nullptr: int32 list ids (VLQ lines) instead of assign64.
int lists_append(ListStore& ls, int64_t n, const int64_t* assign64, const int32_t* assign32, const uint8_t* new_codes,
                 const uint8_t* new_side, const int64_t* xids, int64_t id_base, hipStream_t s, int64_t* placed = nullptr,
                 bool* relaid = nullptr);
// (*relaid: the append rebuilt the layout -- every list may have moved; otherwise the batch sits behind the old ends of the
// lists and ls.ws.cnt[i] (int) is the number of vectors list i received)

int lists_sync_host(ListStore& ls, hipStream_t s);
int lists_relayout(ListStore& ls, std::vector<int64_t>& new_off, hipStream_t s);
int lists_reserve(ListStore& ls, int64_t num_vecs, hipStream_t s);
int lists_reclaim(ListStore& ls, uint64_t* bytes, hipStream_t s);

}  // namespace vlq
