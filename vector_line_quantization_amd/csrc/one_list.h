// What the four flat indexes (pq_api.hip, sqflat_api.hip, knn_api.hip, lsh_api.hip) have in common: rows of one width in a
// ListStore of ONE list, in the order they arrived, ids = positions; every stored row is scored for every query.  The shell owns
// the device context (the device, the private stream, the caller's stream), that list, the workspaces every kind stages through
// and the text of the last scan.  A kind adds its readiness check, its encoder, its plan and the scan of one page.
// Where the kinds answer differently (texts, codes, the 2^32 limits) the check stays in the kind, in front of the shared call.
#pragma once
#include "handle.h"
#include "lists.h"

namespace vlq_detail {

struct OneListShell {
    DevCtx ctx;
    int64_t ntotal = 0;
    vlq::ListStore lists;         // one list: the rows in scan order, ids = positions (the list starts at 0)
    DevBuf ws_x, ws_assign, ws_ids, ws_part, ws_D, ws_I;
    int force_tile = 0, force_s = 0;      // vlq_<kind>_set_scan_split
    char last_scan[224] = "";
};

// a new handle's shell: the device checks of create, the private non-blocking stream, an empty list of row_bytes rows.  On
// failure the caller destroys the handle.
int one_open(OneListShell* o, int device, int row_bytes);
// every DevBuf of the handle frees its block at the delete, before the stream goes (a handle that never got its stream: only
// the delete)
template <class Handle>
void one_destroy(Handle* h) {
    if (!h) return;
    const hipStream_t own = h->ctx.own_stream;
    if (own) {
        (void)hipSetDevice(h->ctx.device);
        (void)hipStreamSynchronize(h->ctx.stream);
    }
    delete h;
    if (own) (void)hipStreamDestroy(own);
}

int one_set_stream(OneListShell* o, void* hip_stream);      // synchronises the old stream first
inline int64_t one_ntotal(const OneListShell* o) { return o ? o->ntotal : -1; }
int one_reset(OneListShell* o);
int one_reserve(OneListShell* o, int64_t num_vecs);         // behind the kind's argument checks
int one_last_scan_info(OneListShell* o, char* buf, int cap);
// query_tile 0, 1, 2 or 4; slices 0 .. max_slices; 0 = the plan decides
int one_set_scan_split(OneListShell* o, int query_tile, int slices, int max_slices);

// add in two steps, the kind's encoder between them: ws_assign = n zeros (every vector goes to list 0), then the n device rows
// behind the stored ones; ntotal grows by the rows placed
int one_route(OneListShell* o, int64_t n);
int one_append(OneListShell* o, int64_t n, const uint8_t* rows_dev);
// rows [n][row_bytes] [h|d] replace the stored ones
int one_load(OneListShell* o, const uint8_t* rows, int64_t n);
// stored rows i0 .. i0 + ni - 1 into out [h|d], behind the kind's range check: synchronises, then a blocking copy
int one_get_rows(OneListShell* o, int64_t i0, int64_t ni, void* out);
// a result of the stream's work into dst [h|d]: an asynchronous copy, then the synchronisation
int one_fetch(const DevCtx* c, void* dst, const void* src, size_t bytes);

int one_search_args(int64_t n, const void* x, int k, const void* D, const void* I);
// The body of search behind the kind's checks (n > 0): the outputs staged (page-locked host rows are written by the kernels),
// the queries of query_bytes each staged into ws_x, then scan_page(ni, x_dev, D_dev, I_dev) for every `page` queries, then
// launched() -- the kind's bookkeeping of a search whose every page is on the stream --, then the rows are waited for.  Plans
// nothing: the page size and what a page launches are the kind's.
struct NothingMore { void operator()() const {} };
template <class ScanPage, class Launched = NothingMore>
int one_search(OneListShell* o, int64_t n, const void* x, size_t query_bytes, int k, float* D, int64_t* I, int64_t page, ScanPage scan_page,
               Launched launched = Launched()) {
    TRY(set_dev(&o->ctx));
    StagedRows out;
    TRY(out.stage(D, (size_t)n * k * 4, o->ws_D, I, (size_t)n * k * 8, o->ws_I, true));
    const void* xd = nullptr;
    TRY(stage_in(&o->ctx, x, (size_t)n * query_bytes, o->ws_x, &xd));
    for (int64_t i0 = 0; i0 < n; i0 += page) {
        const int64_t ni = std::min(page, n - i0);
        TRY(scan_page(ni, (const uint8_t*)xd + (size_t)i0 * query_bytes, (float*)out.D + i0 * k, (int64_t*)out.I + i0 * k));
    }
    launched();
    return out.finish(&o->ctx);
}

}  // namespace vlq_detail
