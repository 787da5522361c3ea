// Launch decision of the exhaustive Hamming scan (scan_hamming.hip, faiss::hammings_knn as faiss::IndexLSH::search calls it): a
// pure host function of the shape, so that it can be stated and tested without a device (tests/cpp/hamming_plan_dump.cpp,
// tests/test_hamming_plan.py).  Every threshold of the scan is stated here, once.  No other plan is touched by this one.
//
// The grid is pq_plan.h's: (query tile of Q) x (code slice of S).  A workgroup of four waves keeps the codes of Q queries in LDS
// (their first piece in scalar registers), walks the stored codes of one slice once -- a lane owns one code per trip of 256 --
// and XOR-popcounts every loaded code against the Q queries.  With S > 1 every (query, slice) leaves k (distance, position)
// keys in scratch and a join launch writes the rows; the keys' order is total, so the rows depend on neither Q nor S.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vlq {

constexpr int kHamMaxK = 1024;               // VLQ_MAX_K
constexpr int kHamMaxCode = 128;             // bytes: 1024 bits, the largest distance still far inside f32's exact integers
constexpr int kHamWaves = 4;                 // waves of a scan workgroup
constexpr int kHamMaxTile = 4;               // Q: one wave joins one query's rows at the end, so Q <= kHamWaves
constexpr int kHamMaxSlices = 64;
constexpr size_t kHamLdsLimit = 160 * 1024;
constexpr int64_t kHamQueryPage = 32768;     // GpuIndex::search pages at 32768 queries (gpu/GpuIndex.cu:29)
constexpr size_t kHamScratchLimit = size_t(256) << 20;      // bytes of partial rows per page
// The numbers below were measured with tools/time_lsh.py on the MI355X (DESIGN.md section 3.16 has the table; median of 5,
// clocks warmed, variants alternating; random codes, ms):
//   kHamTargetGroups  512, pq_plan.h's value, stays.  1024 groups win at 8-byte codes (nq 64, 1e7 codes, k 10: 0.72 at S = 16 against
//                     0.43 at S = 32) and lose at 128-byte codes (6.3 against 14.6).  Supposed, not shown by counters: a trip of 256 lanes
//                     touches 256 rows x 128 B = 32 KB, the size of the L1, and more workgroups per CU push one another's rows out
//                     between a row's eight 16-byte pieces.
//   kHamWideTile      Q = 4 where a slice is long enough to pay for four selections per wave.  nq 10 000, 1e7 codes, k 10: Q = 1
//                     91.7 / 462 / 6901, Q = 2 49.5 / 224 / 3102, Q = 4 33.9 / 128 / 1675 at 8 / 32 / 128 bytes -- the time follows
//                     the passes over the codes, ntotal * code_size * ceil(nq / Q), not the XOR + popcount count.  Q = 4 loses
//                     where a slice is short (nq 64, 1e6 codes in 32 slices, k 100, 8 bytes: 0.283 against 0.194; 32 bytes, k 10:
//                     0.193 against 0.167) and wins from about 2 MiB of codes per slice on (nq 64, 1e7 codes, 8 bytes: 0.43
//                     against 0.72; 1e6 codes of 128 bytes in 32 slices: 0.51 against 0.65).  kHamWideSliceBytes is that bound;
//                     it misjudges nq 10 000 over 1e5 codes of 8 bytes (Q = 2 0.54 where Q = 4 has 0.46) and of 32 bytes, k 10
//                     (Q = 4 1.41 where Q = 2 has 1.13).
//   the join cap      the join launch merges a query's S * k keys in ONE wave: about 30 ns per key (67 ns at k > 256), against
//                     about (16 + code_size) / 16 ns per code of a slice.  One query, 1e6 codes of 8 bytes: k 100: S = 64 0.275,
//                     S = 16 0.146; k 1024: S = 64 4.68, S = 8 1.12.  The two costs balance at
//                     S^2 = ntotal * (16 + code_size) / (512 * k) (half of it at k > 256), which is where the measured minimum sits
//                     (1e7 codes, k 1024: S = 16 of 8, 16, 32, 64 at 8 bytes, S = 32 at 128 bytes); nothing below S = 8 was
//                     measured, so the cap is never below kHamJoinCapMin.
//   kHamMinSlice      4096, pq_plan.h's value, NOT varied on its own: with the join cap in front it decides only below about 1e5
//                     codes, where the whole search takes 0.03 ms.
constexpr int kHamTile = 2;                  // queries per workgroup where the selection leaves room (k <= 256)
constexpr int kHamWideTile = 4;              // ... where a slice holds at least kHamWideSliceBytes of codes
constexpr int64_t kHamWideSliceBytes = int64_t(2) << 20;
constexpr int kHamTargetGroups = 512;        // workgroups wanted in flight: two per CU of the 256
constexpr int64_t kHamMinSlice = 4096;       // codes below which a slice is not worth a workgroup of its own (16 trips of 256 lanes)
constexpr int kHamJoinCapMin = 8;            // the join cap never asks for fewer slices than this

// the widths hammings_knn serves (hamming.cpp:482-505): 4, 8, 16, 32 and every multiple of 8; here up to kHamMaxCode
inline bool hamming_width_served(int code_size) { return code_size == 4 || (code_size >= 8 && code_size <= kHamMaxCode && code_size % 8 == 0); }

// the scan kernel's dynamic LDS, byte offsets: the merge area [Q][4][k] of the waves' rows at 0, the selections' queues
// [4][Q][64], the queries' codes [Q][kHamMaxCode / 4] words
struct HamLayout { int selq, qcode; size_t bytes; };

struct HamPlan {
    bool ok = false;
    const char* why = "";   // !ok: what does not fit
    int Q = 1;              // queries per workgroup
    int S = 1;              // code slices
    int waves = kHamWaves;
    int kpl = 1;            // keys per lane of WaveSelect: 1 (k <= 64), 4 (k <= 256), 16 (k <= 1024)
    int load = 4;           // bytes of a code fetched per load: 16 (code_size % 16 == 0), 8 (% 8 == 0), 4
    bool join = false;      // S > 1: partial rows in scratch, a join launch follows
    int64_t slice_len = 0;  // codes per slice (the last may be shorter)
    int64_t page = 0;       // queries per launch
    HamLayout lay = {0, 0, 0};
};

inline HamLayout hamming_layout(int Q, int k) {
    HamLayout l;
    size_t o = ((size_t)Q * kHamWaves * k * 8 + 15) & ~(size_t)15;
    l.selq = (int)o; o += (size_t)kHamWaves * Q * 64 * 8;
    l.qcode = (int)o; o += (size_t)Q * kHamMaxCode;
    l.bytes = o;
    return l;
}

// force_q / force_s: vlq_lsh_set_scan_split (0 = the plan decides)
inline HamPlan plan_hamming_scan(int64_t nq, int64_t ntotal, int code_size, int k, int force_q = 0, int force_s = 0) {
    HamPlan p;
    if (nq < 1) { p.why = "no queries"; return p; }
    if (ntotal < 0 || ntotal >= (int64_t(1) << 32)) { p.why = "ntotal beyond the key's 32-bit position"; return p; }
    if (!hamming_width_served(code_size)) { p.why = "code width not served: 4, or a multiple of 8 up to 128 bytes (hamming.cpp:482-505)"; return p; }
    if (k < 1 || k > kHamMaxK) { p.why = "k outside 1..1024"; return p; }
    if (force_q != 0 && force_q != 1 && force_q != 2 && force_q != 4) { p.why = "query tile must be 1, 2 or 4"; return p; }
    if (force_s < 0 || force_s > kHamMaxSlices) { p.why = "slices outside 1..64"; return p; }
    p.kpl = k <= 64 ? 1 : k <= 256 ? 4 : 16;
    p.load = code_size % 16 == 0 ? 16 : code_size % 8 == 0 ? 8 : 4;
    // S of a tile of Q: small batches are cut along the codes until kHamTargetGroups workgroups run, no slice shorter than
    // kHamMinSlice, no more slices than the join launch is worth (the join cap above)
    const int64_t page0 = nq < kHamQueryPage ? nq : kHamQueryPage;
    auto slices_of = [&](int Q) -> int64_t {
        if (force_s) return force_s;
        const int64_t tiles = (page0 + Q - 1) / Q;
        int64_t S = (kHamTargetGroups + tiles - 1) / tiles;
        const int64_t by_len = ntotal / kHamMinSlice;
        const int64_t bal = ntotal * (16 + code_size) / (int64_t(512) * k * (p.kpl == 16 ? 2 : 1));      // S^2 at the balance
        int64_t cap = kHamJoinCapMin;
        while (cap < kHamMaxSlices && (cap + 1) * (cap + 1) <= bal) cap++;
        if (S > cap) S = cap;
        if (S > by_len) S = by_len;
        if (S > kHamMaxSlices) S = kHamMaxSlices;
        return S < 1 ? 1 : S;
    };
    // k > 256: one selection of 16 keys per lane is all the registers hold (pq_plan.h's finding; the selection is the same code)
    int Q = force_q;
    if (Q == 0) {
        Q = page0 >= 2 ? kHamTile : 1;
        if (page0 >= kHamWideTile && p.kpl != 16) {
            const int64_t S4 = slices_of(kHamWideTile);
            if ((ntotal + S4 - 1) / S4 * code_size >= kHamWideSliceBytes) Q = kHamWideTile;
        }
    }
    if (p.kpl == 16) Q = 1;
    p.Q = Q;
    p.lay = hamming_layout(Q, k);
    if (p.lay.bytes > kHamLdsLimit) { p.why = "the merge area does not fit 160 KB of LDS"; return p; }
    const int64_t S = slices_of(Q);
    p.S = (int)S;
    p.join = S > 1;
    p.slice_len = ntotal == 0 ? 0 : (ntotal + S - 1) / S;
    // scratch of a page: page * S * k keys of 8 bytes
    int64_t page = kHamQueryPage;
    if (p.join) {
        const int64_t by_scratch = (int64_t)(kHamScratchLimit / ((size_t)S * k * 8));
        if (page > by_scratch) page = by_scratch;
    }
    p.page = page < 1 ? 1 : page;
    p.ok = true;
    return p;
}

}  // namespace vlq
