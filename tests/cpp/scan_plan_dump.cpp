// Host only: prints plan_scan's decision (csrc/scan_plan.h) for a list of named shapes, one line each.  Links neither the
// library nor the HIP runtime; tests/test_scan_plan.py compares the lines with tests/golden/scan_plan.txt, whose rows were
// written by hand from the conditions the decision had when it was spread over scan_dev and the launchers.
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "scan_plan.h"

using vlq::ScanPath;
using vlq::ScanShape;

// the headline: 10 000 queries, nprobe 32, k 10, 1 M vectors of 16-byte codes in 4096 lists, precomputed tables
static ScanShape headline() {
    ScanShape s;
    s.M = 16; s.ksub = 256; s.dsub = 8; s.d = 128; s.nlist = 4096; s.ntotal = 1000000;
    s.table_mode = 1; s.have_rank = true;
    s.ni = s.n = 10000; s.nprobe = 32; s.k = 10;
    return s;
}
static ScanShape code_size(int M, int d) { ScanShape s = headline(); s.M = M; s.d = d; s.dsub = d / M; return s; }
static ScanShape batch(int64_t ni) { ScanShape s = headline(); s.ni = s.n = ni; return s; }
static ScanShape topk(int k) { ScanShape s = headline(); s.k = k; return s; }
static ScanShape long_lists(int k) { ScanShape s = headline(); s.nlist = 256; s.ntotal = 262144; s.k = k; return s; }
static ScanShape multi_index(int M) {       // 2 x 8 bits: 65 536 cells for 1 M vectors
    ScanShape s = code_size(M, 128);
    s.imi_nbits = 8; s.nlist = 65536; s.have_rank = false;
    return s;
}
// the last page of a call of 32 768 + r queries on a small index of 16-byte codes (tests/test_gpu_query_pages.py): 64 lists,
// 4000 vectors (neither short nor long lists), nprobe 32, k 10; M = 8: the same over d = 32 with nprobe 8, as that file's
// "scanm" index is searched
static ScanShape tail_page(int64_t r, int M = 16, int d = 128, int nprobe = 32) {
    ScanShape s = code_size(M, d);
    s.nlist = 64; s.ntotal = 4000; s.nprobe = nprobe;
    s.n = 32768 + r; s.ni = r;
    return s;
}
static ScanShape with(ScanShape s, const std::function<void(ScanShape&)>& f) { f(s); return s; }

static std::string kernel_name(const ScanShape& s, const vlq::ScanPlan& p) {
    const vlq::ScanLaunch& L = p.launch;
    char b[96];
    auto tf = [](bool x) { return x ? "true" : "false"; };
    switch (p.path) {
    case ScanPath::fp16: snprintf(b, sizeof(b), "scan16h_kernel<%d>", L.kpl); break;
    case ScanPath::owned2: snprintf(b, sizeof(b), "scan16o_kernel<%d, %d>", L.kpl, L.nbuf); break;
    case ScanPath::scan16_short: snprintf(b, sizeof(b), "scan16_short_kernel<%d>", L.kpl); break;
    case ScanPath::scan16_bigk: snprintf(b, sizeof(b), "scan16_bigk_kernel<%d, %s>", L.kpl, tf(L.imi)); break;
    case ScanPath::scanm:
        snprintf(b, sizeof(b), "scanm_kernel<%d, %d, %d, %s, %d, %d>", s.M, L.kpl, L.nbuf, tf(L.imi), s.table_mode == 0 ? s.dsub : 0,
                 L.nw != vlq::scanm_waves(s.M) ? L.nw : 0);
        break;
    case ScanPath::scanm_short: snprintf(b, sizeof(b), "scanm_short_kernel<%d, %d>", s.M, L.kpl); break;
    case ScanPath::generic: snprintf(b, sizeof(b), "scan_kernel"); break;
    default:
        snprintf(b, sizeof(b), "scan16_kernel<%d, %d, %d, %s, %s, %s>", L.kpl, L.nw, L.nbuf, tf(L.pipe), tf(L.imi), tf(L.owned));
    }
    return b;
}

int main() {
    static const char* const path_names[] = {"fp16", "owned", "owned2", "scan16_short", "scan16_split", "scan16_bigk", "scan16_tail",
                                             "scan16", "scanm", "scanm_short", "generic"};
    static const char* const order_names[] = {"none", "plain", "walk"};
    const std::vector<std::pair<const char*, ScanShape>> shapes = {
        {"headline", headline()},
        {"headline_slice_1250", batch(1250)},
        {"batch_1500_split_tail", batch(1500)},
        {"batch_64_probe_split", batch(64)},
        {"page_of_a_longer_call", with(headline(), [](ScanShape& s) { s.n = 40000; })},
        {"nprobe_128", with(headline(), [](ScanShape& s) { s.nprobe = 128; })},
        {"k_100", topk(100)},
        {"k_100_nprobe_64", with(topk(100), [](ScanShape& s) { s.nprobe = 64; })},
        {"k_200", topk(200)},
        {"k_600", topk(600)},
        {"k_1000", topk(1000)},
        {"long_lists_k_10", long_lists(10)},
        {"long_lists_k_100", long_lists(100)},
        {"long_lists_k_200", long_lists(200)},
        {"multi_index_m16", multi_index(16)},
        {"multi_index_m8", multi_index(8)},
        {"m8", code_size(8, 128)},
        {"m12", code_size(12, 96)},
        {"m32", code_size(32, 128)},
        {"m64", code_size(64, 128)},
        {"m36_not_engineered", code_size(36, 144)},
        {"fp16_tables", with(headline(), [](ScanShape& s) { s.fp16_tables = true; })},
        {"schedule_2", with(headline(), [](ScanShape& s) { s.scan_schedule = 2; })},
        {"schedule_2_k_600", with(topk(600), [](ScanShape& s) { s.scan_schedule = 2; })},
        {"schedule_3", with(headline(), [](ScanShape& s) { s.scan_schedule = 3; })},
        {"schedule_4", with(headline(), [](ScanShape& s) { s.scan_schedule = 4; })},
        {"variant_1", with(headline(), [](ScanShape& s) { s.scan16_variant = 1; })},
        {"variant_4_slice_1250", with(batch(1250), [](ScanShape& s) { s.scan16_variant = 4; })},
        {"generic_scan_m8", with(code_size(8, 128), [](ScanShape& s) { s.generic_scan = true; })},
        {"generic_scan_m16", with(headline(), [](ScanShape& s) { s.generic_scan = true; })},
        {"walk_first_forced_off", with(headline(), [](ScanShape& s) { s.walk_first = -1; })},
        {"table_mode_0", with(headline(), [](ScanShape& s) { s.table_mode = 0; })},
        {"table_mode_2", with(headline(), [](ScanShape& s) { s.table_mode = 2; })},
        {"tail_page_1", tail_page(1)},
        {"tail_page_7", tail_page(7)},
        {"tail_page_100", tail_page(100)},
        {"tail_page_1100", tail_page(1100)},
        {"tail_page_1500", tail_page(1500)},
        {"tail_page_3100", tail_page(3100)},
        {"tail_page_1500_m8", tail_page(1500, 8, 32, 8)},
        {"tail_page_3100_m8", tail_page(3100, 8, 32, 8)},
    };
    for (const auto& [name, s] : shapes) {
        const vlq::ScanPlan p = vlq::plan_scan(s);
        const vlq::ScanLaunch& L = p.launch;
        printf("%s: path=%s kernel=%s fused=%d order=%s rank=%d hist=%d walk_first=%d auto=%d full=%d class=%d seed_slots=%d "
               "tail_slots=%d long=%d nsplit=%d tail=%dx%d chunk=%d grid=%d lut=%d lds=%zu\n",
               name, path_names[(int)p.path], kernel_name(s, p).c_str(), (int)p.fused_tables, order_names[(int)p.order],
               (int)p.order_by_rank, (int)p.order_hist_ready, p.walk_first, (int)p.walk_auto, (int)p.walk_limit_full, p.walk_class,
               p.walk_seed_slots, p.tail_slots, (int)p.long_lists, L.nsplit, L.tail_r, L.tail_p, L.xcd_chunk, L.grid_per_xcd,
               L.lut_region, L.lds_bytes);
    }
    return 0;
}
