// prints plan_knn_range (csrc/knn_range_plan.h) of the shapes given on the command line as "nq ntotal d force_rows force_s"
// groups: host compiler only, neither the library nor the HIP runtime (tests/test_knn_range_plan.py)
#include <cstdio>
#include <cstdlib>

#include "knn_range_plan.h"

int main(int argc, char** argv) {
    for (int i = 1; i + 4 < argc; i += 5) {
        const long long nq = atoll(argv[i]), ntotal = atoll(argv[i + 1]);
        const int d = atoi(argv[i + 2]), fr = atoi(argv[i + 3]), fs = atoi(argv[i + 4]);
        const vlq::KnnRangePlan p = vlq::plan_knn_range(nq, ntotal, d, fr, fs);
        printf("nq=%lld ntotal=%lld d=%d force=%d,%d: ", nq, ntotal, d, fr, fs);
        if (!p.ok) { printf("%s (%s)\n", p.err == 2 ? "unsupported" : "invalid", p.why); continue; }
        printf("path=%s rows=%d S=%d slice=%lld page=%lld lds=%zu scratch=%zu\n", vlq::knn_path_name(p.path), p.rows, p.S, (long long)p.slice_len,
               (long long)p.page, p.lds, p.scratch);
    }
    return 0;
}
