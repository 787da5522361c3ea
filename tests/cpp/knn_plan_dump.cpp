// prints plan_knn (csrc/knn_plan.h) of the shapes given on the command line as "nq ntotal d k force_rows force_s" groups of six:
// host compiler only, neither the library nor the HIP runtime (tests/test_knn_plan.py)
#include <cstdio>
#include <cstdlib>

#include "knn_plan.h"

int main(int argc, char** argv) {
    for (int i = 1; i + 5 < argc; i += 6) {
        const long long nq = atoll(argv[i]), ntotal = atoll(argv[i + 1]);
        const int d = atoi(argv[i + 2]), k = atoi(argv[i + 3]), fr = atoi(argv[i + 4]), fs = atoi(argv[i + 5]);
        const vlq::KnnPlan p = vlq::plan_knn(nq, ntotal, d, k, fr, fs);
        printf("nq=%lld ntotal=%lld d=%d k=%d fr=%d fs=%d: ", nq, ntotal, d, k, fr, fs);
        if (!p.ok) { printf("unsupported (%s)\n", p.why); continue; }
        printf("path=%s route=%s rows=%d S=%d kpl=%d join=%d slice=%lld chunk=%lld page=%lld lds=%zu scratch=%zu\n", vlq::knn_path_name(p.path),
               vlq::knn_route_name(p.route), p.rows, p.S, p.kpl, (int)p.join, (long long)p.slice_len, (long long)p.chunk, (long long)p.page, p.lds,
               p.scratch);
    }
    return 0;
}
