// prints plan_pq_scan (csrc/pq_plan.h) of the shapes given on the command line as "nq ntotal M ksub k search_type force_q force_s"
// groups of eight: host compiler only, neither the library nor the HIP runtime (tests/test_pq_plan.py)
#include <cstdio>
#include <cstdlib>

#include "pq_plan.h"

int main(int argc, char** argv) {
    for (int i = 1; i + 7 < argc; i += 8) {
        const long long nq = atoll(argv[i]), ntotal = atoll(argv[i + 1]);
        const int M = atoi(argv[i + 2]), ksub = atoi(argv[i + 3]), k = atoi(argv[i + 4]), st = atoi(argv[i + 5]);
        const int fq = atoi(argv[i + 6]), fs = atoi(argv[i + 7]);
        const vlq::PqPlan p = vlq::plan_pq_scan(nq, ntotal, M, ksub, k, st, fq, fs);
        printf("nq=%lld ntotal=%lld M=%d ksub=%d k=%d st=%d fq=%d fs=%d: ", nq, ntotal, M, ksub, k, st, fq, fs);
        if (!p.ok) { printf("unsupported (%s)\n", p.why); continue; }
        printf("Q=%d S=%d waves=%d kpl=%d order=%d filter=%d load=%d join=%d slice=%lld page=%lld lds=%zu\n", p.Q, p.S, p.waves, p.kpl, p.order,
               p.filter, p.load, (int)p.join, (long long)p.slice_len, (long long)p.page, p.lay.bytes);
    }
    return 0;
}
