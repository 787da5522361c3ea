// prints plan_hamming_scan (csrc/hamming_plan.h) of the shapes given on the command line as "nq ntotal code_size k force_q force_s"
// groups of six: host compiler only, neither the library nor the HIP runtime (tests/test_hamming_plan.py)
#include <cstdio>
#include <cstdlib>

#include "hamming_plan.h"

int main(int argc, char** argv) {
    for (int i = 1; i + 5 < argc; i += 6) {
        const long long nq = atoll(argv[i]), ntotal = atoll(argv[i + 1]);
        const int cs = atoi(argv[i + 2]), k = atoi(argv[i + 3]), fq = atoi(argv[i + 4]), fs = atoi(argv[i + 5]);
        const vlq::HamPlan p = vlq::plan_hamming_scan(nq, ntotal, cs, k, fq, fs);
        printf("nq=%lld ntotal=%lld cs=%d k=%d fq=%d fs=%d: ", nq, ntotal, cs, k, fq, fs);
        if (!p.ok) { printf("unsupported (%s)\n", p.why); continue; }
        printf("Q=%d S=%d waves=%d kpl=%d load=%d join=%d slice=%lld page=%lld selq=%d qcode=%d lds=%zu\n", p.Q, p.S, p.waves, p.kpl, p.load,
               (int)p.join, (long long)p.slice_len, (long long)p.page, p.lay.selq, p.lay.qcode, p.lay.bytes);
    }
    return 0;
}
