// prints plan_sqflat_scan (csrc/sqflat_plan.h) of the shapes given on the command line as "nq ntotal d qtype k force_q force_s"
// groups of seven: host compiler only, neither the library nor the HIP runtime (tests/test_sqflat_plan.py)
#include <cstdio>
#include <cstdlib>

#include "sqflat_plan.h"

int main(int argc, char** argv) {
    for (int i = 1; i + 6 < argc; i += 7) {
        const long long nq = atoll(argv[i]), ntotal = atoll(argv[i + 1]);
        const int d = atoi(argv[i + 2]), qt = atoi(argv[i + 3]), k = atoi(argv[i + 4]), fq = atoi(argv[i + 5]), fs = atoi(argv[i + 6]);
        const vlq::SqFlatPlan p = vlq::plan_sqflat_scan(nq, ntotal, d, qt, k, fq, fs);
        printf("nq=%lld ntotal=%lld d=%d qtype=%d k=%d fq=%d fs=%d: ", nq, ntotal, d, qt, k, fq, fs);
        if (!p.ok) { printf("unsupported (%s)\n", p.why); continue; }
        printf("Q=%d S=%d kpl=%d order8=%d read=%s bits=%d uniform=%d code_size=%d join=%d slice=%lld page=%lld selq=%d sq=%d vmin=%d vdiff=%d lds=%zu\n",
               p.Q, p.S, p.kpl, (int)p.order8, vlq::sq_read_name(p.read), p.bits, (int)p.uniform, p.code_size, (int)p.join, (long long)p.slice_len,
               (long long)p.page, p.lay.selq, p.lay.sq, p.lay.vmin, p.lay.vdiff, p.lay.bytes);
    }
    return 0;
}
