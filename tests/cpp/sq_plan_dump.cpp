// prints plan_sq_scan (csrc/sq_plan.h) of the shapes given on the command line as "d qtype nprobe k" quadruples: host compiler
// only, neither the library nor the HIP runtime (tests/test_sq_plan.py)
#include <cstdio>
#include <cstdlib>

#include "sq_plan.h"

int main(int argc, char** argv) {
    for (int i = 1; i + 3 < argc; i += 4) {
        const int d = atoi(argv[i]), qtype = atoi(argv[i + 1]), nprobe = atoi(argv[i + 2]), k = atoi(argv[i + 3]);
        const vlq::SqPlan p = vlq::plan_sq_scan(d, qtype, nprobe, k);
        if (!p.ok) { printf("d=%d qtype=%d nprobe=%d k=%d: unsupported\n", d, qtype, nprobe, k); continue; }
        printf("d=%d qtype=%d nprobe=%d k=%d: kpl=%d bits=%d uniform=%d order8=%d code_size=%d read=%s lds=%zu\n", d, qtype, nprobe, k, p.kpl,
               p.bits, (int)p.uniform, (int)p.order8, p.code_size, vlq::sq_read_name(p.read), p.lay.bytes);
    }
    return 0;
}
