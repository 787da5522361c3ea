// prints plan_flat_range (csrc/range_plan.h) of the shapes given on the command line as "d nprobe" pairs: host compiler only,
// neither the library nor the HIP runtime (tests/test_range_plan.py)
#include <cstdio>
#include <cstdlib>

#include "range_plan.h"

int main(int argc, char** argv) {
    for (int i = 1; i + 1 < argc; i += 2) {
        const int d = atoi(argv[i]), nprobe = atoi(argv[i + 1]);
        const vlq::RangePlan p = vlq::plan_flat_range(d, nprobe);
        if (!p.ok) { printf("d=%d nprobe=%d: unsupported\n", d, nprobe); continue; }
        printf("d=%d nprobe=%d: read=%s xch=%d meta=%d sq=%d lds=%zu\n", d, nprobe, vlq::flat_read_name(p.read), p.lay.xch, p.lay.meta,
               p.lay.sq, p.lay.bytes);
    }
    return 0;
}
