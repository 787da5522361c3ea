// prints plan_refine_flat (csrc/refine_flat_plan.h) of the shapes given on the command line as "d k_base k select" groups of
// four: host compiler only, neither the library nor the HIP runtime (tests/test_refine_flat_plan.py)
#include <cstdio>
#include <cstdlib>

#include "refine_flat_plan.h"

int main(int argc, char** argv) {
    for (int i = 1; i + 3 < argc; i += 4) {
        const int d = atoi(argv[i]), k_base = atoi(argv[i + 1]), k = atoi(argv[i + 2]), select = atoi(argv[i + 3]);
        const vlq::RefineFlatPlan p = vlq::plan_refine_flat(d, k_base, k, select != 0);
        printf("d=%d k_base=%d k=%d select=%d: ", d, k_base, k, select);
        if (!p.ok) { printf("%s (%s)\n", p.err == 2 ? "unsupported" : "invalid", p.why); continue; }
        printf("read=%s trips=%d slots=%d waves=%d page=%lld keys=%d labels=%d sq=%d lds=%zu\n", vlq::flat_read_name(p.read), p.trips, p.slots,
               p.waves, (long long)p.page, p.lay.keys, p.lay.labels, p.lay.sq, p.lds);
    }
    return 0;
}
