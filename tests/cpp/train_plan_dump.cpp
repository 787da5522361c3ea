// Prints the launch plans of the training kernels (csrc/kmeans_plan.h, pq_train_plan.h, moments_plan.h): host compiler only,
// over tests/cpp/hip_stub.  One shape per line of standard input, one plan per line of output:
//   pq n d M nbits            plan_pq_assign
//   km n k d                  plan_kmeans_update
//   mom n dx dy sym kr fs     plan_moments (sym 1: the symmetric case, dy ignored; kr / fs: what set_split forces, 0 = the plan's)
// tests/test_train_plans.py compares the output with values written by hand from the headers' rules.
#include "kmeans_plan.h"
#include "moments_plan.h"
#include "pq_train_plan.h"

#include <cstdio>
#include <cstring>

int main() {
    char kind[16];
    long long v[6];
    while (scanf("%15s", kind) == 1) {
        const int want = !strcmp(kind, "pq") ? 4 : !strcmp(kind, "km") ? 3 : !strcmp(kind, "mom") ? 6 : 0;
        if (!want) { fprintf(stderr, "unknown plan '%s'\n", kind); return 2; }
        for (int i = 0; i < want; i++)
            if (scanf("%lld", &v[i]) != 1) { fprintf(stderr, "%s: %d numbers expected\n", kind, want); return 2; }
        if (want == 4) {
            const vlq::PqTrainPlan p = vlq::plan_pq_assign(v[0], (int)v[1], (int)v[2], (int)v[3]);
            if (!p.ok) { printf("pq n=%lld d=%lld M=%lld nbits=%lld: unsupported (%s)\n", v[0], v[1], v[2], v[3], p.why); continue; }
            printf("pq n=%lld d=%lld M=%lld nbits=%lld: route=%s dsub=%d ksub=%d cols=%d kq=%d stride=%d group=%d ngroups=%d vec=%d lds=%zu grid=%ux%u why=%s\n",
                   v[0], v[1], v[2], v[3], p.route_name, p.dsub, p.ksub, p.cols, p.kq, p.stride, p.group, p.ngroups, p.vec ? 1 : 0, p.lds, p.grid.x,
                   p.grid.y, p.why);
        } else if (want == 3) {
            const vlq::KMeansPlan p = vlq::plan_kmeans_update(v[0], v[1], (int)v[2]);
            printf("km n=%lld k=%lld d=%lld: kernel=%s packed=%d waves=%d slices=%d key_row_bits=%d key_bits=%d grid=%ux%u\n", v[0], v[1], v[2], p.kernel,
                   p.packed ? 1 : 0, p.waves, p.slices, p.key_row_bits, p.key_bits, p.grid.x, p.grid.y);
        } else {
            const bool sym = v[3] != 0;
            const vlq::MomentsPlan p = vlq::plan_moments(v[0], (int)v[1], sym ? (int)v[1] : (int)v[2], sym, (int)v[4], (int)v[5]);
            printf("mom n=%lld dx=%lld dy=%lld sym=%d kr=%lld fs=%lld: kr=%d tiles=%dx%d pairs=%d S=%d slice_len=%lld lds=%zu scratch=%zu col_slices=%d "
                   "col_slice_len=%lld\n",
                   v[0], v[1], v[2], sym ? 1 : 0, v[4], v[5], p.kr, p.tiles_x, p.tiles_y, p.pairs, p.S, (long long)p.slice_len, p.lds, p.scratch,
                   p.col_slices, (long long)p.col_slice_len);
        }
    }
    return 0;
}
