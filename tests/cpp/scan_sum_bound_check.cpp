// CPU check of csrc/scan_sum_bound.h (tests/test_scan_sum_bound.py builds this with -fsanitize=address,undefined): random
// term-2 rows, per-query tables and codes; A (what the stored-sums loop selects on) and D (the reference's value) formed in
// fp32 exactly as scan16.hip forms them; |A - D| <= eps(B) in every case, and a non-finite input gives a non-finite eps.
// Built with -ffp-contract=off -O1: every operation below is one rounded fp32 add.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "scan_sum_bound.h"

static volatile float g_sink;
static float add(float a, float b) { volatile float r = a + b; return r; }      // one rounding, never fused or widened

struct Case { const char* name; float mag_lo, mag_hi, offset; bool cancel; };

int main() {
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    const Case cases[] = {
        {"small", 1e-4f, 1e-2f, 0.f, false},   {"unit", 0.1f, 10.f, 0.f, false},       {"bytes", 1e3f, 1e6f, 0.f, false},
        {"mixed", 1e-4f, 1e6f, 0.f, false},    {"cancel", 1e2f, 1e5f, 0.f, true},      {"offset", 1.f, 50.f, 3e5f, false},
        {"offset-cancel", 1.f, 50.f, 3e5f, true},
    };
    long checked = 0;
    double worst = 0.0;
    for (const Case& c : cases) {
        for (int rep = 0; rep < 40; rep++) {
            std::vector<float> t2(16 * 256), q(16 * 256);
            auto draw = [&](float off) {
                const double m = std::exp(std::log((double)c.mag_lo) + uni(rng) * (std::log((double)c.mag_hi) - std::log((double)c.mag_lo)));
                return (float)((uni(rng) < 0.5 ? -m : m) + off);
            };
            for (int i = 0; i < 16 * 256; i++) {
                t2[i] = draw(c.offset);
                // heavy cancellation: the per-query part nearly undoes term 2 (the distance is a small difference of large terms)
                q[i] = c.cancel ? -t2[i] * (float)(1.0 + 1e-3 * (uni(rng) - 0.5)) : draw(-c.offset);
            }
            float t2abs = 0.f, qabs = 0.f;
            for (int m = 0; m < 16; m++) {
                float mt = 0.f, mq = 0.f;
                for (int j = 0; j < 256; j++) { mt = std::fmax(mt, std::fabs(t2[m * 256 + j])); mq = std::fmax(mq, std::fabs(q[m * 256 + j])); }
                t2abs = vlq::scan_sum_up(add(t2abs, mt));
                qabs = vlq::scan_sum_up(add(qabs, mq));
            }
            for (int code = 0; code < 500; code++) {
                const float dis0 = c.cancel && (code & 1) ? -draw(0.f) * 16.f : std::fabs(draw(c.offset)) * 16.f;
                int cm[16];
                for (int m = 0; m < 16; m++) cm[m] = (int)(rng() & 255);
                float D = dis0;
                for (int m = 0; m < 16; m++) D = add(D, add(t2[m * 256 + cm[m]], q[m * 256 + cm[m]]));
                float S = t2[cm[0]];
                for (int m = 1; m < 16; m++) S = add(S, t2[m * 256 + cm[m]]);
                float A = add(dis0, S);
                for (int m = 0; m < 16; m++) A = add(A, q[m * 256 + cm[m]]);
                const float B = vlq::scan_sum_magnitude(std::fabs(dis0), t2abs, qabs);
                const float eps = vlq::scan_sum_bound(B);
                const double err = std::fabs((double)A - (double)D);
                if (!(err <= (double)eps)) {
                    std::printf("FAIL %s: A=%.9g D=%.9g |A-D|=%.9g eps=%.9g B=%.9g\n", c.name, A, D, err, eps, B);
                    return 1;
                }
                if (eps > 0.f && err / eps > worst) worst = err / eps;
                checked++;
            }
        }
    }
    const float inf = INFINITY, nan = NAN;
    const float bad[][3] = {{inf, 1.f, 1.f}, {1.f, inf, 1.f}, {1.f, 1.f, inf}, {nan, 1.f, 1.f}, {1.f, nan, 1.f}, {1.f, 1.f, nan}, {3e38f, 3e38f, 1.f}};
    for (const auto& b : bad) {
        const float eps = vlq::scan_sum_bound(vlq::scan_sum_magnitude(b[0], b[1], b[2]));
        if (std::isfinite(eps)) { std::printf("FAIL: finite eps %.9g for a non-finite magnitude\n", eps); return 1; }
    }
    g_sink = (float)worst;
    std::printf("OK %ld codes, worst |A-D| / eps = %.4f\n", checked, worst);
    return 0;
}
