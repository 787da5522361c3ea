// Error bound of the 16-byte scan's screened distance (scan16.hip, the stored-sums loop).  Plain C++, host and device
// (like placement_key.h): tests/cpp/scan_sum_bound_check.cpp draws tables and asserts it on the CPU.
//
// For one stored code (c_0 .. c_15) of list l and one query, with t_m = term2[l][m][c_m], q_m = (-2 <x_m, cent>)[m][c_m],
// every operation an fp32 add rounded to nearest (u = 2^-24), the kernels form
//   D = (..((dis0 + fl(t_0 + q_0)) + fl(t_1 + q_1)) .. + fl(t_15 + q_15))                the reference's value
//   S = (..((t_0 + t_1) + t_2) .. + t_15)                                                stored per code (code_sums)
//   A = (..((fl(dis0 + S) + q_0) + q_1) .. + q_15)                                       what the running selection sees
// t_m and q_m enter both values as the same stored floats, so only the additions differ.  With the usual bound of a
// recursive sum of n additions, |fl(sum) - sum| <= g(n) * sum of magnitudes, g(n) = n u / (1 - n u):
//   D:  16 entry roundings, u * |t_m + q_m| each, carried through at most 16 further additions: <= u (1 + g(16)) T
//       the chain of 16 additions over dis0 and the rounded entries:                             <= g(16) (1 + u) T
//   S:  15 additions:                                                                              <= g(15) T
//   A:  17 additions over dis0, S and the q_m, |S| <= (1 + g(15)) T:                               <= g(17) (1 + g(15)) T
// where T = |dis0| + sum |t_m| + sum |q_m|.  Together (1 + 16 + 15 + 17) u T (1 + 40 u) < 50 u T.  The kernel does not
// know T per code; it uses
//   B = |dis0| + t2abs[l] + qabs >= T,   t2abs[l] = sum_m max_c |term2[l][m][c]|,  qabs = sum_m max_c |q[m][c]|,
// each sum formed in fp32 and rounded up by scan_sum_up(), and
//   eps(B) = 2^-18 * B * (1 + 2^-20) >= 50 * 2^-24 * B * 1.28 :
// the factor 1.28 = 2^-18 / (50 u) is far more than the fp32 rounding of B's own 34 additions (34 u) can take away.
// A non-finite B (a NaN or infinite input) gives a non-finite eps: the caller then does not screen.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VLQ_SSB_HD __host__ __device__ inline
#else
#define VLQ_SSB_HD inline
#endif

namespace vlq {

// x * (1 + 2^-20), at least x for x >= 0: makes an fp32 sum of non-negative terms an upper bound of the exact one (the sum of
// two floats is off by at most 2^-24 of itself; both products here are exact or rounded by less than that)
VLQ_SSB_HD float scan_sum_up(float x) { return x * 1.00000095367431640625f; }

// B of the header comment from its three parts (each already an upper bound)
VLQ_SSB_HD float scan_sum_magnitude(float abs_dis0, float t2abs, float qabs) {
    return scan_sum_up(scan_sum_up(abs_dis0 + t2abs) + qabs);
}

// eps(B) >= |A - D| for every code whose magnitudes B bounds
VLQ_SSB_HD float scan_sum_bound(float B) { return scan_sum_up(B * 3.814697265625e-06f); }      // 2^-18

}  // namespace vlq
