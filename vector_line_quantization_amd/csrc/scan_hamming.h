// Internal: what crosses scan_hamming.hip and lsh_api.hip (faiss::IndexLSH on the device).
#pragma once
#include "hamming_plan.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vlq {

// apply_preprocess + fvecs2bitvecs (IndexLSH.cpp:50-81, hamming.cpp:353-379) of n rows x [n][d].
//   At != nullptr   rotate_data: xt[j] = fmaf chain over i = 0 .. d-1 ascending of A[j * d + i] * x[i], starting from b[j] (b ==
//                   nullptr: from 0.0f).  At is the TRANSPOSE of rrot.A, [d][nbits], so that the 64 lanes of a wave read one line.
//   At == nullptr   xt[j] = x[j], the first nbits components (d >= nbits)
//   thr != nullptr  xt[j] = xt[j] - thr[j], one subtraction, after the transform
// bit j of the code = xt[j] >= 0 (-0.0f sets it, NaN does not); dimension 0 is the least significant bit of byte 0; the code has
// (nbits + 7) / 8 bytes, pad bits zero.  One wave ballot gives 64 bits of a code.  xt_out [n][nbits] and codes_out
// [n][(nbits + 7) / 8]: either may be nullptr and is then not written -- a row of xt reaches memory only on request.
void launch_lsh_encode(const float* x, int64_t n, int d, int nbits, const float* At, const float* b, const float* thr, float* xt_out,
                       uint8_t* codes_out, hipStream_t s);

// hammings_knn (hamming.cpp:264-341, :474-506) of one page of query codes [nq][code_size] against codes [ntotal][code_size].
// Grid, tile, slices and LDS are plan_hamming_scan's decision (hamming_plan.h); the caller copies its S and slice_len here.
// part: [nq][S][k] keys of scratch when S > 1.  Rows ascending by (distance, position), padded (float)INT_MAX / -1
// (Heap.h:76-78, IndexLSH.cpp:154-155).  false: not built.
struct HamScanArgs {
    const uint8_t* codes;
    const uint8_t* qcodes;
    float* D;
    int64_t* I;
    unsigned long long* part;
    int64_t nq, ntotal, slice_len;
    int code_size, k, S;
};
bool launch_scan_hamming(const HamScanArgs& a, const HamPlan& P, hipStream_t s);

}  // namespace vlq
