// Host-compiler stand-in for <hip/hip_runtime.h>: the three names the training plan headers (kmeans_plan.h, pq_train_plan.h,
// moments_plan.h) take from it.  Their plan functions are pure host code; the launch declarations beside them only need the types
// to exist.  tests/test_train_plans.py puts this directory in front of the include path, so the test runs without a HIP toolchain.
#pragma once

struct dim3 {
    unsigned x, y, z;
    constexpr dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
typedef struct ihipStream_t* hipStream_t;
typedef int hipError_t;
