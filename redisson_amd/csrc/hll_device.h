// hll_device.h -- the PFCOUNT estimator's tail (redis hllCount, Ertl) for the kernels that end in it: k_hll_count
// (hll_kernels.hip) and the grouped union count (hllgroups_kernels.hip).  One copy, so the two cannot drift:
// the Makefile's -ffp-contract=off keeps a*b+c as two IEEE operations in both.
#pragma once
#include <hip/hip_runtime.h>

namespace rbx {

__device__ inline double hll_sigma(double x) {
    if (x == 1.) return __builtin_inf();
    double zPrime;
    double y = 1;
    double z = x;
    do {
        x *= x;
        zPrime = z;
        z += x * y;
        y += y;
    } while (zPrime != z);
    return z;
}

// The cardinality of a 64-bin register histogram over 16384 registers, or ~0 when a register holds 51: the
// hllTau branch, which the host evaluates with glibc pow (redis semantics).
__device__ inline unsigned long long hll_estimate(const int *rh) {
    if (rh[51] != 0) return ~0ULL;
    const double m = 16384;
    double z = 0.0;  // m * hllTau(1.0) == 0
    for (int j = 50; j >= 1; --j) {
        z += rh[j];
        z *= 0.5;
    }
    z += m * hll_sigma(rh[0] / (double)m);
    const double E = (double)llround(0.721347520444481703680 * m * m / z);
    return (unsigned long long)E;
}

}  // namespace rbx
