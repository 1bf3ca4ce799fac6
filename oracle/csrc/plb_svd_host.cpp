// TEST INFRASTRUCTURE.  dsvd3 of the f64 kernels (unidom_amd/csrc/plb_svd.h, the device's own source) compiled by the host compiler, for
// tests/test_devfn_cpu.py.  The three hardware seeds become IEEE operations here -- exact where the device's have >= 14 good bits -- so
// this build shares the device's algorithm (sweeps, thresholds, Newton steps, FMAs), not its bits: the tests hold both to the same bars.
#define UD_HOST_BUILD 1
#include <cmath>
#define __builtin_amdgcn_rcp(x) (1.0 / (x))
#define __builtin_amdgcn_rsq(x) (1.0 / std::sqrt(x))
#define __any(x) (x)

#include "../../unidom_amd/csrc/plb_svd.h"

extern "C" {

// A, U, Vh [n][9] row-major, S [n][3]
void oc_dev_dsvd3_f64(long n, const double* A, double* U, double* S, double* Vh) {
  for (long i = 0; i < n; ++i) ud::dsvd3(A + i * 9, U + i * 9, S + i * 3, Vh + i * 9);
}

}  // extern "C"
