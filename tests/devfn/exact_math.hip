// TEST INFRASTRUCTURE (tests/devfn/libdevfn.so, never part of libunidom_hip.so): every function of unidom_amd/csrc/exact_math.h, one element
// (pair forms: one pair; the 2x4 form: eight elements) per lane, compiled with -ffp-contract=off as the objects that use them.
#include "../../unidom_amd/csrc/exact_math.h"

// Launchers: device pointers and a count, launched on the null stream, the hipError_t returned.
namespace {

enum { SQRT_INRANGE, RCP_INRANGE, SQRT_ANY, SQRT_INRANGE2, RCP_INRANGE2, RCP_SQRT_2X4 };
enum { DIV_ANY, DIV_PREPPED, DIV_PREPPED_NZ, DIV_SHARED };

template <int OP>
__global__ void unary_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (OP == SQRT_INRANGE || OP == RCP_INRANGE || OP == SQRT_ANY) {
    if (i >= n) return;
    y[i] = OP == SQRT_INRANGE ? ud::sqrt_rn_inrange(x[i]) : (OP == RCP_INRANGE ? ud::rcp_rn_inrange(x[i]) : ud::sqrt_rn(x[i]));
  } else if (OP == SQRT_INRANGE2 || OP == RCP_INRANGE2) {     // n is a multiple of 2 (the launcher checks)
    if (i * 2 >= n) return;
    const ud::f2 v = {x[i * 2], x[i * 2 + 1]};
    const ud::f2 r = OP == SQRT_INRANGE2 ? ud::sqrt_rn_inrange2(v) : ud::rcp_rn_inrange2(v);
    y[i * 2] = r.x; y[i * 2 + 1] = r.y;
  } else {                                                     // n is a multiple of 8
    if (i * 8 >= n) return;
    ud::f2 v[4], r[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) v[p] = ud::f2{x[i * 8 + 2 * p], x[i * 8 + 2 * p + 1]};
    ud::rcp_sqrt_rn_inrange2x4(v, r);
#pragma unroll
    for (int p = 0; p < 4; ++p) { y[i * 8 + 2 * p] = r[p].x; y[i * 8 + 2 * p + 1] = r[p].y; }
  }
}

template <int OP>
__global__ void div_kernel(const float* __restrict__ a, const float* __restrict__ d, float* __restrict__ q, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float ai = a[i], di = d[i];
  q[i] = OP == DIV_ANY ? ud::div_rn(ai, di)
       : OP == DIV_PREPPED ? ud::div_rn_prepped(ai, di, ud::div_prep(di))
       : OP == DIV_PREPPED_NZ ? ud::div_rn_prepped_nz(ai, di, ud::div_prep(di))
                              : ud::div_rn_shared(ai, di, ud::div_prep(di), ud::div_den_inrange(di));
}

template <int OP, int PER_LANE>
int launch_unary(const float* x, float* y, long n) {
  if (n <= 0 || n % PER_LANE) return (int)hipErrorInvalidValue;
  const long lanes = n / PER_LANE;
  hipLaunchKernelGGL(unary_kernel<OP>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, 0, x, y, n);
  return (int)hipGetLastError();
}
template <int OP>
int launch_div(const float* a, const float* d, float* q, long n) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(div_kernel<OP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, a, d, q, n);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int devfn_sqrt_rn_inrange(const float* x, float* y, long n) { return launch_unary<SQRT_INRANGE, 1>(x, y, n); }
int devfn_rcp_rn_inrange(const float* x, float* y, long n) { return launch_unary<RCP_INRANGE, 1>(x, y, n); }
int devfn_sqrt_rn(const float* x, float* y, long n) { return launch_unary<SQRT_ANY, 1>(x, y, n); }
int devfn_sqrt_rn_inrange2(const float* x, float* y, long n) { return launch_unary<SQRT_INRANGE2, 2>(x, y, n); }
int devfn_rcp_rn_inrange2(const float* x, float* y, long n) { return launch_unary<RCP_INRANGE2, 2>(x, y, n); }
int devfn_rcp_sqrt_rn_inrange2x4(const float* x, float* y, long n) { return launch_unary<RCP_SQRT_2X4, 8>(x, y, n); }
int devfn_div_rn(const float* a, const float* d, float* q, long n) { return launch_div<DIV_ANY>(a, d, q, n); }
int devfn_div_rn_prepped(const float* a, const float* d, float* q, long n) { return launch_div<DIV_PREPPED>(a, d, q, n); }
int devfn_div_rn_prepped_nz(const float* a, const float* d, float* q, long n) { return launch_div<DIV_PREPPED_NZ>(a, d, q, n); }
int devfn_div_rn_shared(const float* a, const float* d, float* q, long n) { return launch_div<DIV_SHARED>(a, d, q, n); }

}  // extern "C"
