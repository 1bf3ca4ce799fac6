// TEST INFRASTRUCTURE (tests/devfn/libdevfn.so, never part of libunidom_hip.so): the f64 device math of unidom_amd/csrc/plb_common.h -- dsvd3
// (one matrix per lane) and the seed + Newton reciprocal / sqrt / rsqrt it is built on -- compiled with the flags of plb.o (the Makefile's
// default rule, -ffp-contract=off).
#include "../../unidom_amd/csrc/plb_common.h"

namespace {

// Launchers: device pointers and a count, launched on the null stream, the hipError_t returned.
// A, U, Vh [n][9] row-major, S [n][3].  Lanes past n leave before the SVD: the last wave runs dsvd3's __any with inactive lanes.
__global__ void dsvd3_kernel(const double* __restrict__ A, double* __restrict__ U, double* __restrict__ S, double* __restrict__ Vh, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a[9], u[9], s[3], vh[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) a[k] = A[i * 9 + k];
  ud::dsvd3(a, u, s, vh);
#pragma unroll
  for (int k = 0; k < 9; ++k) { U[i * 9 + k] = u[k]; Vh[i * 9 + k] = vh[k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) S[i * 3 + k] = s[k];
}

template <int OP>   // 0 ud_rcp_nr, 1 ud_sqrt_nr, 2 ud_rsqrt_nr
__global__ void nr_kernel(const double* __restrict__ x, double* __restrict__ y, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = OP == 0 ? ud::ud_rcp_nr(x[i]) : (OP == 1 ? ud::ud_sqrt_nr(x[i]) : ud::ud_rsqrt_nr(x[i]));
}

template <int OP>
int launch_nr(const double* x, double* y, long n) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(nr_kernel<OP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, x, y, n);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int devfn_dsvd3(const double* A, double* U, double* S, double* Vh, long n) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(dsvd3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, A, U, S, Vh, n);
  return (int)hipGetLastError();
}
int devfn_rcp_nr(const double* x, double* y, long n) { return launch_nr<0>(x, y, n); }
int devfn_sqrt_nr(const double* x, double* y, long n) { return launch_nr<1>(x, y, n); }
int devfn_rsqrt_nr(const double* x, double* y, long n) { return launch_nr<2>(x, y, n); }

}  // extern "C"
