// TEST INFRASTRUCTURE (tests/devfn/libdevfn.so, never part of libunidom_hip.so): svd3 of unidom_amd/csrc/mpm_device.h, one matrix per lane.
// Compiled twice by the `devfn` target of unidom_amd/csrc/Makefile, each time with exactly the flags of the product object that uses the
// function: $(MPMFLAGS) as mpm.o / mpm_large.o (-> devfn_svd3_fast), and -ffp-contract=off -DUD_MPM_EXACT=1 as mpm_det.o (-> devfn_svd3_exact
// and devfn_expf, the deterministic mode's plain-IEEE exp of mpm_collide.h).
#include "../../unidom_amd/csrc/mpm_collide.h"

#ifdef UD_MPM_EXACT
#define DEVFN_SVD3 devfn_svd3_exact
#define DEVFN_SVD3_KERNEL svd3_exact_kernel
#else
#define DEVFN_SVD3 devfn_svd3_fast
#define DEVFN_SVD3_KERNEL svd3_fast_kernel
#endif

namespace {

// The launchers take device pointers and a count, launch on the null stream (which is torch's current stream unless a test changes it; the
// tests synchronise the device before reading) and return the hipError_t.
// A, U, Vh [n][9] row-major, S [n][3].  Lanes past n leave before the SVD: the last wave runs svd3's __any with inactive lanes.
__global__ void DEVFN_SVD3_KERNEL(const float* __restrict__ A, float* __restrict__ U, float* __restrict__ S, float* __restrict__ Vh, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float a[9], u[9], s[3], vh[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) a[k] = A[i * 9 + k];
  ud::svd3(a, u, s, vh);
#pragma unroll
  for (int k = 0; k < 9; ++k) { U[i * 9 + k] = u[k]; Vh[i * 9 + k] = vh[k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) S[i * 3 + k] = s[k];
}

#ifdef UD_MPM_EXACT
__global__ void expf_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = ud::ud_expf(x[i]);
}
#endif

}  // namespace

extern "C" {

int DEVFN_SVD3(const float* A, float* U, float* S, float* Vh, long n) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(DEVFN_SVD3_KERNEL, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, A, U, S, Vh, n);
  return (int)hipGetLastError();
}

#ifdef UD_MPM_EXACT
int devfn_expf(const float* x, float* y, long n) {
  if (n <= 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(expf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, x, y, n);
  return (int)hipGetLastError();
}
#endif

}  // extern "C"
