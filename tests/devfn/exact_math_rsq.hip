// TEST INFRASTRUCTURE (tests/devfn/libdevfn.so, never part of libunidom_hip.so): exhaustive sweeps of exact_math.h's select-free
// 1 / sqrt (rcp_sqrt_rn_rsq2x4 and its scalar form rcp_sqrt_rn_rsq) over ranges of f32 bit patterns, compared on the device with the
// function they replace; compiled with -ffp-contract=off as the objects that use them.  Plus the host-side guard of the isV use.
#include "../../unidom_amd/csrc/cloth_v2_force.h"

namespace {

// the compiler's own IEEE expansion: what cloth_v2.hip's isV was before, and is where the launch's constants fail the guard
__device__ __forceinline__ float rcp_sqrt_compiler(float x) { return 1.0f / sqrtf(x); }

__device__ __forceinline__ bool same(float a, float b) {
  return __builtin_bit_cast(unsigned, a) == __builtin_bit_cast(unsigned, b) || (a != a && b != b);
}

// Patterns lo .. hi (inclusive), eight consecutive ones per lane and trip (a tail group repeats hi).
// AGAINST_COMPILER = false: pair form and scalar form against rcp_sqrt_rn_inrange2x4;  true: scalar form against 1.0f / sqrtf(x).
// res[0] = mismatching patterns of the pair form, res[1] = of the scalar form, res[2] = the lowest mismatching pattern (~0 if none).
template <bool AGAINST_COMPILER>
__global__ void __launch_bounds__(256) sweep_kernel(unsigned lo, unsigned hi, unsigned long long* res) {
  const unsigned long long groups = ((unsigned long long)(hi - lo) + 8ull) / 8ull;
  unsigned long long bad2 = 0, bad1 = 0, first = ~0ull;
  for (unsigned long long gi = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (unsigned long long)gridDim.x * blockDim.x) {
    ud::f2 x[4], want[4], got[4];
    unsigned pat[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const unsigned long long p = (unsigned long long)lo + gi * 8ull + q;
      pat[q] = p > hi ? hi : (unsigned)p;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) x[p] = ud::f2{__builtin_bit_cast(float, pat[2 * p]), __builtin_bit_cast(float, pat[2 * p + 1])};
    if (AGAINST_COMPILER) {
#pragma unroll
      for (int p = 0; p < 4; ++p) want[p] = ud::f2{rcp_sqrt_compiler(x[p].x), rcp_sqrt_compiler(x[p].y)};
    } else {
      ud::rcp_sqrt_rn_inrange2x4(x, want);
      ud::rcp_sqrt_rn_rsq2x4(x, got);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float xq = q & 1 ? x[q >> 1].y : x[q >> 1].x, wq = q & 1 ? want[q >> 1].y : want[q >> 1].x;
      const bool dup = q > 0 && pat[q] == pat[q - 1];
      const bool b2 = !AGAINST_COMPILER && !same(q & 1 ? got[q >> 1].y : got[q >> 1].x, wq);
      const bool b1 = !same(ud::rcp_sqrt_rn_rsq(xq), wq);
      if (!dup && b2) ++bad2;
      if (!dup && b1) ++bad1;
      if ((b1 || b2) && pat[q] < first) first = pat[q];
    }
  }
  if (bad2) atomicAdd(&res[0], bad2);
  if (bad1) atomicAdd(&res[1], bad1);
  if (first != ~0ull) atomicMin(&res[2], first);
}

}  // namespace

extern "C" {

// res: three device uint64, res[0] = res[1] = 0 and res[2] = ~0 on entry (the caller accumulates several ranges into one triple)
int devfn_rcp_sqrt_rsq_sweep(unsigned lo, unsigned hi, int against_compiler, unsigned long long* res) {
  if (hi < lo) return (int)hipErrorInvalidValue;
  const unsigned long long groups = ((unsigned long long)(hi - lo) + 8ull) / 8ull;
  const unsigned blocks = (unsigned)(groups < 256ull * 8 * 256 ? (groups + 255) / 256 : 256 * 8);
  if (against_compiler) hipLaunchKernelGGL(sweep_kernel<true>, dim3(blocks), dim3(256), 0, 0, lo, hi, res);
  else hipLaunchKernelGGL(sweep_kernel<false>, dim3(blocks), dim3(256), 0, 0, lo, hi, res);
  return (int)hipGetLastError();
}

// host only: the per-launch check that lets cloth_v2.hip / cloth_cluster_fwd.hip use rcp_sqrt_rn_rsq for isV
int devfn_cloth_isv_consts_ok(float small_num, float max_v) {
  ud::ClothConst c = {};
  c.eps = small_num; c.max_v = max_v;
  return ud::cloth_isv_consts_ok(c) ? 1 : 0;
}

}  // extern "C"
