// Cloth DEPTH observation: the top-down height map of the particle cloud, forward and adjoint.
//   state_to_depth  core/envs/basic/cloth_env.py:71-92
//     points = x + (0, z_offset, 0); iz = argsort(points.y); px = clip(floor(x / pixel_size), 0, W-1),
//     py = clip(floor(z / pixel_size), 0, H-1); heightmap = zeros.at[py, px].set(points.y)
// Op by op that is an argsort, a gather, two divides, floors, clips and a scatter whose duplicate-index order the device leaves
// open.  Here it is one launch, one workgroup per image, and the winner of a pixel is fixed by the specification: the particle
// that comes last in ascending (height, particle index) order among those landing there (stable argsort, last write wins), NaN
// heights above +inf.  The workgroup
//   1. issues the zero fill of its image (wide stores; they drain while the sort runs),
//   2. packs (pixel | monotone key of h | p) into one u64 per particle and sorts the keys in LDS (bitonic, padded with
//      sentinels to a power of two): an element owns its pixel iff its successor has another pixel,
//   3. after a wait for its fill stores and a workgroup barrier, which order the owners' stores behind the zero fill, stores h
//      at the owned pixels.
// No global atomics, nothing depends on arrival order: the same input gives the same bits on every run.
// x / pixel_size is a true IEEE f32 division (this file is built by the generic -ffp-contract=off rule with hipcc's correctly
// rounded divide): multiplying by 320 instead moves the f32 value just below 84 of the 321 pixel edges into the next pixel.
// The clip is taken on the float before the conversion, so -inf and NaN coordinates land in pixel 0 and +inf in the last one
// (what XLA's CPU convert and clip give) and every index is in range.
// The adjoint is a gather: g_x[p].y = g_img[owner[p]] for the particle that owns its pixel, 0 elsewhere; floor has no gradient.
#include "common.h"

namespace ud {

constexpr int DEPTH_T = 512;          // threads per workgroup
constexpr int DEPTH_MAXPTS = 4096;    // = GLUE_MAXPTS of env_glue.hip, the cloth path's maximum: 32 KB of keys in LDS
constexpr int DEPTH_MAXPIX = 131072;  // pixel index fits the 17 bits above the height key with room for the sentinel
constexpr unsigned long long DEPTH_SENTINEL = ~0ull;   // pixel field above every real pixel: sorts last

// u32 whose unsigned order is the order argsort gives floats: -inf < ... < -0 = +0 < ... < +inf < NaN
__device__ __forceinline__ unsigned int height_key(float h) {
  if (h != h) return 0xFFFFFFFFu;
  const unsigned int u = h == 0.f ? 0u : __builtin_bit_cast(unsigned int, h);   // -0 ties with +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// clip(floor(c / pixel_size), 0, n - 1) on the float, then the conversion; NaN -> 0 (fmaxf returns the number)
__device__ __forceinline__ int pixel_of(float c, float pixel_size, int n) {
  return (int)fminf(fmaxf(floorf(c / pixel_size), 0.f), (float)(n - 1));
}

// grid (M).  key = pixel << 44 | height_key << 12 | p; n = P rounded up to a power of two (>= 2); LDS = n keys.
__global__ void __launch_bounds__(DEPTH_T) depth_fwd_kernel(int P, int n, int H, int W, float pixel_size, float z_offset, int wide,
                                                            const float* __restrict__ x, float* __restrict__ img, int* __restrict__ owner) {
  extern __shared__ unsigned long long keys[];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int HW = H * W;
  const float* xm = x + (size_t)m * P * 3;
  float* im = img + (size_t)m * HW;

  if (wide) {   // HW % 4 == 0 and a 16-byte aligned base
    float4* im4 = (float4*)im;
    const float4 z4 = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < HW / 4; i += DEPTH_T) im4[i] = z4;
  } else {
    for (int i = tid; i < HW; i += DEPTH_T) im[i] = 0.f;
  }

  for (int p = tid; p < n; p += DEPTH_T) {
    unsigned long long k = DEPTH_SENTINEL;
    if (p < P) {
      const int px = pixel_of(xm[p * 3], pixel_size, W), py = pixel_of(xm[p * 3 + 2], pixel_size, H);
      const float h = xm[p * 3 + 1] + z_offset;
      k = ((unsigned long long)(py * W + px) << 44) | ((unsigned long long)height_key(h) << 12) | (unsigned long long)p;
    }
    keys[p] = k;
  }
  __syncthreads();

  // bitonic sort, ascending: every compare-exchange pair (i, i + j) belongs to one thread, so one barrier per stage
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (n >> 1); t += DEPTH_T) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const unsigned long long a = keys[i], b = keys[i + j];
        const bool up = (i & k) == 0;
        if ((a > b) == up) { keys[i] = b; keys[i + j] = a; }
      }
      __syncthreads();
    }
  }
  // the owners' stores go behind the zero fill: every wave retires its own fill stores, then the workgroup meets (by now the
  // fill has drained behind the sort, so the wait is short)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int i = tid; i < P; i += DEPTH_T) {
    const unsigned long long k = keys[i];
    const int pix = (int)(k >> 44), p = (int)(k & 0xFFFull);
    const bool owns = i + 1 == n || (int)(keys[i + 1] >> 44) != pix;
    if (owns) im[pix] = xm[p * 3 + 1] + z_offset;
    if (owner) owner[(size_t)m * P + p] = owns ? pix : -1;
  }
}

// grid (M, blocks over the 3P floats of an image's g_x): g_x is written in full
__global__ void __launch_bounds__(256) depth_bwd_kernel(int P, int HW, const int* __restrict__ owner, const float* __restrict__ g_img,
                                                        float* __restrict__ g_x) {
  const int m = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;
  if (i >= P * 3) return;
  const int p = i / 3;
  float g = 0.f;
  if (i - p * 3 == 1) {
    const int o = owner[(size_t)m * P + p];
    if (o >= 0) g = g_img[(size_t)m * HW + o];
  }
  g_x[(size_t)m * P * 3 + i] = g;
}

}  // namespace ud

using namespace ud;

extern "C" {

int ud_cloth_depth_fwd(int M, int P, int H, int W, float pixel_size, float z_offset, const float* x, float* img, int* owner, void* stream) {
  if (M <= 0 || P <= 0 || H <= 0 || W <= 0 || !x || !img) { set_error("ud_cloth_depth_fwd: bad argument"); return UD_ERR_INVALID; }
  if (P > DEPTH_MAXPTS) { set_error("ud_cloth_depth_fwd: P=%d above the %d keys sorted in LDS", P, DEPTH_MAXPTS); return UD_ERR_UNSUPPORTED; }
  if ((long long)H * W > DEPTH_MAXPIX) { set_error("ud_cloth_depth_fwd: H*W=%lld above %d pixels", (long long)H * W, DEPTH_MAXPIX); return UD_ERR_UNSUPPORTED; }
  int n = 2;
  while (n < P) n <<= 1;
  const int wide = (H * W) % 4 == 0 && ((size_t)img & 15) == 0;
  hipLaunchKernelGGL(depth_fwd_kernel, dim3(M), dim3(DEPTH_T), (size_t)n * sizeof(unsigned long long), (hipStream_t)stream, P, n, H, W,
                     pixel_size, z_offset, wide, x, img, owner);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

int ud_cloth_depth_bwd(int M, int P, int H, int W, const int* owner, const float* g_img, float* g_x, void* stream) {
  if (M <= 0 || P <= 0 || H <= 0 || W <= 0 || !owner || !g_img || !g_x) { set_error("ud_cloth_depth_bwd: bad argument"); return UD_ERR_INVALID; }
  if (P > DEPTH_MAXPTS) { set_error("ud_cloth_depth_bwd: P=%d above %d", P, DEPTH_MAXPTS); return UD_ERR_UNSUPPORTED; }
  if ((long long)H * W > DEPTH_MAXPIX) { set_error("ud_cloth_depth_bwd: H*W=%lld above %d pixels", (long long)H * W, DEPTH_MAXPIX); return UD_ERR_UNSUPPORTED; }
  hipLaunchKernelGGL(depth_bwd_kernel, dim3(M, (P * 3 + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, H * W, owner, g_img, g_x);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

}  // extern "C"
