// Point-cloud sampling and grouping (gfx950, f32): the PointNet++ ops of GenORM policy/tf_ops (sampling/tf_sampling_g.cu farthest point
// sampling + gather_point, grouping/tf_grouping_g.cu query_ball_point + group_point and its gradient) behind ud_pc_* (include/unidom_hip.h,
// "Point-cloud policy").  Handle-free, launches only: no allocation, no synchronisation, no atomics; the same input gives the same bits.
//
//   pc_fps         one cloud per workgroup.  A lane keeps PPL consecutive points and their running minimum distances in registers (point
//                  k sits in slot k % PPL of lane (k / PPL) % 64 of wave k / (64 PPL)).  Per sample: the distance update and the lane's own
//                  best slot, one DPP max over the wave, a ballot for the lowest tied lane, four readlanes for the winner's index and
//                  coordinates (no dependent memory access).  n <= 256 is one wave and no barrier at all; larger clouds run 16 waves that
//                  exchange (distance, index, coordinates) through LDS with one barrier per sample (the partials are double-buffered).
//                  Slots past n hold a copy of point 0: their minimum distance is 0 from the first sample on and a tie goes to the lower
//                  index, so they are never selected.
//   pc_ball        one wave per centre over the cloud staged in LDS (chunks of 1024 points), 64 candidates per step, ballot + prefix count
//                  for the ascending order, early exit at nsample.
//   pc_group_fwd   one thread per output element.
//   pc_group_bwd   gather, not scatter: one wave per point scans the index list in order (16 x 64 entries in flight), lists the matching
//                  entries in LDS, gathers their rows with parallel loads and adds them one after the other in ascending (j, k), lane =
//                  channel.  pc_group_bwd_centre (one thread per centre coordinate) runs first.
#include "common.h"

namespace {

constexpr int FPS_NW = 16;        // waves of the multi-wave FPS path
constexpr int BALL_CHUNK = 1024;  // points staged per pass of the ball query
constexpr int BALL_WAVES = 4;

template <int CTRL>
__device__ __forceinline__ unsigned dpp_u(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}

// max over the 64 lanes, every lane returns it (the butterflies of ud::wave_sum)
__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
  v = max(v, dpp_u<0xB1>(v));
  v = max(v, dpp_u<0x4E>(v));
  v = max(v, dpp_u<0x141>(v));
  v = max(v, dpp_u<0x140>(v));
  unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 0), r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
  unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 32), r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
  return max(max(r0, r1), max(r2, r3));
}

__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

struct FpsPartial {   // one wave's candidate for one sample
  unsigned bits;      // its largest minimum distance (>= +0: the bits order as the floats do)
  int k;
  float x, y, z;
  int pad[3];
};

template <int PPL, int NW>
__global__ __launch_bounds__(64 * NW) void pc_fps(int n, int m, const float* __restrict__ xyz, int* __restrict__ idx, float* __restrict__ new_xyz) {
  __shared__ FpsPartial part[2][NW];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* p = xyz + (size_t)b * n * 3;
  int* oi = idx + (size_t)b * m;
  float* ox = new_xyz + (size_t)b * m * 3;
  const int k0 = (wave * 64 + lane) * PPL;
  float px[PPL], py[PPL], pz[PPL], mind[PPL];
#pragma unroll
  for (int i = 0; i < PPL; ++i) {
    const int k = (k0 + i < n) ? k0 + i : 0;
    px[i] = p[3 * k];
    py[i] = p[3 * k + 1];
    pz[i] = p[3 * k + 2];
    mind[i] = 1e38f;
  }
  float cx = p[0], cy = p[1], cz = p[2];
  if (threadIdx.x == 0) {
    oi[0] = 0;
    ox[0] = cx;
    ox[1] = cy;
    ox[2] = cz;
  }
  for (int j = 1; j < m; ++j) {
    unsigned bb = 0;
    int bi = 0;
    float bx = px[0], by = py[0], bz = pz[0];
#pragma unroll
    for (int i = 0; i < PPL; ++i) {
      const float dx = px[i] - cx, dy = py[i] - cy, dz = pz[i] - cz;
      const float d = (dx * dx + dy * dy) + dz * dz;
      mind[i] = fminf(mind[i], d);
      const unsigned u = __builtin_bit_cast(unsigned, mind[i]);
      const bool take = (i == 0) || (u > bb);      // strictly larger: the lowest slot among equals
      bb = take ? u : bb;
      bi = take ? i : bi;
      bx = take ? px[i] : bx;
      by = take ? py[i] : by;
      bz = take ? pz[i] : bz;
    }
    unsigned wm = wave_max_u(bb);
    const int win = __builtin_ctzll(__ballot(bb == wm));      // the lowest tied lane holds the lowest tied index
    int wk = __builtin_amdgcn_readlane(k0 + bi, win);
    cx = readlane_f(bx, win);
    cy = readlane_f(by, win);
    cz = readlane_f(bz, win);
    if (NW > 1) {
      FpsPartial* buf = part[j & 1];
      if (lane == 0) {
        buf[wave].bits = wm;
        buf[wave].k = wk;
        buf[wave].x = cx;
        buf[wave].y = cy;
        buf[wave].z = cz;
      }
      __syncthreads();
      const unsigned wb = (lane < NW) ? buf[lane].bits : 0u;
      const unsigned gm = wave_max_u(wb);
      const int ww = __builtin_ctzll(__ballot(lane < NW && wb == gm));   // waves hold ascending index ranges
      wk = buf[ww].k;
      cx = buf[ww].x;
      cy = buf[ww].y;
      cz = buf[ww].z;
    }
    if (threadIdx.x == 0) {
      oi[j] = wk;
      ox[3 * j] = cx;
      ox[3 * j + 1] = cy;
      ox[3 * j + 2] = cz;
    }
  }
}

__global__ __launch_bounds__(64 * BALL_WAVES) void pc_ball(int n, int m, float radius, int nsample, const float* __restrict__ xyz,
                                                           const float* __restrict__ new_xyz, int* __restrict__ idx, int* __restrict__ cnt_out) {
  __shared__ float sx[BALL_CHUNK], sy[BALL_CHUNK], sz[BALL_CHUNK];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * BALL_WAVES + wave;
  const bool live = j < m;
  const float* p = xyz + (size_t)b * n * 3;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  int* row = nullptr;
  if (live) {
    const float* q = new_xyz + ((size_t)b * m + j) * 3;
    qx = q[0];
    qy = q[1];
    qz = q[2];
    row = idx + ((size_t)b * m + j) * nsample;
  }
  int cnt = 0, first = 0;
  for (int base = 0; base < n; base += BALL_CHUNK) {
    const int len = min(BALL_CHUNK, n - base);
    if (base) __syncthreads();
    for (int t = threadIdx.x; t < len; t += 64 * BALL_WAVES) {
      sx[t] = p[3 * (base + t)];
      sy[t] = p[3 * (base + t) + 1];
      sz[t] = p[3 * (base + t) + 2];
    }
    __syncthreads();
    if (!live || cnt >= nsample) continue;      // wave-uniform; the wave still meets the barriers
    for (int s = 0; s < len; s += 64) {
      const int t = s + lane;
      bool pass = false;
      if (t < len) {
        const float dx = sx[t] - qx, dy = sy[t] - qy, dz = sz[t] - qz;
        pass = fmaxf(sqrtf((dx * dx + dy * dy) + dz * dz), 1e-20f) < radius;
      }
      const unsigned long long mask = __ballot(pass);
      if (mask == 0) continue;
      if (cnt == 0) first = base + s + __builtin_ctzll(mask);
      const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
      if (pass && pos < nsample) row[pos] = base + t;
      cnt += __builtin_popcountll(mask);
      if (cnt >= nsample) break;
    }
  }
  if (!live) return;
  cnt = min(cnt, nsample);
  for (int s = cnt + lane; s < nsample; s += 64) row[s] = first;      // the first hit; zeros for an empty ball
  if (lane == 0) cnt_out[(size_t)b * m + j] = cnt;
}

// per_b = m * nsample * W elements of one cloud (< 2^31, checked by the caller)
__global__ __launch_bounds__(256) void pc_group_fwd(int n, int m, int nsample, int C, const float* __restrict__ xyz, const float* __restrict__ feats,
                                                    const float* __restrict__ new_xyz, const int* __restrict__ idx, float* __restrict__ out) {
  const int W = 3 + C, per_b = m * nsample * W;
  const int e = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (e >= per_b) return;
  const int r = e / W, c = e - r * W, j = r / nsample;
  const int id = idx[(size_t)b * m * nsample + r];
  float val = 0.0f;                                  // an index outside [0, n): zeros, nothing read
  if (id >= 0 && id < n) {
    if (c < 3) val = xyz[((size_t)b * n + id) * 3 + c] - new_xyz[((size_t)b * m + j) * 3 + c];
    else val = feats[((size_t)b * n + id) * C + (c - 3)];
  }
  out[(size_t)b * per_b + e] = val;
}

__global__ __launch_bounds__(256) void pc_group_bwd_centre(int m, int nsample, int W, long total, const float* __restrict__ g_out,
                                                           float* __restrict__ g_new_xyz) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;      // (b m + j) 3 + c
  if (t >= total) return;
  const long r = t / 3;
  const int c = (int)(t - r * 3);
  const float* g = g_out + (size_t)r * nsample * W + c;
  float s = 0.0f;
  for (int k = 0; k < nsample; ++k) s += g[(size_t)k * W];
  g_new_xyz[t] = -s;
}

constexpr int BWD_HITS = 128;   // a wave's list of matching entries (flushed once it holds more than 64: a step adds at most 64)
constexpr int BWD_VALS = 1024;  // floats of gathered rows per wave

// acc += src[hits[r] * stride + c0 + lane] for r = 0 .. count-1 in that order.  The rows are gathered into LDS with every lane loading
// (independent loads, as many rows as fit), then summed one after the other by the lane of each channel: the order of the additions is
// the order of the list, only the loads are parallel.  One wave; LDS accesses of a wave are served in program order.
__device__ __forceinline__ void bwd_flush(const int* hits, int count, const float* __restrict__ src, int stride, int c0, int Wt, float* vals,
                                          int lane, float& acc) {
  const int G = BWD_VALS / Wt;
  for (int r0 = 0; r0 < count; r0 += G) {
    const int rows = min(G, count - r0), total = rows * Wt;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < total; t += 64) {
      const int r = t / Wt, c = t - r * Wt;
      vals[t] = src[(size_t)hits[r0 + r] * stride + c0 + c];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < Wt)
      for (int r = 0; r < rows; ++r) acc += vals[r * Wt + lane];
  }
}

// the entries e of list[0 .. E) equal to target, in ascending e: their rows of src (row width stride, channels c0 .. c0 + Wt) added to acc
__device__ __forceinline__ void bwd_accumulate(const int* __restrict__ list, int E, int target, const float* __restrict__ src, int stride, int c0,
                                               int Wt, int* hits, float* vals, int lane, float& acc) {
  int count = 0;
  for (int s = 0; s < E; s += 1024) {                       // sixteen loads in flight, consumed in order
    int v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = s + 64 * q + lane;
      v[q] = (e < E) ? list[e] : -1;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const bool hit = v[q] == target;
      const unsigned long long mask = __ballot(hit);
      if (mask == 0) continue;
      if (count > BWD_HITS - 64) {
        bwd_flush(hits, count, src, stride, c0, Wt, vals, lane, acc);
        count = 0;
      }
      if (hit) hits[count + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u))] = s + 64 * q + lane;
      count += __builtin_popcountll(mask);
    }
  }
  bwd_flush(hits, count, src, stride, c0, Wt, vals, lane, acc);
}

// one wave per point i of cloud b; lane = channel within a tile of 64 channels
__global__ __launch_bounds__(256) void pc_group_bwd(int n, int m, int nsample, int C, const int* __restrict__ idx, const int* __restrict__ centre_idx,
                                                    const float* __restrict__ g_out, const float* __restrict__ g_new_xyz,
                                                    float* __restrict__ g_xyz, float* __restrict__ g_feats) {
  __shared__ int s_hits[4][BWD_HITS];
  __shared__ float s_vals[4][BWD_VALS];
  const int W = 3 + C, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n) return;                                       // wave-uniform, no workgroup barrier below
  const int E = m * nsample;
  const int* ib = idx + (size_t)b * E;
  const float* gb = g_out + (size_t)b * E * W;
  for (int c0 = 0; c0 < W; c0 += 64) {
    const int c = c0 + lane;
    float acc = 0.0f;
    bwd_accumulate(ib, E, i, gb, W, c0, min(64, W - c0), s_hits[wave], s_vals[wave], lane, acc);      // ascending (j, k)
    if (c0 == 0 && centre_idx)                              // then the centres this point was sampled as, ascending j
      bwd_accumulate(centre_idx + (size_t)b * m, m, i, g_new_xyz + (size_t)b * m * 3, 3, 0, 3, s_hits[wave], s_vals[wave], lane, acc);
    if (c < 3) g_xyz[((size_t)b * n + i) * 3 + c] = acc;
    else if (c < W) g_feats[((size_t)b * n + i) * C + (c - 3)] = acc;
  }
}

template <int PPL, int NW>
void launch_fps(int B, int n, int m, const float* xyz, int* idx, float* new_xyz, hipStream_t st) {
  hipLaunchKernelGGL((pc_fps<PPL, NW>), dim3(B), dim3(64 * NW), 0, st, n, m, xyz, idx, new_xyz);
}

}  // namespace

extern "C" {

int ud_pc_fps(int B, int n, int m, const float* xyz, int* idx, float* new_xyz, void* stream) {
  if (B < 1 || n < 1 || m < 1 || !xyz || !idx || !new_xyz) {
    ud::set_error("ud_pc_fps: bad argument (B=%d, n=%d, m=%d; no pointer may be null)", B, n, m);
    return UD_ERR_INVALID;
  }
  if (n > 8192 || B > 65535) {
    ud::set_error("ud_pc_fps: n=%d above 8192 or B=%d above 65535", n, B);
    return UD_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n <= 64) launch_fps<1, 1>(B, n, m, xyz, idx, new_xyz, st);
  else if (n <= 128) launch_fps<2, 1>(B, n, m, xyz, idx, new_xyz, st);
  else if (n <= 256) launch_fps<4, 1>(B, n, m, xyz, idx, new_xyz, st);
  else if (n <= 1024) launch_fps<1, FPS_NW>(B, n, m, xyz, idx, new_xyz, st);
  else if (n <= 2048) launch_fps<2, FPS_NW>(B, n, m, xyz, idx, new_xyz, st);
  else if (n <= 4096) launch_fps<4, FPS_NW>(B, n, m, xyz, idx, new_xyz, st);
  else launch_fps<8, FPS_NW>(B, n, m, xyz, idx, new_xyz, st);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

int ud_pc_ball_query(int B, int n, int m, float radius, int nsample, const float* xyz, const float* new_xyz, int* idx, int* cnt, void* stream) {
  if (B < 1 || n < 1 || m < 1 || nsample < 1 || !xyz || !new_xyz || !idx || !cnt) {
    ud::set_error("ud_pc_ball_query: bad argument (B=%d, n=%d, m=%d, nsample=%d; no pointer may be null)", B, n, m, nsample);
    return UD_ERR_INVALID;
  }
  if (B > 65535) {
    ud::set_error("ud_pc_ball_query: B=%d above 65535", B);
    return UD_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(pc_ball, dim3((m + BALL_WAVES - 1) / BALL_WAVES, B), dim3(64 * BALL_WAVES), 0, (hipStream_t)stream, n, m, radius, nsample, xyz,
                     new_xyz, idx, cnt);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

int ud_pc_group_fwd(int B, int n, int m, int nsample, int C, const float* xyz, const float* feats, const float* new_xyz, const int* idx,
                    float* out, void* stream) {
  if (B < 1 || n < 1 || m < 1 || nsample < 1 || C < 0 || !xyz || (C > 0 && !feats) || !new_xyz || !idx || !out) {
    ud::set_error("ud_pc_group_fwd: bad argument (B=%d, n=%d, m=%d, nsample=%d, C=%d; only feats may be null, with C = 0)", B, n, m, nsample, C);
    return UD_ERR_INVALID;
  }
  const long per_b = (long)m * nsample * (3L + C);
  if (B > 65535 || per_b > 0x7fffff00L) {
    ud::set_error("ud_pc_group_fwd: B=%d above 65535 or m nsample (3 + C) = %ld above 2^31 - 256", B, per_b);
    return UD_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(pc_group_fwd, dim3((unsigned)((per_b + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, n, m, nsample, C, xyz, feats, new_xyz,
                     idx, out);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

int ud_pc_group_bwd(int B, int n, int m, int nsample, int C, const int* idx, const int* centre_idx, const float* g_out, float* g_xyz,
                    float* g_feats, float* g_new_xyz, void* stream) {
  if (B < 1 || n < 1 || m < 1 || nsample < 1 || C < 0 || !idx || !g_out || !g_xyz || (C > 0 && !g_feats) || !g_new_xyz) {
    ud::set_error("ud_pc_group_bwd: bad argument (B=%d, n=%d, m=%d, nsample=%d, C=%d; only centre_idx, and g_feats with C = 0, may be null)", B, n, m,
                  nsample, C);
    return UD_ERR_INVALID;
  }
  const long per_b = (long)m * nsample * (3L + C);
  if (B > 65535 || per_b > 0x7fffff00L) {
    ud::set_error("ud_pc_group_bwd: B=%d above 65535 or m nsample (3 + C) = %ld above 2^31 - 256", B, per_b);
    return UD_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)B * m * 3;
  hipLaunchKernelGGL(pc_group_bwd_centre, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, m, nsample, 3 + C, total, g_out, g_new_xyz);
  hipLaunchKernelGGL(pc_group_bwd, dim3((n + 3) / 4, B), dim3(256), 0, st, n, m, nsample, C, idx, centre_idx, g_out, (const float*)g_new_xyz, g_xyz,
                     g_feats);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

}  // extern "C"
