// The PlasticineLab renderer (GenORM/policy/pbm/plb/engine/renderer/renderer.py) for B envs at once: particle SDF bake, first-hit
// G-buffer and the path-traced image.  f32 throughout, as the reference's fields are; built with -ffp-contract=off and correctly rounded
// divide / sqrt, every operation written in the order include/unidom_hip.h states, so that tests/plb_render_twin.py (NumPy f32) is bit-equal
// to the bake and to the G-buffer of the body, the ground and the background plane.  Primitive distances and normals are the f64 shape layer
// of plb_prim.h, cast to f32.  Only cosf / sinf of the bounce directions are not pinned (an ulp).
//
// The random draws are THIS PROJECT'S OWN: ti.random cannot be pinned (its state is Taichi's, per thread, not specified), so a draw is a hash of
// (seed, pixel, sample, k) -- render_rand below; the header gives the formula.
//
// Mapping.  Bake: one thread per (env, particle, offset) for the 64-bit atomic minima, one thread per cell for the two smoothing passes.
// G-buffer / image: one thread per (env, pixel), a wave holds an 8 x 8 tile of pixels (their rays walk neighbouring cells of the volume), a
// workgroup four tiles (16 x 16).  The image thread runs its spp samples one after the other and sums them in a register in the reference's
// order, so nothing is atomic and the result is bit-identical from run to run.  Every loop is bounded (200 / 500 / 20 steps, max_ray_depth,
// spp); no workgroup waits for another.
//
// The image kernel is compiled once per (directional light, roulette) -- the reference's two ti.static switches -- and the handle says which
// instance a call runs (ud_plb_render_set_light); <false, false> is the kernel as it was before the switches existed.  The lit instances send
// one shadow ray per bounce from the lanes that face the light, answered by render_occluded, an any-hit walk over next_hit's candidates.
#include "common.h"
#include "plb_prim.h"

namespace ud {

constexpr int RP = UD_PLB_RENDER_MAX_PRIM;
constexpr float R_INF = 1e10f, R_DIST_LIMIT = 100.0f, R_FOV = 0.23f, R_EXPOSURE = 1.5f;
constexpr int PRIM_STRIDE = 12;   // per primitive and env: position 3, rotation 4, conj(rotation) / |rotation| 4, gap 1

struct RenderK {                  // constants of a handle, passed to every kernel by value
  int res[3], bake, img[2], depth, np, N;
  long long cells;
  float dx, inv_dx, thr, cam[3], mat[9], fov_aspect;
  int kind[RP];
  double radius[RP], h[RP], shape[RP][3];
  float color[RP][3];
};

}  // namespace ud

struct ud_plb_render {
  ud::RenderK k;
  int max_envs, spp;
  long long* vol;     // [max_envs][cells] packed (quantised distance << 24) + colour
  float *sdf, *tmp;   // [max_envs][cells] each
  float* bbox;        // [max_envs][2][3]
  int* status;        // [max_envs]
  double* prim;       // [max_envs][RP][PRIM_STRIDE]
  int light, roulette;   // ud_plb_render_set_light: which instance of k_render_image runs
  float light_dir[3];    // light_direction, rounded to f32 at the call
};

namespace ud {

// ---------------------------------------------------------------- bake
__global__ void __launch_bounds__(256) k_render_bbox(RenderK k, const double* __restrict__ x, float* __restrict__ bbox, int* __restrict__ status,
                                                     float* __restrict__ bbox_out, int* __restrict__ status_out) {
  __shared__ float s[6][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  float lo[3] = {R_INF, R_INF, R_INF}, hi[3] = {-R_INF, -R_INF, -R_INF};
  for (int i = tid; i < k.N; i += 256)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float px = (float)x[((long long)b * k.N + i) * 3 + c];
      const float v = (floorf(px * k.inv_dx) - 6.0f) * k.dx;
      lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v);
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) { s[c][tid] = lo[c]; s[3 + c][tid] = hi[c]; }
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w)
#pragma unroll
      for (int c = 0; c < 3; ++c) { s[c][tid] = fminf(s[c][tid], s[c][tid + w]); s[3 + c][tid] = fmaxf(s[3 + c][tid], s[3 + c][tid + w]); }
    __syncthreads();
  }
  if (tid == 0) {
    int st = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float b0 = s[c][0], h1 = s[3 + c][0];
      if (!((h1 - b0) / k.dx < (float)k.res[c])) st = 1;     // the reference's assert a < b
      const float b1 = (float)((double)b0 + (double)k.res[c] * (double)k.dx);
      bbox[b * 6 + c] = b0; bbox[b * 6 + 3 + c] = b1;
      bbox_out[b * 6 + c] = b0; bbox_out[b * 6 + 3 + c] = b1;
    }
    status[b] = st; status_out[b] = st;
  }
}

__global__ void __launch_bounds__(256) k_render_fill(long long total, long long* __restrict__ vol) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) vol[i] = 0xFFFFFFFFLL;   // (2^31 - 1 + 1) * 2 - 1
}

__global__ void __launch_bounds__(256) k_render_splat(RenderK k, long long total, const double* __restrict__ x, const int* __restrict__ color,
                                                      const float* __restrict__ bbox, const int* __restrict__ status, long long* __restrict__ vol) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int S = 2 * k.bake + 2;
  const int ok = (int)(t % S), oj = (int)((t / S) % S), oi = (int)((t / ((long long)S * S)) % S);
  const long long pe = t / ((long long)S * S * S);
  const int id = (int)(pe % k.N), b = (int)(pe / k.N);
  if (status[b]) return;
  const int off[3] = {oi - k.bake - 1, oj - k.bake - 1, ok - k.bake - 1};
  float p[3];
  int idx[3];
  bool in = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float px = (float)x[((long long)b * k.N + id) * 3 + c];
    p[c] = (px - bbox[b * 6 + c]) * k.inv_dx;
    idx[c] = (int)p[c] + off[c];
    in = in && idx[c] >= 0 && idx[c] < k.res[c];
  }
  if (!in) return;
  const float d0 = (float)idx[0] - p[0], d1 = (float)idx[1] - p[1], d2 = (float)idx[2] - p[2];
  const float dist = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
  const float q = fminf(fmaxf(0.0f, 51.0f * dist), 255.0f);
  const unsigned long long v = (unsigned long long)(((long long)q << 24) + (long long)color[id]);
  const long long cell = ((long long)idx[0] * k.res[1] + idx[1]) * k.res[2] + idx[2];
  atomicMin(reinterpret_cast<unsigned long long*>(vol) + (long long)b * k.cells + cell, v);
}

__device__ __forceinline__ float render_unpack_sdf(long long c) { return (float)((c >> 24) & 255) / 255.0f; }

// one smoothing pass; FIRST reads the packed volume (the unpack of the reference, fused), the second the first's output
template <bool FIRST>
__global__ void __launch_bounds__(256) k_render_smooth(RenderK k, long long total, const long long* __restrict__ vol, const float* __restrict__ in,
                                                       float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long long cell = t % k.cells, base = t - cell;
  const int z = (int)(cell % k.res[2]), y = (int)((cell / k.res[2]) % k.res[1]), x = (int)(cell / ((long long)k.res[1] * k.res[2]));
  float r = 1.0f;
  if (x >= 1 && y >= 1 && z >= 1 && x < k.res[0] - 1 && y < k.res[1] - 1 && z < k.res[2] - 1) {
    float sum = 0.0f;
    for (int i = -1; i < 2; ++i)
      for (int j = -1; j < 2; ++j)
#pragma unroll
        for (int l = -1; l < 2; ++l) {
          const long long n = base + ((long long)(x + i) * k.res[1] + (y + j)) * k.res[2] + (z + l);
          if constexpr (FIRST) sum += render_unpack_sdf(vol[n]); else sum += in[n];
        }
    r = sum / 27.0f;
  }
  out[t] = r;
}

// ---------------------------------------------------------------- primitives of an env: position, rotation, its inverse, gap
__global__ void k_render_prims(RenderK k, int B, const double* __restrict__ pos, const double* __restrict__ rot, const double* __restrict__ gap,
                               double* __restrict__ prim) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B * k.np) return;
  const int b = t / k.np, i = t % k.np;
  double* o = prim + ((long long)b * RP + i) * PRIM_STRIDE;
  double q[4] = {1.0, 0.0, 0.0, 0.0};
  if (rot) for (int c = 0; c < 4; ++c) q[c] = rot[(long long)t * 4 + c];
  for (int c = 0; c < 3; ++c) o[c] = pos[(long long)t * 3 + c];
  for (int c = 0; c < 4; ++c) o[3 + c] = q[c];
  plb_qinv(q, o + 7);
  o[11] = gap ? gap[t] : 0.0;
}

// ---------------------------------------------------------------- sampling
struct RenderEnv {
  const long long* vol;
  const float* sdf;
  const double* prim;
  float b0[3], b1[3];
};

__device__ __forceinline__ float render_norm(const float* v) { return sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
__device__ __forceinline__ void render_normalize(float* v) {      // Vector.normalized(): invlen = 1 / norm, invlen * v
  const float il = 1.0f / render_norm(v);
  v[0] = il * v[0]; v[1] = il * v[1]; v[2] = il * v[2];
}

// the texture coordinate of sample_sdf / sample_color: false outside [0, 1]^3 (and for NaN)
__device__ __forceinline__ bool render_tex_pos(const RenderEnv& e, const float* pos, float* q) {
  bool in = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    q[c] = (pos[c] - e.b0[c]) / (e.b1[c] - e.b0[c]);
    in = in && q[c] >= 0.0f && q[c] <= 1.0f;
  }
  return in;
}
// sample_tex's clamped corners and weights
struct RenderTex { long long i[8]; float f[3]; };
__device__ __forceinline__ void render_tex_setup(const RenderK& k, const float* q, RenderTex& t) {
  int b[3], b1[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p = q[c] * (float)k.res[c];
    b[c] = max(min((int)p, k.res[c] - 1), 0);
    t.f[c] = p - (float)b[c];
    b1[c] = min(b[c] + 1, k.res[c] - 1);
  }
  const long long sy = k.res[2], sx = (long long)k.res[1] * k.res[2];
  t.i[0] = b[0] * sx + b[1] * sy + b[2];   t.i[1] = b1[0] * sx + b[1] * sy + b[2];    // (x, y, z), (x1, y, z)
  t.i[2] = b[0] * sx + b[1] * sy + b1[2];  t.i[3] = b1[0] * sx + b[1] * sy + b1[2];   // (x, y, z1), (x1, y, z1)
  t.i[4] = b[0] * sx + b1[1] * sy + b[2];  t.i[5] = b1[0] * sx + b1[1] * sy + b[2];   // (x, y1, z), (x1, y1, z)
  t.i[6] = b[0] * sx + b1[1] * sy + b1[2]; t.i[7] = b1[0] * sx + b1[1] * sy + b1[2];  // (x, y1, z1), (x1, y1, z1)
}
__device__ __forceinline__ float render_tex_mix(const float* v, const float* f) {
  const float c00 = v[0] * (1.0f - f[0]) + v[1] * f[0];
  const float c01 = v[2] * (1.0f - f[0]) + v[3] * f[0];
  const float c10 = v[4] * (1.0f - f[0]) + v[5] * f[0];
  const float c11 = v[6] * (1.0f - f[0]) + v[7] * f[0];
  const float c0 = c00 * (1.0f - f[1]) + c10 * f[1];
  const float c1 = c01 * (1.0f - f[1]) + c11 * f[1];
  return c0 * (1.0f - f[2]) + c1 * f[2];
}
__device__ __forceinline__ float render_sample_sdf(const RenderK& k, const RenderEnv& e, const float* pos) {
  float q[3];
  if (!render_tex_pos(e, pos, q)) return 0.0f;
  RenderTex t;
  render_tex_setup(k, q, t);
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = e.sdf[t.i[c]];
  return render_tex_mix(v, t.f) - k.thr;
}
__device__ __forceinline__ void render_sample_color(const RenderK& k, const RenderEnv& e, const float* pos, float* out) {
  float q[3];
  out[0] = out[1] = out[2] = 0.0f;
  if (!render_tex_pos(e, pos, q)) return;
  RenderTex t;
  render_tex_setup(k, q, t);
  long long pk[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) pk[c] = e.vol[t.i[c]];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {          // channel 0 = bits 16-23, 1 = bits 8-15, 2 = the low byte
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = (float)((pk[c] >> (8 * (2 - ch))) & 255) / 255.0f;
    out[ch] = render_tex_mix(v, t.f);
  }
}
__device__ __forceinline__ void render_sample_normal(const RenderK& k, const RenderEnv& e, const float* p, float* n) {
  const float d = 1e-3f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float inc[3] = {p[0], p[1], p[2]}, dec[3] = {p[0], p[1], p[2]};
    inc[i] += d; dec[i] -= d;
    n[i] = 500.0f * (render_sample_sdf(k, e, inc) - render_sample_sdf(k, e, dec));
  }
  render_normalize(n);
}

__device__ __forceinline__ float render_prim_sdf(const RenderK& k, const RenderEnv& e, int i, const float* pp) {
  const double* P = e.prim + i * PRIM_STRIDE;
  const double d[3] = {(double)pp[0] - P[0], (double)pp[1] - P[1], (double)pp[2] - P[2]};
  double pl[3];
  plb_qrot(P + 7, d, pl);
  return (float)plb_shape_sdf<2>(k.kind[i], k.kind[i] == 6 ? P + 11 : k.shape[i], k.h[i], k.radius[i], pl);
}
__device__ __forceinline__ void render_prim_normal(const RenderK& k, const RenderEnv& e, int i, const float* pp, float* n) {
  const double* P = e.prim + i * PRIM_STRIDE;
  const double d[3] = {(double)pp[0] - P[0], (double)pp[1] - P[1], (double)pp[2] - P[2]};
  double pl[3], nl[3], nw[3];
  plb_qrot(P + 7, d, pl);
  plb_shape_normal<2>(k.kind[i], k.kind[i] == 6 ? P + 11 : k.shape[i], k.h[i], pl, nl);
  plb_qrot(P + 3, nl, nw);
  n[0] = (float)nw[0]; n[1] = (float)nw[1]; n[2] = (float)nw[2];
}

struct RenderHit { float t, n[3], c[3], rough; int kind; };

// next_hit (renderer.py:202-325)
__device__ void render_next_hit(const RenderK& k, const RenderEnv& e, const float* o, const float* d, RenderHit& h) {
  h.t = R_INF; h.rough = 0.05f; h.kind = 0;
  h.n[0] = h.n[1] = h.n[2] = 0.0f; h.c[0] = h.c[1] = h.c[2] = 0.0f;
  if (d[2] != 0.0f) {                                   // background plane z = -5.5
    const float rc = -(o[2] + 5.5f) / d[2];
    if (rc > 0.0f && rc < h.t) {
      h.t = rc; h.n[0] = 0.0f; h.n[1] = 0.0f; h.n[2] = 1.0f; h.c[0] = 0.6f; h.c[1] = 0.7f; h.c[2] = 0.7f; h.rough = 0.0f; h.kind = 1;
    }
  }
  if (d[1] < 0.0f) {                                    // ground
    const float gd = (o[1] + 0.002f) / (-d[1]);
    if (gd < R_DIST_LIMIT && gd < h.t) {
      h.t = gd; h.n[0] = 0.0f; h.n[1] = 1.0f; h.n[2] = 0.0f; h.rough = 0.0f; h.kind = 2;
      const float p0 = o[0] + d[0] * gd, p2 = o[2] + d[2] * gd;
      float f = 0.4f;
      if (p0 <= 1.0f && p0 >= 0.0f && p2 <= 1.0f && p2 >= 0.0f) f = (float)(((int)(p0 / 0.25f) + (int)(p2 / 0.25f)) % 2) * 0.2f + 0.35f;
      h.c[0] = 0.3f * f; h.c[1] = 0.5f * f; h.c[2] = 0.7f * f;
    }
  }
  if (k.np > 0) {                                       // primitives: 200 steps of sphere tracing
    int j = 0, id = 0;
    float dist = 0.0f, sv = R_INF;
    while (j < 200 && dist < R_DIST_LIMIT && sv > 1e-8f) {
      const float pp[3] = {o[0] + dist * d[0], o[1] + dist * d[1], o[2] + dist * d[2]};
      sv = R_INF;
      for (int i = 0; i < k.np; ++i) {
        const float dd = render_prim_sdf(k, e, i, pp);
        if (dd < sv) { sv = dd; id = i; }
      }
      dist += sv;
      ++j;
    }
    if (dist < h.t && dist < R_DIST_LIMIT) {
      h.t = dist; h.kind = 3 + id; h.rough = 0.0f;
      const float pp[3] = {o[0] + dist * d[0], o[1] + dist * d[1], o[2] + dist * d[2]};
      render_prim_normal(k, e, id, pp, h.n);
      h.c[0] = k.color[id][0]; h.c[1] = k.color[id][1]; h.c[2] = k.color[id][2];
    }
  }
  {                                                     // the body: ray_aabb_intersection, 500-step march, 20 halvings back
    bool hit = true;
    float tn = -R_INF, tf = R_INF;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (d[i] == 0.0f) {
        if (o[i] < e.b0[i] || o[i] > e.b1[i]) hit = false;
      } else {
        const float i1 = (e.b0[i] - o[i]) / d[i], i2 = (e.b1[i] - o[i]) / d[i];
        tf = fminf(fmaxf(i1, i2), tf);
        tn = fmaxf(fminf(i1, i2), tn);
      }
    }
    if (tn > tf) hit = false;
    if (hit) {
      tn = fmaxf(tn, 0.0f);
      const float t0 = tn + 1e-4f;
      float pos[3] = {o[0] + d[0] * t0, o[1] + d[1] * t0, o[2] + d[2] * t0};
      float step[3] = {0.0f, 0.0f, 0.0f};
      for (int j = 0; j < 500; ++j) {
        const float s = render_sample_sdf(k, e, pos);
        if (s < 0.0f) {
          float bs[3] = {step[0], step[1], step[2]};
          for (int l = 0; l < 20; ++l) {
            bs[0] = bs[0] * 0.5f; bs[1] = bs[1] * 0.5f; bs[2] = bs[2] * 0.5f;
            const float q[3] = {pos[0] - bs[0], pos[1] - bs[1], pos[2] - bs[2]};
            if (render_sample_sdf(k, e, q) < 0.0f) { pos[0] = q[0]; pos[1] = q[1]; pos[2] = q[2]; }
          }
          const float od[3] = {o[0] - pos[0], o[1] - pos[1], o[2] - pos[2]};
          const float dist = render_norm(od);
          if (dist < h.t) {
            h.t = dist; h.kind = 16;
            render_sample_normal(k, e, pos, h.n);
            render_sample_color(k, e, pos, h.c);
          }
          break;
        }
        const float m = fmaxf(s * 0.05f, 0.01f);
        step[0] = d[0] * m; step[1] = d[1] * m; step[2] = d[2] * m;
        pos[0] += step[0]; pos[1] += step[1]; pos[2] += step[2];
      }
    }
  }
}

// The shadow ray of the directional light (renderer.py:383-384): true when next_hit(o, d) would return a distance <= 100.  next_hit takes a
// candidate only when it lies below the closest so far, so its result is the smallest candidate and "closest > dist_limit" is "no candidate
// <= 100": the candidates are tested in next_hit's order with next_hit's own conditions, the first one within reach ends the search, and no
// normal or colour is fetched.
__device__ bool render_occluded(const RenderK& k, const RenderEnv& e, const float* o, const float* d) {
  if (d[2] != 0.0f) {                                   // background plane: part of the scene for a shadow ray too
    const float rc = -(o[2] + 5.5f) / d[2];
    if (rc > 0.0f && rc <= R_DIST_LIMIT) return true;
  }
  if (d[1] < 0.0f) {                                    // ground
    const float gd = (o[1] + 0.002f) / (-d[1]);
    if (gd < R_DIST_LIMIT) return true;
  }
  if (k.np > 0) {                                       // primitives
    int j = 0;
    float dist = 0.0f, sv = R_INF;
    while (j < 200 && dist < R_DIST_LIMIT && sv > 1e-8f) {
      const float pp[3] = {o[0] + dist * d[0], o[1] + dist * d[1], o[2] + dist * d[2]};
      sv = R_INF;
      for (int i = 0; i < k.np; ++i) sv = fminf(sv, render_prim_sdf(k, e, i, pp));
      dist += sv;
      ++j;
    }
    if (dist < R_DIST_LIMIT) return true;
  }
  bool hit = true;                                      // the body
  float tn = -R_INF, tf = R_INF;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (d[i] == 0.0f) {
      if (o[i] < e.b0[i] || o[i] > e.b1[i]) hit = false;
    } else {
      const float i1 = (e.b0[i] - o[i]) / d[i], i2 = (e.b1[i] - o[i]) / d[i];
      tf = fminf(fmaxf(i1, i2), tf);
      tn = fmaxf(fminf(i1, i2), tn);
    }
  }
  if (tn > tf || !hit) return false;
  tn = fmaxf(tn, 0.0f);
  const float t0 = tn + 1e-4f;
  float pos[3] = {o[0] + d[0] * t0, o[1] + d[1] * t0, o[2] + d[2] * t0};
  float step[3] = {0.0f, 0.0f, 0.0f};
  for (int j = 0; j < 500; ++j) {
    const float s = render_sample_sdf(k, e, pos);
    if (s < 0.0f) {
      for (int l = 0; l < 20; ++l) {
        step[0] = step[0] * 0.5f; step[1] = step[1] * 0.5f; step[2] = step[2] * 0.5f;
        const float q[3] = {pos[0] - step[0], pos[1] - step[1], pos[2] - step[2]};
        if (render_sample_sdf(k, e, q) < 0.0f) { pos[0] = q[0]; pos[1] = q[1]; pos[2] = q[2]; }
      }
      const float od[3] = {o[0] - pos[0], o[1] - pos[1], o[2] - pos[2]};
      return render_norm(od) <= R_DIST_LIMIT;
    }
    const float m = fmaxf(s * 0.05f, 0.01f);
    step[0] = d[0] * m; step[1] = d[1] * m; step[2] = d[2] * m;
    pos[0] += step[0]; pos[1] += step[1]; pos[2] += step[2];
  }
  return false;
}

// ---------------------------------------------------------------- random draws, camera
__device__ __forceinline__ unsigned render_lowbias32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ float render_rand(unsigned seed, unsigned pixel, unsigned sample, unsigned kk) {
  const unsigned h = render_lowbias32(seed ^ (pixel * 0x9E3779B9u + sample * 0x85EBCA6Bu + kk * 0xC2B2AE35u));
  return (float)(h >> 8) * 5.9604644775390625e-08f;     // 2^-24
}
__device__ __forceinline__ void render_camera_ray(const RenderK& k, int u, int v, float ju, float jv, float* d) {
  float c[3];
  c[0] = ((0.46f * ((float)u + ju)) / (float)k.img[1] - k.fov_aspect) - 1e-5f;
  c[1] = ((0.46f * ((float)v + jv)) / (float)k.img[1] - R_FOV) - 1e-5f;
  c[2] = -1.0f;
  render_normalize(c);
#pragma unroll
  for (int r = 0; r < 3; ++r) d[r] = (k.mat[3 * r] * c[0] + k.mat[3 * r + 1] * c[1]) + k.mat[3 * r + 2] * c[2];
}
__device__ __forceinline__ void render_cross(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// pixel (u, v) of this thread: a wave is an 8 x 8 tile, a workgroup 2 x 2 tiles
__device__ __forceinline__ bool render_pixel(const RenderK& k, int& u, int& v) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  u = blockIdx.x * 16 + (w & 1) * 8 + (l & 7);
  v = blockIdx.y * 16 + (w >> 1) * 8 + (l >> 3);
  return u < k.img[0] && v < k.img[1];
}
__device__ __forceinline__ void render_env(const ud_plb_render& H, int b, RenderEnv& e) {
  e.vol = H.vol + (long long)b * H.k.cells;
  e.sdf = H.sdf + (long long)b * H.k.cells;
  e.prim = H.prim + (long long)b * RP * PRIM_STRIDE;
#pragma unroll
  for (int c = 0; c < 3; ++c) { e.b0[c] = H.bbox[b * 6 + c]; e.b1[c] = H.bbox[b * 6 + 3 + c]; }
}

__global__ void __launch_bounds__(256) k_render_gbuffer(ud_plb_render H, int* __restrict__ kind, float* __restrict__ t, float* __restrict__ normal,
                                                        float* __restrict__ albedo) {
  const RenderK& k = H.k;
  int u, v;
  if (!render_pixel(k, u, v)) return;
  const int b = blockIdx.z;
  const long long px = ((long long)b * k.img[0] + u) * k.img[1] + v;
  RenderHit h;
  h.kind = 0; h.t = 0.0f; h.n[0] = h.n[1] = h.n[2] = 0.0f; h.c[0] = h.c[1] = h.c[2] = 0.0f;
  if (!H.status[b]) {
    RenderEnv e;
    render_env(H, b, e);
    float d[3];
    render_camera_ray(k, u, v, 0.5f, 0.5f, d);
    render_next_hit(k, e, k.cam, d, h);
  }
  kind[px] = h.kind; t[px] = h.t;
#pragma unroll
  for (int c = 0; c < 3; ++c) { normal[px * 3 + c] = h.n[c]; albedo[px * 3 + c] = h.c[c]; }
}

// LIGHT / ROULETTE: use_directional_light / use_roulette of the reference's trace, ti.static there and template parameters here;
// <false, false> is the image of a handle whose light was never set.  Draws of bounce b: k = 2^30 + 4b + 0..2 the light noise, + 3 the roulette.
template <bool LIGHT, bool ROULETTE>
__global__ void __launch_bounds__(256) k_render_image(ud_plb_render H, int spp, unsigned seed, float* __restrict__ img) {
  const RenderK& k = H.k;
  int u, v;
  if (!render_pixel(k, u, v)) return;
  const int b = blockIdx.z;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  const bool live = !H.status[b];
  if (live) {
    RenderEnv e;
    render_env(H, b, e);
    const unsigned pixel = (unsigned)(u * k.img[1] + v);
    for (int s = 0; s < spp; ++s) {
      float pos[3] = {k.cam[0], k.cam[1], k.cam[2]}, d[3], thr[3] = {1.0f, 1.0f, 1.0f};
      [[maybe_unused]] float contrib[3] = {0.0f, 0.0f, 0.0f};
      render_camera_ray(k, u, v, render_rand(seed, pixel, s, 0), render_rand(seed, pixel, s, 1), d);
      int depth = 0;
      while (depth < k.depth) {                          // trace (renderer.py:346-411), material always DIFFUSE
        RenderHit h;
        render_next_hit(k, e, pos, d, h);
        const float hp[3] = {pos[0] + h.t * d[0], pos[1] + h.t * d[1], pos[2] + h.t * d[2]};
        const unsigned kk = 2u + 4u * (unsigned)depth;
        [[maybe_unused]] const unsigned kl = 0x40000000u + 4u * (unsigned)depth;
        ++depth;
        if (render_norm(h.n) != 0.0f) {
          float a[3] = {1.0f, 0.0f, 0.0f}, w[3];          // out_dir (renderer_utils.py:8-18)
          if (fabsf(h.n[1]) < 0.999f) {
            const float up[3] = {0.0f, 1.0f, 0.0f};
            render_cross(h.n, up, a);
            render_normalize(a);
          }
          render_cross(h.n, a, w);
          const float phi = 6.2831855f * render_rand(seed, pixel, s, kk);
          const float r = render_rand(seed, pixel, s, kk + 1);
          const float ay = sqrtf(r), ax = sqrtf(1.0f - r);
          const float cp = cosf(phi), sp = sinf(phi);
          const float su = render_rand(seed, pixel, s, kk + 2), sv = render_rand(seed, pixel, s, kk + 3);   // sample_sphere
          const float sx = su * 2.0f - 1.0f, sphi = (sv * 2.0f) * 3.1415927f, yz = sqrtf(1.0f - sx * sx);
          const float g[3] = {sx * h.rough, (yz * cosf(sphi)) * h.rough, (yz * sinf(sphi)) * h.rough};
#pragma unroll
          for (int c = 0; c < 3; ++c) d[c] = (ax * (cp * a[c] + sp * w[c]) + ay * h.n[c]) + g[c];
          render_normalize(d);
#pragma unroll
          for (int c = 0; c < 3; ++c) { pos[c] = hp[c] + 1e-4f * d[c]; thr[c] = thr[c] * h.c[c]; }
          if constexpr (LIGHT) {                         // :374-386, light_color = 1 (throughput * 1.0f is throughput)
            float direct[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) direct[c] = H.light_dir[c] + (render_rand(seed, pixel, s, kl + c) - 0.5f) * 0.03f;
            render_normalize(direct);
            const float dot = (direct[0] * h.n[0] + direct[1] * h.n[1]) + direct[2] * h.n[2];
            if (dot > 0.0f && !render_occluded(k, e, pos, direct))
#pragma unroll
              for (int c = 0; c < 3; ++c) contrib[c] += thr[c] * dot;
          }
        } else {
          depth = k.depth;                               // the sky
        }
        if constexpr (ROULETTE) {                        // :391-397, after every iteration, the sky's included; 0 / 0 as the reference's
          const float mc = fmaxf(fmaxf(thr[0], thr[1]), thr[2]);
          if (render_rand(seed, pixel, s, kl + 3u) > mc) {
            depth = k.depth;
            thr[0] = thr[1] = thr[2] = 0.0f;
          } else {
            thr[0] = thr[0] / mc; thr[1] = thr[1] / mc; thr[2] = thr[2] / mc;
          }
        }
      }
      if constexpr (LIGHT) {                             // :408-410: the sample is contrib, the sky term is not added
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += contrib[c];
      } else {
        float c1 = ((d[0] * 0.8f + d[1] * 0.65f) + d[2] * 0.15f) * 0.5f + 0.5f;      // sky_color
        c1 = fmaxf(fminf(c1, 1.0f), 0.0f);
        const float sky[3] = {(c1 * 0.9f + (1.0f - c1) * 0.7f) * 1.5f, (c1 * 0.9f + (1.0f - c1) * 0.7f) * 1.5f, (c1 * 0.9f + (1.0f - c1) * 0.8f) * 1.5f};
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += thr[c] * sky[c];
      }
    }
  }
  // copy (:414-426) and render_frame's img[:, ::-1].transpose(1, 0, 2): row = res1 - 1 - v, column = u
  const float fu = (float)u / (float)k.img[0], fv = (float)v / (float)k.img[1];
  const float du = fu - 0.5f, dv = fv - 0.5f;
  const float darken = 1.0f - 0.9f * fmaxf(sqrtf(du * du + dv * dv) - 0.0f, 0.0f);
  const long long o = (((long long)b * k.img[1] + (k.img[1] - 1 - v)) * k.img[0] + u) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) img[o + c] = live ? sqrtf(((acc[c] * darken) * R_EXPOSURE) / (float)spp) : 0.0f;
}

static int render_check_call(const char* fn, const ud_plb_render* h, int B) {
  if (!h) { set_error("%s: null handle", fn); return UD_ERR_INVALID; }
  if (B < 1 || B > h->max_envs) { set_error("%s: B=%d outside [1, max_envs=%d]", fn, B, h->max_envs); return UD_ERR_INVALID; }
  return UD_OK;
}

static int render_prims(const char* fn, ud_plb_render* h, int B, const double* pos, const double* rot, const double* gap, hipStream_t st) {
  if (h->k.np == 0) return UD_OK;
  if (!pos) { set_error("%s: null prim_pos on a handle with %d primitives", fn, h->k.np); return UD_ERR_INVALID; }
  for (int i = 0; i < h->k.np; ++i)
    if (h->k.kind[i] == 6 && !gap) { set_error("%s: null prim_gap on a handle with a Chopsticks", fn); return UD_ERR_INVALID; }
  const int n = B * h->k.np;
  hipLaunchKernelGGL(k_render_prims, dim3((n + 63) / 64), dim3(64), 0, st, h->k, B, pos, rot, gap, h->prim);
  return UD_OK;
}

}  // namespace ud

using namespace ud;

extern "C" {

int ud_plb_render_create(const ud_plb_render_conf* c, ud_plb_render** out) {
  if (!c || !out) { set_error("ud_plb_render_create: null argument"); return UD_ERR_INVALID; }
  if (c->use_directional_light || c->use_roulette) {
    set_error("ud_plb_render_create: use_directional_light / use_roulette of the conf must be 0: lighting is handle state, see ud_plb_render_set_light");
    return UD_ERR_UNSUPPORTED;
  }
  if (!(c->dx > 0.0) || c->bake_size < 0 || c->n_particles < 1 || c->max_envs < 1 || c->spp < 1 || c->max_ray_depth < 1 || c->image_res[0] < 1 ||
      c->image_res[1] < 1 || c->n_primitives < 0 || c->n_primitives > RP) {
    set_error("ud_plb_render_create: dx, bake_size, n_particles, max_envs, spp, max_ray_depth, image_res or n_primitives (0..%d) out of range", RP);
    return UD_ERR_INVALID;
  }
  for (int a = 0; a < 3; ++a)
    if (c->voxel_res[a] < 2 * c->bake_size || c->voxel_res[a] < 2 || c->voxel_res[a] > 1024) {
      set_error("ud_plb_render_create: voxel_res[%d]=%d below 2 * bake_size=%d (or outside [2, 1024])", a, c->voxel_res[a], 2 * c->bake_size);
      return UD_ERR_INVALID;
    }
  for (int i = 0; i < c->n_primitives; ++i)
    if (c->prim_kind[i] < 0 || c->prim_kind[i] > 6) { set_error("ud_plb_render_create: prim_kind[%d]=%d outside 0..6", i, c->prim_kind[i]); return UD_ERR_INVALID; }
  ud_plb_render* h = new ud_plb_render();
  RenderK& k = h->k;
  for (int a = 0; a < 3; ++a) { k.res[a] = c->voxel_res[a]; k.cam[a] = (float)c->camera_pos[a]; }
  k.bake = c->bake_size; k.img[0] = c->image_res[0]; k.img[1] = c->image_res[1]; k.depth = c->max_ray_depth; k.np = c->n_primitives; k.N = c->n_particles;
  k.cells = (long long)k.res[0] * k.res[1] * k.res[2];
  k.dx = (float)c->dx; k.inv_dx = (float)(1.0 / c->dx); k.thr = (float)c->sdf_threshold;
  k.fov_aspect = (float)(0.23 * ((double)c->image_res[0] / (double)c->image_res[1]));
  {  // renderer.py:433-441, in f64
    const double c0 = cos(c->camera_rot[0]), s0 = sin(c->camera_rot[0]), c1 = cos(c->camera_rot[1]), s1 = sin(c->camera_rot[1]);
    const double A[3][3] = {{c1, 0, s1}, {0, 1, 0}, {-s1, 0, c1}}, Bm[3][3] = {{1, 0, 0}, {0, c0, s0}, {0, -s0, c0}};
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) k.mat[3 * r + q] = (float)((A[r][0] * Bm[0][q] + A[r][1] * Bm[1][q]) + A[r][2] * Bm[2][q]);
  }
  for (int i = 0; i < RP; ++i) {
    const bool on = i < k.np;
    k.kind[i] = on ? c->prim_kind[i] : 0; k.radius[i] = on ? c->prim_radius[i] : 0.0; k.h[i] = on ? c->prim_h[i] : 0.0;
    for (int a = 0; a < 3; ++a) { k.shape[i][a] = on ? c->prim_shape[i][a] : 0.0; k.color[i][a] = on ? c->prim_color[i][a] : 0.0f; }
  }
  h->max_envs = c->max_envs; h->spp = c->spp;
  const size_t E = (size_t)c->max_envs, cells = (size_t)k.cells;
  hipError_t e = hipMalloc(&h->vol, E * cells * 8);
  if (e == hipSuccess) e = hipMalloc(&h->sdf, E * cells * 4);
  if (e == hipSuccess) e = hipMalloc(&h->tmp, E * cells * 4);
  if (e == hipSuccess) e = hipMalloc(&h->bbox, E * 6 * 4);
  if (e == hipSuccess) e = hipMalloc(&h->status, E * 4);
  if (e == hipSuccess) e = hipMalloc(&h->prim, E * RP * PRIM_STRIDE * 8);
  if (e == hipSuccess) e = hipMemset(h->prim, 0, E * RP * PRIM_STRIDE * 8);
  if (e == hipSuccess) e = hipMemset(h->status, 0, E * 4);
  if (e == hipSuccess) e = hipMemset(h->bbox, 0, E * 6 * 4);
  if (e != hipSuccess) {
    set_error("ud_plb_render_create: allocating %zu bytes per env for %d envs failed: %s", cells * 16, c->max_envs, hipGetErrorString(e));
    ud_plb_render_destroy(h);
    return UD_ERR_HIP;
  }
  *out = h;
  return UD_OK;
}

int ud_plb_render_destroy(ud_plb_render* h) {
  if (!h) return UD_OK;
  (void)hipFree(h->vol); (void)hipFree(h->sdf); (void)hipFree(h->tmp); (void)hipFree(h->bbox); (void)hipFree(h->status); (void)hipFree(h->prim);
  delete h;
  return UD_OK;
}

int ud_plb_render_set_light(ud_plb_render* h, const ud_plb_render_light* l) {
  if (!h || !l) { set_error("ud_plb_render_set_light: null argument"); return UD_ERR_INVALID; }
  float dir[3];
  for (int a = 0; a < 3; ++a) {
    if (!(fabs(l->light_direction[a]) <= 3.4028234663852886e38)) {       // NaN, inf, or beyond the largest f32
      set_error("ud_plb_render_set_light: light_direction (%g, %g, %g) is not finite in f32", l->light_direction[0], l->light_direction[1], l->light_direction[2]);
      return UD_ERR_INVALID;
    }
    dir[a] = (float)l->light_direction[a];
  }
  if (l->use_directional_light && dir[0] == 0.0f && dir[1] == 0.0f && dir[2] == 0.0f) {
    set_error("ud_plb_render_set_light: use_directional_light with a zero light_direction");
    return UD_ERR_INVALID;
  }
  h->light = l->use_directional_light != 0; h->roulette = l->use_roulette != 0;
  for (int a = 0; a < 3; ++a) h->light_dir[a] = dir[a];
  return UD_OK;
}

int ud_plb_render_bake(ud_plb_render* h, int B, const double* x, const int* color, float* bbox, int* status, void* stream) {
  if (int rc = render_check_call("ud_plb_render_bake", h, B)) return rc;
  if (!x || !color || !bbox || !status) { set_error("ud_plb_render_bake: null x / color / bbox / status"); return UD_ERR_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  const RenderK& k = h->k;
  const long long total = (long long)B * k.cells, S = 2 * k.bake + 2, splat = (long long)B * k.N * S * S * S;
  hipLaunchKernelGGL(k_render_bbox, dim3(B), dim3(256), 0, st, k, x, h->bbox, h->status, bbox, status);
  hipLaunchKernelGGL(k_render_fill, dim3((unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536)), dim3(256), 0, st, total, h->vol);
  hipLaunchKernelGGL(k_render_splat, dim3((unsigned)((splat + 255) / 256)), dim3(256), 0, st, k, splat, x, color, h->bbox, h->status, h->vol);
  hipLaunchKernelGGL(k_render_smooth<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, k, total, h->vol, (const float*)nullptr, h->tmp);
  hipLaunchKernelGGL(k_render_smooth<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, k, total, (const long long*)nullptr, h->tmp, h->sdf);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

int ud_plb_render_read_volume(ud_plb_render* h, int B, long long* packed, float* sdf, void* stream) {
  if (int rc = render_check_call("ud_plb_render_read_volume", h, B)) return rc;
  if (!packed && !sdf) { set_error("ud_plb_render_read_volume: null packed and sdf"); return UD_ERR_INVALID; }
  const size_t n = (size_t)B * (size_t)h->k.cells;
  if (packed) UD_HIP_CHECK(hipMemcpyAsync(packed, h->vol, n * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (sdf) UD_HIP_CHECK(hipMemcpyAsync(sdf, h->sdf, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return UD_OK;
}

int ud_plb_render_gbuffer(ud_plb_render* h, int B, const double* prim_pos, const double* prim_rot, const double* prim_gap, int* kind, float* t,
                          float* normal, float* albedo, void* stream) {
  if (int rc = render_check_call("ud_plb_render_gbuffer", h, B)) return rc;
  if (!kind || !t || !normal || !albedo) { set_error("ud_plb_render_gbuffer: null kind / t / normal / albedo"); return UD_ERR_INVALID; }
  if (int rc = render_prims("ud_plb_render_gbuffer", h, B, prim_pos, prim_rot, prim_gap, (hipStream_t)stream)) return rc;
  const dim3 grid((h->k.img[0] + 15) / 16, (h->k.img[1] + 15) / 16, B);
  hipLaunchKernelGGL(k_render_gbuffer, grid, dim3(256), 0, (hipStream_t)stream, *h, kind, t, normal, albedo);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

int ud_plb_render_image(ud_plb_render* h, int B, const double* prim_pos, const double* prim_rot, const double* prim_gap, int spp, unsigned int seed,
                        float* img, void* stream) {
  if (int rc = render_check_call("ud_plb_render_image", h, B)) return rc;
  if (!img) { set_error("ud_plb_render_image: null img"); return UD_ERR_INVALID; }
  if (spp < 0 || spp > 65536) { set_error("ud_plb_render_image: spp=%d outside [0, 65536] (0 = the conf's)", spp); return UD_ERR_INVALID; }
  if (int rc = render_prims("ud_plb_render_image", h, B, prim_pos, prim_rot, prim_gap, (hipStream_t)stream)) return rc;
  const dim3 grid((h->k.img[0] + 15) / 16, (h->k.img[1] + 15) / 16, B);
  auto kern = h->light ? (h->roulette ? k_render_image<true, true> : k_render_image<true, false>)
                       : (h->roulette ? k_render_image<false, true> : k_render_image<false, false>);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, *h, spp ? spp : h->spp, seed, img);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

}  // extern "C"
