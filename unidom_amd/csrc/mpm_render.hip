// The MLS-MPM envs' camera view (ParticlePyRenderer / WaterPyRenderer of the reference, daxbench/core/engine/pyrender/py_render.py:120-174,
// and the primitive drawing of envs/basic/mpm_env.py:200-236) for M frames per call: one analytic sphere (mode 0) or one screen-space
// point (mode 1) per particle, the primitives the particles collide with (oriented boxes or cut hollow spheres, drawn from the simulator's
// own transform) and the ground rectangle, seen by the reference's camera, as colour (u8 RGB), depth (f32, eye-space -z) and an id image.
// f32 throughout, built with -ffp-contract=off and correctly rounded divide / sqrt, every operation written in the order
// include/unidom_hip.h states, so that tests/mpm_render_twin.py (NumPy f32, brute force over all pixels) is bit-equal in every pixel.
// Camera, pixel rays, ground, shading and u8 rounding are the cloth renderer's (cloth_render.hip; the few device functions are copied, not
// shared, so that file stays as it is).  NOT the reference's: analytic spheres for uv_sphere meshes, one-layer point blending, primitive
// pose without the Euler detour, a sphere-traced bowl for its marching-cubes mesh, whole-particle drop at the near plane, this project's
// shading and colours, a flat ground.
//
// Mapping.  k_mr_setup: one thread per (frame, particle) -> eye-space centre and projection, in a handle arena (20 B per particle and
// frame), plus one thread per (frame, primitive) -> the sim-to-local matrix and the camera in the local frame (48 B).  k_mr_tile: one
// workgroup of 256 per (frame, 32 x 32 pixel tile).  It walks the frame's particle list in chunks of 1024: each thread tests four
// particles against the tile (drop rule, then a conservative screen-space window) and appends the survivors to an LDS list; then each of
// the four waves takes every fourth survivor and evaluates the exact per-pixel test over the part of its window that lies in the tile,
// one lane per pixel (points up to 4 pixels wide: one lane per survivor instead), into an LDS z-buffer of packed
// (depth bits << 32 | particle id) with one 64-bit LDS atomic minimum per covered pixel.  Depth is positive, so the minimum of the packed word is "nearest, then lowest particle id" whatever the arrival order.  The
// window only culls: the per-pixel test is the specification's, which has no window at all.  The resolve phase runs per pixel:
// primitives and ground analytically, the nearest of all, shading, blending in point mode, and the stores.  No global atomics, no clear
// pass, every loop bounded, no workgroup waits for another.
#include "common.h"

namespace ud {

constexpr int MR_TILE = 32, MR_CHUNK = 1024, MR_THREADS = 256;
constexpr int MR_MAX_DIM = 4096, MR_MAX_PARTICLES = 1 << 20, MR_MAX_PRIMS = 16, MR_MAX_FRAMES = 65535;
constexpr int MR_MARCH_K = 64;                   // sphere-trace iterations of the cut hollow sphere
constexpr float MR_MARCH_EPS = 1.0e-4f;          // hit when the SDF falls to this
constexpr float MR_NORMAL_STEP = 1.0e-4f;        // central-difference step of its normal
constexpr float MR_SMALL_POINT_HALF = 2.0f;      // points up to 4 pixels wide take the lane-per-particle path of k_mr_tile
constexpr int MR_PRIM_FLOATS = 12;               // per (frame, primitive): A[3][3] row-major, then the camera in the local frame

struct MpmRenderK {     // constants of a handle, formed in f64 at create and rounded to f32 once; passed to both kernels by value
  int W, H, N, NP, mode, kind;
  float R[3][3];        // rows: the camera's x, y, z axes in the render frame
  float P[3];           // camera (= light) position, render frame
  float fx, fy, cx, cy, znear;
  float gmin[2], gmax[2], gz;
  float cos_outer, cos_range, inv_pi;
  float pcol[3], alpha, oma;   // particle RGB, alpha and 1 - alpha (f32 subtraction)
  float col[2][3];             // primitive, ground (RGB)
  float rad, half, dmin;       // sphere radius; point_size / 2; the drop threshold znear + rad (mode 0) or znear (mode 1)
};

// sim-order point (x, y, z) -> render frame (x, z, y) -> eye frame
__device__ __forceinline__ void mr_eye(const MpmRenderK& k, float x, float y, float z, float& xe, float& ye, float& ze) {
  const float dx = x - k.P[0], dy = z - k.P[1], dz = y - k.P[2];
  xe = (k.R[0][0] * dx + k.R[0][1] * dy) + k.R[0][2] * dz;
  ye = (k.R[1][0] * dx + k.R[1][1] * dy) + k.R[1][2] * dz;
  ze = (k.R[2][0] * dx + k.R[2][1] * dy) + k.R[2][2] * dz;
}

// qrot_batch (primitives.py:95-102) in the order csrc/mpm_collide.h::qrot_x states it
__device__ __forceinline__ void mr_qrot(const float* q, float v0, float v1, float v2, float* o) {
  const float uv0 = q[2] * v2 - q[3] * v1, uv1 = q[3] * v0 - q[1] * v2, uv2 = q[1] * v1 - q[2] * v0;
  const float w0 = q[2] * uv2 - q[3] * uv1, w1 = q[3] * uv0 - q[1] * uv2, w2 = q[1] * uv1 - q[2] * uv0;
  o[0] = v0 + 2.0f * (q[0] * uv0 + w0);
  o[1] = v1 + 2.0f * (q[0] * uv1 + w1);
  o[2] = v2 + 2.0f * (q[0] * uv2 + w2);
}

__global__ void __launch_bounds__(MR_THREADS) k_mr_setup(MpmRenderK k, long long n_part, long long n_prim, const float* __restrict__ x,
                                                         const float* __restrict__ prim_pos, const float* __restrict__ prim_rot,
                                                         float4* __restrict__ pa, float* __restrict__ psy, float* __restrict__ pf) {
  const long long i = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
  if (i < n_part) {
    const float x0 = x[3 * i], x1 = x[3 * i + 1], x2 = x[3 * i + 2];
    const bool fin = fabsf(x0) <= 3.4028235e38f && fabsf(x1) <= 3.4028235e38f && fabsf(x2) <= 3.4028235e38f;
    float xe, ye, ze;
    mr_eye(k, x0, x1, x2, xe, ye, ze);
    const float d = -ze;
    if (fin) {
      pa[i] = make_float4(xe, ye, d, k.cx + (k.fx * xe) / d);
      psy[i] = k.cy - (k.fy * ye) / d;
    } else {
      pa[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // depth 0 is below every drop threshold (znear > 0)
      psy[i] = 0.0f;
    }
    return;
  }
  const long long j = i - n_part;
  if (j >= n_prim) return;
  const float* q = prim_rot + 4 * j;
  const float* p = prim_pos + 3 * j;
  const float c0 = q[0], c1 = -q[1], c2 = -q[2], c3 = -q[3];                       // inv_trans_batch, primitives.py:105-109
  const float nq = sqrtf(((c0 * c0 + c1 * c1) + c2 * c2) + c3 * c3) + 1e-12f;
  const float iq[4] = {c0 / nq, c1 / nq, c2 / nq, c3 / nq};
  float e0[3], e1[3], e2[3], ol[3];
  mr_qrot(iq, 1.0f, 0.0f, 0.0f, e0);
  mr_qrot(iq, 0.0f, 1.0f, 0.0f, e1);
  mr_qrot(iq, 0.0f, 0.0f, 1.0f, e2);
  mr_qrot(iq, k.P[0] - p[0], k.P[2] - p[1], k.P[1] - p[2], ol);                    // the camera, sim order, in the local frame
  float* f = pf + MR_PRIM_FLOATS * j;
  for (int a = 0; a < 3; ++a) { f[3 * a] = e0[a]; f[3 * a + 1] = e1[a]; f[3 * a + 2] = e2[a]; f[9 + a] = ol[a]; }
}

// The conservative pixel window of a particle inside the tile; false: the particle is dropped or puts nothing into this tile.
// a = (xe, ye, d, sx).  Mode 0: every point of the sphere has depth in [d - r, d + r] (d - r > 0 by the drop rule) and eye x in
// [xe - r, xe + r], so x / depth lies between the two corner quotients below; one more pixel each way covers the roundings.
// Mode 1: the square of the specification, one more pixel each way.  A NaN bound falls back to the tile's own edge (fmaxf / fminf
// return the other operand), never to an index outside the tile.
__device__ __forceinline__ bool mr_window(const MpmRenderK& k, const float4& a, float sy, int tx0, int tx1, int ty0, int ty1, int& x0, int& x1,
                                          int& y0, int& y1) {
  if (!(a.z >= k.dmin)) return false;
  float lox, hix, loy, hiy;
  if (k.mode == 0) {
    const float r = k.rad, zn = a.z - r, zf = a.z + r;
    const float xh = a.x + r, xl = a.x - r, yh = a.y + r, yl = a.y - r;
    lox = k.cx + k.fx * (xl / (xl <= 0.0f ? zn : zf)); hix = k.cx + k.fx * (xh / (xh >= 0.0f ? zn : zf));
    loy = k.cy - k.fy * (yh / (yh >= 0.0f ? zn : zf)); hiy = k.cy - k.fy * (yl / (yl <= 0.0f ? zn : zf));
  } else {
    lox = a.w - k.half; hix = a.w + k.half; loy = sy - k.half; hiy = sy + k.half;
  }
  const float lx = fmaxf(ceilf(lox - 0.5f) - 1.0f, (float)tx0), hx = fminf(floorf(hix - 0.5f) + 1.0f, (float)(tx1 - 1));
  const float ly = fmaxf(ceilf(loy - 0.5f) - 1.0f, (float)ty0), hy = fminf(floorf(hiy - 0.5f) + 1.0f, (float)(ty1 - 1));
  if (!(lx <= hx) || !(ly <= hy)) return false;
  x0 = (int)lx; x1 = (int)hx; y0 = (int)ly; y1 = (int)hy;     // each inside [tile start, tile end): finite, so the casts are defined
  return true;
}

// Lambert under the ambient term, the directional light along the eye's -z and the spot light at the eye; n (unit) and e in the eye frame
__device__ __forceinline__ float mr_lit(const MpmRenderK& k, float nx, float ny, float nz, float ex, float ey, float ez) {
  const float ne = (nx * ex + ny * ey) + nz * ez;
  if (ne > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
  const float ndl_d = fmaxf(nz, 0.0f);
  const float r2 = (ex * ex + ey * ey) + ez * ez;
  const float rl = sqrtf(r2);
  const float ndl_s = fmaxf(-((nx * ex + ny * ey) + nz * ez) / rl, 0.0f);
  const float cosang = -ez / rl;
  const float s = fminf(fmaxf((cosang - k.cos_outer) / k.cos_range, 0.0f), 1.0f);
  const float spot = (s * s) * (3.0f - 2.0f * s);
  return 0.05f + (1.0f * ndl_d + ((10.0f * spot) * ndl_s) / r2) * k.inv_pi;
}

__device__ __forceinline__ float mr_clamp01(float c) { return fminf(fmaxf(c, 0.0f), 1.0f); }
__device__ __forceinline__ unsigned char mr_u8(float c) { return (unsigned char)(int)(mr_clamp01(c) * 255.0f + 0.5f); }

// container.py:8-16 (cut hollow sphere, size = (r, h, t)) as csrc/mpm_collide.h::container_sdf_x states it; w = sqrt(r r - h h)
__device__ __forceinline__ float mr_bowl_sdf(float r, float h, float t, float w, float p0, float p1, float p2) {
  const float q0 = sqrtf((p0 * p0 + p2 * p2) + 1e-12f), q1 = p1;
  const bool mask = h * q0 < w * q1;
  const float d0 = q0 - w, d1 = q1 - h;
  const float val1 = sqrtf((d0 * d0 + d1 * d1) + 1e-12f) - t;
  const float val2 = fabsf(sqrtf((q0 * q0 + q1 * q1) + 1e-12f) - r) - t;
  return mask ? val1 : val2;
}

// box: slab test in the local frame (o + t dl); true on a hit, with its depth and the local normal
__device__ __forceinline__ bool mr_box(const float* s, const float* o, const float* dl, float znear, float& th, float* nl) {
  float tnear = -INFINITY, tfar = INFINITY;
  int ax = 0;
  for (int a = 0; a < 3; ++a) {
    if (dl[a] == 0.0f) {
      if (!(fabsf(o[a]) <= s[a])) return false;
      continue;
    }
    const float t1 = (-s[a] - o[a]) / dl[a], t2 = (s[a] - o[a]) / dl[a];
    const float tn = fminf(t1, t2), tf = fmaxf(t1, t2);
    if (tn > tnear) { tnear = tn; ax = a; }
    tfar = fminf(tfar, tf);
  }
  if (!(tnear <= tfar) || !(tnear >= znear)) return false;
  th = tnear;
  nl[0] = 0.0f; nl[1] = 0.0f; nl[2] = 0.0f;
  nl[ax] = dl[ax] > 0.0f ? -1.0f : 1.0f;
  return true;
}

// cut hollow sphere: sphere-trace its SDF between the entry and the exit of the bounding sphere of radius r + t
__device__ __forceinline__ bool mr_bowl(const float* s, const float* o, const float* dl, float znear, float& th, float* nl) {
  const float r = s[0], h = s[1], t = s[2];
  const float aa = (dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2];
  const float bq = (o[0] * dl[0] + o[1] * dl[1]) + o[2] * dl[2];
  const float tcb = -bq / aa;
  const float q0 = o[0] + tcb * dl[0], q1 = o[1] + tcb * dl[1], q2 = o[2] + tcb * dl[2];
  const float rb = r + t;
  const float h2 = rb * rb - ((q0 * q0 + q1 * q1) + q2 * q2);
  if (!(h2 >= 0.0f)) return false;
  const float hs = sqrtf(h2 / aa);
  const float tout = tcb + hs;
  float tt = fmaxf(tcb - hs, znear);
  if (!(tt <= tout)) return false;
  const float len = sqrtf(aa), w = sqrtf(r * r - h * h);
  bool hit = false;
  for (int it = 0; it < MR_MARCH_K; ++it) {
    const float v = mr_bowl_sdf(r, h, t, w, o[0] + tt * dl[0], o[1] + tt * dl[1], o[2] + tt * dl[2]);
    if (v <= MR_MARCH_EPS) { hit = true; break; }
    tt = tt + v / len;
    if (!(tt <= tout)) break;
  }
  if (!hit) return false;
  th = tt;
  const float p0 = o[0] + tt * dl[0], p1 = o[1] + tt * dl[1], p2 = o[2] + tt * dl[2], e = MR_NORMAL_STEP;
  const float n0 = mr_bowl_sdf(r, h, t, w, p0 + e, p1, p2) - mr_bowl_sdf(r, h, t, w, p0 - e, p1, p2);
  const float n1 = mr_bowl_sdf(r, h, t, w, p0, p1 + e, p2) - mr_bowl_sdf(r, h, t, w, p0, p1 - e, p2);
  const float n2 = mr_bowl_sdf(r, h, t, w, p0, p1, p2 + e) - mr_bowl_sdf(r, h, t, w, p0, p1, p2 - e);
  const float ln = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
  if (ln > 0.0f) { nl[0] = n0 / ln; nl[1] = n1 / ln; nl[2] = n2 / ln; } else { nl[0] = 0.0f; nl[1] = 0.0f; nl[2] = 1.0f; }
  return true;
}

__global__ void __launch_bounds__(MR_THREADS) k_mr_tile(MpmRenderK k, const float4* __restrict__ pa_all, const float* __restrict__ psy_all,
                                                        const float* __restrict__ pf_all, const float* __restrict__ psize,
                                                        unsigned char* __restrict__ color, float* __restrict__ depth, int* __restrict__ idimg) {
  __shared__ unsigned long long zb[MR_TILE * MR_TILE];
  __shared__ int list[MR_CHUNK];
  __shared__ int nlist;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (k.W + MR_TILE - 1) / MR_TILE;
  const int tx0 = (int)(blockIdx.x % tiles_x) * MR_TILE, ty0 = (int)(blockIdx.x / tiles_x) * MR_TILE;
  const int tx1 = min(tx0 + MR_TILE, k.W), ty1 = min(ty0 + MR_TILE, k.H);
  const size_t m = blockIdx.y;
  const float4* __restrict__ pa = pa_all + m * (size_t)k.N;
  const float* __restrict__ psy = psy_all + m * (size_t)k.N;

  for (int i = tid; i < MR_TILE * MR_TILE; i += MR_THREADS) zb[i] = ~0ull;
  for (int base = 0; base < k.N; base += MR_CHUNK) {
    if (tid == 0) nlist = 0;
    __syncthreads();
    for (int j = 0; j < MR_CHUNK / MR_THREADS; ++j) {
      const int t = base + j * MR_THREADS + tid;
      int x0, x1, y0, y1;
      if (t < k.N && mr_window(k, pa[t], psy[t], tx0, tx1, ty0, ty1, x0, x1, y0, y1)) list[atomicAdd(&nlist, 1)] = t;   // at most MR_CHUNK appends
    }
    __syncthreads();
    const int n = nlist;
    if (k.mode == 1 && k.half <= MR_SMALL_POINT_HALF) {
      // small points (a window of at most 6 x 6 pixels): one lane per survivor; a wave per survivor would leave 63 lanes idle, and a
      // tile under a heap of liquid holds thousands of them.  The same test, the same atomic minimum: the same image.
      for (int s = tid; s < n; s += MR_THREADS) {
        const int t = list[s];
        const float4 a = pa[t];
        const float sy = psy[t];
        int x0, x1, y0, y1;
        if (!mr_window(k, a, sy, tx0, tx1, ty0, ty1, x0, x1, y0, y1)) continue;
        const float plo = a.w - k.half, phi = a.w + k.half, qlo = sy - k.half, qhi = sy + k.half;
        const unsigned long long key = ((unsigned long long)__float_as_uint(a.z) << 32) | (unsigned)t;
        for (int y = y0; y <= y1; ++y) {
          const float py = (float)y + 0.5f;
          if (!(qlo <= py && py < qhi)) continue;
          for (int x = x0; x <= x1; ++x) {
            const float px = (float)x + 0.5f;
            if (plo <= px && px < phi) atomicMin(&zb[(y - ty0) * MR_TILE + (x - tx0)], key);   // inside the tile, as below
          }
        }
      }
    } else
    for (int s = wave; s < n; s += MR_THREADS / 64) {
      const int t = list[s];
      const float4 a = pa[t];
      const float sy = psy[t];
      int x0, x1, y0, y1;
      if (!mr_window(k, a, sy, tx0, tx1, ty0, ty1, x0, x1, y0, y1)) continue;   // the same answer as above; wave-uniform
      const int bw = x1 - x0 + 1;                                               // 1 .. 32
      const int sh = bw > 1 ? 32 - __clz(bw - 1) : 0;                           // lanes per row: the next power of two
      const int x = x0 + (lane & ((1 << sh) - 1)), rows = 64 >> sh;
      if (x > x1) continue;
      const float px = (float)x + 0.5f;
      const float rx = (px - k.cx) / k.fx;
      const float plo = a.w - k.half, phi = a.w + k.half, qlo = sy - k.half, qhi = sy + k.half;
      for (int y = y0 + (lane >> sh); y <= y1; y += rows) {
        const float py = (float)y + 0.5f;
        float dep;
        if (k.mode == 0) {
          const float ry = (k.cy - py) / k.fy;
          const float qa = (rx * rx + ry * ry) + 1.0f;
          const float cze = -a.z;
          const float tc = ((rx * a.x + ry * a.y) - cze) / qa;
          const float qx = a.x - tc * rx, qy = a.y - tc * ry, qz = cze + tc;
          const float h2 = k.rad * k.rad - ((qx * qx + qy * qy) + qz * qz);
          if (!(h2 >= 0.0f)) continue;
          dep = tc - sqrtf(h2 / qa);
          if (!(dep >= k.znear)) continue;
        } else {
          if (!(plo <= px && px < phi && qlo <= py && py < qhi)) continue;
          dep = a.z;
        }
        const unsigned long long key = ((unsigned long long)__float_as_uint(dep) << 32) | (unsigned)t;
        atomicMin(&zb[(y - ty0) * MR_TILE + (x - tx0)], key);   // x in [tx0, tx1), y in [ty0, ty1): inside the tile
      }
    }
    __syncthreads();
  }
  __syncthreads();

  const float* __restrict__ pf = pf_all + m * (size_t)k.NP * MR_PRIM_FLOATS;
  for (int i = tid; i < MR_TILE * MR_TILE; i += MR_THREADS) {
    const int x = tx0 + (i & (MR_TILE - 1)), y = ty0 + i / MR_TILE;
    if (x >= k.W || y >= k.H) continue;
    const float rx = (((float)x + 0.5f) - k.cx) / k.fx, ry = (k.cy - ((float)y + 0.5f)) / k.fy;
    const unsigned long long key = zb[i];
    int pid = -1;
    float pdep = 0.0f;
    if (key != ~0ull) { pid = (int)(unsigned)(key & 0xffffffffull); pdep = __uint_as_float((unsigned)(key >> 32)); }
    int id = -1;
    float best = 0.0f;
    if (k.mode == 0 && pid >= 0) { id = pid; best = pdep; }
    // the ray in the render frame; in sim order it is (D0, D2, D1)
    const float D0 = (k.R[0][0] * rx + k.R[1][0] * ry) - k.R[2][0], D1 = (k.R[0][1] * rx + k.R[1][1] * ry) - k.R[2][1],
                D2 = (k.R[0][2] * rx + k.R[1][2] * ry) - k.R[2][2];
    // primitives, each in its local frame
    float nx = 0.0f, ny = 0.0f, nz = 1.0f;
    for (int j = 0; j < k.NP; ++j) {
      const float* f = pf + j * MR_PRIM_FLOATS;
      const float* s = psize + 3 * j;
      const float dl[3] = {(f[0] * D0 + f[1] * D2) + f[2] * D1, (f[3] * D0 + f[4] * D2) + f[5] * D1, (f[6] * D0 + f[7] * D2) + f[8] * D1};
      const float ol[3] = {f[9], f[10], f[11]};
      const float sz[3] = {s[0], s[1], s[2]};
      float th, nl[3];
      const bool hit = k.kind == 0 ? mr_box(sz, ol, dl, k.znear, th, nl) : mr_bowl(sz, ol, dl, k.znear, th, nl);
      if (!hit) continue;
      if (id == -1 || th < best) {
        id = -4 - j; best = th;
        // local -> sim (the transpose of A) -> render (swap) -> eye
        const float s0 = (f[0] * nl[0] + f[3] * nl[1]) + f[6] * nl[2], s1 = (f[1] * nl[0] + f[4] * nl[1]) + f[7] * nl[2],
                    s2 = (f[2] * nl[0] + f[5] * nl[1]) + f[8] * nl[2];
        nx = (k.R[0][0] * s0 + k.R[0][1] * s2) + k.R[0][2] * s1;
        ny = (k.R[1][0] * s0 + k.R[1][1] * s2) + k.R[1][2] * s1;
        nz = (k.R[2][0] * s0 + k.R[2][1] * s2) + k.R[2][2] * s1;
      }
    }
    // ground, in the render frame
    if (D2 < 0.0f) {
      const float tg = (k.gz - k.P[2]) / D2;
      const float hx = k.P[0] + tg * D0, hy = k.P[1] + tg * D1;
      if (tg >= k.znear && hx >= k.gmin[0] && hx <= k.gmax[0] && hy >= k.gmin[1] && hy <= k.gmax[1] && (id == -1 || tg < best)) { id = -3; best = tg; }
    }
    // shade the nearest opaque thing
    float c0 = 1.0f, c1 = 1.0f, c2 = 1.0f;
    if (id != -1) {
      const float ex = best * rx, ey = best * ry, ez = -best;
      const float* base;
      if (id >= 0) {
        const float4 a = pa[id];
        nx = (best * rx - a.x) / k.rad; ny = (best * ry - a.y) / k.rad; nz = (-best - (-a.z)) / k.rad;
        base = k.pcol;
      } else if (id == -3) {
        nx = k.R[0][2]; ny = k.R[1][2]; nz = k.R[2][2]; base = k.col[1];
      } else {
        base = k.col[0];
      }
      const float lit = mr_lit(k, nx, ny, nz, ex, ey, ez);
      c0 = mr_clamp01(base[0] * lit); c1 = mr_clamp01(base[1] * lit); c2 = mr_clamp01(base[2] * lit);
    }
    // point mode: the nearest point of the pixel, unlit, blended over what is behind it
    if (k.mode == 1 && pid >= 0 && (id == -1 || pdep < best)) {
      id = pid; best = pdep;
      c0 = k.alpha * k.pcol[0] + k.oma * c0; c1 = k.alpha * k.pcol[1] + k.oma * c1; c2 = k.alpha * k.pcol[2] + k.oma * c2;
    }
    const size_t o = (m * (size_t)k.H + (size_t)y) * (size_t)k.W + (size_t)x;   // not mirrored, RGB
    color[3 * o] = mr_u8(c0); color[3 * o + 1] = mr_u8(c1); color[3 * o + 2] = mr_u8(c2);
    depth[o] = best;
    if (idimg) idimg[o] = id;
  }
}

}  // namespace ud

struct ud_mpm_render {
  ud::MpmRenderK k;
  int max_frames;
  float4* pa;      // [max_frames][N]  (eye x, eye y, depth, sx)
  float* psy;      // [max_frames][N]  sy
  float* pf;       // [max_frames][NP][12]
  float* psize;    // [NP][3]
};

using namespace ud;

extern "C" {

int ud_mpm_render_create(const ud_mpm_render_conf* c, const float* prim_sizes, ud_mpm_render** out) {
  if (!c || !out || (!prim_sizes && c->n_prims > 0)) { set_error("ud_mpm_render_create: null argument"); return UD_ERR_INVALID; }
  if (c->width < 1 || c->height < 1 || c->n_particles < 1 || c->n_prims < 0 || c->max_frames < 1 || !(c->yfov > 0.0 && c->yfov < 3.14159) ||
      !(c->znear > 0.0) || c->mode < 0 || c->mode > 1 || c->prim_kind < 0 || c->prim_kind > 1 || (c->mode == 0 && !(c->radius > 0.0)) ||
      c->point_size < 1) {
    set_error("ud_mpm_render_create: width, height, n_particles, n_prims, max_frames, yfov (0, pi), znear (> 0), mode (0, 1), prim_kind (0, 1), "
              "radius (> 0 in sphere mode) or point_size (>= 1) out of range");
    return UD_ERR_INVALID;
  }
  if (c->width > MR_MAX_DIM || c->height > MR_MAX_DIM || c->n_particles > MR_MAX_PARTICLES || c->n_prims > MR_MAX_PRIMS ||
      c->max_frames > MR_MAX_FRAMES || (long long)c->max_frames * c->n_particles > 0x7fffff00ll) {
    set_error("ud_mpm_render_create: supported are images up to %d x %d, %d particles, %d primitives, %d frames and max_frames * n_particles < 2^31",
              MR_MAX_DIM, MR_MAX_DIM, MR_MAX_PARTICLES, MR_MAX_PRIMS, MR_MAX_FRAMES);
    return UD_ERR_UNSUPPORTED;
  }
  // look_at (py_render.py:50-70) in f64: z = normalize(position - target), x = normalize(up x z), y = z x x
  double z[3], x[3], y[3];
  for (int a = 0; a < 3; ++a) z[a] = c->camera_pos[a] - c->camera_target[a];
  const double zn = sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
  if (!(zn > 0.0)) { set_error("ud_mpm_render_create: camera_pos equals camera_target"); return UD_ERR_INVALID; }
  for (int a = 0; a < 3; ++a) z[a] /= zn;
  const double* u = c->camera_up;
  x[0] = u[1] * z[2] - u[2] * z[1]; x[1] = u[2] * z[0] - u[0] * z[2]; x[2] = u[0] * z[1] - u[1] * z[0];
  const double xn = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
  if (!(xn > 0.0)) { set_error("ud_mpm_render_create: camera_up is parallel to the viewing direction"); return UD_ERR_INVALID; }
  for (int a = 0; a < 3; ++a) x[a] /= xn;
  y[0] = z[1] * x[2] - z[2] * x[1]; y[1] = z[2] * x[0] - z[0] * x[2]; y[2] = z[0] * x[1] - z[1] * x[0];

  ud_mpm_render* h = new ud_mpm_render();
  MpmRenderK& k = h->k;
  k.W = c->width; k.H = c->height; k.N = c->n_particles; k.NP = c->n_prims; k.mode = c->mode; k.kind = c->prim_kind;
  for (int a = 0; a < 3; ++a) { k.R[0][a] = (float)x[a]; k.R[1][a] = (float)y[a]; k.R[2][a] = (float)z[a]; k.P[a] = (float)c->camera_pos[a]; }
  const double th = tan(0.5 * c->yfov), aspect = (double)c->width / (double)c->height;
  k.fx = (float)((0.5 * c->width) / (aspect * th)); k.fy = (float)((0.5 * c->height) / th);
  k.cx = (float)(0.5 * c->width); k.cy = (float)(0.5 * c->height); k.znear = (float)c->znear;
  for (int a = 0; a < 2; ++a) { k.gmin[a] = (float)c->ground_min[a]; k.gmax[a] = (float)c->ground_max[a]; }
  k.gz = (float)c->ground_z;
  const double pi = 3.14159265358979323846, co = cos(pi / 6.0), ci = cos(pi / 16.0);
  k.cos_outer = (float)co; k.cos_range = (float)(ci - co); k.inv_pi = (float)(1.0 / pi);
  for (int a = 0; a < 3; ++a) { k.pcol[a] = c->particle_color[a]; k.col[0][a] = c->prim_color[a]; k.col[1][a] = c->ground_color[a]; }
  k.alpha = c->particle_color[3]; k.oma = 1.0f - k.alpha;
  k.rad = (float)c->radius; k.half = (float)c->point_size * 0.5f;
  k.dmin = c->mode == 0 ? k.znear + k.rad : k.znear;
  h->max_frames = c->max_frames;
  const size_t MN = (size_t)c->max_frames * (size_t)c->n_particles, NP1 = (size_t)(c->n_prims > 0 ? c->n_prims : 1);
  const size_t PFB = (size_t)c->max_frames * NP1 * MR_PRIM_FLOATS * 4;
  hipError_t e = hipMalloc(&h->pa, MN * 16);
  if (e == hipSuccess) e = hipMalloc(&h->psy, MN * 4);
  if (e == hipSuccess) e = hipMalloc(&h->pf, PFB);
  if (e == hipSuccess) e = hipMalloc(&h->psize, NP1 * 12);
  if (e == hipSuccess && c->n_prims > 0) e = hipMemcpy(h->psize, prim_sizes, (size_t)c->n_prims * 12, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_error("ud_mpm_render_create: allocating %zu bytes for %d frames failed: %s", MN * 20 + PFB + NP1 * 12, c->max_frames, hipGetErrorString(e));
    ud_mpm_render_destroy(h);
    return UD_ERR_HIP;
  }
  *out = h;
  return UD_OK;
}

int ud_mpm_render_destroy(ud_mpm_render* h) {
  if (!h) return UD_OK;
  (void)hipFree(h->pa); (void)hipFree(h->psy); (void)hipFree(h->pf); (void)hipFree(h->psize);
  delete h;
  return UD_OK;
}

int ud_mpm_render_frames(ud_mpm_render* h, int M, const float* x, const float* prim_pos, const float* prim_rot, unsigned char* color, float* depth,
                         int* id, void* stream) {
  if (!h) { set_error("ud_mpm_render_frames: null handle"); return UD_ERR_INVALID; }
  if (M < 1 || M > h->max_frames) { set_error("ud_mpm_render_frames: M=%d outside [1, max_frames=%d]", M, h->max_frames); return UD_ERR_INVALID; }
  if (!x || !color || !depth || (h->k.NP > 0 && (!prim_pos || !prim_rot))) {
    set_error("ud_mpm_render_frames: null x / color / depth (or prim_pos / prim_rot on a handle with %d primitives)", h->k.NP);
    return UD_ERR_INVALID;
  }
  const MpmRenderK& k = h->k;
  hipStream_t st = (hipStream_t)stream;
  const long long n_part = (long long)M * k.N, n_prim = (long long)M * k.NP, total = n_part + n_prim;
  hipLaunchKernelGGL(k_mr_setup, dim3((unsigned)((total + MR_THREADS - 1) / MR_THREADS)), dim3(MR_THREADS), 0, st, k, n_part, n_prim, x, prim_pos,
                     prim_rot, h->pa, h->psy, h->pf);
  const unsigned tiles = (unsigned)(((k.W + MR_TILE - 1) / MR_TILE) * ((k.H + MR_TILE - 1) / MR_TILE));
  hipLaunchKernelGGL(k_mr_tile, dim3(tiles, (unsigned)M), dim3(MR_THREADS), 0, st, k, h->pa, h->psy, h->pf, h->psize, color, depth, id);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

}  // extern "C"
