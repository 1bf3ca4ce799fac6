// The cloth envs' camera view (MeshPyRenderer.render of the reference, daxbench/core/engine/pyrender/py_render.py) for M frames per call:
// the cloth's triangle mesh, one analytic sphere per gripper and the ground rectangle, seen by the reference's camera, as colour (u8),
// depth (f32, eye-space -z) and the winning triangle id.  f32 throughout, built with -ffp-contract=off and correctly rounded divide / sqrt,
// every operation written in the order include/unidom_hip.h states, so that tests/cloth_render_twin.py (NumPy f32) is bit-equal in every
// pixel.  The geometry (camera, projection, coverage, depth, mirror, channel order) is the reference's; the SHADING IS THIS PROJECT'S OWN
// (pyrender's PBR shader cannot be pinned here), the ground is one flat colour (the wood texture is not shipped), the gripper an analytic
// sphere (the reference draws an icosphere) and a triangle with a vertex nearer than znear is dropped whole instead of clipped.
//
// Mapping.  k_cr_setup: one thread per (frame, vertex) -> eye-space position and projection, in a handle arena (20 B per vertex and
// frame).  k_cr_tile: one workgroup of 256 per (frame, 32 x 32 pixel tile).  It walks the frame's triangle list in chunks of 1024: each
// thread tests four triangles against the tile (near plane, zero area, bounding box) and appends the survivors to an LDS list; then each
// of the four waves takes every fourth survivor and rasterises the part of its bounding box that lies in the tile, one lane per pixel (a
// box narrower than 32 pixels packs several rows into one pass), into an LDS z-buffer of packed (depth bits << 32 | triangle id) with one
// 64-bit LDS atomic minimum per covered pixel (ds_min_u64).  Depth is positive, so the bit order is the numeric order, and the minimum
// of the packed word is "nearest, then lowest triangle id" whatever the arrival order: the result is bit-identical from run to run.
// The resolve phase runs per pixel: spheres and ground analytically, the nearest of the three, shading, and the stores, already
// mirrored.  No global atomics, no clear pass, every loop bounded, no workgroup waits for another.
#include "common.h"

namespace ud {

constexpr int CR_TILE = 32, CR_CHUNK = 1024, CR_THREADS = 256;
constexpr int CR_MAX_DIM = 4096, CR_MAX_VERTS = 1 << 20, CR_MAX_FACES = 1 << 20, CR_MAX_SPHERES = 16, CR_MAX_FRAMES = 65535;

struct ClothRenderK {   // constants of a handle, formed in f64 at create and rounded to f32 once; passed to both kernels by value
  int W, H, V, F, S;
  float R[3][3];        // rows: the camera's x, y, z axes in the render frame
  float P[3];           // camera (= light) position, render frame
  float fx, fy, cx, cy, znear;
  float gmin[2], gmax[2], gz;
  float cos_outer, cos_range, inv_pi;
  float col[3][3];      // cloth, sphere, ground (RGB)
};

struct CrVert { float sx, sy, d, xe, ye; };

// sim-order point (x, y, z) -> render frame (x, z, y) -> eye frame
__device__ __forceinline__ void cr_eye(const ClothRenderK& k, float x, float y, float z, float& xe, float& ye, float& ze) {
  const float dx = x - k.P[0], dy = z - k.P[1], dz = y - k.P[2];
  xe = (k.R[0][0] * dx + k.R[0][1] * dy) + k.R[0][2] * dz;
  ye = (k.R[1][0] * dx + k.R[1][1] * dy) + k.R[1][2] * dz;
  ze = (k.R[2][0] * dx + k.R[2][1] * dy) + k.R[2][2] * dz;
}

__global__ void __launch_bounds__(CR_THREADS) k_cr_setup(ClothRenderK k, long long total, const float* __restrict__ verts,
                                                         float4* __restrict__ pv, float* __restrict__ pye) {
  const long long i = (long long)blockIdx.x * CR_THREADS + threadIdx.x;
  if (i >= total) return;
  float xe, ye, ze;
  cr_eye(k, verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], xe, ye, ze);
  const float d = -ze;
  pv[i] = make_float4(k.cx + (k.fx * xe) / d, k.cy - (k.fy * ye) / d, d, xe);
  pye[i] = ye;
}

// edge function of the directed edge p -> q at (px, py), evaluated from the endpoint with the lower vertex index so that the two
// triangles sharing an edge compute exact negatives of one another (no hole, no matter how the roundings fall)
__device__ __forceinline__ float cr_edge(const float4& p, const float4& q, int ip, int iq, float px, float py) {
  const bool fwd = ip < iq;
  const float x0 = fwd ? p.x : q.x, y0 = fwd ? p.y : q.y, x1 = fwd ? q.x : p.x, y1 = fwd ? q.y : p.y;
  const float e = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0);
  return fwd ? e : -e;
}

struct CrTri {
  float4 a, b, c;
  int ia, ib, ic;
  float s;                // +1 / -1: the sign of the doubled screen area
  int x0, x1, y0, y1;     // bounding box of pixel centres, clipped to the tile (inclusive)
};

// false: the triangle puts nothing into this tile
__device__ __forceinline__ bool cr_tri_setup(const ClothRenderK& k, const int* __restrict__ faces, const float4* __restrict__ pv, int t, int tx0, int tx1,
                                             int ty0, int ty1, CrTri& T) {
  T.ia = faces[3 * t]; T.ib = faces[3 * t + 1]; T.ic = faces[3 * t + 2];
  T.a = pv[T.ia]; T.b = pv[T.ib]; T.c = pv[T.ic];
  if (!(T.a.z >= k.znear) || !(T.b.z >= k.znear) || !(T.c.z >= k.znear)) return false;
  const float area = (T.b.x - T.a.x) * (T.c.y - T.a.y) - (T.b.y - T.a.y) * (T.c.x - T.a.x);
  if (!(area > 0.0f || area < 0.0f)) return false;
  T.s = area > 0.0f ? 1.0f : -1.0f;
  const float lx = fmaxf(ceilf(fminf(fminf(T.a.x, T.b.x), T.c.x) - 0.5f), (float)tx0);
  const float hx = fminf(floorf(fmaxf(fmaxf(T.a.x, T.b.x), T.c.x) - 0.5f), (float)(tx1 - 1));
  const float ly = fmaxf(ceilf(fminf(fminf(T.a.y, T.b.y), T.c.y) - 0.5f), (float)ty0);
  const float hy = fminf(floorf(fmaxf(fmaxf(T.a.y, T.b.y), T.c.y) - 0.5f), (float)(ty1 - 1));
  if (!(lx <= hx) || !(ly <= hy)) return false;
  T.x0 = (int)lx; T.x1 = (int)hx; T.y0 = (int)ly; T.y1 = (int)hy;
  return true;
}

// Lambert under the ambient term, the directional light along the eye's -z and the spot light at the eye; n (unit) and e in the eye frame
__device__ __forceinline__ float cr_lit(const ClothRenderK& k, float nx, float ny, float nz, float ex, float ey, float ez) {
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

__device__ __forceinline__ unsigned char cr_u8(float c) { return (unsigned char)(int)(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f + 0.5f); }

__global__ void __launch_bounds__(CR_THREADS) k_cr_tile(ClothRenderK k, const int* __restrict__ faces, const float4* __restrict__ pv_all,
                                                        const float* __restrict__ pye_all, const float* __restrict__ spheres,
                                                        unsigned char* __restrict__ color, float* __restrict__ depth, int* __restrict__ tri) {
  __shared__ unsigned long long zb[CR_TILE * CR_TILE];
  __shared__ int list[CR_CHUNK];
  __shared__ int nlist;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = (k.W + CR_TILE - 1) / CR_TILE;
  const int tx0 = (int)(blockIdx.x % tiles_x) * CR_TILE, ty0 = (int)(blockIdx.x / tiles_x) * CR_TILE;
  const int tx1 = min(tx0 + CR_TILE, k.W), ty1 = min(ty0 + CR_TILE, k.H);
  const size_t m = blockIdx.y;
  const float4* __restrict__ pv = pv_all + m * (size_t)k.V;
  const float* __restrict__ pye = pye_all + m * (size_t)k.V;

  for (int i = tid; i < CR_TILE * CR_TILE; i += CR_THREADS) zb[i] = ~0ull;
  for (int base = 0; base < k.F; base += CR_CHUNK) {
    if (tid == 0) nlist = 0;
    __syncthreads();
    for (int j = 0; j < CR_CHUNK / CR_THREADS; ++j) {
      const int t = base + j * CR_THREADS + tid;
      CrTri T;
      if (t < k.F && cr_tri_setup(k, faces, pv, t, tx0, tx1, ty0, ty1, T)) list[atomicAdd(&nlist, 1)] = t;   // at most CR_CHUNK appends
    }
    __syncthreads();
    const int n = nlist;
    for (int s = wave; s < n; s += CR_THREADS / 64) {
      const int t = list[s];
      CrTri T;
      if (!cr_tri_setup(k, faces, pv, t, tx0, tx1, ty0, ty1, T)) continue;   // the same answer as above; wave-uniform
      const int bw = T.x1 - T.x0 + 1;                                         // 1 .. 32
      const int sh = bw > 1 ? 32 - __clz(bw - 1) : 0;                         // lanes per row: the next power of two
      const int x = T.x0 + (lane & ((1 << sh) - 1)), rows = 64 >> sh;
      if (x > T.x1) continue;
      const float px = (float)x + 0.5f;
      for (int y = T.y0 + (lane >> sh); y <= T.y1; y += rows) {
        const float py = (float)y + 0.5f;
        const float e0 = cr_edge(T.b, T.c, T.ib, T.ic, px, py), e1 = cr_edge(T.c, T.a, T.ic, T.ia, px, py), e2 = cr_edge(T.a, T.b, T.ia, T.ib, px, py);
        if (!(T.s * e0 >= 0.0f && T.s * e1 >= 0.0f && T.s * e2 >= 0.0f)) continue;
        const float esum = (e0 + e1) + e2;
        if (!(T.s * esum > 0.0f)) continue;
        const float w = (e0 / T.a.z + e1 / T.b.z) + e2 / T.c.z;
        const float dep = esum / w;
        if (!(dep >= k.znear)) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(dep) << 32) | (unsigned)t;
        atomicMin(&zb[(y - ty0) * CR_TILE + (x - tx0)], key);   // x in [tx0, tx1), y in [ty0, ty1): inside the tile
      }
    }
    __syncthreads();
  }
  __syncthreads();

  for (int i = tid; i < CR_TILE * CR_TILE; i += CR_THREADS) {
    const int x = tx0 + (i & (CR_TILE - 1)), y = ty0 + i / CR_TILE;
    if (x >= k.W || y >= k.H) continue;
    const float rx = (((float)x + 0.5f) - k.cx) / k.fx, ry = (k.cy - ((float)y + 0.5f)) / k.fy;
    // mesh
    const unsigned long long key = zb[i];
    int id = -1;
    float best = 0.0f;
    if (key != ~0ull) { id = (int)(unsigned)(key & 0xffffffffull); best = __uint_as_float((unsigned)(key >> 32)); }
    // spheres, in the eye frame: ray t * (rx, ry, -1)
    float snx = 0.0f, sny = 0.0f, snz = 0.0f;
    const float qa = (rx * rx + ry * ry) + 1.0f;
    for (int j = 0; j < k.S; ++j) {
      const float* sp = spheres + (m * (size_t)k.S + j) * 4;
      const float r = sp[3];
      if (!(r > 0.0f)) continue;
      float cxe, cye, cze;
      cr_eye(k, sp[0], sp[1], sp[2], cxe, cye, cze);
      const float tc = ((rx * cxe + ry * cye) - cze) / qa;
      const float qx = cxe - tc * rx, qy = cye - tc * ry, qz = cze + tc;
      const float h2 = r * r - ((qx * qx + qy * qy) + qz * qz);
      if (!(h2 >= 0.0f)) continue;
      const float ts = tc - sqrtf(h2 / qa);
      if (!(ts >= k.znear)) continue;
      if (id == -1 || ts < best) {
        id = -2; best = ts;
        snx = (ts * rx - cxe) / r; sny = (ts * ry - cye) / r; snz = (-ts - cze) / r;
      }
    }
    // ground, in the render frame
    const float D0 = (k.R[0][0] * rx + k.R[1][0] * ry) - k.R[2][0], D1 = (k.R[0][1] * rx + k.R[1][1] * ry) - k.R[2][1],
                D2 = (k.R[0][2] * rx + k.R[1][2] * ry) - k.R[2][2];
    if (D2 < 0.0f) {
      const float tg = (k.gz - k.P[2]) / D2;
      const float hx = k.P[0] + tg * D0, hy = k.P[1] + tg * D1;
      if (tg >= k.znear && hx >= k.gmin[0] && hx <= k.gmax[0] && hy >= k.gmin[1] && hy <= k.gmax[1] && (id == -1 || tg < best)) { id = -3; best = tg; }
    }
    // shade
    unsigned char c0 = 255, c1 = 255, c2 = 255;
    if (id != -1) {
      const float ex = best * rx, ey = best * ry, ez = -best;
      float nx, ny, nz;
      int mat;
      if (id >= 0) {
        const int ia = faces[3 * id], ib = faces[3 * id + 1], ic = faces[3 * id + 2];
        const float4 a = pv[ia], b = pv[ib], c = pv[ic];
        const float ux = b.w - a.w, uy = pye[ib] - pye[ia], uz = a.z - b.z;   // eye z = -d
        const float vx = c.w - a.w, vy = pye[ic] - pye[ia], vz = a.z - c.z;
        nx = uy * vz - uz * vy; ny = uz * vx - ux * vz; nz = ux * vy - uy * vx;
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        if (len > 0.0f) { nx = nx / len; ny = ny / len; nz = nz / len; } else { nx = 0.0f; ny = 0.0f; nz = 1.0f; }
        mat = 0;
      } else if (id == -2) {
        nx = snx; ny = sny; nz = snz; mat = 1;
      } else {
        nx = k.R[0][2]; ny = k.R[1][2]; nz = k.R[2][2]; mat = 2;
      }
      const float lit = cr_lit(k, nx, ny, nz, ex, ey, ez);
      c0 = cr_u8(k.col[mat][0] * lit); c1 = cr_u8(k.col[mat][1] * lit); c2 = cr_u8(k.col[mat][2] * lit);
    }
    const size_t o = (m * (size_t)k.H + (size_t)y) * (size_t)k.W + (size_t)(k.W - 1 - x);   // mirrored left-right
    color[3 * o] = c2; color[3 * o + 1] = c1; color[3 * o + 2] = c0;                          // channels reversed (BGR)
    depth[o] = best;
    if (tri) tri[o] = id;
  }
}

}  // namespace ud

struct ud_cloth_render {
  ud::ClothRenderK k;
  int max_frames;
  int* faces;      // [F][3]
  float4* pv;      // [max_frames][V]  (sx, sy, depth, eye x)
  float* pye;      // [max_frames][V]  eye y
};

using namespace ud;

extern "C" {

int ud_cloth_render_create(const ud_cloth_render_conf* c, const int* faces, ud_cloth_render** out) {
  if (!c || !out || (!faces && c->n_faces > 0)) { set_error("ud_cloth_render_create: null argument"); return UD_ERR_INVALID; }
  if (c->width < 1 || c->height < 1 || c->n_vertices < 1 || c->n_faces < 0 || c->n_spheres < 0 || c->max_frames < 1 ||
      !(c->yfov > 0.0 && c->yfov < 3.14159) || !(c->znear > 0.0)) {
    set_error("ud_cloth_render_create: width, height, n_vertices, n_faces, n_spheres, max_frames, yfov (0, pi) or znear (> 0) out of range");
    return UD_ERR_INVALID;
  }
  if (c->width > CR_MAX_DIM || c->height > CR_MAX_DIM || c->n_vertices > CR_MAX_VERTS || c->n_faces > CR_MAX_FACES || c->n_spheres > CR_MAX_SPHERES ||
      c->max_frames > CR_MAX_FRAMES || (long long)c->max_frames * c->n_vertices > 0x7fffff00ll) {
    set_error("ud_cloth_render_create: supported are images up to %d x %d, %d vertices, %d faces, %d spheres, %d frames and max_frames * n_vertices < 2^31",
              CR_MAX_DIM, CR_MAX_DIM, CR_MAX_VERTS, CR_MAX_FACES, CR_MAX_SPHERES, CR_MAX_FRAMES);
    return UD_ERR_UNSUPPORTED;
  }
  for (long long i = 0; i < 3ll * c->n_faces; ++i)
    if (faces[i] < 0 || faces[i] >= c->n_vertices) {
      set_error("ud_cloth_render_create: faces[%lld][%lld]=%d outside [0, n_vertices=%d)", i / 3, i % 3, faces[i], c->n_vertices);
      return UD_ERR_INVALID;
    }
  // look_at (py_render.py:50-70) in f64: z = normalize(position - target), x = normalize(up x z), y = z x x
  double z[3], x[3], y[3];
  for (int a = 0; a < 3; ++a) z[a] = c->camera_pos[a] - c->camera_target[a];
  const double zn = sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
  if (!(zn > 0.0)) { set_error("ud_cloth_render_create: camera_pos equals camera_target"); return UD_ERR_INVALID; }
  for (int a = 0; a < 3; ++a) z[a] /= zn;
  const double* u = c->camera_up;
  x[0] = u[1] * z[2] - u[2] * z[1]; x[1] = u[2] * z[0] - u[0] * z[2]; x[2] = u[0] * z[1] - u[1] * z[0];
  const double xn = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
  if (!(xn > 0.0)) { set_error("ud_cloth_render_create: camera_up is parallel to the viewing direction"); return UD_ERR_INVALID; }
  for (int a = 0; a < 3; ++a) x[a] /= xn;
  y[0] = z[1] * x[2] - z[2] * x[1]; y[1] = z[2] * x[0] - z[0] * x[2]; y[2] = z[0] * x[1] - z[1] * x[0];

  ud_cloth_render* h = new ud_cloth_render();
  ClothRenderK& k = h->k;
  k.W = c->width; k.H = c->height; k.V = c->n_vertices; k.F = c->n_faces; k.S = c->n_spheres;
  for (int a = 0; a < 3; ++a) { k.R[0][a] = (float)x[a]; k.R[1][a] = (float)y[a]; k.R[2][a] = (float)z[a]; k.P[a] = (float)c->camera_pos[a]; }
  const double th = tan(0.5 * c->yfov), aspect = (double)c->width / (double)c->height;
  k.fx = (float)((0.5 * c->width) / (aspect * th)); k.fy = (float)((0.5 * c->height) / th);
  k.cx = (float)(0.5 * c->width); k.cy = (float)(0.5 * c->height); k.znear = (float)c->znear;
  for (int a = 0; a < 2; ++a) { k.gmin[a] = (float)c->ground_min[a]; k.gmax[a] = (float)c->ground_max[a]; }
  k.gz = (float)c->ground_z;
  const double pi = 3.14159265358979323846, co = cos(pi / 6.0), ci = cos(pi / 16.0);
  k.cos_outer = (float)co; k.cos_range = (float)(ci - co); k.inv_pi = (float)(1.0 / pi);
  for (int a = 0; a < 3; ++a) { k.col[0][a] = c->cloth_color[a]; k.col[1][a] = c->sphere_color[a]; k.col[2][a] = c->ground_color[a]; }
  h->max_frames = c->max_frames;
  const size_t MV = (size_t)c->max_frames * (size_t)c->n_vertices, FB = (size_t)(c->n_faces > 0 ? c->n_faces : 1) * 12;
  hipError_t e = hipMalloc(&h->faces, FB);
  if (e == hipSuccess) e = hipMalloc(&h->pv, MV * 16);
  if (e == hipSuccess) e = hipMalloc(&h->pye, MV * 4);
  if (e == hipSuccess && c->n_faces > 0) e = hipMemcpy(h->faces, faces, (size_t)c->n_faces * 12, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_error("ud_cloth_render_create: allocating %zu bytes for %d frames failed: %s", MV * 20 + FB, c->max_frames, hipGetErrorString(e));
    ud_cloth_render_destroy(h);
    return UD_ERR_HIP;
  }
  *out = h;
  return UD_OK;
}

int ud_cloth_render_destroy(ud_cloth_render* h) {
  if (!h) return UD_OK;
  (void)hipFree(h->faces); (void)hipFree(h->pv); (void)hipFree(h->pye);
  delete h;
  return UD_OK;
}

int ud_cloth_render_frames(ud_cloth_render* h, int M, const float* vertices, const float* spheres, unsigned char* color, float* depth, int* tri,
                           void* stream) {
  if (!h) { set_error("ud_cloth_render_frames: null handle"); return UD_ERR_INVALID; }
  if (M < 1 || M > h->max_frames) { set_error("ud_cloth_render_frames: M=%d outside [1, max_frames=%d]", M, h->max_frames); return UD_ERR_INVALID; }
  if (!vertices || !color || !depth || (h->k.S > 0 && !spheres)) {
    set_error("ud_cloth_render_frames: null vertices / color / depth (or spheres on a handle with %d)", h->k.S);
    return UD_ERR_INVALID;
  }
  const ClothRenderK& k = h->k;
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)M * k.V;
  hipLaunchKernelGGL(k_cr_setup, dim3((unsigned)((total + CR_THREADS - 1) / CR_THREADS)), dim3(CR_THREADS), 0, st, k, total, vertices, h->pv, h->pye);
  const unsigned tiles = (unsigned)(((k.W + CR_TILE - 1) / CR_TILE) * ((k.H + CR_TILE - 1) / CR_TILE));
  hipLaunchKernelGGL(k_cr_tile, dim3(tiles, (unsigned)M), dim3(CR_THREADS), 0, st, k, h->faces, h->pv, h->pye, spheres, color, depth, tri);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

}  // extern "C"
