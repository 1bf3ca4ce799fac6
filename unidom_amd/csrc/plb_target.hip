// PLB goals: the target SDF of a target density (Loss.update_target / update_target_sdf, engine/losses/loss.py:77-106) and the soft
// IoU of two densities (iou_kernel, :239-254).  Handle-free: the caller owns every buffer; nothing is allocated, nothing synchronises.
//
// The map (one sweep, every cell I independently, from the copies S_c / P_c of the previous sweep; S_c = 1000 everywhere at the start):
//   density[I] > threshold:  S = 0, P = I
//   otherwise:               S = 1000; for o in {-3..2}^3 \ {0}, lexicographic with ox slowest, v = I + o inside the grid:
//                              if S_c[v] < 1000:  d = sqrt(dx^2 + dy^2 + dz^2 + 1e-8) of x_I - x_{P_c[v]}, x_J = J * (1 / n_grid);
//                                                 if d < S (strict): S = d, P = P_c[v]
// The sweep reads only "has v a nearest cell" and "which one": S_c[v] < 1000 holds exactly when v has one (d <= sqrt(3 + 1e-8)), and S
// is a function of (I, P).  So the whole state is one int32 per cell:
//   bit 31  no nearest cell yet (S = 1000)          bit 30  the cell is occupied (density > threshold; set once, never changes)
//   bits 0-29  P as (i << 20 | j << 10 | k): n_grid <= 1024, and no integer division to unpack it
// and x_J is recomputed from the index.  The state ping-pongs between two [T][G] int32 buffers in `work`.
//
// One launch per sweep, all of them enqueued; workgroups never wait for one another.  work holds one word per target, `last`: a sweep
// s (0-based) that changes any cell of target t raises last[t] to s + 1 (atomic max).  Launch s of target t returns at entry when
// last[t] < s, i.e. when sweep s - 1 changed nothing: the map is deterministic, so that state is a fixed point, both buffers hold it, and
// every later launch returns the same way (nobody raises last[t] again).  The result is that of all the sweeps.  While launch s runs
// last[t] is s or s + 1, both >= s, so a workgroup that starts late takes the same decision as one that started early.
//
// Exactness.  Candidates are compared as the map says, d < S on correctly rounded f64 square roots, but the root is taken only when it can
// matter: q >= q_S implies sqrt(q) >= sqrt(q_S) = S (sqrt is monotone), so such a candidate can never satisfy d < S and is dropped on
// the argument of the root; and a candidate with the same P as the one evaluated just before has the same d, which is not < S either.
// Both shortcuts drop only candidates the strict comparison would reject, so S and P are those of the literal loop, bit for bit
// (tests/test_plb_target_gpu.py against tests/plb_target_twin.py, also on a grid that is no power of two, where
// fl(i h) - fl(j h) != fl((i - j) h)).  Built with -ffp-contract=off: dx^2 + dy^2 + dz^2 + 1e-8 is summed left to right, unfused.
#include "common.h"

namespace ud {

constexpr int TGT_TX = 4, TGT_TY = 8, TGT_TZ = 8;           // tile: 256 threads, one wave per x-slab of 8 x 8 cells
constexpr int TGT_LO = 3, TGT_HI = 2;                       // the window reaches 3 cells down and 2 up
constexpr int TGT_SX = TGT_TX + TGT_LO + TGT_HI, TGT_SY = TGT_TY + TGT_LO + TGT_HI, TGT_SZ = TGT_TZ + TGT_LO + TGT_HI;   // 9 x 13 x 13 ints = 5.9 KiB
constexpr int TGT_CELLS = TGT_SX * TGT_SY * TGT_SZ;
constexpr int TGT_NONE = (int)0x80000000u;
constexpr int TGT_OCC = 0x40000000;
constexpr int TGT_PMASK = 0x3FFFFFFF;
constexpr int TGT_MAXN = 1024;
constexpr int TGT_MAXT = 65535;                             // targets per call (grid.y)
__host__ __device__ constexpr size_t tgt_head(int T) { return ((size_t)T * sizeof(int) + 255) & ~(size_t)255; }   // the `last` words in front of the two state buffers

// the start state, and the per-target words put back to 0 (T <= TG).  A kernel, not a memset: the call is launches only, and a memset node of a
// captured graph is one more thing a replay has to get right
__global__ void __launch_bounds__(256) plb_target_init(long TG, int T, double threshold, const double* density, int* st, int* last) {
  const long I = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (I < T) last[I] = 0;
  if (I < TG) st[I] = TGT_NONE | (density[I] > threshold ? TGT_OCC : 0);
}

__global__ void __launch_bounds__(256) plb_target_sweep(int n, int nbj, int nbk, long G, int s, double h, const int* in, int* out, int* last,
                                                        int* sweeps_run) {
  __shared__ int tile[TGT_CELLS];
  const int t = blockIdx.y, tid = threadIdx.x;
  if (s > 0 && __hip_atomic_load(last + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < s) return;   // the previous sweep changed nothing (uniform)
  int bid = blockIdx.x;
  const int bk = bid % nbk;
  bid /= nbk;
  const int bj = bid % nbj, bi = bid / nbj;
  const int i0 = bi * TGT_TX, j0 = bj * TGT_TY, k0 = bk * TGT_TZ;
  in += (long)t * G;
  out += (long)t * G;
  for (int e = tid; e < TGT_CELLS; e += 256) {   // tile + halo; cells outside the grid read as "no nearest cell", which is how the sweep skips them
    const int a = e / (TGT_SY * TGT_SZ), r = e - a * (TGT_SY * TGT_SZ), b = r / TGT_SZ, c = r - b * TGT_SZ;
    const int gi = i0 - TGT_LO + a, gj = j0 - TGT_LO + b, gk = k0 - TGT_LO + c;
    const bool ok = (unsigned)gi < (unsigned)n && (unsigned)gj < (unsigned)n && (unsigned)gk < (unsigned)n;
    tile[e] = ok ? in[((long)gi * n + gj) * n + gk] : TGT_NONE;
  }
  __syncthreads();
  const int lz = tid & 7, ly = (tid >> 3) & 7, lx = tid >> 6;
  const int i = i0 + lx, j = j0 + ly, k = k0 + lz;
  int changed = 0;
  if (i < n && j < n && k < n) {
    const int old = tile[((lx + TGT_LO) * TGT_SY + ly + TGT_LO) * TGT_SZ + lz + TGT_LO];
    int nw;
    if (old & TGT_OCC) {
      nw = TGT_OCC | (i << 20) | (j << 10) | k;
    } else {
      const double xi = (double)i * h, xj = (double)j * h, xk = (double)k * h;
      double S = 1000.0, qS = INFINITY;
      int best = TGT_NONE, seen = -1;
      for (int ox = 0; ox < TGT_SX - TGT_TX + 1; ++ox)
        for (int oy = 0; oy < TGT_SY - TGT_TY + 1; ++oy)
#pragma unroll
          for (int oz = 0; oz < TGT_SZ - TGT_TZ + 1; ++oz) {
            if (ox == TGT_LO && oy == TGT_LO && oz == TGT_LO) continue;
            const int v = tile[((lx + ox) * TGT_SY + ly + oy) * TGT_SZ + lz + oz];
            if (v < 0) continue;
            const int p = v & TGT_PMASK;
            if (p == seen) continue;
            seen = p;
            const double dx = xi - (double)(p >> 20) * h, dy = xj - (double)((p >> 10) & 1023) * h, dz = xk - (double)(p & 1023) * h;
            const double q = dx * dx + dy * dy + dz * dz + 1e-8;
            if (q < qS) {
              const double d = sqrt(q);
              if (d < S) { S = d; qS = q; best = p; }
            }
          }
      nw = best;
    }
    changed = nw != old;
    out[((long)i * n + j) * n + k] = nw;
  }
  const int any = __syncthreads_or(changed);
  if (tid == 0) {
    if (any) atomicMax(last + t, s + 1);
    if (blockIdx.x == 0 && sweeps_run) sweeps_run[t] = s + 1;   // launches of one stream run in order: the last one that ran leaves its number
  }
}

__global__ void __launch_bounds__(256) plb_target_finish(int n, long G, long TG, double h, const int* st, double* sdf, int* nearest) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= TG) return;
  const int v = st[idx];
  double S = 1000.0;
  int near = -1;
  if (v >= 0) {
    const int p = v & TGT_PMASK;
    const int pi = p >> 20, pj = (p >> 10) & 1023, pk = p & 1023;
    near = (pi * n + pj) * n + pk;
    if (v & TGT_OCC) {
      S = 0.0;
    } else {
      const long I = idx % G;
      const int k = (int)(I % n), j = (int)((I / n) % n), i = (int)(I / ((long)n * n));
      const double dx = (double)i * h - (double)pi * h, dy = (double)j * h - (double)pj * h, dz = (double)k * h - (double)pk * h;
      S = sqrt(dx * dx + dy * dy + dz * dz + 1e-8);
    }
  }
  sdf[idx] = S;
  if (nearest) nearest[idx] = near;
}

// ---- soft IoU (iou_kernel): two stages, every sum in a fixed order --------------------------------------------------------------
constexpr int IOU_NB = 64;   // partial sums per target

struct IouAcc { double ma, mb, sab, sa, sb; };

__device__ __forceinline__ void iou_merge(IouAcc& x, const IouAcc& y) {
  x.ma = fmax(x.ma, y.ma); x.mb = fmax(x.mb, y.mb);
  x.sab += y.sab; x.sa += y.sa; x.sb += y.sb;
}

template <int NT>
__device__ __forceinline__ void iou_block_reduce(IouAcc& acc, IouAcc* sh) {   // binary tree over the NT threads: the same order on every run
  sh[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) iou_merge(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  acc = sh[0];
}

__global__ void __launch_bounds__(256) plb_iou_partial(long G, const double* a, const double* b, int b_batched, IouAcc* part) {
  __shared__ IouAcc sh[256];
  const int t = blockIdx.y;
  a += (long)t * G;
  if (b_batched) b += (long)t * G;
  IouAcc acc{0.0, 0.0, 0.0, 0.0, 0.0};   // the reference starts both maxima at 0
  for (long I = (long)blockIdx.x * 256 + threadIdx.x; I < G; I += (long)IOU_NB * 256) {
    const double va = a[I], vb = b[I];
    acc.ma = fmax(acc.ma, va); acc.mb = fmax(acc.mb, vb);
    acc.sab += va * vb; acc.sa += va; acc.sb += vb;
  }
  iou_block_reduce<256>(acc, sh);
  if (threadIdx.x == 0) part[(long)t * IOU_NB + blockIdx.x] = acc;
}

__global__ void __launch_bounds__(IOU_NB) plb_iou_finish(const IouAcc* part, double* iou) {
  __shared__ IouAcc sh[IOU_NB];
  const int t = blockIdx.x;
  IouAcc acc = part[(long)t * IOU_NB + threadIdx.x];
  iou_block_reduce<IOU_NB>(acc, sh);
  if (threadIdx.x == 0) {
    const double I = acc.sab / acc.ma / acc.mb;
    const double U = acc.sa / acc.ma + acc.sb / acc.mb;
    iou[t] = I / (U - I);
  }
}

}  // namespace ud

using namespace ud;

extern "C" {

size_t ud_plb_target_work_bytes(int n_grid, int T) {
  if (n_grid < 1 || n_grid > TGT_MAXN || T < 1 || T > TGT_MAXT) return 0;
  return tgt_head(T) + 2 * (size_t)T * n_grid * n_grid * n_grid * sizeof(int);
}

int ud_plb_target_sdf(int n_grid, int T, const double* density, double threshold, int sweeps, double* sdf, int* nearest, int* sweeps_run,
                      void* work, void* stream) {
  if (n_grid < 1 || T < 1 || sweeps < 0 || !density || !sdf || !work) {
    set_error("ud_plb_target_sdf: bad argument (n_grid=%d, T=%d, sweeps=%d, density, sdf and work must not be null)", n_grid, T, sweeps);
    return UD_ERR_INVALID;
  }
  if (n_grid > TGT_MAXN) { set_error("ud_plb_target_sdf: n_grid=%d above %d (a cell index is packed into 3 x 10 bits)", n_grid, TGT_MAXN); return UD_ERR_UNSUPPORTED; }
  if (T > TGT_MAXT) { set_error("ud_plb_target_sdf: T=%d above %d targets per call", T, TGT_MAXT); return UD_ERR_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  const int n = n_grid;
  const long G = (long)n * n * n, TG = (long)T * G;
  if (sweeps == 0) sweeps = 2 * n;
  int* last = (int*)work;
  int* buf[2] = {(int*)((char*)work + tgt_head(T)), (int*)((char*)work + tgt_head(T)) + TG};
  const double h = 1.0 / (double)n;
  const int nbi = (n + TGT_TX - 1) / TGT_TX, nbj = (n + TGT_TY - 1) / TGT_TY, nbk = (n + TGT_TZ - 1) / TGT_TZ;
  const unsigned flat = (unsigned)((TG + 255) / 256);
  hipLaunchKernelGGL(plb_target_init, dim3(flat), dim3(256), 0, st, TG, T, threshold, density, buf[0], last);
  for (int s = 0; s < sweeps; ++s)
    hipLaunchKernelGGL(plb_target_sweep, dim3((unsigned)nbi * nbj * nbk, T), dim3(256), 0, st, n, nbj, nbk, G, s, h, (const int*)buf[s & 1], buf[(s + 1) & 1],
                       last, sweeps_run);
  hipLaunchKernelGGL(plb_target_finish, dim3(flat), dim3(256), 0, st, n, G, TG, h, (const int*)buf[sweeps & 1], sdf, nearest);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

size_t ud_plb_density_iou_work_bytes(int T) { return T < 1 ? 0 : (size_t)T * IOU_NB * sizeof(IouAcc); }

int ud_plb_density_iou(long G, int T, const double* a, const double* b, int b_batched, double* iou, void* work, void* stream) {
  if (G < 1 || T < 1 || T > 65535 || !a || !b || !iou || !work) { set_error("ud_plb_density_iou: bad argument (G=%ld, T=%d; no pointer may be null)", G, T); return UD_ERR_INVALID; }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(plb_iou_partial, dim3(IOU_NB, T), dim3(256), 0, st, G, a, b, b_batched, (IouAcc*)work);
  hipLaunchKernelGGL(plb_iou_finish, dim3(T), dim3(IOU_NB), 0, st, (const IouAcc*)work, iou);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

}  // extern "C"
