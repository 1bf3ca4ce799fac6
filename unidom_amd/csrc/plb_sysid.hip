// PLB system identification: the density loss of a sequence of particle clouds against per-item targets (the sim2sim / real2sim loss
// `sum_f sum_I |grid_mass(x_f)_I - target[f]_I|`, PlasticineLab/sim2sim/plb/engine/losses/loss.py) with its adjoint, and the chamfer
// distance the reference reports at the end of an identification (optimizer/solver.py:187-196).  The calls read the handle's constants
// only (PlbConst) and touch none of its arenas: the number of items M is not bound by max_envs.  Launches only: nothing is allocated,
// nothing synchronises, no workgroup waits for another one.
//
// Sequence loss, forward.  An item is one cloud [N,3].  The items are taken in chunks of C = work_bytes / (8 G): every chunk scatters
// its particle masses (the p2g of plb_loss_mass: same weights, same clamping into the grid) with f64 atomics into the dense scratch
// [C][G], then ONE sweep reads each cell once, takes df = gm - target, adds |df| to the item's loss, records sign(df) and puts the
// cell back to zero -- the scratch is zero again for the next chunk (it is zeroed once, by a kernel, at the start of the call).
// The sign field: per item ceil(G / 64) pairs of 64-bit wave ballots (df > 0, df < 0) of 64 consecutive cells, i.e. three-valued, 0
// where df == 0 (and where df is NaN), as plb_loss_bwd_kernel decides it.  One lane of a wave stores the pair: no atomics on the field.
// An item whose target index is outside [0, T) scatters nothing, reads no target, gets loss = NaN and an all-zero sign field.
//
// Backward.  One gather per particle over its 27 cells: g_x = inv_dx * sum_I (g_loss * sign_I * p_mass) * grad w_I, in the order of
// plb_loss_bwd_kernel's loop.  No scatter, no atomics, no scratch: the same sign field gives the same bits.
//
// Chamfer.  out = mean_i min_j d(a_i, b_j) + mean_j min_i d(a_i, b_j), d = sqrt((dx dx + dy dy) + dz dz).  One owner lane per point, the
// other cloud tiled through LDS.  The minimum is taken over q = (dx dx + dy dy) + dz dz and the root once at the end: the f64 root is
// correctly rounded, hence monotone, so sqrt(min q) == min sqrt(q) bit for bit (contraction is off for this file: q is summed as written).
// NaN propagates as np.min does: a NaN candidate replaces the minimum and nothing replaces a NaN.  The means are fixed-order sums (each
// of 256 threads adds its points in ascending order, then a binary tree over the threads): the same input gives the same bits.
#include "plb_device.h"

namespace ud {

constexpr size_t SEQ_WORK_CAP = (size_t)256 << 20;   // ud_plb_density_seq_work_bytes never asks for more (but always for one item)
constexpr long SEQ_MAX_CHUNK = 65535;                // items per chunk: the sweep's grid.y
constexpr int SEQ_SWEEP_NB = 128;                    // sweep blocks per item (each loops over its share of the cells)

__host__ __device__ constexpr long seq_words(long G) { return (G + 63) >> 6; }   // ballot pairs per item

// 256 threads, binary tree in a fixed order; the result in thread 0
__device__ __forceinline__ double sysid_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

// the scratch and the losses to zero.  A kernel, not a memset (plb_target.hip: a memset node is one more thing a graph replay has to get right)
__global__ void __launch_bounds__(256) plb_seq_zero(long n, double* scratch, long M, double* loss) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) scratch[i] = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) loss[i] = 0.0;
}

// p2g of the masses of the items m0 .. m0 + cm - 1 into scratch [cm][G]: plb_loss_mass, flat over (item, particle)
__global__ void __launch_bounds__(256) plb_seq_scatter(PlbConst c, long G, long m0, long cm, int T, const int* tidx, const double* x, double* gm) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= cm * c.N) return;
  const long item = idx / c.N, m = m0 + item;
  const int p = (int)(idx - item * c.N);
  const int t = tidx ? tidx[m] : 0;
  if ((unsigned)t >= (unsigned)T) return;
  const double* xm = x + (m * c.N + p) * 3;
  const double xp[3] = {xm[0], xm[1], xm[2]};
  int base[3];
  double fx[3], w[9], dw[9];
  plb_weights(c, xp, base, fx, w, dw);
  double* g = gm + item * G;
#pragma unroll 1
  for (int cidx = 0; cidx < 27; ++cidx) {
    const int i = cidx / 9, j = (cidx / 3) % 3, k = cidx % 3;
    const int ci = min(max(base[0] + i, 0), c.n_grid - 1), cj = min(max(base[1] + j, 0), c.n_grid - 1), ck = min(max(base[2] + k, 0), c.n_grid - 1);
    atomicAdd(g + plb_lin(c, ci, cj, ck), dsel3(w, 0, i) * dsel3(w, 1, j) * dsel3(w, 2, k) * c.p_mass);
  }
}

// one pass over the chunk's cells: loss, sign field, scratch back to zero.  grid (SEQ_SWEEP_NB, cm); a wave always holds 64 consecutive
// cells starting at a multiple of 64, and every lane reaches both ballots
__global__ void __launch_bounds__(256) plb_seq_sweep(long G, long m0, int T, const int* tidx, const double* targets, double* gm, double* loss,
                                                     unsigned long long* sign) {
  __shared__ double sh[256];
  const long item = blockIdx.y, m = m0 + item;
  const int t = tidx ? tidx[m] : 0;
  const bool valid = (unsigned)t < (unsigned)T;
  double* g = gm + item * G;
  const double* td = targets + (long)(valid ? t : 0) * G;
  ulonglong2* sp = sign ? (ulonglong2*)sign + m * seq_words(G) : nullptr;
  double acc = 0.0;
  for (long b0 = (long)blockIdx.x * 256; b0 < G; b0 += (long)gridDim.x * 256) {
    const long I = b0 + threadIdx.x;
    double df = 0.0;
    if (I < G) {
      const double mI = g[I];
      g[I] = 0.0;
      if (valid) df = mI - td[I];
    }
    acc += fabs(df);
    const unsigned long long pos = __ballot(df > 0), neg = __ballot(df < 0);
    if (sp && (threadIdx.x & 63) == 0 && I < G) sp[I >> 6] = make_ulonglong2(pos, neg);
  }
  acc = sysid_block_sum(acc, sh);
  if (threadIdx.x == 0) {
    if (valid) atomicAdd(loss + m, acc);
    else if (blockIdx.x == 0) loss[m] = __builtin_nan("");
  }
}

__global__ void __launch_bounds__(256) plb_seq_bwd_kernel(PlbConst c, long G, long M, const double* x, const unsigned long long* sign, const double* g_loss,
                                                         double* g_x) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * c.N) return;
  const long m = idx / c.N;
  const double gl = g_loss[m];
  const double* xm = x + idx * 3;
  const double xp[3] = {xm[0], xm[1], xm[2]};
  const ulonglong2* sp = (const ulonglong2*)sign + m * seq_words(G);
  int base[3];
  double fx[3], w[9], dw[9];
  plb_weights(c, xp, base, fx, w, dw);
  double gfx[3] = {0, 0, 0};
#pragma unroll 1
  for (int cidx = 0; cidx < 27; ++cidx) {
    const int i = cidx / 9, j = (cidx / 3) % 3, k = cidx % 3;
    const int ci = min(max(base[0] + i, 0), c.n_grid - 1), cj = min(max(base[1] + j, 0), c.n_grid - 1), ck = min(max(base[2] + k, 0), c.n_grid - 1);
    const long I = plb_lin(c, ci, cj, ck);
    const ulonglong2 s = sp[I >> 6];
    const int bit = (int)(I & 63);
    const double sg = (double)((int)((s.x >> bit) & 1) - (int)((s.y >> bit) & 1));
    const double gmI = gl * sg * c.p_mass;
    const double wi = dsel3(w, 0, i), wj = dsel3(w, 1, j), wk = dsel3(w, 2, k);
    gfx[0] += gmI * dsel3(dw, 0, i) * wj * wk;
    gfx[1] += gmI * wi * dsel3(dw, 1, j) * wk;
    gfx[2] += gmI * wi * wj * dsel3(dw, 2, k);
  }
  double* o = g_x + idx * 3;
  o[0] = c.inv_dx * gfx[0]; o[1] = c.inv_dx * gfx[1]; o[2] = c.inv_dx * gfx[2];
}

// ---- chamfer ----------------------------------------------------------------------------------------------------------------------
// min_j |p - o_j| for this lane's point p (own = false: the lane only helps loading the tiles), the cloud o [n,3] tiled through LDS
__device__ __forceinline__ double chamfer_min(bool own, const double* p, const double* o, int n, double (*tile)[3]) {
  double q = INFINITY;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int cnt = min(256, n - j0);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      const double* s = o + (long)(j0 + threadIdx.x) * 3;
      tile[threadIdx.x][0] = s[0]; tile[threadIdx.x][1] = s[1]; tile[threadIdx.x][2] = s[2];
    }
    __syncthreads();
    if (own)
      for (int j = 0; j < cnt; ++j) {
        const double dx = p[0] - tile[j][0], dy = p[1] - tile[j][1], dz = p[2] - tile[j][2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        q = (d < q || d != d) ? d : q;   // np.min: a NaN takes the minimum and keeps it
      }
  }
  return sqrt(q);
}

// mean of v [n] in a fixed order: thread t adds v[t], v[t + 256], ..., then the tree
__device__ __forceinline__ double chamfer_mean(const double* v, int n, double* sh) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += v[i];
  return sysid_block_sum(s, sh) / (double)n;
}

// both min arrays are the caller's: grid (ceil(Na / 256) + ceil(Nb / 256), M), every block owns 256 points of one direction
__global__ void __launch_bounds__(256) plb_chamfer_min_kernel(int Na, int Nb, int Tb, int nba, const double* a, const double* b, const int* bidx,
                                                             double* min_ab, double* min_ba) {
  __shared__ double tile[256][3];
  const long m = blockIdx.y;
  const int t = bidx ? bidx[m] : 0;
  const bool ab = (int)blockIdx.x < nba;
  const int blk = ab ? blockIdx.x : blockIdx.x - nba;
  const int n_own = ab ? Na : Nb, n_oth = ab ? Nb : Na;
  const int i = blk * 256 + threadIdx.x;
  double* out = (ab ? min_ab + m * Na : min_ba + m * Nb);
  if ((unsigned)t >= (unsigned)Tb) {   // uniform over the block
    if (i < n_own) out[i] = __builtin_nan("");
    return;
  }
  const double* am = a + m * Na * 3;
  const double* bt = b + (long)t * Nb * 3;
  const double* own = ab ? am : bt;
  const double* oth = ab ? bt : am;
  const bool mine = i < n_own;
  double p[3] = {0, 0, 0};
  if (mine) { p[0] = own[(long)i * 3]; p[1] = own[(long)i * 3 + 1]; p[2] = own[(long)i * 3 + 2]; }
  const double d = chamfer_min(mine, p, oth, n_oth, tile);
  if (mine) out[i] = d;
}

__global__ void __launch_bounds__(256) plb_chamfer_mean_kernel(int Na, int Nb, const double* min_ab, const double* min_ba, double* out) {
  __shared__ double sh[256];
  const long m = blockIdx.x;
  const double sa = chamfer_mean(min_ab + m * Na, Na, sh);
  __syncthreads();
  const double sb = chamfer_mean(min_ba + m * Nb, Nb, sh);
  if (threadIdx.x == 0) out[m] = sa + sb;
}

// a min array is missing: one block per item does both directions, each thread owning the points t, t + 256, ... -- the sums are the
// ones of plb_chamfer_mean_kernel, term for term
__global__ void __launch_bounds__(256) plb_chamfer_one_kernel(int Na, int Nb, int Tb, const double* a, const double* b, const int* bidx, double* out,
                                                             double* min_ab, double* min_ba) {
  __shared__ double tile[256][3];
  __shared__ double sh[256];
  const long m = blockIdx.x;
  const int t = bidx ? bidx[m] : 0;
  const bool valid = (unsigned)t < (unsigned)Tb;
  const double* am = a + m * Na * 3;
  const double* bt = b + (long)(valid ? t : 0) * Nb * 3;
  double mean[2];
  for (int dir = 0; dir < 2; ++dir) {
    const double* own = dir ? bt : am;
    const double* oth = dir ? am : bt;
    const int n_own = dir ? Nb : Na, n_oth = dir ? Na : Nb;
    double* mo = dir ? (min_ba ? min_ba + m * Nb : nullptr) : (min_ab ? min_ab + m * Na : nullptr);
    double s = 0.0;
    for (int i0 = 0; i0 < n_own; i0 += 256) {   // uniform trip count: every thread takes part in the tile loads
      const int i = i0 + threadIdx.x;
      const bool mine = i < n_own;
      double p[3] = {0, 0, 0}, d = __builtin_nan("");
      if (valid) {
        if (mine) { p[0] = own[(long)i * 3]; p[1] = own[(long)i * 3 + 1]; p[2] = own[(long)i * 3 + 2]; }
        d = chamfer_min(mine, p, oth, n_oth, tile);
      }
      if (mine) { s += d; if (mo) mo[i] = d; }
    }
    __syncthreads();
    mean[dir] = sysid_block_sum(s, sh) / (double)n_own;
    __syncthreads();
  }
  if (threadIdx.x == 0) out[m] = mean[0] + mean[1];
}

}  // namespace ud

using namespace ud;

static long seq_chunk_cap(long G) {
  const long c = (long)(SEQ_WORK_CAP / ((size_t)G * 8));
  return c < 1 ? 1 : (c > SEQ_MAX_CHUNK ? SEQ_MAX_CHUNK : c);
}

extern "C" {

size_t ud_plb_density_seq_work_bytes(const ud_plb* h, long M) {
  if (!h || M < 1) return 0;
  const long cap = seq_chunk_cap(h->G);
  return (size_t)8 * h->G * (M < cap ? M : cap);
}

size_t ud_plb_density_seq_sign_bytes(const ud_plb* h, long M) {
  if (!h || M < 1) return 0;
  return (size_t)M * seq_words(h->G) * 16;
}

int ud_plb_density_seq_fwd(ud_plb* h, long M, const double* x, const double* targets, int T, const int* target_index, double* loss, void* sign,
                           void* work, size_t work_bytes, void* stream) {
  if (!h || M < 1 || T < 1 || !x || !targets || !loss || !work) {
    set_error("ud_plb_density_seq_fwd: bad argument (M=%ld, T=%d; handle, x, targets, loss and work must not be null)", M, T);
    return UD_ERR_INVALID;
  }
  const long G = h->G;
  long chunk = (long)(work_bytes / ((size_t)G * 8));
  if (chunk < 1) {
    set_error("ud_plb_density_seq_fwd: work_bytes=%zu holds less than one item (%zu bytes)", work_bytes, (size_t)G * 8);
    return UD_ERR_INVALID;
  }
  if (chunk > M) chunk = M;
  if (chunk > SEQ_MAX_CHUNK) chunk = SEQ_MAX_CHUNK;
  if (chunk * h->c.N > (long)0x7fffffff * 256) { set_error("ud_plb_density_seq_fwd: %ld particles per chunk", chunk * h->c.N); return UD_ERR_UNSUPPORTED; }
  hipStream_t st = (hipStream_t)stream;
  double* gm = (double*)work;
  const long nz = chunk * G;
  const long zb = (nz + 255) / 256;
  hipLaunchKernelGGL(plb_seq_zero, dim3((unsigned)(zb < 65536 ? zb : 65536)), dim3(256), 0, st, nz, gm, M, loss);
  const long nbs = (G + 255) / 256;
  const unsigned sweep_nb = (unsigned)(nbs < SEQ_SWEEP_NB ? nbs : SEQ_SWEEP_NB);
  for (long m0 = 0; m0 < M; m0 += chunk) {
    const long cm = (M - m0 < chunk) ? M - m0 : chunk;
    hipLaunchKernelGGL(plb_seq_scatter, dim3((unsigned)((cm * h->c.N + 255) / 256)), dim3(256), 0, st, h->c, G, m0, cm, T, target_index, x, gm);
    hipLaunchKernelGGL(plb_seq_sweep, dim3(sweep_nb, (unsigned)cm), dim3(256), 0, st, G, m0, T, target_index, targets, gm, loss,
                       (unsigned long long*)sign);
  }
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

int ud_plb_density_seq_bwd(ud_plb* h, long M, const double* x, const void* sign, const double* g_loss, double* g_x, void* stream) {
  if (!h || M < 1 || !x || !sign || !g_loss || !g_x) {
    set_error("ud_plb_density_seq_bwd: bad argument (M=%ld; no pointer may be null)", M);
    return UD_ERR_INVALID;
  }
  const long nb = (M * h->c.N + 255) / 256;
  if (nb > 0x7fffffff) { set_error("ud_plb_density_seq_bwd: M=%ld items of %d particles", M, h->c.N); return UD_ERR_UNSUPPORTED; }
  hipLaunchKernelGGL(plb_seq_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, h->c, h->G, M, x, (const unsigned long long*)sign, g_loss, g_x);
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

int ud_plb_chamfer(long M, int Na, const double* a, int Tb, int Nb, const double* b, const int* b_index, double* out, double* min_ab, double* min_ba,
                   void* stream) {
  if (M < 1 || Na < 1 || Nb < 1 || Tb < 1 || !a || !b || !out) {
    set_error("ud_plb_chamfer: bad argument (M=%ld, Na=%d, Tb=%d, Nb=%d; a, b and out must not be null)", M, Na, Tb, Nb);
    return UD_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  if (min_ab && min_ba && M <= 65535) {
    const int nba = (Na + 255) / 256, nbb = (Nb + 255) / 256;
    hipLaunchKernelGGL(plb_chamfer_min_kernel, dim3((unsigned)(nba + nbb), (unsigned)M), dim3(256), 0, st, Na, Nb, Tb, nba, a, b, b_index, min_ab, min_ba);
    hipLaunchKernelGGL(plb_chamfer_mean_kernel, dim3((unsigned)M), dim3(256), 0, st, Na, Nb, (const double*)min_ab, (const double*)min_ba, out);
  } else {
    if (M > 0x7fffffff) { set_error("ud_plb_chamfer: M=%ld", M); return UD_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(plb_chamfer_one_kernel, dim3((unsigned)M), dim3(256), 0, st, Na, Nb, Tb, a, b, b_index, out, min_ab, min_ba);
  }
  UD_HIP_CHECK(hipGetLastError());
  return UD_OK;
}

}  // extern "C"
