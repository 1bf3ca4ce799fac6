// TEST INFRASTRUCTURE (tests/devfn/libdevfn.so, never part of libunidom_hip.so): the shape layer of unidom_amd/csrc/plb_prim.h -- plb_shape_sdf,
// plb_shape_normal and plb_shape_adj, one local point per lane -- compiled with the flags of plb.o / plb_adj.o (the Makefile's default rule,
// -ffp-contract=off).
#include "../../unidom_amd/csrc/plb_prim.h"

namespace {

// kind: 1 Capsule, 3 Box, 4 Cylinder, 5 Torus; sc[3] the kind's constants, ch / radius the Capsule's.  pl, gnl [n][3], gdist [n] in;
// dist [n], nl [n][3], g [n][3] (the cotangent of pl) out.  Lanes past n leave at once.
__global__ void plb_shape_kernel(int kind, double sc0, double sc1, double sc2, double ch, double radius, const double* __restrict__ pl,
                                 const double* __restrict__ gdist, const double* __restrict__ gnl, double* __restrict__ dist, double* __restrict__ nl,
                                 double* __restrict__ g, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double sc[3] = {sc0, sc1, sc2};
  const double p[3] = {pl[i * 3], pl[i * 3 + 1], pl[i * 3 + 2]}, gn[3] = {gnl[i * 3], gnl[i * 3 + 1], gnl[i * 3 + 2]};
  double o[3], go[3];
  dist[i] = ud::plb_shape_sdf(kind, sc, ch, radius, p);
  ud::plb_shape_normal(kind, sc, ch, p, o);
  ud::plb_shape_adj(kind, sc, ch, p, gdist[i], gn, go);
#pragma unroll
  for (int k = 0; k < 3; ++k) { nl[i * 3 + k] = o[k]; g[i * 3 + k] = go[k]; }
}

}  // namespace

extern "C" {

// device pointers and a count, launched on the null stream, the hipError_t returned
int devfn_plb_shape(int kind, const double* consts5, const double* pl, const double* gdist, const double* gnl, double* dist, double* nl, double* g, long n) {
  if (n <= 0 || !(kind == 1 || (kind >= 3 && kind <= 5))) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(plb_shape_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, kind, consts5[0], consts5[1], consts5[2], consts5[3], consts5[4], pl,
                     gdist, gnl, dist, nl, g, n);
  return (int)hipGetLastError();
}

}  // extern "C"
