// Test infrastructure.  Force-included in front of CUDA C that uses nothing of CUDA beyond the kernel language, so that a host
// compiler accepts it: the qualifiers vanish, block-shared arrays become statics (blocks run one after the other), the index
// variables are globals that driver.cpp sets, an atomic add is an add (one thread runs at a time) and a barrier is a call into
// the driver.  Our own text; the files it is put in front of are copied at build time and never committed.
#pragma once
#include <algorithm>
#include <cmath>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
extern dim3 threadIdx, blockIdx, blockDim, gridDim;
extern "C" void ref_pc_barrier();
using std::min; using std::max;
template <class T> inline T atomicAdd(T* p, T v) { T old = *p; *p = old + v; return old; }
#define __global__
#define __restrict__
#define __shared__ static
#define __syncthreads() ref_pc_barrier()
