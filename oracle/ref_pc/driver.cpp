// Test infrastructure: runs kernels written in CUDA C on the CPU, one block after the other.  The threads of a block are ucontext
// coroutines, resumed round-robin, each until its next barrier (or its end): deterministic, no OS threads.  Compiled together with
// build-time copies of the reference's point-cloud sampling / grouping kernels (oracle/Makefile, target ref_pc); the entry points
// below take the argument lists of the reference's launchers and use its launch shapes.
//
// SCHEDULE: within a round the threads are resumed in DESCENDING order, thread 0 last.  The reference's farthest-point kernel
// has every thread read slot 0 of its reduction array after the last barrier of a sample, and thread 0 overwrites that slot at
// the start of the next sample before any further barrier.  Resumed in ascending order, threads 1.. would read thread 0's new
// value and the kernel returns garbage; with thread 0 last every thread reads the reduction's result, which is what the
// hardware gives in practice and the only schedule under which the kernel samples farthest points.
//
// A block whose threads do not all pass the same number of barriers, and a coroutine that overruns its stack, end the process
// with a message: neither may return numbers.
#include <signal.h>
#include <sys/mman.h>
#include <ucontext.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "cuda_shim.h"

dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace {
// per coroutine: one inaccessible guard page, then STACK bytes that grow down towards it; an overrun faults on the guard
constexpr size_t STACK = 64 * 1024, GUARD = 4096;
ucontext_t g_main;
std::vector<ucontext_t> g_ctx;
std::vector<char> g_done;
unsigned char* g_stacks;
size_t g_stacks_bytes;
const std::function<void()>* g_body;
unsigned g_cur;
alignas(16) unsigned char g_sigstack[64 * 1024];

[[noreturn]] void die(const char* what) {
    std::fprintf(stderr, "ref_pc driver: %s (block %u,%u thread %u)\n", what, blockIdx.x, blockIdx.y, g_cur);
    std::fflush(stderr);
    std::_Exit(3);
}

void on_segv(int, siginfo_t* si, void*) {                   // runs on g_sigstack: the faulting coroutine has no stack left
    const uintptr_t a = uintptr_t(si->si_addr), lo = uintptr_t(g_stacks);
    if (a >= lo && a < lo + g_stacks_bytes && (a - lo) % (STACK + GUARD) < GUARD) {
        static const char msg[] = "ref_pc driver: coroutine stack too small\n";
        (void)!write(2, msg, sizeof msg - 1);
        _exit(3);
    }
    signal(SIGSEGV, SIG_DFL);                                // not ours: fault again, with the default action
}

void trampoline() {
    (*g_body)();
    g_done[g_cur] = 1;                                       // uc_link returns to the driver
}

void launch(dim3 grid, dim3 block, const std::function<void()>& body) {
    const unsigned T = block.x;
    gridDim = grid, blockDim = block, g_body = &body;
    g_ctx.resize(T), g_done.resize(T);
    if (g_stacks_bytes < T * (STACK + GUARD)) {
        if (g_stacks) munmap(g_stacks, g_stacks_bytes);
        g_stacks_bytes = T * (STACK + GUARD);
        void* p = mmap(nullptr, g_stacks_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) die("cannot map the coroutine stacks");
        g_stacks = static_cast<unsigned char*>(p);
        for (unsigned t = 0; t < T; t++)
            if (mprotect(g_stacks + t * (STACK + GUARD), GUARD, PROT_NONE)) die("cannot protect a guard page");
    }
    stack_t ss{}, old_ss{};
    ss.ss_sp = g_sigstack, ss.ss_size = sizeof g_sigstack;
    struct sigaction sa{}, old_sa{};
    sa.sa_sigaction = on_segv, sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
    sigemptyset(&sa.sa_mask);
    sigaltstack(&ss, &old_ss), sigaction(SIGSEGV, &sa, &old_sa);
    for (unsigned by = 0; by < grid.y; by++)
        for (unsigned bx = 0; bx < grid.x; bx++) {
            blockIdx = dim3(bx, by, 0);
            for (unsigned t = 0; t < T; t++) {
                getcontext(&g_ctx[t]);
                g_ctx[t].uc_stack.ss_sp = g_stacks + t * (STACK + GUARD) + GUARD;
                g_ctx[t].uc_stack.ss_size = STACK, g_ctx[t].uc_link = &g_main;
                makecontext(&g_ctx[t], trampoline, 0);
                g_done[t] = 0;
            }
            for (;;) {                                       // one round = every thread up to its next barrier
                unsigned ended = 0;
                for (unsigned t = T; t-- > 0;) {             // descending: see SCHEDULE above
                    g_cur = t, threadIdx = dim3(t, 0, 0);
                    swapcontext(&g_main, &g_ctx[t]);
                    ended += g_done[t];
                }
                if (ended == T) break;
                if (ended) die("threads of one block passed different numbers of barriers");
            }
        }
    sigaction(SIGSEGV, &old_sa, nullptr), sigaltstack(&old_ss, nullptr);
}
}  // namespace

extern "C" void ref_pc_barrier() { swapcontext(&g_ctx[g_cur], &g_main); }

// the kernels of the two copied files (C++ linkage, as compiled)
void farthestpointsamplingKernel(int, int, int, const float*, float*, int*);
void gatherpointKernel(int, int, int, const float*, const int*, float*);
void scatteraddpointKernel(int, int, int, const float*, const int*, float*);
void query_ball_point_gpu(int, int, int, float, int, const float*, const float*, int*, int*);
void group_point_gpu(int, int, int, int, int, const float*, const int*, float*);
void group_point_grad_gpu(int, int, int, int, int, const float*, const int*, float*);

extern "C" {
// temp: 32 * n floats of scratch, as the reference's launcher requires
void ref_pc_fps(int b, int n, int m, const float* inp, float* temp, int* out) {
    launch(dim3(32), dim3(512), [=] { farthestpointsamplingKernel(b, n, m, inp, temp, out); });
}
void ref_pc_gather(int b, int n, int m, const float* inp, const int* idx, float* out) {
    launch(dim3(2, 8, 1), dim3(512), [=] { gatherpointKernel(b, n, m, inp, idx, out); });
}
void ref_pc_scatter_add(int b, int n, int m, const float* out_g, const int* idx, float* inp_g) {
    launch(dim3(2, 8, 1), dim3(512), [=] { scatteraddpointKernel(b, n, m, out_g, idx, inp_g); });
}
void ref_pc_ball_query(int b, int n, int m, float radius, int nsample, const float* xyz1, const float* xyz2, int* idx, int* pts_cnt) {
    launch(dim3(b), dim3(256), [=] { query_ball_point_gpu(b, n, m, radius, nsample, xyz1, xyz2, idx, pts_cnt); });
}
void ref_pc_group(int b, int n, int c, int m, int nsample, const float* points, const int* idx, float* out) {
    launch(dim3(b), dim3(256), [=] { group_point_gpu(b, n, c, m, nsample, points, idx, out); });
}
void ref_pc_group_grad(int b, int n, int c, int m, int nsample, const float* grad_out, const int* idx, float* grad_points) {
    launch(dim3(b), dim3(256), [=] { group_point_grad_gpu(b, n, c, m, nsample, grad_out, idx, grad_points); });
}
}
