// What the kernel emulation programs (tests/solve_multi_kernel_emulation.cpp, tests/solve_trans_kernel_emulation.cpp) put in place of
// the device: the kernel headers of pangulu_amd/csrc/platform are compiled as plain C++ behind these shims -- a workgroup is 256
// std::threads, __syncthreads / wave_lds_fence / __shfl_down are barriers over the workgroup / the wavefront, atomics are
// compare-and-swap loops, the LDS is one array.  The v_* operators and ptr0 restate pg_hip_platform.hip (the
// descriptors SolveBlkD / SolveRowD are the product's own, pg_hip_block_solve_multi.h); an intrinsic or operator a kernel starts to use is added HERE, once.  Include it before the kernel headers.
#pragma once
#include <algorithm>
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>
typedef unsigned int u32; typedef unsigned short u16; typedef unsigned long long u64;
#ifdef PANGULU_COMPLEX
struct val_t { double re, im; };
#else
typedef double val_t;
#endif
typedef double real_t;
#define PANGULU_SPTRSV_TOL 1e-16
#define __global__
#define __device__
#define __host__
#define __shared__
#define __align__(x)
#define __launch_bounds__(x)
#define __restrict__
struct dim3e { unsigned x; };
thread_local dim3e threadIdx, blockIdx;
alignas(16) unsigned char smem_raw[160 << 10];
std::barrier<> *g_block_bar; std::barrier<> *g_wave_bar[4];
double g_shfl[4][64];
inline void __syncthreads() { g_block_bar->arrive_and_wait(); }
inline void wave_lds_fence() { g_wave_bar[threadIdx.x >> 6]->arrive_and_wait(); }
inline double __shfl_down(double v, int off, int) {
    int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_shfl[w][l] = v; g_wave_bar[w]->arrive_and_wait();
    double r = l + off < 64 ? g_shfl[w][l + off] : v; g_wave_bar[w]->arrive_and_wait(); return r; }
inline void atomicAdd(double *p, double v) { std::atomic_ref<double> a(*p); double o = a.load(); while (!a.compare_exchange_weak(o, o + v)) {} }
using std::max; using std::min;
#ifdef PANGULU_COMPLEX
inline val_t v_make(real_t r) { return val_t{r, 0}; }
inline val_t v_mul(val_t a, val_t b) { return val_t{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline val_t v_add(val_t a, val_t b) { return val_t{a.re + b.re, a.im + b.im}; }
inline val_t v_sub(val_t a, val_t b) { return val_t{a.re - b.re, a.im - b.im}; }
inline val_t v_submul(val_t a, val_t b, val_t c) { return val_t{a.re - (b.re * c.re - b.im * c.im), a.im - (b.re * c.im + b.im * c.re)}; }
inline val_t v_div(val_t a, val_t b) { real_t d = b.re * b.re + b.im * b.im; return val_t{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d}; }
inline real_t v_realpart(val_t a) { return a.re; }
inline val_t v_conj(val_t a) { return val_t{a.re, -a.im}; }
inline void lds_atomic_sub(val_t *d, val_t v) { atomicAdd(&d->re, -v.re); atomicAdd(&d->im, -v.im); }
inline void v_atomic_add(val_t *d, val_t v) { if (v.re != 0) atomicAdd(&d->re, v.re); if (v.im != 0) atomicAdd(&d->im, v.im); }
inline double vabs(val_t a) { return std::hypot(a.re, a.im); }
#else
inline val_t v_make(real_t r) { return r; }
inline val_t v_mul(val_t a, val_t b) { return a * b; }
inline val_t v_add(val_t a, val_t b) { return a + b; }
inline val_t v_sub(val_t a, val_t b) { return a - b; }
inline val_t v_submul(val_t a, val_t b, val_t c) { return a - b * c; }
inline val_t v_div(val_t a, val_t b) { return a / b; }
inline real_t v_realpart(val_t a) { return a; }
inline val_t v_conj(val_t a) { return a; }
inline void lds_atomic_sub(val_t *d, val_t v) { atomicAdd(d, -v); }
inline void v_atomic_add(val_t *d, val_t v) { if (v != 0) atomicAdd(d, v); }
inline double vabs(val_t a) { return std::fabs(a); }
#endif
inline u32 ptr0(const u32 *p, int i) { return i == 0 ? 0u : p[i]; }

// one launch: the workgroups one after the other, f() on each of the 256 threads of a workgroup
template <class F> void launch(unsigned grid, F f) {
    for (unsigned b = 0; b < grid; b++) {
        std::barrier<> bb(256), w0(64), w1(64), w2(64), w3(64);
        g_block_bar = &bb; g_wave_bar[0] = &w0; g_wave_bar[1] = &w1; g_wave_bar[2] = &w2; g_wave_bar[3] = &w3;
        std::vector<std::thread> th;
        for (unsigned t = 0; t < 256; t++) th.emplace_back([=] { threadIdx.x = t; blockIdx.x = b; f(); });
        for (auto &t : th) t.join();
    }
}
