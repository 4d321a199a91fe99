// pg_hip_solve_arith.h -- the two pieces of arithmetic every triangular-solve kernel shares (pg_hip_solve_ops.h, pg_hip_block_solve.h,
// pg_hip_block_solve_multi.h).  Included by pg_hip_platform.hip after the v_* operators, and by the CPU emulation of the panel kernels
// (tests/hip_emulation_shims.h supplies the operators there).
#pragma once

// the divisor a sweep uses for a diagonal entry: PANGULU_SPTRSV_TOL in place of a diagonal whose real part is within the tolerance
// of zero (real part only for complex, as the sptrsv of ...0100000.c:435-506 does; written so that a NaN clamps as well)
__host__ __device__ inline val_t solve_clamped_divisor(val_t d)
{
    const real_t dr = v_realpart(d);
    if (!((dr < 0 ? -dr : dr) > (real_t)PANGULU_SPTRSV_TOL))
        d = v_make((real_t)PANGULU_SPTRSV_TOL);
    return d;
}

// sum over the lanes l, l + W, l + 2 W, ... of an aligned group of `span` lanes (span / W a power of two): lanes 0 .. W - 1 of the
// group end up with the sums.  Every lane of the wavefront must call it.
template <int W>
__device__ inline val_t solve_group_sum(val_t part, int span)
{
    for (int off = span >> 1; off >= W; off >>= 1)
    {
#ifdef PANGULU_COMPLEX
        part.re += __shfl_down(part.re, off, 64);
        part.im += __shfl_down(part.im, off, 64);
#else
        part += __shfl_down(part, off, 64);
#endif
    }
    return part;
}
