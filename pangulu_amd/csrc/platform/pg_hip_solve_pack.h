// pg_hip_solve_pack.h -- the way in and out of factor space for right-hand sides that live on the device
// (pangulu_platform_0201001_block_trsm_multi_device): the user's column-major matrix <-> one panel of the solve kernels of
// pg_hip_block_solve_multi.h, X[i * W + r] with the right-hand side fastest.  A column goes in as a gather and comes out as a scatter
// through the handle's index/scale maps (pg_host.h, SolveMaps):
//     in:   X[i * W + r] = s_in[i] * rhs[(j0 + r) * ldb + in_idx[i]]     a padding row (in_idx[i] == SOLVE_MAP_PAD) gives 0
//     out:  rhs[(j0 + r) * ldb + out_idx[i]] = s_out[i] * X[i * W + r]   a padding row is skipped
// s_in / s_out are real and may be absent (a handle without scaling: plain copies).  Included inside the anonymous namespace of
// pg_hip_platform.hip and, as plain C++, by tests/solve_device_rhs_kernel_emulation.cpp.
//
// One work-item per (i, r), r fastest, workgroups of 256: the panel side of either kernel is one contiguous stream.  The rhs side is a
// gather through the permutation whatever the assignment (W lanes of a row hit W columns ldb apart); at n = 331 776 and 16 columns it
// is 40 MB each way against a sweep of 0.75 s.
#pragma once

constexpr u32 SOLVE_MAP_PAD = 0xffffffffu;

// v * s as the host's value_times does it: in double, rounded once to the value type; both parts of a complex value
__host__ __device__ inline val_t solve_value_times(val_t v, double s)
{
#ifdef PANGULU_COMPLEX
    val_t o;
    o.re = (decltype(o.re))((double)v.re * s);
    o.im = (decltype(o.im))((double)v.im * s);
    return o;
#else
    return (val_t)((double)v * s);
#endif
}

// columns j0 .. j0 + nc - 1 of rhs into the panel x of xlen x W values.  EVERY value of the panel is written: rows n .. xlen - 1 (the
// tail of the last block), padding rows and the columns nc .. W - 1 that pad the panel to its power of two are zero -- the buffer
// is reused between panels and calls.
template <int W>
__global__ __launch_bounds__(256) void solve_pack_panel_kernel(const val_t *__restrict__ rhs, unsigned long long ldb, u32 j0, u32 nc,
                                                               const u32 *__restrict__ in_idx, const double *__restrict__ s_in, u32 n,
                                                               unsigned long long xlen, val_t *__restrict__ x)
{
    const unsigned long long k = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (k >= xlen * (unsigned long long)W)
        return;
    const unsigned long long i = k / W;
    const u32 r = (u32)(k % W);
    val_t v = v_make(0);
    if (i < n && r < nc)
    {
        const u32 src = in_idx[i];
        if (src != SOLVE_MAP_PAD)
        {
            v = rhs[(unsigned long long)(j0 + r) * ldb + src];
            if (s_in)
                v = solve_value_times(v, s_in[i]);
        }
    }
    x[k] = v;
}

// the panel x back into columns j0 .. j0 + nc - 1 of rhs: the rows out_idx names and nothing else (rows beyond the matrix's order of
// a column with ldb > n, and every other column, keep their contents)
template <int W>
__global__ __launch_bounds__(256) void solve_unpack_panel_kernel(val_t *__restrict__ rhs, unsigned long long ldb, u32 j0, u32 nc,
                                                                 const u32 *__restrict__ out_idx, const double *__restrict__ s_out, u32 n,
                                                                 const val_t *__restrict__ x)
{
    const unsigned long long k = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (k >= (unsigned long long)n * W)
        return;
    const unsigned long long i = k / W;
    const u32 r = (u32)(k % W);
    if (r >= nc)
        return;
    const u32 dst = out_idx[i];
    if (dst == SOLVE_MAP_PAD)
        return;
    const val_t v = x[k];
    rhs[(unsigned long long)(j0 + r) * ldb + dst] = s_out ? solve_value_times(v, s_out[i]) : v;
}

// workgroups of 256 for `items` work-items
inline unsigned solve_pack_grid(unsigned long long items) { return (unsigned)((items + 255ull) / 256ull); }
