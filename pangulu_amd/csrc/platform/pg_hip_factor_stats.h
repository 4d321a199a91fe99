// pg_hip_factor_stats.h -- what pangulu_amd_factor_stats and pangulu_amd_rcond run on the device:
//   factor_stats_kernel     one workgroup per listed block record: largest modulus, non-finite count, entry count and, for an upper
//                           diagonal half, the pivots' minimum (first index), maximum, clamp count and product
//                           (pangulu_platform_0201001_factor_stats);
//   condest_*_kernel        the steps between two solves of Higham's 1-norm estimator on a device vector
//                           (pangulu_platform_0201001_condest_vector).
// Included inside the anonymous namespace of pg_hip_platform.hip and, as plain C++, by tests/factor_stats_kernel_emulation.cpp.
//
// Reductions.  Every workgroup has 256 work-items = 4 wavefronts.  A work-item folds its own items in index order; the 64 partials
// of a wavefront are folded by __shfl_down with the offsets 32, 16, .. 1; lane 0 of each wavefront puts its partial in LDS and
// work-item 0 folds the four in wavefront order; one partial per workgroup leaves by a plain store.  The tree is the same for every
// launch with the same sizes, and nothing is accumulated by atomics, so sums and products do not depend on the order in which
// wavefronts or workgroups happen to run: the same input gives the same bits.  All arithmetic is in double, whatever val_t is.
//
// The pivot product would leave double's range long before n = 1000 (log|det| = 1908 and -7302 on the test matrices), so it is
// carried as a mantissa and a binary exponent and renormalised with frexp at every multiplication.
#pragma once

constexpr int FS_THREADS = 256;
constexpr double FS_PIVOT_CLAMP = 1e-16; // clamp_pivot / solve_clamped_divisor: |Re| below it is divided by it instead
#ifndef PG_CONDEST_MAX_GROUPS
#define PG_CONDEST_MAX_GROUPS 256 // (at most 256: the last stage takes one partial per work-item; the emulation test also builds with 4)
#endif
constexpr unsigned CONDEST_MAX_GROUPS = PG_CONDEST_MAX_GROUPS;
static_assert(CONDEST_MAX_GROUPS >= 1 && CONDEST_MAX_GROUPS <= 256, "one partial per work-item of the last stage");

// a block record as the statistics kernel reads it
struct FactorStatsBlkD
{
    const val_t *val;
    const u32 *rowptr; // upper diagonal half: its CSR row pointer (the pivot is the first entry of its row); nullptr otherwise
    unsigned long long nnz;
    unsigned long long row0; // upper diagonal half: row of the factors' ordering its first row is
};

__host__ __device__ inline double fs_re(val_t v)
{
#ifdef PANGULU_COMPLEX
    return (double)v.re;
#else
    return (double)v;
#endif
}
__host__ __device__ inline double fs_im(val_t v)
{
#ifdef PANGULU_COMPLEX
    return (double)v.im;
#else
    (void)v;
    return 0.0;
#endif
}
__host__ __device__ inline bool fs_finite(double a) { return a - a == 0.0; } // false for NaN and +-Inf
__host__ __device__ inline double fs_abs(double re, double im) { return im == 0.0 ? fabs(re) : hypot(re, im); }

// ---- the folded quantities and how two of them combine ---------------------------------------------------------------------------
struct FsMax // the entry of largest modulus; NaN never wins (key -1), an empty set has key -1
{
    double key, re, im;
    unsigned long long idx;
};
__host__ __device__ inline FsMax fs_max_none() { return FsMax{-1.0, 0.0, 0.0, ~0ull}; }
__host__ __device__ inline FsMax fs_max_of(double re, double im, unsigned long long idx)
{
    const double a = fs_abs(re, im);
    return FsMax{a == a ? a : -1.0, re, im, idx};
}
__host__ __device__ inline FsMax fs_max_combine(FsMax a, FsMax b) // the first index on a tie
{
    return (b.key > a.key || (b.key == a.key && b.idx < a.idx)) ? b : a;
}
struct FsMin // the entry of smallest modulus, first index on a tie; NaN never wins; idx == ~0: empty
{
    double key, re, im;
    unsigned long long idx;
};
__host__ __device__ inline FsMin fs_min_none() { return FsMin{0.0, 0.0, 0.0, ~0ull}; }
__host__ __device__ inline FsMin fs_min_combine(FsMin a, FsMin b)
{
    if (b.idx == ~0ull)
        return a;
    if (a.idx == ~0ull)
        return b;
    return (b.key < a.key || (b.key == a.key && b.idx < a.idx)) ? b : a;
}
struct FsProd // (re + i im) * 2^e with 0.5 <= max(|re|, |im|) < 1, or 0 * 2^0; a non-finite mantissa stays as it is
{
    double re, im;
    long long e;
};
__host__ __device__ inline FsProd fs_prod_one() { return FsProd{0.5, 0.0, 1}; }
__host__ __device__ inline FsProd fs_prod_normalise(FsProd p)
{
    const double m = fabs(p.re) > fabs(p.im) ? fabs(p.re) : fabs(p.im);
    if (!fs_finite(p.re) || !fs_finite(p.im))
        return p;
    if (m == 0.0)
        return FsProd{0.0, 0.0, 0};
    int k = 0;
    (void)frexp(m, &k);
    return FsProd{ldexp(p.re, -k), ldexp(p.im, -k), p.e + k};
}
__host__ __device__ inline FsProd fs_prod_combine(FsProd a, FsProd b)
{
    FsProd r;
    if (a.im == 0.0 && b.im == 0.0) // (real types, and real pivots of complex ones: one rounding)
    {
        r.re = a.re * b.re;
        r.im = 0.0;
    }
    else
    {
        r.re = a.re * b.re - a.im * b.im;
        r.im = a.re * b.im + a.im * b.re;
    }
    r.e = a.e + b.e;
    return fs_prod_normalise(r);
}
struct FsSum
{
    double v;
};
__host__ __device__ inline FsSum fs_sum_combine(FsSum a, FsSum b) { return FsSum{a.v + b.v}; }
struct FsCount
{
    unsigned long long v;
};
__host__ __device__ inline FsCount fs_count_combine(FsCount a, FsCount b) { return FsCount{a.v + b.v}; }

// ---- the fixed tree ----------------------------------------------------------------------------------------------------------------
template <class T>
__device__ inline T fs_shfl_down(T v, int off)
{
    static_assert(sizeof(T) % 8 == 0, "folded in 64-bit words");
    constexpr int NW = (int)(sizeof(T) / 8);
    unsigned long long w[NW];
    memcpy(w, &v, sizeof(T));
    for (int i = 0; i < NW; i++)
        w[i] = __shfl_down(w[i], off, 64);
    T r;
    memcpy(&r, w, sizeof(T));
    return r;
}
// every work-item of the workgroup calls it; the result is valid in work-item 0.  `lds` holds 4 values of T and may be reused after
// the call (it ends with a barrier)
template <class T, class Op>
__device__ inline T fs_block_fold(T v, Op op, T *lds)
{
    for (int off = 32; off > 0; off >>= 1)
    {
        const T o = fs_shfl_down(v, off);
        if ((int)(threadIdx.x & 63) + off < 64) // (a lane past the end would fold its own value in twice)
            v = op(v, o);
    }
    if ((threadIdx.x & 63) == 0)
        lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        v = op(op(op(lds[0], lds[1]), lds[2]), lds[3]);
    __syncthreads();
    return v;
}

// ---- block records -----------------------------------------------------------------------------------------------------------------
// One partial per record (pangulu_factor_stats_partial_t of include/pangulu_platform.h, restated: the kernel headers do not see it).
struct FactorStatsPartialD
{
    double max_re, max_im;
    unsigned long long nonfinite, entries;
    double minp_re, minp_im;
    unsigned long long minp_row;
    double maxp_re, maxp_im;
    unsigned long long clamped, pivots;
    double prod_re, prod_im;
    long long prod_exp;
};

// pad[i] != 0: row i of the factors' ordering is a padding row (unit pivot, not the user's); pad == nullptr: none
__global__ __launch_bounds__(256) void factor_stats_kernel(const FactorStatsBlkD *__restrict__ blks, int nb, const unsigned char *__restrict__ pad,
                                                           FactorStatsPartialD *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const FactorStatsBlkD B = blks[blockIdx.x];
    FsMax mx = fs_max_none();
    FsCount bad{0};
    for (unsigned long long p = threadIdx.x; p < B.nnz; p += FS_THREADS)
    {
        const double re = fs_re(B.val[p]), im = fs_im(B.val[p]);
        mx = fs_max_combine(mx, fs_max_of(re, im, p));
        bad.v += (fs_finite(re) && fs_finite(im)) ? 0u : 1u;
    }
    mx = fs_block_fold(mx, fs_max_combine, reinterpret_cast<FsMax *>(smem_raw));
    bad = fs_block_fold(bad, fs_count_combine, reinterpret_cast<FsCount *>(smem_raw));
    FsMin pmin = fs_min_none();
    FsMax pmax = fs_max_none();
    FsCount clamped{0}, pivots{0};
    FsProd prod = fs_prod_one();
    if (B.rowptr) // (uniform over the workgroup)
    {
        for (int r = threadIdx.x; r < nb; r += FS_THREADS)
        {
            const u32 b = ptr0(B.rowptr, r), e = B.rowptr[r + 1];
            const unsigned long long row = B.row0 + (unsigned long long)r;
            if (b == e || (pad && pad[row]))
                continue;
            const double re = fs_re(B.val[b]), im = fs_im(B.val[b]);
            const FsMax m = fs_max_of(re, im, row);
            pmax = fs_max_combine(pmax, m);
            pmin = fs_min_combine(pmin, FsMin{m.key < 0 ? HUGE_VAL : m.key, re, im, row});
            clamped.v += fabs(re) < FS_PIVOT_CLAMP ? 1u : 0u;
            pivots.v += 1;
            prod = fs_prod_combine(prod, fs_prod_normalise(FsProd{re, im, 0}));
        }
        pmin = fs_block_fold(pmin, fs_min_combine, reinterpret_cast<FsMin *>(smem_raw));
        pmax = fs_block_fold(pmax, fs_max_combine, reinterpret_cast<FsMax *>(smem_raw));
        clamped = fs_block_fold(clamped, fs_count_combine, reinterpret_cast<FsCount *>(smem_raw));
        pivots = fs_block_fold(pivots, fs_count_combine, reinterpret_cast<FsCount *>(smem_raw));
        prod = fs_block_fold(prod, fs_prod_combine, reinterpret_cast<FsProd *>(smem_raw));
    }
    if (threadIdx.x == 0)
    {
        FactorStatsPartialD o;
        o.max_re = mx.re;
        o.max_im = mx.im;
        o.nonfinite = bad.v;
        o.entries = B.nnz;
        o.minp_re = pmin.re;
        o.minp_im = pmin.im;
        o.minp_row = pmin.idx;
        o.maxp_re = pmax.re;
        o.maxp_im = pmax.im;
        o.clamped = clamped.v;
        o.pivots = pivots.v;
        o.prod_re = prod.re;
        o.prod_im = prod.im;
        o.prod_exp = prod.e;
        out[blockIdx.x] = o;
    }
}

// ---- the estimator's vector steps --------------------------------------------------------------------------------------------------
// What the host reads back after a step (pangulu_condest_result_t of include/pangulu_platform.h, restated).
struct CondestResultD
{
    double norm1;               // sum |x_i| (NORM1_SIGN, NORM1)
    double absmax, abs_prev;    // ARGMAX: |x_argmax| and |x_jprev|
    unsigned long long argmax;  // ARGMAX: the first index of the largest modulus
    unsigned long long unchanged; // NORM1_SIGN, real types: 1 when every sign equals the saved one
};
// per-workgroup partials of one step
struct CondestPartialD
{
    double sum;
    double key;
    unsigned long long idx;
    unsigned long long changed;
};

__host__ __device__ inline val_t condest_value(double re)
{
#ifdef PANGULU_COMPLEX
    val_t o;
    o.re = (decltype(o.re))re;
    o.im = 0;
    return o;
#else
    return (val_t)re;
#endif
}
// the sign vector of xLACN2: real sign(1, x) by the sign bit (1 for +0, -1 for -0 as Fortran's SIGN; a NaN by its sign bit as well); complex x / |x|, 1 where |x| is below the smallest normal
__host__ __device__ inline val_t condest_sign(val_t x)
{
#ifdef PANGULU_COMPLEX
    const double re = (double)x.re, im = (double)x.im, a = hypot(re, im);
    val_t o;
    if (a > 2.2250738585072014e-308)
    {
        o.re = (decltype(o.re))(re / a);
        o.im = (decltype(o.im))(im / a);
    }
    else
    {
        o.re = 1;
        o.im = 0;
    }
    return o;
#else
    return (val_t)(__builtin_signbit((double)x) ? -1.0 : 1.0);
#endif
}
__host__ __device__ inline double condest_alt(unsigned long long i, unsigned long long n)
{
    const double v = 1.0 + (double)i / (double)(n > 1 ? n - 1 : 1);
    return (i & 1ull) ? -v : v;
}
// workgroups a step over n values runs with: a function of n alone
__host__ __device__ inline unsigned condest_groups(unsigned long long n)
{
    const unsigned long long g = (n + FS_THREADS - 1) / FS_THREADS;
    return (unsigned)(g < 1 ? 1 : (g > CONDEST_MAX_GROUPS ? CONDEST_MAX_GROUPS : g));
}

constexpr int CONDEST_FILL_INV_N = 0, CONDEST_SET_EJ = 1, CONDEST_FILL_ALT = 2;
__global__ __launch_bounds__(256) void condest_fill_kernel(int what, val_t *__restrict__ x, unsigned long long n, unsigned long long j, unsigned groups)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * FS_THREADS + threadIdx.x; i < n; i += (unsigned long long)groups * FS_THREADS)
        x[i] = condest_value(what == CONDEST_FILL_INV_N ? 1.0 / (double)n : what == CONDEST_SET_EJ ? (i == j ? 1.0 : 0.0) : condest_alt(i, n));
}

// sum |x_i| per workgroup; with_sign: x becomes its sign vector and (real types, save != nullptr) is compared with and copied to `save`
__global__ __launch_bounds__(256) void condest_norm1_kernel(val_t *__restrict__ x, val_t *__restrict__ save, unsigned long long n, int with_sign,
                                                            unsigned groups, CondestPartialD *__restrict__ part)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    FsSum s{0.0};
    FsCount changed{0};
    for (unsigned long long i = (unsigned long long)blockIdx.x * FS_THREADS + threadIdx.x; i < n; i += (unsigned long long)groups * FS_THREADS)
    {
        const val_t v = x[i];
        s.v += fs_abs(fs_re(v), fs_im(v));
        if (with_sign)
        {
            const val_t sg = condest_sign(v);
            x[i] = sg;
#ifndef PANGULU_COMPLEX
            if (save)
            {
                changed.v += save[i] == sg ? 0u : 1u;
                save[i] = sg;
            }
#endif
        }
    }
    s = fs_block_fold(s, fs_sum_combine, reinterpret_cast<FsSum *>(smem_raw));
    changed = fs_block_fold(changed, fs_count_combine, reinterpret_cast<FsCount *>(smem_raw));
    if (threadIdx.x == 0)
    {
        part[blockIdx.x].sum = s.v;
        part[blockIdx.x].changed = changed.v;
    }
}

__global__ __launch_bounds__(256) void condest_argmax_kernel(const val_t *__restrict__ x, unsigned long long n, unsigned groups,
                                                             CondestPartialD *__restrict__ part)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    FsMax m = fs_max_none();
    for (unsigned long long i = (unsigned long long)blockIdx.x * FS_THREADS + threadIdx.x; i < n; i += (unsigned long long)groups * FS_THREADS)
        m = fs_max_combine(m, fs_max_of(fs_re(x[i]), fs_im(x[i]), i));
    m = fs_block_fold(m, fs_max_combine, reinterpret_cast<FsMax *>(smem_raw));
    if (threadIdx.x == 0)
    {
        part[blockIdx.x].key = m.key;
        part[blockIdx.x].idx = m.idx;
    }
}

// the last stage, one workgroup: the partials of `groups` <= 256 workgroups, one per work-item, through the same tree
constexpr int CONDEST_LAST_NORM1 = 0, CONDEST_LAST_ARGMAX = 1;
__global__ __launch_bounds__(256) void condest_last_kernel(int what, const CondestPartialD *__restrict__ part, unsigned groups, const val_t *__restrict__ x,
                                                           unsigned long long n, unsigned long long jprev, int compared, CondestResultD *__restrict__ res)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    if (what == CONDEST_LAST_NORM1)
    {
        FsSum s{threadIdx.x < groups ? part[threadIdx.x].sum : 0.0};
        FsCount c{threadIdx.x < groups ? part[threadIdx.x].changed : 0ull};
        s = fs_block_fold(s, fs_sum_combine, reinterpret_cast<FsSum *>(smem_raw));
        c = fs_block_fold(c, fs_count_combine, reinterpret_cast<FsCount *>(smem_raw));
        if (threadIdx.x == 0)
        {
            res->norm1 = s.v;
#ifdef PANGULU_COMPLEX
            res->unchanged = 0ull; // (xLACN2 has no repeated-sign test for complex vectors)
#else
            res->unchanged = (compared && c.v == 0) ? 1ull : 0ull;
#endif
        }
    }
    else
    {
        FsMax m = fs_max_none();
        if (threadIdx.x < groups)
        {
            m.key = part[threadIdx.x].key;
            m.idx = part[threadIdx.x].idx;
        }
        m = fs_block_fold(m, fs_max_combine, reinterpret_cast<FsMax *>(smem_raw));
        if (threadIdx.x == 0)
        {
            res->argmax = m.idx;
            res->absmax = m.idx < n ? fs_abs(fs_re(x[m.idx]), fs_im(x[m.idx])) : 0.0;
            res->abs_prev = jprev < n ? fs_abs(fs_re(x[jprev]), fs_im(x[jprev])) : 0.0;
        }
    }
}
