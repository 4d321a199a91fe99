// pg_hip_block_solve_multi.h -- the device kernels of the level-scheduled block triangular solve: a PANEL of W right-hand sides per
// launch, W = 1 for pangulu_gstrs and up to 16 for pangulu_amd_gstrs_multi (pangulu_platform_0201001_block_trsv and
// ..._block_trsm_multi launch the same instances).  Included inside the anonymous namespace of pg_hip_platform.hip, after
// pg_hip_block_solve.h (descriptors SolveBlkD / SolveRowD, the column-by-column kernels of PANGULU_HIP_SOLVE_CHUNKED=0).
#pragma once

// -----------------------------------------------------------------------------------------------------------------
// Round 4: two launches per level, built around where the column-by-column kernels' time went (fem27(112): 540 launches, 394 ms).
// That gather kernel walks a block column by column, sixteen lanes a column, every entry a floating-point atomic on the row's
// 256 words in HBM (hundreds of blocks of a row near the root contend for them): 98 % of its wave cycles waiting.  That level
// kernel sweeps a diagonal half column by column straight from HBM: nb dependent round trips.
//  * gather: the block's entries flat over the workgroup (coalesced loads, the column of an entry by bisection in an LDS copy of the
//    column pointers), products accumulated in LDS (ds_add_f64), ONE global atomic per touched row of the segment at the end;
//  * level: the diagonal half streams through LDS in chunks of `ch` columns (rows for the upper sweep), double-buffered: three
//    wavefronts fetch chunk k + 1 while the first one sweeps chunk k out of LDS -- a dependent step costs LDS round trips, not HBM ones.
//
// A sweep is an HBM stream of the factor records plus two launches per level; neither depends on how many vectors ride along.
// Every factor entry is read once and applied to W values.
//
// A panel is stored with the right-hand side fastest: X[i * W + r], i = row of the padded system, r = right-hand side.  In LDS
// a segment is an nb x W tile with a row pitch of W + 1 values (W = 1: no padding): the W lanes of one entry touch W contiguous
// words and never conflict among themselves; which rows two different entries of a wavefront step touch is data, and with a
// pitch of W values (a power of two) rows i and i + 32 / (W words) would always share their banks -- the odd pitch spreads them.
//
// Same per-block arithmetic as the column-by-column kernels: spmv, unit-lower column sweep, upper row sweep with the
// PANGULU_SPTRSV_TOL clamp (real part only for complex); sums across blocks arrive in a different order.
// -----------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int solve_multi_pitch(int w) { return w > 1 ? w + 1 : 1; }

// X_row -= A(row, j) X_j for every off-diagonal block of the level: one workgroup per block, the block's entries flat over the
// workgroup as 256 / W entry slots x W lanes, products accumulated in an LDS tile, one global atomic per touched (row, r)
template <int W>
__global__ __launch_bounds__(256) void block_trsm_gather_multi_kernel(const SolveBlkD *__restrict__ blks, int nb, val_t *__restrict__ x)
{
    constexpr int P = solve_multi_pitch(W);
    extern __shared__ __align__(16) unsigned char smem_raw[];
    val_t *acc = reinterpret_cast<val_t *>(smem_raw);
    val_t *xs = acc + (size_t)nb * P;
    u32 *cp = reinterpret_cast<u32 *>(xs + (size_t)nb * P);
    u32 *touched = cp + nb + 1;
    const SolveBlkD B = blks[blockIdx.x];
    const val_t *xj = x + (size_t)B.bcol * nb * W;
    val_t *xr = x + (size_t)B.brow * nb * W;
    const int tid = threadIdx.x;
    for (int k = tid; k < nb * W; k += 256)
    {
        const int i = k / W, r = k % W;
        acc[i * P + r] = v_make(0);
        xs[i * P + r] = xj[k];
    }
    for (int i = tid; i < nb; i += 256)
        touched[i] = 0;
    for (int i = tid; i <= nb; i += 256)
        cp[i] = i == 0 ? 0u : B.cp[i];
    __syncthreads();
    const u32 nnz = cp[nb];
    const int slot = tid / W, r = tid % W;
    for (u32 p = (u32)slot; p < nnz; p += 256 / W)
    {
        // column of entry p: the last c with cp[c] <= p
        int lo = 0, hi = nb;
        while (hi - lo > 1)
        {
            const int mid = (lo + hi) >> 1;
            if (cp[mid] <= p)
                lo = mid;
            else
                hi = mid;
        }
        const int row = B.ri[p];
        lds_atomic_sub(&acc[row * P + r], v_mul(B.val[p], xs[lo * P + r]));
        if (r == 0)
            touched[row] = 1;
    }
    __syncthreads();
    for (int k = tid; k < nb * W; k += 256)
    {
        const int i = k / W;
        if (touched[i])
            v_atomic_add(&xr[k], acc[i * P + k % W]);
    }
}

// The diagonal halves of the level's block rows: one workgroup per row, the nb x W segment in LDS, the diagonal half streamed
// through LDS in double-buffered chunks of `ch` columns (rows for the upper sweep) -- three wavefronts fetch chunk k + 1 while
// the first one sweeps chunk k.  A wavefront step is 64 / W entries x W right-hand sides.
template <bool UPPER, int W>
__global__ __launch_bounds__(256) void block_trsm_level_multi_kernel(const SolveRowD *__restrict__ rows, int nb, val_t *__restrict__ x, int ch)
{
    constexpr int P = solve_multi_pitch(W);
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const size_t cap = (size_t)ch * (size_t)nb; // entries a chunk can hold
    val_t *seg = reinterpret_cast<val_t *>(smem_raw);
    val_t *bv0 = seg + (size_t)nb * P, *bv1 = bv0 + cap;
    u32 *ptr = reinterpret_cast<u32 *>(bv1 + cap);
    u16 *bi0 = reinterpret_cast<u16 *>(ptr + nb + 2), *bi1 = bi0 + cap;
    const SolveRowD R = rows[blockIdx.x];
    val_t *xr = x + (size_t)R.brow * nb * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < nb * W; k += 256)
        seg[(k / W) * P + k % W] = xr[k];
    for (int i = tid; i <= nb; i += 256)
        ptr[i] = (!UPPER && i == 0) ? 0u : R.dptr[i];
    __syncthreads();
    const int nchunk = (nb + ch - 1) / ch;
    // chunk k: columns [k ch, (k + 1) ch) of the lower half in ascending order; rows [nb - (k + 1) ch, nb - k ch) of the upper half, descending
    auto lo_of = [&](int k) -> int { return UPPER ? max(0, nb - (k + 1) * ch) : k * ch; };
    auto hi_of = [&](int k) -> int { return UPPER ? nb - k * ch : min(nb, (k + 1) * ch); };
    auto fetch = [&](int k, int first, int nthr)
    {
        val_t *bv = (k & 1) ? bv1 : bv0;
        u16 *bi = (k & 1) ? bi1 : bi0;
        const u32 p0 = ptr[lo_of(k)], p1 = ptr[hi_of(k)];
        for (u32 p = p0 + (u32)first; p < p1; p += (u32)nthr)
        {
            bv[p - p0] = R.dval[p];
            bi[p - p0] = R.didx[p];
        }
    };
    fetch(0, tid, 256);
    __syncthreads();
    const int eslot = lane / W, r = lane % W;
    for (int k = 0; k < nchunk; k++)
    {
        if (wave != 0)
        {
            if (k + 1 < nchunk)
                fetch(k + 1, tid - 64, 192);
        }
        else
        {
            const val_t *bv = (k & 1) ? bv1 : bv0;
            const u16 *bi = (k & 1) ? bi1 : bi0;
            const int c0 = lo_of(k), c1 = hi_of(k);
            const u32 base = ptr[c0];
            if (!UPPER)
            {
                for (int c = c0; c < c1; c++)
                {
                    const u32 p0 = ptr[c] - base, p1 = ptr[c + 1] - base;
                    if (p0 == p1)
                        continue;
                    const val_t xc = seg[c * P + r];
                    for (u32 p = p0 + eslot; p < p1; p += 64 / W)
                    {
                        val_t *d = &seg[bi[p] * P + r];
                        *d = v_submul(*d, bv[p], xc);
                    }
                    wave_lds_fence();
                }
            }
            else
            {
                for (int row = c1 - 1; row >= c0; row--)
                {
                    const u32 b = ptr[row] - base, e = ptr[row + 1] - base;
                    if (b == e)
                        continue;
                    // each lane group accumulates its partial dot for its right-hand side; lanes 0 .. W - 1 end up with the sums
#ifdef PANGULU_COMPLEX
                    val_t part = v_make(0);
                    for (u32 p = b + 1 + eslot; p < e; p += 64 / W)
                    {
                        const val_t m = v_mul(bv[p], seg[bi[p] * P + r]);
                        part.re += m.re;
                        part.im += m.im;
                    }
                    for (int off = 32; off >= W; off >>= 1)
                    {
                        part.re += __shfl_down(part.re, off, 64);
                        part.im += __shfl_down(part.im, off, 64);
                    }
#else
                    val_t part = 0;
                    for (u32 p = b + 1 + eslot; p < e; p += 64 / W)
                        part += bv[p] * seg[bi[p] * P + r];
                    for (int off = 32; off >= W; off >>= 1)
                        part += __shfl_down(part, off, 64);
#endif
                    if (lane < W)
                    {
                        val_t d = bv[b];
                        const real_t dr = v_realpart(d);
                        if (!((dr < 0 ? -dr : dr) > (real_t)PANGULU_SPTRSV_TOL))
                            d = v_make((real_t)PANGULU_SPTRSV_TOL);
                        seg[row * P + lane] = v_div(v_sub(seg[row * P + lane], part), d);
                    }
                    wave_lds_fence();
                }
            }
        }
        __syncthreads();
    }
    for (int k = tid; k < nb * W; k += 256)
        xr[k] = seg[(k / W) * P + k % W];
}

// LDS demand of the two kernels for a panel of w right-hand sides, and the chunk depth the level kernel gets out of `budget` bytes
// (at most 16 columns; 0: not even one fits beside the segment)
inline size_t solve_multi_lds_gather(size_t nb, int w)
{
    return 2 * sizeof(val_t) * nb * (size_t)solve_multi_pitch(w) + sizeof(u32) * (nb + 1) + sizeof(u32) * nb;
}
inline int solve_multi_chunk(size_t nb, int w, size_t budget)
{
    const size_t fixed = sizeof(val_t) * nb * (size_t)solve_multi_pitch(w) + sizeof(u32) * (nb + 2) + 16;
    const size_t per_col = 2 * nb * (sizeof(val_t) + sizeof(u16)); // both buffers
    if (fixed + per_col > budget)
        return 0;
    return (int)std::min<size_t>(std::min<size_t>(16, nb), (budget - fixed) / per_col);
}
inline size_t solve_multi_lds_level(size_t nb, int w, int ch)
{
    return sizeof(val_t) * nb * (size_t)solve_multi_pitch(w) + 2 * (size_t)ch * nb * (sizeof(val_t) + sizeof(u16)) + sizeof(u32) * (nb + 2) + 16;
}
