// pg_hip_block_solve_trans.h -- the device kernels of the TRANSPOSED level-scheduled block triangular solve: A^T X = B and A^H X = B
// on the records of A = L U as they lie in HBM (pangulu_platform_0201001_block_trsm_multi_trans).  Included inside the anonymous
// namespace of pg_hip_platform.hip, after pg_hip_block_solve_multi.h, whose panel layout, LDS tile (pitch W + 1, right-hand side
// fastest), chunk streaming and LDS arithmetic these kernels share.
#pragma once

// -----------------------------------------------------------------------------------------------------------------
// A^T = U^T L^T: a forward sweep with U^T, then a backward sweep with L^T, on the same records read "the other way round".
//  * gather: segment i receives -B^T x_k from the block B = A(k, i) of its own block COLUMN.  B is stored CSC, so the entries that
//    add into one destination value are the contiguous entries of one column: a dot product, not a scatter.  Swapping row and column
//    in the flat loop of block_trsm_gather_multi_kernel would send the LDS atomics of a wavefront step to the same word.  Here
//    LANE GROUPS OWN COLUMNS: a group of g entry slots x W lanes walks one column, sums by shuffle and issues the column's one global
//    atomic per right-hand side; no LDS atomics, no accumulator tile, no bisection.  g is the power of two next above the block's
//    mean column length (uniform per workgroup), so that short columns of a sparse block do not idle a whole wavefront; neighbouring
//    groups take neighbouring columns, which keeps a wavefront's loads on one contiguous stretch of the record.
//  * U^T level: the upper half is CSR with the diagonal first -- its transpose is CSC with the diagonal first.  Columns ascending:
//    x[c] /= op(d_c) with the PANGULU_SPTRSV_TOL clamp on the real part, then x[idx[p]] -= op(val[p]) x[c] for the rest of the row
//    record (a scatter into distinct rows: plain LDS read-modify-write).  An empty row record is skipped like in the upper sweep.
//  * L^T level: the lower half is strictly-lower CSC, unit diagonal, colptr[0] read as 0 -- its transpose is strictly-upper CSR.
//    Rows descending: x[c] -= sum_p op(val[p]) x[idx[p]], a lane-group dot product with a shuffle reduction.
// op() conjugates for A^H (CONJ, complex builds only).  Both level kernels use exactly the LDS layout of
// block_trsm_level_multi_kernel (solve_multi_chunk / solve_multi_lds_level); the gather needs one tile and the column pointers,
// less than solve_multi_lds_gather: solve_widest_panel() holds for both directions.
// -----------------------------------------------------------------------------------------------------------------
template <bool CONJ>
__host__ __device__ inline val_t solve_trans_op(val_t v)
{
    if constexpr (CONJ)
        return v_conj(v);
    else
        return v;
}

// sum over the lanes l, l + W, l + 2 W, ... of an aligned group of `span` lanes (span / W a power of two): lanes 0 .. W - 1 of the
// group end up with the sums.  Every lane of the wavefront must call it.
template <int W>
__device__ inline val_t solve_trans_group_sum(val_t part, int span)
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

// entry slots per column group for a block with nnz entries: the power of two next above nnz / nb, between 1 and 64 / W
__host__ __device__ inline int solve_trans_group_slots(u32 nnz, int nb, int w)
{
    const u32 mean = (nnz + (u32)nb - 1) / (u32)nb;
    int g = 1;
    while (g < 64 / w && (u32)g < mean)
        g <<= 1;
    return g;
}

// X_dst -= op(B)^T X_src for every off-diagonal block of the level: one workgroup per block (B.bcol: the source segment = the
// block's own block row; B.brow: the destination segment = its block column), the source segment in LDS
template <int W, bool CONJ>
__global__ __launch_bounds__(256) void block_trsm_gather_trans_kernel(const SolveBlkD *__restrict__ blks, int nb, val_t *__restrict__ x)
{
    constexpr int P = solve_multi_pitch(W);
    extern __shared__ __align__(16) unsigned char smem_raw[];
    val_t *xs = reinterpret_cast<val_t *>(smem_raw);
    u32 *cp = reinterpret_cast<u32 *>(xs + (size_t)nb * P);
    const SolveBlkD B = blks[blockIdx.x];
    const val_t *xsrc = x + (size_t)B.bcol * nb * W;
    val_t *xdst = x + (size_t)B.brow * nb * W;
    const int tid = threadIdx.x;
    for (int k = tid; k < nb * W; k += 256)
        xs[(k / W) * P + k % W] = xsrc[k];
    for (int i = tid; i <= nb; i += 256)
        cp[i] = i == 0 ? 0u : B.cp[i];
    __syncthreads();
    const int g = solve_trans_group_slots(cp[nb], nb, W); // uniform over the workgroup
    const int span = g * W, ngroup = 256 / span;
    const int group = tid / span, slot = (tid % span) / W, r = tid % W;
    for (int c0 = 0; c0 < nb; c0 += ngroup) // (uniform trip count: the shuffles below are executed by whole wavefronts)
    {
        const int c = c0 + group;
        val_t part = v_make(0);
        u32 p0 = 0, p1 = 0;
        if (c < nb)
        {
            p0 = cp[c];
            p1 = cp[c + 1];
        }
        for (u32 p = p0 + (u32)slot; p < p1; p += (u32)g)
        {
            const val_t m = v_mul(solve_trans_op<CONJ>(B.val[p]), xs[B.ri[p] * P + r]);
#ifdef PANGULU_COMPLEX
            part.re += m.re;
            part.im += m.im;
#else
            part += m;
#endif
        }
        part = solve_trans_group_sum<W>(part, span);
        if (slot == 0 && p0 != p1)
            v_atomic_add(&xdst[c * W + r], v_sub(v_make(0), part));
    }
}

// The diagonal halves of the level's segments: one workgroup per segment, the nb x W segment in LDS, the diagonal half streamed
// through LDS in double-buffered chunks of `ch` records exactly as block_trsm_level_multi_kernel does.  LT = false: U^T, rows of
// the CSR upper half in ascending order (forward sweep); LT = true: L^T, columns of the strictly-lower CSC half in descending order.
template <bool LT, int W, bool CONJ>
__global__ __launch_bounds__(256) void block_trsm_level_trans_kernel(const SolveRowD *__restrict__ rows, int nb, val_t *__restrict__ x, int ch)
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
        ptr[i] = (LT && i == 0) ? 0u : R.dptr[i];
    __syncthreads();
    const int nchunk = (nb + ch - 1) / ch;
    // chunk k: records [k ch, (k + 1) ch) of the upper half ascending; records [nb - (k + 1) ch, nb - k ch) of the lower half, descending
    auto lo_of = [&](int k) -> int { return LT ? max(0, nb - (k + 1) * ch) : k * ch; };
    auto hi_of = [&](int k) -> int { return LT ? nb - k * ch : min(nb, (k + 1) * ch); };
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
            if (!LT)
            {
                for (int c = c0; c < c1; c++)
                {
                    const u32 b = ptr[c] - base, e = ptr[c + 1] - base;
                    if (b == e)
                        continue;
                    if (lane < W)
                    {
                        val_t d = solve_trans_op<CONJ>(bv[b]);
                        const real_t dr = v_realpart(d);
                        if (!((dr < 0 ? -dr : dr) > (real_t)PANGULU_SPTRSV_TOL))
                            d = v_make((real_t)PANGULU_SPTRSV_TOL);
                        seg[c * P + lane] = v_div(seg[c * P + lane], d);
                    }
                    wave_lds_fence();
                    const val_t xc = seg[c * P + r];
                    for (u32 p = b + 1 + eslot; p < e; p += 64 / W)
                    {
                        val_t *d = &seg[bi[p] * P + r];
                        *d = v_submul(*d, solve_trans_op<CONJ>(bv[p]), xc);
                    }
                    wave_lds_fence();
                }
            }
            else
            {
                for (int c = c1 - 1; c >= c0; c--)
                {
                    const u32 b = ptr[c] - base, e = ptr[c + 1] - base;
                    if (b == e)
                        continue;
                    val_t part = v_make(0);
                    for (u32 p = b + eslot; p < e; p += 64 / W)
                    {
                        const val_t m = v_mul(solve_trans_op<CONJ>(bv[p]), seg[bi[p] * P + r]);
#ifdef PANGULU_COMPLEX
                        part.re += m.re;
                        part.im += m.im;
#else
                        part += m;
#endif
                    }
                    part = solve_trans_group_sum<W>(part, 64);
                    if (lane < W)
                        seg[c * P + lane] = v_sub(seg[c * P + lane], part);
                    wave_lds_fence();
                }
            }
        }
        __syncthreads();
    }
    for (int k = tid; k < nb * W; k += 256)
        xr[k] = seg[(k / W) * P + k % W];
}

// LDS demand of the transposed gather (the level kernels take solve_multi_lds_level): never more than solve_multi_lds_gather
inline size_t solve_trans_lds_gather(size_t nb, int w)
{
    return sizeof(val_t) * nb * (size_t)solve_multi_pitch(w) + sizeof(u32) * (nb + 1);
}
