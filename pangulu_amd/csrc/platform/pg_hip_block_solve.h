// pg_hip_block_solve.h -- the column-by-column kernels of the level-scheduled block triangular solve and the kernel of the
// device-side factor check.  Included inside the anonymous namespace of pg_hip_platform.hip, after pg_hip_block_solve_multi.h
// (the descriptors SolveBlkD / SolveRowD).
#pragma once

// -----------------------------------------------------------------------------------------------------------------
// Level-scheduled block triangular solve on a single rank (pangulu_gstrs, pangulu_amd_gstrs_multi).
// The reference sweeps block row by block row with one spmv / sptrsv platform call per block on the CPU platform
// (src/pangulu_sptrsv.c:24-191); here block rows whose inputs are final form a LEVEL of the block dependency graph and one
// level is two launches: one workgroup per off-diagonal block subtracts  A(row, j) x_j  from the row's segment (floating-
// point atomics), then one workgroup per block row solves with the row's diagonal half and writes the finished segment.
// Same per-block arithmetic as ...0100000.c:435-506 (spmv, unit-lower column sweep, upper row sweep with the
// PANGULU_SPTRSV_TOL clamp); sums across blocks arrive in a different order.
//
// The kernels every solve launches by default are in pg_hip_block_solve_multi.h (a single vector is a panel of width 1).  The
// pair here -- block_trsv_gather_kernel / block_trsv_level_kernel, rounds 2-3 -- walks the records column by column straight
// from HBM and takes single vectors only: PANGULU_HIP_SOLVE_CHUNKED=0 selects it, and it is what is left when nb is so large
// that not even one chunk column of a diagonal half fits in LDS beside the segment.
// -----------------------------------------------------------------------------------------------------------------
// x_row -= A(row, j) x_j for every off-diagonal block of the level: one workgroup per block (rows near the root of the
// tree have hundreds of blocks: a workgroup per row would walk them one after the other), floating-point atomics on
// the destination segment
__global__ __launch_bounds__(256) void block_trsv_gather_kernel(const SolveBlkD *__restrict__ blks, int nb, val_t *__restrict__ x)
{
    const SolveBlkD B = blks[blockIdx.x];
    const val_t *xj = x + (size_t)B.bcol * nb;
    val_t *xr = x + (size_t)B.brow * nb;
    const int sub = threadIdx.x >> 4, l16 = threadIdx.x & 15, nsub = blockDim.x >> 4;
    for (int c = sub; c < nb; c += nsub)
    {
        const u32 p0 = ptr0(B.cp, c), p1 = B.cp[c + 1];
        if (p0 == p1)
            continue;
        const val_t xc = xj[c];
        for (u32 p = p0 + l16; p < p1; p += 16)
        {
            const val_t m = v_mul(B.val[p], xc);
#ifdef PANGULU_COMPLEX
            v_atomic_add(&xr[B.ri[p]], val_t{-m.re, -m.im});
#else
            v_atomic_add(&xr[B.ri[p]], -m);
#endif
        }
    }
}

// y_dst += A x_src for a list of blocks (factor check: t = U 1, then y = L t): one workgroup per block, 16 lanes per
// column (CSC record) or row (CSR record: upper diagonal half), floating-point atomics on y
struct SpmvBlkD
{
    const u32 *ptr;
    const u16 *idx;
    const val_t *val;
    u32 src, dst;
    u32 csr, pad_;
};
__global__ __launch_bounds__(256) void block_spmv_add_kernel(const SpmvBlkD *__restrict__ blks, int nb, const val_t *__restrict__ x, val_t *__restrict__ y)
{
    const SpmvBlkD B = blks[blockIdx.x];
    const val_t *xs = x + (size_t)B.src * nb;
    val_t *yd = y + (size_t)B.dst * nb;
    const int sub = threadIdx.x >> 4, l16 = threadIdx.x & 15, nsub = blockDim.x >> 4;
    for (int c = sub; c < nb; c += nsub)
    {
        const u32 p0 = ptr0(B.ptr, c), p1 = B.ptr[c + 1];
        if (p0 == p1)
            continue;
        if (!B.csr)
        {
            const val_t xc = xs[c];
            for (u32 p = p0 + l16; p < p1; p += 16)
                v_atomic_add(&yd[B.idx[p]], v_mul(B.val[p], xc));
        }
        else
        {
            val_t part = v_make(0);
            for (u32 p = p0 + l16; p < p1; p += 16)
                part = v_add(part, v_mul(B.val[p], xs[B.idx[p]]));
            v_atomic_add(&yd[c], part); // (16 partial sums per row)
        }
    }
}

// the diagonal halves of the level's block rows: one wavefront per row, the segment in LDS
template <bool UPPER>
__global__ __launch_bounds__(64) void block_trsv_level_kernel(const SolveRowD *__restrict__ rows, int nb, val_t *__restrict__ x)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    val_t *seg = reinterpret_cast<val_t *>(smem_raw);
    const SolveRowD R = rows[blockIdx.x];
    val_t *xr = x + (size_t)R.brow * nb;
    for (int i = threadIdx.x; i < nb; i += blockDim.x)
        seg[i] = xr[i];
    __syncthreads();
    // the diagonal half, by one wavefront (LDS operations of a wavefront complete in order: no barriers in the sweep)
    if (threadIdx.x < 64)
    {
        const int lane = threadIdx.x;
        if (!UPPER)
        {
            for (int c = 0; c < nb; c++)
            {
                const u32 p0 = ptr0(R.dptr, c), p1 = R.dptr[c + 1];
                if (p0 == p1)
                    continue;
                const val_t xc = seg[c];
                for (u32 p = p0 + lane; p < p1; p += 64)
                    seg[R.didx[p]] = v_submul(seg[R.didx[p]], R.dval[p], xc);
                wave_lds_fence();
            }
        }
        else
        {
            for (int r = nb - 1; r >= 0; r--)
            {
                const u32 b = R.dptr[r], e = R.dptr[r + 1];
                if (b == e)
                    continue;
                val_t part = v_make(0);
                for (u32 p = b + 1 + lane; p < e; p += 64)
                    part = v_add(part, v_mul(R.dval[p], seg[R.didx[p]]));
                part = solve_group_sum<1>(part, 64);
                if (lane == 0)
                    seg[r] = v_div(v_sub(seg[r], part), solve_clamped_divisor(R.dval[b]));
                wave_lds_fence();
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += blockDim.x)
        xr[i] = seg[i];
}

