// pg_hip_block_solve_multi.h -- the device kernels of the level-scheduled block triangular solve: a PANEL of W right-hand sides per
// launch, W = 1 for pangulu_gstrs and up to 16 for pangulu_amd_gstrs_multi (pangulu_platform_0201001_block_trsv and
// ..._block_trsm_multi launch the same instances), and the same for the TRANSPOSED solve, A^T X = B and A^H X = B, on the records of
// A = L U as they lie in HBM (pangulu_platform_0201001_block_trsm_multi_trans); and the descriptors SolveBlkD / SolveRowD that every
// solve kernel reads.  Included inside the anonymous namespace of pg_hip_platform.hip, before pg_hip_block_solve.h (the
// column-by-column kernels of PANGULU_HIP_SOLVE_CHUNKED=0) and pg_hip_launch_solve.h (the host side).
#pragma once

// One off-diagonal block and one segment (block row, or destination segment of a transposed sweep) with its diagonal half, as the
// kernels of a level read them.  They hold device addresses of the block records.
struct SolveBlkD
{
    const u32 *cp; // CSC
    const u16 *ri;
    const val_t *val;
    u32 bcol;
    u32 brow; // destination segment
};
struct SolveRowD
{
    u32 brow, nblk;
    unsigned long long first; // into the SolveBlkD array
    const u32 *dptr;          // diagonal half: lower = strictly-lower CSC column pointer, upper = CSR row pointer (diagonal first)
    const u16 *didx;
    const val_t *dval;
};


// -----------------------------------------------------------------------------------------------------------------
// Round 4: two launches per level, built around where the column-by-column kernels' time went (fem27(112): 540 launches, 394 ms).
// That gather kernel walks a block column by column, sixteen lanes a column, every entry a floating-point atomic on the row's
// 256 words in HBM (hundreds of blocks of a row near the root contend for them): 98 % of its wave cycles waiting.  That level
// kernel sweeps a diagonal half column by column straight from HBM: nb dependent round trips.
//  * gather: the block's entries flat over the workgroup (coalesced loads, the column of an entry by bisection in an LDS copy of the
//    column pointers), products accumulated in LDS (ds_add_f64), ONE global atomic per touched row of the segment at the end;
//  * level: the diagonal half streams through LDS in chunks of `ch` records, double-buffered: three wavefronts fetch chunk k + 1
//    while the first one sweeps chunk k out of LDS -- a dependent step costs LDS round trips, not HBM ones.
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
//
// The four sweeps.  A x = b is a forward sweep with L, then a backward one with U; A^T = U^T L^T is a forward sweep with U^T, then a
// backward one with L^T, on the same records read "the other way round".  The lower half of a diagonal block is strictly-lower CSC,
// unit diagonal, colptr[0] read as 0; the upper half is CSR with the diagonal first.  Record c of either half is walked in one of two
// ways, and the level kernel is those two steps times "does the record carry its diagonal first":
//
//   sweep        records      step                                                        diagonal in record
//   SOLVE_LOWER  ascending    scatter: x[idx[p]] -= op(val[p]) x[c]                       no  (unit)
//   SOLVE_UT     ascending    scatter, after x[c] /= op(d_c)                              yes
//   SOLVE_UPPER  descending   dot:     x[c] = (x[c] - sum_p op(val[p]) x[idx[p]]) / d_c   yes
//   SOLVE_LT     descending   dot:     x[c] -= sum_p op(val[p]) x[idx[p]]                 no  (unit)
//
// A scatter goes into distinct rows: plain LDS read-modify-write.  A dot is a lane-group partial sum per right-hand side with a
// shuffle reduction.  d_c is divided by under the PANGULU_SPTRSV_TOL clamp (solve_clamped_divisor); an empty record is skipped, and
// x[c] stays.  op() conjugates for A^H (CONJ: the transposed sweeps of complex builds only).
//
// The transposed gather: segment i receives -op(B)^T x_k from the block B = A(k, i) of its own block COLUMN.  B is stored CSC, so the
// entries that add into one destination value are the contiguous entries of one column: a dot product, not a scatter.  Swapping row
// and column in the flat loop of block_trsm_gather_multi_kernel would send the LDS atomics of a wavefront step to the same word.
// There LANE GROUPS OWN COLUMNS: a group of g entry slots x W lanes walks one column, sums by shuffle and issues the column's one
// global atomic per right-hand side; no LDS atomics, no accumulator tile, no bisection.  g is the power of two next above the block's
// mean column length (uniform per workgroup), so that short columns of a sparse block do not idle a whole wavefront; neighbouring
// groups take neighbouring columns, which keeps a wavefront's loads on one contiguous stretch of the record.  It needs one tile and
// the column pointers, less than solve_multi_lds_gather: solve_widest_panel() holds for both directions.
// -----------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int solve_multi_pitch(int w) { return w > 1 ? w + 1 : 1; }

// What a sweep does with its records (the table above).  A run-time mode is one of the four sweeps, plus SOLVE_CONJ for A^H.
enum
{
    SOLVE_LOWER = 0,
    SOLVE_UPPER = 1,
    SOLVE_UT = 2,
    SOLVE_LT = 3,
    SOLVE_CONJ = 4
};
__host__ __device__ constexpr bool solve_sweep_dot(int sweep) { return sweep == SOLVE_UPPER || sweep == SOLVE_LT; }        // dot step, records descending
__host__ __device__ constexpr bool solve_sweep_diag_first(int sweep) { return sweep == SOLVE_UPPER || sweep == SOLVE_UT; } // the upper halves
__host__ __device__ constexpr bool solve_sweep_transposed(int sweep) { return sweep == SOLVE_UT || sweep == SOLVE_LT; }

template <bool CONJ>
__host__ __device__ inline val_t solve_trans_op(val_t v)
{
    if constexpr (CONJ)
        return v_conj(v);
    else
        return v;
}

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
            part = v_add(part, v_mul(solve_trans_op<CONJ>(B.val[p]), xs[B.ri[p] * P + r]));
        part = solve_group_sum<W>(part, span);
        if (slot == 0 && p0 != p1)
            v_atomic_add(&xdst[c * W + r], v_sub(v_make(0), part));
    }
}

// -----------------------------------------------------------------------------------------------------------------
// The REPRODUCIBLE gather for single vectors (pangulu_amd_rcond: the same factors and the same vector must give the same bits).  The
// two kernels above leave the order of their sums to the hardware: LDS atomics inside a block, one global atomic per block and row
// across the blocks of a segment.  Here nothing is added by an atomic:
//  * solve_gather_part_kernel, one workgroup per block: the block's contribution -B x_src (or -op(B)^T x_src) as nb values of its own
//    in `part`, every one of them written.  Transposed: the lane groups' dots of the kernel above, stored instead of added.
//    Untransposed: a scatter -- wavefront w takes the columns c = w, w + 4, ... one after the other into a tile of its own (the entries
//    of one column go to distinct rows: plain read-modify-write, columns in ascending order), and the four tiles are added in
//    wavefront order;
//  * solve_gather_sum_kernel, one workgroup per segment of the level: x_row += part of its blocks, in the order of the descriptor list.
// The level kernel that follows sweeps a diagonal half with one wavefront and shuffle sums in a fixed pattern: reproducible as it is.
// Twice the launches of the atomic pair and nb values of traffic per block each way: only where reproducibility is asked for.
// -----------------------------------------------------------------------------------------------------------------
inline size_t solve_repro_lds_gather(size_t nb) { return 5 * sizeof(val_t) * nb + sizeof(u32) * (nb + 1); }

template <bool TRANS, bool CONJ>
__global__ __launch_bounds__(256) void solve_gather_part_kernel(const SolveBlkD *__restrict__ blks, int nb, const val_t *__restrict__ x,
                                                                val_t *__restrict__ part)
{
    extern __shared__ __align__(16) unsigned char smem_raw[];
    val_t *xs = reinterpret_cast<val_t *>(smem_raw);
    val_t *acc = xs + nb; // untransposed: four tiles of nb values
    u32 *cp = reinterpret_cast<u32 *>(xs + (size_t)5 * nb);
    const SolveBlkD B = blks[blockIdx.x];
    const val_t *xsrc = x + (size_t)B.bcol * nb;
    val_t *out = part + (size_t)blockIdx.x * nb;
    const int tid = threadIdx.x;
    for (int k = tid; k < nb; k += 256)
        xs[k] = xsrc[k];
    for (int i = tid; i <= nb; i += 256)
        cp[i] = i == 0 ? 0u : B.cp[i];
    if constexpr (!TRANS)
        for (int k = tid; k < 4 * nb; k += 256)
            acc[k] = v_make(0);
    __syncthreads();
    if constexpr (TRANS)
    {
        const int g = solve_trans_group_slots(cp[nb], nb, 1); // uniform over the workgroup
        const int ngroup = 256 / g;
        const int group = tid / g, slot = tid % g;
        for (int c0 = 0; c0 < nb; c0 += ngroup) // (uniform trip count: the shuffles below are executed by whole wavefronts)
        {
            const int c = c0 + group;
            val_t sum = v_make(0);
            u32 p0 = 0, p1 = 0;
            if (c < nb)
            {
                p0 = cp[c];
                p1 = cp[c + 1];
            }
            for (u32 p = p0 + (u32)slot; p < p1; p += (u32)g)
                sum = v_add(sum, v_mul(solve_trans_op<CONJ>(B.val[p]), xs[B.ri[p]]));
            sum = solve_group_sum<1>(sum, g);
            if (slot == 0 && c < nb)
                out[c] = v_sub(v_make(0), sum);
        }
    }
    else
    {
        const int wave = tid >> 6, lane = tid & 63;
        val_t *mine = acc + (size_t)wave * nb;
        for (int c = wave; c < nb; c += 4)
        {
            const u32 p0 = cp[c], p1 = cp[c + 1];
            if (p0 == p1)
                continue; // (uniform over the wavefront)
            const val_t xc = xs[c];
            for (u32 p = p0 + (u32)lane; p < p1; p += 64)
            {
                val_t *d = &mine[B.ri[p]];
                *d = v_submul(*d, B.val[p], xc);
            }
            wave_lds_fence();
        }
        __syncthreads();
        for (int i = tid; i < nb; i += 256)
            out[i] = v_add(v_add(v_add(acc[i], acc[nb + i]), acc[2 * nb + i]), acc[3 * nb + i]);
    }
}

// rows[blockIdx.x].first counts from the sweep's first block, `level_first` is the level's first block counted the same way, and
// `part` holds the level's blocks from 0
__global__ __launch_bounds__(256) void solve_gather_sum_kernel(const SolveRowD *__restrict__ rows, unsigned long long level_first, int nb,
                                                               const val_t *__restrict__ part, val_t *__restrict__ x)
{
    const SolveRowD R = rows[blockIdx.x];
    val_t *xr = x + (size_t)R.brow * nb;
    const val_t *first = part + (size_t)(R.first - level_first) * nb;
    for (int i = threadIdx.x; i < nb; i += 256)
    {
        val_t s = xr[i];
        for (u32 b = 0; b < R.nblk; b++)
            s = v_add(s, first[(size_t)b * nb + i]);
        xr[i] = s;
    }
}

// One record of a diagonal half out of its chunk in LDS (the table above), by the sweeping wavefront: record c is bv / bi[ptr[c] - base
// .. ptr[c + 1] - base), lane = entry slot `eslot` x right-hand side `r`.  (A function of values, not a lambda over the kernel's
// locals: the compiler then keeps what does not depend on c out of the record loop, as it did in a loop written out per sweep.)
template <int SWEEP, int W, bool CONJ>
__device__ inline void solve_level_step(int c, const u32 *ptr, u32 base, const val_t *bv, const u16 *bi, val_t *seg, int lane, int eslot, int r)
{
    constexpr bool DOT = solve_sweep_dot(SWEEP), DIAG = solve_sweep_diag_first(SWEEP);
    constexpr int P = solve_multi_pitch(W);
    const u32 b = ptr[c] - base, e = ptr[c + 1] - base;
    if (b == e)
        return;
    const u32 first = b + (DIAG ? 1 : 0) + eslot; // this lane's first entry past the diagonal
    if constexpr (!DOT)
    {
        if constexpr (DIAG)
        {
            if (lane < W)
                seg[c * P + lane] = v_div(seg[c * P + lane], solve_clamped_divisor(solve_trans_op<CONJ>(bv[b])));
            wave_lds_fence();
        }
        const val_t xc = seg[c * P + r];
        for (u32 p = first; p < e; p += 64 / W)
        {
            val_t *d = &seg[bi[p] * P + r];
            *d = v_submul(*d, solve_trans_op<CONJ>(bv[p]), xc);
        }
    }
    else
    {
        // each lane group accumulates its partial dot for its right-hand side; lanes 0 .. W - 1 end up with the sums
        val_t part = v_make(0);
        for (u32 p = first; p < e; p += 64 / W)
            part = v_add(part, v_mul(solve_trans_op<CONJ>(bv[p]), seg[bi[p] * P + r]));
        part = solve_group_sum<W>(part, 64);
        if (lane < W)
        {
            const val_t num = v_sub(seg[c * P + lane], part);
            if constexpr (DIAG)
                seg[c * P + lane] = v_div(num, solve_clamped_divisor(solve_trans_op<CONJ>(bv[b])));
            else
                seg[c * P + lane] = num;
        }
    }
    wave_lds_fence();
}

// The diagonal halves of the level's segments, any of the four sweeps: one workgroup per segment, the nb x W segment in LDS, the
// diagonal half streamed through LDS in double-buffered chunks of `ch` records -- three wavefronts fetch chunk k + 1 while the
// first one sweeps chunk k.  A wavefront step is 64 / W entries x W right-hand sides.
template <int SWEEP, int W, bool CONJ>
__global__ __launch_bounds__(256) void block_trsm_level_kernel(const SolveRowD *__restrict__ rows, int nb, val_t *__restrict__ x, int ch)
{
    static_assert(!CONJ || solve_sweep_transposed(SWEEP), "only the transposed sweeps conjugate");
    constexpr bool DOT = solve_sweep_dot(SWEEP), DIAG = solve_sweep_diag_first(SWEEP);
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
        ptr[i] = (!DIAG && i == 0) ? 0u : R.dptr[i];
    __syncthreads();
    const int nchunk = (nb + ch - 1) / ch;
    // chunk k: records [k ch, (k + 1) ch) in ascending order for the scatters; records [nb - (k + 1) ch, nb - k ch), descending, for the dots
    auto lo_of = [&](int k) -> int { return DOT ? max(0, nb - (k + 1) * ch) : k * ch; };
    auto hi_of = [&](int k) -> int { return DOT ? nb - k * ch : min(nb, (k + 1) * ch); };
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
            if constexpr (DOT)
                for (int c = c1 - 1; c >= c0; c--)
                    solve_level_step<SWEEP, W, CONJ>(c, ptr, base, bv, bi, seg, lane, eslot, r);
            else
                for (int c = c0; c < c1; c++)
                    solve_level_step<SWEEP, W, CONJ>(c, ptr, base, bv, bi, seg, lane, eslot, r);
        }
        __syncthreads();
    }
    for (int k = tid; k < nb * W; k += 256)
        xr[k] = seg[(k / W) * P + k % W];
}

// LDS demand of the kernels for a panel of w right-hand sides (the transposed gather: never more than solve_multi_lds_gather), and
// the chunk depth the level kernel gets out of `budget` bytes (at most 16 records; 0: not even one fits beside the segment)
inline size_t solve_multi_lds_gather(size_t nb, int w)
{
    return 2 * sizeof(val_t) * nb * (size_t)solve_multi_pitch(w) + sizeof(u32) * (nb + 1) + sizeof(u32) * nb;
}
inline size_t solve_trans_lds_gather(size_t nb, int w)
{
    return sizeof(val_t) * nb * (size_t)solve_multi_pitch(w) + sizeof(u32) * (nb + 1);
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
