// pg_hip_launch_solve.h -- host side of the level-scheduled block solves on the device-resident factors: the descriptors of a
// sweep and their way up, which kernels a panel width and an nb get within the LDS budget, the launches of a level, of a panel and
// of the panels of a HOST buffer, and what the device-resident solve keeps between calls (SolveWorkspace, pack / unpack launches).
// The extern "C" operators that call this are in pg_hip_platform.hip.  Included inside its anonymous namespace, after the kernel
// headers (pg_hip_block_solve_multi.h, pg_hip_block_solve.h, pg_hip_solve_pack.h, pg_hip_factor_stats.h) and pg_hip_backend.h.
#pragma once

// A sweep's run-time mode (pg_hip_block_solve_multi.h): SOLVE_LOWER / SOLVE_UPPER, or SOLVE_UT / SOLVE_LT with SOLVE_CONJ added for A^H
inline int solve_mode_sweep(int mode) { return mode & 3; }
inline bool solve_mode_upper_half(int mode) { return solve_sweep_diag_first(solve_mode_sweep(mode)); }

// device-side descriptors of one sweep, appended to hr / hb: rows keep their order, the blocks of level l are
// hb[blk_level_ptr[l] .. blk_level_ptr[l + 1]) counted from the first block appended here.  `mode`: see above (a transposed
// sweep's rows are destination segments, blk_bcol its blocks' source segments: the descriptors are the same)
void append_solve_descriptors(int mode, const pangulu_hip_solve_sweep_t &sw, std::vector<SolveRowD> &hr, std::vector<SolveBlkD> &hb,
                              std::vector<size_t> &blk_level_ptr)
{
    const bool upper = solve_mode_upper_half(mode);
    const size_t r0 = hr.size(), b0 = hb.size();
    hr.resize(r0 + (size_t)sw.level_ptr[sw.nlevel]);
    blk_level_ptr.assign((size_t)sw.nlevel + 1, 0);
    for (size_t l = 0; l < (size_t)sw.nlevel; l++)
    {
        for (size_t r = (size_t)sw.level_ptr[l]; r < (size_t)sw.level_ptr[l + 1]; r++)
        {
            const pangulu_hip_solve_row_t &row = sw.rows[r];
            const slot_t *d = row.diag;
            SolveRowD &R = hr[r0 + r];
            R.brow = row.brow;
            R.nblk = row.nblk;
            R.first = hb.size() - b0;
            R.dptr = upper ? d->d_rowpointer : d->d_columnpointer;
            R.didx = upper ? d->d_columnindex : d->d_rowindex;
            R.dval = d->d_value;
            for (size_t b = 0; b < row.nblk; b++)
            {
                const slot_t *sb = sw.blk_slots[row.first + b];
                SolveBlkD D;
                D.cp = sb->d_columnpointer;
                D.ri = sb->d_rowindex;
                D.val = sb->d_value;
                D.bcol = sw.blk_bcol[row.first + b];
                D.brow = row.brow;
                hb.push_back(D);
            }
        }
        blk_level_ptr[l + 1] = hb.size() - b0;
    }
}

// The solve kernels allow themselves 96 KB of LDS.  PANGULU_HIP_SOLVE_CHUNKED=0, or an nb at which not even one chunk column of a
// diagonal half fits beside the segment, leaves the column-by-column kernels of pg_hip_block_solve.h, which take single vectors.
constexpr size_t SOLVE_LDS_BUDGET = (size_t)96 << 10;
bool solve_by_column(size_t nb)
{
    static const bool chunked_on = !(getenv("PANGULU_HIP_SOLVE_CHUNKED") && atoi(getenv("PANGULU_HIP_SOLVE_CHUNKED")) == 0);
    return !chunked_on || solve_multi_chunk(nb, 1, SOLVE_LDS_BUDGET) < 1;
}
// the widest panel: a tile row of at most 128 bytes (16 real values, 8 double-complex ones), and both kernels within the budget
int solve_widest_panel(size_t nb)
{
    if (solve_by_column(nb))
        return 1;
    int wmax = (int)std::min<size_t>(16, 128 / sizeof(val_t));
    while (wmax > 1 && (solve_multi_lds_gather(nb, wmax) > SOLVE_LDS_BUDGET || solve_multi_chunk(nb, wmax, SOLVE_LDS_BUDGET) < 1))
        wmax >>= 1;
    return wmax;
}
// The widths of an operator's panels: each a power of two up to wmax, or the process ends with the operator's name in the message.
// Returns the number of columns they hold.
pangulu_uint64_t solve_checked_panel_widths(const char *op, int nb, int wmax, size_t npanel, const int *w)
{
    pangulu_uint64_t held = 0;
    for (size_t p = 0; p < npanel; p++)
    {
        if (w[p] < 1 || w[p] > wmax || (w[p] & (w[p] - 1)))
        {
            fprintf(stderr, "[PanguLU-AMD ERROR] %s: panel width %d (nb = %d takes powers of two up to %d)\n", op, w[p], nb, wmax);
            exit(EXIT_FAILURE);
        }
        held += (pangulu_uint64_t)w[p];
    }
    return held;
}
// SOLVE_CONJ on top of the transposed sweeps' modes for A^H, or 0
inline int solve_conj_mode(bool conjugate)
{
#ifdef PANGULU_COMPLEX
    return conjugate ? SOLVE_CONJ : 0;
#else
    (void)conjugate; // (real values: A^H = A^T)
    return 0;
#endif
}
// a panel width solve_widest_panel() allows, as the compile-time W of the kernels: f(std::integral_constant<int, W>())
template <class F>
void solve_with_panel_width(int w, F &&f)
{
    switch (w)
    {
    case 1:
        return f(std::integral_constant<int, 1>());
    case 2:
        return f(std::integral_constant<int, 2>());
    case 4:
        return f(std::integral_constant<int, 4>());
    case 8:
        return f(std::integral_constant<int, 8>());
    default:
        return f(std::integral_constant<int, 16>());
    }
}

// what one sweep of a solve has on the device: its rows and blocks start at row0 / blk0 of the descriptor arrays it shares with the
// other sweep; the rows of level l are level_ptr[l] .. level_ptr[l + 1] (a copy: a workspace outlives the host's description)
struct SolveSweepD
{
    int mode; // SOLVE_LOWER / SOLVE_UPPER, or a transposed mode
    std::vector<pangulu_uint64_t> level_ptr;
    size_t row0, blk0;
    std::vector<size_t> blk_level_ptr;
};

// lets one kernel instantiation ask for `lds` bytes of dynamic LDS; each instantiation remembers the most it has been granted
template <auto KERNEL>
void solve_allow_lds(size_t lds)
{
    static size_t allowed = 0;
    if (lds > allowed)
    {
        HIP_CHECK(hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        allowed = lds;
    }
}

// one level of one sweep on a panel of W right-hand sides: the gather over the level's nbl blocks, then the diagonal halves of its n segments
// repro_part (single vectors only): the reproducible gather pair into that buffer of nbl x nb values instead of the atomic gather;
// level_first: the level's first block counted from the sweep's first
template <int SWEEP, int W, bool CONJ>
void launch_solve_level_as(int nb, int ch, size_t nbl, size_t n, const SolveBlkD *blks, const SolveRowD *rows, val_t *d_x, val_t *repro_part = nullptr,
                           size_t level_first = 0)
{
    const size_t lds_level = solve_multi_lds_level((size_t)nb, W, ch);
    if (W == 1 && repro_part)
    {
        constexpr bool TRANS = solve_sweep_transposed(SWEEP);
        const size_t lds_gather = solve_repro_lds_gather((size_t)nb);
        solve_allow_lds<solve_gather_part_kernel<TRANS, CONJ>>(lds_gather);
        if (nbl)
        {
            hipLaunchKernelGGL((solve_gather_part_kernel<TRANS, CONJ>), dim3((unsigned)nbl), dim3(256), lds_gather, B.stream, blks, nb, d_x, repro_part);
            hipLaunchKernelGGL(solve_gather_sum_kernel, dim3((unsigned)n), dim3(256), 0, B.stream, rows, (unsigned long long)level_first, nb, repro_part, d_x);
        }
    }
    else if constexpr (solve_sweep_transposed(SWEEP))
    {
        const size_t lds_gather = solve_trans_lds_gather((size_t)nb, W);
        solve_allow_lds<block_trsm_gather_trans_kernel<W, CONJ>>(lds_gather);
        if (nbl)
            hipLaunchKernelGGL((block_trsm_gather_trans_kernel<W, CONJ>), dim3((unsigned)nbl), dim3(256), lds_gather, B.stream, blks, nb, d_x);
    }
    else
    {
        const size_t lds_gather = solve_multi_lds_gather((size_t)nb, W);
        solve_allow_lds<block_trsm_gather_multi_kernel<W>>(lds_gather);
        if (nbl)
            hipLaunchKernelGGL(block_trsm_gather_multi_kernel<W>, dim3((unsigned)nbl), dim3(256), lds_gather, B.stream, blks, nb, d_x);
    }
    solve_allow_lds<block_trsm_level_kernel<SWEEP, W, CONJ>>(lds_level);
    hipLaunchKernelGGL((block_trsm_level_kernel<SWEEP, W, CONJ>), dim3((unsigned)n), dim3(256), lds_level, B.stream, rows, nb, d_x, ch);
}

// the same for a run-time mode.  by_column: the column-by-column pair of pg_hip_block_solve.h (single vectors, untransposed sweeps: the
// operator offers no transposed sweep where that pair would run)
template <int W>
void launch_solve_level(int mode, bool by_column, int nb, int ch, size_t nbl, size_t n, const SolveBlkD *blks, const SolveRowD *rows, val_t *d_x,
                        val_t *repro_part = nullptr, size_t level_first = 0)
{
    if (by_column)
    {
        const size_t lds = sizeof(val_t) * (size_t)nb;
        if (nbl)
            hipLaunchKernelGGL(block_trsv_gather_kernel, dim3((unsigned)nbl), dim3(256), 0, B.stream, blks, nb, d_x);
        if (solve_mode_sweep(mode) == SOLVE_UPPER)
            hipLaunchKernelGGL(block_trsv_level_kernel<true>, dim3((unsigned)n), dim3(64), lds, B.stream, rows, nb, d_x);
        else
            hipLaunchKernelGGL(block_trsv_level_kernel<false>, dim3((unsigned)n), dim3(64), lds, B.stream, rows, nb, d_x);
        return;
    }
    switch (mode)
    {
    case SOLVE_LOWER:
        return launch_solve_level_as<SOLVE_LOWER, W, false>(nb, ch, nbl, n, blks, rows, d_x, repro_part, level_first);
    case SOLVE_UPPER:
        return launch_solve_level_as<SOLVE_UPPER, W, false>(nb, ch, nbl, n, blks, rows, d_x, repro_part, level_first);
    case SOLVE_UT:
        return launch_solve_level_as<SOLVE_UT, W, false>(nb, ch, nbl, n, blks, rows, d_x, repro_part, level_first);
    case SOLVE_LT:
        return launch_solve_level_as<SOLVE_LT, W, false>(nb, ch, nbl, n, blks, rows, d_x, repro_part, level_first);
#ifdef PANGULU_COMPLEX // (real builds: A^H is A^T, the operator never adds SOLVE_CONJ)
    case SOLVE_UT | SOLVE_CONJ:
        return launch_solve_level_as<SOLVE_UT, W, true>(nb, ch, nbl, n, blks, rows, d_x, repro_part, level_first);
    case SOLVE_LT | SOLVE_CONJ:
        return launch_solve_level_as<SOLVE_LT, W, true>(nb, ch, nbl, n, blks, rows, d_x, repro_part, level_first);
#endif
    }
}

// the launches of one panel of W right-hand sides in d_x: the sweeps one after the other, a gather and a level launch per level
template <int W>
void launch_solve_panel(int nb, const std::vector<SolveSweepD> &sweeps, int conj, const SolveRowD *d_rows, const SolveBlkD *d_blks, val_t *d_x,
                        val_t *repro_part = nullptr)
{
    const bool by_column = W == 1 && solve_by_column((size_t)nb);
    const int ch = by_column ? 0 : solve_multi_chunk((size_t)nb, W, SOLVE_LDS_BUDGET);
    for (const SolveSweepD &S : sweeps)
        for (size_t l = 0; l + 1 < S.level_ptr.size(); l++)
        {
            const pangulu_uint64_t *lp = S.level_ptr.data();
            const size_t n = (size_t)(lp[l + 1] - lp[l]), nbl = S.blk_level_ptr[l + 1] - S.blk_level_ptr[l];
            if (!n)
                continue;
            const SolveBlkD *blks = d_blks + S.blk0 + S.blk_level_ptr[l];
            const SolveRowD *rows = d_rows + S.row0 + lp[l];
            launch_solve_level<W>(S.mode | conj, by_column, nb, ch, nbl, n, blks, rows, d_x, repro_part, S.blk_level_ptr[l]);
        }
}

// ... of a panel of w right-hand sides, w a width solve_widest_panel() allows.  conj: SOLVE_CONJ on top of the sweeps' (transposed) modes, or 0
void launch_solve_panel_of(int w, int nb, const std::vector<SolveSweepD> &sweeps, int conj, const SolveRowD *d_rows, const SolveBlkD *d_blks, val_t *d_x,
                           val_t *repro_part = nullptr)
{
    solve_with_panel_width(w, [&](auto width)
                           {
                               constexpr int W = decltype(width)::value;
                               launch_solve_panel<W>(nb, sweeps, conj, d_rows, d_blks, d_x, W == 1 ? repro_part : nullptr); // (the reproducible variant: single vectors)
                           });
    HIP_CHECK(hipGetLastError());
}

// What every solve on the device-resident factors does first, B.mutex held: whatever still writes factor records -- a held
// factorisation, the records stream, background updates -- is ordered before what B.stream gets next
void solve_join_factor_streams()
{
    flush_pending_getrf();
    HIP_CHECK(hipSetDevice(B.device));
    join_records(B.stream); // the sparse records of finished blocks are written on the records stream
    join_background(B.stream);
}

// The descriptors of the given sweeps (one, or the lower and then the upper one; or U^T and then L^T), one after the other in hr / hb
// (never empty afterwards: they are allocated as they are), and on their way up B.stream into two device arrays that
// alloc(&pointer, count) provides.  hr / hb are the host copies of what goes up: the caller keeps them until it has synchronised.
template <class Alloc>
void upload_solve_sweeps(const std::vector<const pangulu_hip_solve_sweep_t *> &sw, const std::vector<int> &mode, std::vector<SolveRowD> &hr,
                         std::vector<SolveBlkD> &hb, std::vector<SolveSweepD> &sweeps, SolveRowD **d_rows, SolveBlkD **d_blks, Alloc &&alloc)
{
    sweeps.assign(sw.size(), SolveSweepD());
    for (size_t s = 0; s < sw.size(); s++)
    {
        sweeps[s].mode = mode[s];
        sweeps[s].level_ptr.assign(sw[s]->level_ptr, sw[s]->level_ptr + sw[s]->nlevel + 1);
        sweeps[s].row0 = hr.size();
        sweeps[s].blk0 = hb.size();
        append_solve_descriptors(mode[s], *sw[s], hr, hb, sweeps[s].blk_level_ptr);
    }
    if (hr.empty())
        hr.resize(1);
    if (hb.empty())
        hb.resize(1);
    alloc(d_rows, hr.size());
    alloc(d_blks, hb.size());
    HIP_CHECK(hipMemcpyAsync(*d_rows, hr.data(), sizeof(SolveRowD) * hr.size(), hipMemcpyHostToDevice, B.stream));
    HIP_CHECK(hipMemcpyAsync(*d_blks, hb.data(), sizeof(SolveBlkD) * hb.size(), hipMemcpyHostToDevice, B.stream));
}

// The level-scheduled block triangular solve, both operators' body: the descriptors of the given sweeps (one, or the lower and then
// the upper one; or U^T and then L^T) go up once; the panels of the HOST buffer X (panel p: xlen x w[p] values, right-hand side fastest, w[p] a width
// solve_widest_panel() allows) then pass through one device buffer one after the other: upload, the sweeps, download.  Everything
// on the device is allocated for the call and freed at its end.
void block_solve_panels(int nb, const std::vector<const pangulu_hip_solve_sweep_t *> &sw, const std::vector<int> &mode, val_t *X, size_t xlen, size_t npanel,
                        const int *w)
{
    ensure_ready();
    std::lock_guard<std::mutex> g(B.mutex);
    solve_join_factor_streams();
    std::vector<SolveRowD> hr;
    std::vector<SolveBlkD> hb;
    std::vector<SolveSweepD> sweeps;
    SolveRowD *d_rows = nullptr;
    SolveBlkD *d_blks = nullptr;
    val_t *d_x = nullptr;
    const int wtop = *std::max_element(w, w + npanel);
    HIP_CHECK(hipMalloc((void **)&d_x, sizeof(val_t) * xlen * (size_t)wtop)); // (every allocation before the first copy is queued)
    upload_solve_sweeps(sw, mode, hr, hb, sweeps, &d_rows, &d_blks, [](auto **p, size_t count) { HIP_CHECK(hipMalloc((void **)p, sizeof(**p) * count)); });
    for (size_t p = 0; p < npanel; p++)
    {
        const size_t bytes = sizeof(val_t) * xlen * (size_t)w[p];
        HIP_CHECK(hipMemcpyAsync(d_x, X, bytes, hipMemcpyHostToDevice, B.stream));
        launch_solve_panel_of(w[p], nb, sweeps, 0, d_rows, d_blks, d_x);
        HIP_CHECK(hipMemcpyAsync(X, d_x, bytes, hipMemcpyDeviceToHost, B.stream));
        X += xlen * (size_t)w[p];
    }
    HIP_CHECK(hipStreamSynchronize(B.stream));
    HIP_CHECK(hipFree(d_rows));
    HIP_CHECK(hipFree(d_blks));
    HIP_CHECK(hipFree(d_x));
}

// What a handle's device-resident solves keep on the device between calls (pangulu_platform_0201001_block_trsm_multi_device): per
// direction ([0] A, [1] A^T and A^H) the descriptors of both sweeps and the index/scale maps, each built on first use, and one panel
// buffer.  The descriptors hold device addresses of block records: the host frees the workspace before the records change.
struct SolveWorkspace
{
    struct Direction
    {
        bool ready = false;
        std::vector<SolveSweepD> sweeps;
        SolveRowD *d_rows = nullptr;
        SolveBlkD *d_blks = nullptr;
        u32 *d_in_idx = nullptr, *d_out_idx = nullptr;
        double *d_s_in = nullptr, *d_s_out = nullptr;
    } dir[2];
    int nb = 0;
    size_t xlen = 0, n = 0;
    val_t *d_x = nullptr; // xlen x the widest panel
    // pangulu_platform_0201001_condest_vector: the workgroups' partials and the result of a step
    CondestPartialD *d_condest_part = nullptr;
    CondestResultD *d_condest_res = nullptr;
    // the reproducible single-vector solve: one nb-vector per block of the fullest level
    val_t *d_repro_part = nullptr;
    size_t repro_part_values = 0;
    hipEvent_t after_caller = nullptr;
    size_t bytes = 0;
};
size_t g_solve_workspace_bytes = 0; // (under B.mutex)

template <class T>
void solve_workspace_alloc(SolveWorkspace &ws, T **p, size_t count)
{
    HIP_CHECK(hipMalloc((void **)p, sizeof(T) * count));
    ws.bytes += sizeof(T) * count;
    g_solve_workspace_bytes += sizeof(T) * count;
}

void solve_workspace_release(SolveWorkspace *ws) // B.mutex held
{
    HIP_CHECK(hipSetDevice(B.device));
    HIP_CHECK(hipStreamSynchronize(B.stream));
    for (SolveWorkspace::Direction &D : ws->dir)
        for (void *p : {(void *)D.d_rows, (void *)D.d_blks, (void *)D.d_in_idx, (void *)D.d_out_idx, (void *)D.d_s_in, (void *)D.d_s_out})
            if (p)
                HIP_CHECK(hipFree(p));
    for (void *p : {(void *)ws->d_x, (void *)ws->d_condest_part, (void *)ws->d_condest_res, (void *)ws->d_repro_part})
        if (p)
            HIP_CHECK(hipFree(p));
    if (ws->after_caller)
        HIP_CHECK(hipEventDestroy(ws->after_caller));
    g_solve_workspace_bytes -= ws->bytes;
    delete ws;
}

// the handle's workspace for a system of these sizes, made when it is not there (B.mutex held)
SolveWorkspace *solve_workspace_of(void **workspace, int nb, size_t xlen, size_t n)
{
    SolveWorkspace *ws = (SolveWorkspace *)*workspace;
    if (ws && (ws->nb != nb || ws->xlen != xlen || ws->n != n))
    {
        solve_workspace_release(ws); // (another system behind the same pointer: start again)
        ws = nullptr;
    }
    if (!ws)
    {
        ws = new SolveWorkspace();
        ws->nb = nb;
        ws->xlen = xlen;
        ws->n = n;
        solve_workspace_alloc(*ws, &ws->d_x, xlen * (size_t)solve_widest_panel((size_t)nb));
        HIP_CHECK(hipEventCreateWithFlags(&ws->after_caller, hipEventDisableTiming));
        *workspace = ws;
    }
    return ws;
}

// true: [p, p + bytes) is device memory of the back-end's device.  Asked of the runtime on the host: no kernel sees a pointer that fails.
bool solve_pointer_on_device(const void *p, size_t bytes)
{
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof(attr));
    if (hipPointerGetAttributes(&attr, p) != hipSuccess)
    {
        (void)hipGetLastError(); // (an unregistered host pointer is reported as an error: not one of ours)
        return false;
    }
    if (attr.type != hipMemoryTypeDevice || attr.device != B.device)
        return false;
    void *base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange((hipDeviceptr_t *)&base, &size, (hipDeviceptr_t)p) != hipSuccess)
    {
        (void)hipGetLastError();
        return false;
    }
    return (const char *)p >= (const char *)base && (const char *)p + bytes <= (const char *)base + size;
}

// What pangulu_platform_0201001_values_refresh keeps on the device for a handle: the lists of pangulu_hip_values_map_t and the table of
// the arena's chunks.  They depend on the pattern and on where the records live, so they stay until the host releases them.
struct ValuesRefreshMapD
{
    unsigned long long *d_user_dst = nullptr, *d_const_dst = nullptr, *d_slice_off = nullptr;
    val_t *d_const_value = nullptr;
    u32 *d_slice_count = nullptr;
    val_t **d_chunks = nullptr;
    size_t nuser = 0, nconst = 0, nslice = 0, vpc = 0;
    int chunk_shift = -1; // vpc == 1 << chunk_shift, or -1
    unsigned ncu = 1;
    hipEvent_t after_caller = nullptr;
    size_t bytes = 0;
};
size_t g_values_refresh_bytes = 0; // (under B.mutex)

void values_refresh_map_release(ValuesRefreshMapD *D) // B.mutex held
{
    HIP_CHECK(hipSetDevice(B.device));
    HIP_CHECK(hipStreamSynchronize(B.stream));
    for (void *p : {(void *)D->d_user_dst, (void *)D->d_const_dst, (void *)D->d_slice_off, (void *)D->d_const_value, (void *)D->d_slice_count, (void *)D->d_chunks})
        if (p)
            HIP_CHECK(hipFree(p));
    if (D->after_caller)
        HIP_CHECK(hipEventDestroy(D->after_caller));
    g_values_refresh_bytes -= D->bytes;
    delete D;
}

// the handle's lists on the device, checked and uploaded when they are not there (B.mutex held).  Every place the kernels will write
// is checked against the arena here, on the host, once: no kernel sees a list that fails.
ValuesRefreshMapD *values_refresh_map_of(void **device_map, const pangulu_hip_values_map_t &M)
{
    if (*device_map)
        return (ValuesRefreshMapD *)*device_map;
    const unsigned long long vpc = M.values_per_chunk;
    bool ok = vpc > 0 && M.nchunk > 0 && M.chunks && M.arena_values <= M.nchunk * vpc && M.arena_values > (M.nchunk - 1) * vpc;
    for (unsigned long long c = 0; ok && c < M.nchunk; c++)
        ok = M.chunks[c] != nullptr;
    for (unsigned long long k = 0; ok && k < M.nuser; k++)
        ok = M.user_dst[k] < M.arena_values;
    for (unsigned long long k = 0; ok && k < M.nconst; k++)
        ok = M.const_dst[k] < M.arena_values;
    for (unsigned long long s = 0; ok && s < M.nslice; s++)
    {
        const unsigned long long o = M.slice_off[s], n = M.slice_count[s];
        ok = n > 0 && o < M.arena_values && n <= M.arena_values - o && o / vpc == (o + n - 1) / vpc && (o % vpc) * sizeof(val_t) % 16 == 0;
    }
    if (!ok)
    {
        fprintf(stderr, "[PanguLU-AMD ERROR] values_refresh: a destination outside the arena of %llu values in %llu chunks of %llu\n",
                (unsigned long long)M.arena_values, (unsigned long long)M.nchunk, vpc);
        exit(EXIT_FAILURE);
    }
    ValuesRefreshMapD *D = new ValuesRefreshMapD();
    D->nuser = (size_t)M.nuser;
    D->nconst = (size_t)M.nconst;
    D->nslice = (size_t)M.nslice;
    D->vpc = (size_t)vpc;
    if ((vpc & (vpc - 1)) == 0)
        for (D->chunk_shift = 0; (1ull << D->chunk_shift) != vpc; D->chunk_shift++)
        {
        }
    int ncu = 0;
    HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, B.device));
    D->ncu = (unsigned)std::max(ncu, 1);
    // (an empty list still gets an allocation: the kernels take the pointer and read nothing)
    auto up = [&](auto **p, const auto *src, size_t count)
    {
        const size_t bytes = sizeof(**p) * std::max<size_t>(count, 1);
        HIP_CHECK(hipMalloc((void **)p, bytes));
        D->bytes += bytes;
        g_values_refresh_bytes += bytes;
        if (count)
            HIP_CHECK(hipMemcpyAsync(*p, src, sizeof(**p) * count, hipMemcpyHostToDevice, B.stream));
    };
    up(&D->d_user_dst, M.user_dst, D->nuser);
    up(&D->d_const_dst, M.const_dst, D->nconst);
    up(&D->d_const_value, (const val_t *)M.const_value, D->nconst);
    up(&D->d_slice_off, M.slice_off, D->nslice);
    up(&D->d_slice_count, M.slice_count, D->nslice);
    up(&D->d_chunks, (val_t *const *)M.chunks, (size_t)M.nchunk);
    HIP_CHECK(hipStreamSynchronize(B.stream)); // (the caller's lists may go once this returns)
    HIP_CHECK(hipEventCreateWithFlags(&D->after_caller, hipEventDisableTiming));
    *device_map = D;
    return D;
}

// pack (into = true) or unpack a panel of w right-hand sides
void launch_solve_pack_of(int w, bool into, val_t *d_rhs, size_t ldb, u32 j0, u32 nc, const SolveWorkspace &ws, const SolveWorkspace::Direction &D)
{
    solve_with_panel_width(w, [&](auto width)
                           {
                               constexpr int W = decltype(width)::value;
                               if (into)
                                   hipLaunchKernelGGL(solve_pack_panel_kernel<W>, dim3(solve_pack_grid((unsigned long long)ws.xlen * W)), dim3(256), 0, B.stream,
                                                      d_rhs, (unsigned long long)ldb, j0, nc, D.d_in_idx, D.d_s_in, (u32)ws.n, (unsigned long long)ws.xlen, ws.d_x);
                               else
                                   hipLaunchKernelGGL(solve_unpack_panel_kernel<W>, dim3(solve_pack_grid((unsigned long long)ws.n * W)), dim3(256), 0, B.stream,
                                                      d_rhs, (unsigned long long)ldb, j0, nc, D.d_out_idx, D.d_s_out, (u32)ws.n, ws.d_x);
                           });
    HIP_CHECK(hipGetLastError());
}
