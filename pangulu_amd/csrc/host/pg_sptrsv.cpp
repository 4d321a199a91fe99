// pg_sptrsv.cpp -- block forward/backward substitution for pangulu_gstrs ("next" row f1 of SURVEY.md §8).
//
// Same sweep as the reference (src/pangulu_sptrsv.c:24-191): block row by block row, every rank that owns
// blocks of the row (the diagonal owner's process row, or any rank under the subtree mapping) adds their products, the diagonal owner sums the partial
// vectors, solves with its diagonal half and broadcasts the finished segment.  Like the reference (which pins
// the solve to PANGULU_PLATFORM_CPU_NAIVE, src/pangulu_sptrsv.c:62,94,126,159) it runs on the host copies of
// the factors; the in-block kernels follow ...0100000.c:435-506.
#include <cmath>

#include "pg_host.h"

namespace pg
{

namespace
{

#ifdef PANGULU_COMPLEX
inline val_t vmul(val_t a, val_t b) { return val_t{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
inline val_t vsub(val_t a, val_t b) { return val_t{a.re - b.re, a.im - b.im}; }
inline val_t vadd(val_t a, val_t b) { return val_t{a.re + b.re, a.im + b.im}; }
inline val_t vdiv(val_t a, val_t b)
{
    calculate_real_type d = b.re * b.re + b.im * b.im;
    return val_t{(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
inline double vreal(val_t a) { return (double)a.re; }
inline val_t vmake(double r) { return val_t{(calculate_real_type)r, 0}; }
inline val_t vop(val_t a, bool conj) { return conj ? val_t{a.re, -a.im} : a; }
#else
inline val_t vmul(val_t a, val_t b) { return a * b; }
inline val_t vsub(val_t a, val_t b) { return a - b; }
inline val_t vadd(val_t a, val_t b) { return a + b; }
inline val_t vdiv(val_t a, val_t b) { return a / b; }
inline double vreal(val_t a) { return (double)a; }
inline val_t vmake(double r) { return (val_t)r; }
inline val_t vop(val_t a, bool) { return a; }
#endif

// y -= A x for a CSC block
void block_spmv(u32 nb, const slot_t *a, const val_t *x, val_t *y)
{
    for (u32 c = 0; c < nb; c++)
    {
        val_t xc = x[c];
        for (u32 p = a->columnpointer[c]; p < a->columnpointer[c + 1]; p++)
            y[a->rowindex[p]] = vsub(y[a->rowindex[p]], vmul(a->value[p], xc));
    }
}

void block_lower_solve(u32 nb, const slot_t *l, val_t *x)
{
    for (u32 c = 0; c < nb; c++)
    {
        val_t xc = x[c];
        for (u32 p = l->columnpointer[c]; p < l->columnpointer[c + 1]; p++)
            x[l->rowindex[p]] = vsub(x[l->rowindex[p]], vmul(l->value[p], xc));
    }
}

void block_upper_solve(u32 nb, const slot_t *u, val_t *x)
{
    for (i64 r = (i64)nb - 1; r >= 0; r--)
    {
        u32 b = u->columnpointer[r], e = u->columnpointer[r + 1];
        if (b == e)
            continue;
        val_t acc = x[r];
        for (u32 p = b + 1; p < e; p++)
            acc = vsub(acc, vmul(u->value[p], x[u->rowindex[p]]));
        val_t d = u->value[b];
        x[r] = (std::fabs(vreal(d)) > PANGULU_SPTRSV_TOL) ? vdiv(acc, d) : vdiv(acc, vmake(PANGULU_SPTRSV_TOL));
    }
}

// The in-block routines of the transposed sweeps; op() conjugates for A^H.
// y -= op(A)^T x for a CSC block: column c of A is row c of A^T
void block_spmv_trans(u32 nb, const slot_t *a, const val_t *x, val_t *y, bool conj)
{
    for (u32 c = 0; c < nb; c++)
    {
        val_t acc = y[c];
        for (u32 p = a->columnpointer[c]; p < a->columnpointer[c + 1]; p++)
            acc = vsub(acc, vmul(vop(a->value[p], conj), x[a->rowindex[p]]));
        y[c] = acc;
    }
}

// forward solve with op(U)^T from the CSR record of U (diagonal first): row r of U is column r of U^T
void block_upper_trans_solve(u32 nb, const slot_t *u, val_t *x, bool conj)
{
    for (u32 r = 0; r < nb; r++)
    {
        u32 b = u->columnpointer[r], e = u->columnpointer[r + 1];
        if (b == e)
            continue;
        val_t d = vop(u->value[b], conj);
        val_t xr = (std::fabs(vreal(d)) > PANGULU_SPTRSV_TOL) ? vdiv(x[r], d) : vdiv(x[r], vmake(PANGULU_SPTRSV_TOL));
        x[r] = xr;
        for (u32 p = b + 1; p < e; p++)
            x[u->rowindex[p]] = vsub(x[u->rowindex[p]], vmul(vop(u->value[p], conj), xr));
    }
}

// backward solve with op(L)^T (unit diagonal) from the strictly-lower CSC record of L: column c of L is row c of L^T
void block_lower_trans_solve(u32 nb, const slot_t *l, val_t *x, bool conj)
{
    for (i64 c = (i64)nb - 1; c >= 0; c--)
    {
        val_t acc = x[c];
        for (u32 p = l->columnpointer[c]; p < l->columnpointer[c + 1]; p++)
            acc = vsub(acc, vmul(vop(l->value[p], conj), x[l->rowindex[p]]));
        x[c] = acc;
    }
}

} // namespace

// One of the four sweeps of a solve -- L then U for A x = b, U^T then L^T for A^T x = b / A^H x = b -- as what it reads of the block
// pattern.  Segment i of the vector receives the products of the blocks at the pattern positions begin[i] .. end[i]; position r is
// block (i, neighbour[r]) of the block-CSR side (L, U) and reads segment neighbour[r], block (neighbour[r], i) of the block-CSC side
// (U^T, L^T: block row i of U^T is block column i of U, so segment i reads the segments k < i of the blocks A(k, i), and with L^T
// the segments k > i).  Then the diagonal owner solves with diag[i].
struct SweepShape
{
    const u64 *begin, *end;   // per segment: pointers into BlockPattern (`end` possibly + 1)
    const u32 *neighbour;     // colidx or rowidx
    const u64 *to_block;      // position -> index of slot_of: csr_to_csc on the block-CSR side, nullptr (the position itself) on the block-CSC side
    slot_t *const *diag;      // diag_lower or diag_upper
    bool ascending;           // segments 0 .. nbk-1, or nbk-1 .. 0
    u64 block_of(u64 r) const { return to_block ? to_block[r] : r; }
    int owner_of(const Solver &S, u32 i, u64 r) const { return to_block ? S.owner(i, neighbour[r]) : S.owner(neighbour[r], i); }
    u32 segment_at(u32 step, u32 nbk) const { return ascending ? step : nbk - 1 - step; }
};

static SweepShape sweep_shape(const Solver &S, bool transposed, int sweep)
{
    const BlockPattern &P = S.pat;
    if (!transposed)
        return sweep == 0 ? SweepShape{P.rowptr.data(), P.first_after_diag_csr.data(), P.colidx.data(), P.csr_to_csc.data(), S.diag_lower.data(), true}
                          : SweepShape{P.first_after_diag_csr.data(), P.rowptr.data() + 1, P.colidx.data(), P.csr_to_csc.data(), S.diag_upper.data(), false};
    return sweep == 0 ? SweepShape{P.colptr.data(), P.first_after_diag.data(), P.rowidx.data(), nullptr, S.diag_upper.data(), true}
                      : SweepShape{P.first_after_diag.data(), P.colptr.data() + 1, P.rowidx.data(), nullptr, S.diag_lower.data(), false};
}

// The level structure of one sweep of the device solve: a pure function of the block pattern (and of the slots the records sit in).
// `brow` of a row is the destination segment i, blk_bcol the source segment, `diag` the sweep's diagonal half.
static void build_sweep_plan(const Solver &S, const SweepShape &sweep, SolveSweepPlan &plan)
{
    const u32 nbk = S.nbk;
    // level of a segment = 1 + the highest level among the segments its off-diagonal blocks (on the sweep's side) read
    std::vector<u32> level(nbk, 0);
    u32 nlevel = 0;
    for (u32 step = 0; step < nbk; step++)
    {
        const u32 i = sweep.segment_at(step, nbk);
        u32 lv = 0;
        for (u64 r = sweep.begin[i]; r < sweep.end[i]; r++)
            lv = std::max(lv, level[sweep.neighbour[r]] + 1);
        level[i] = lv;
        nlevel = std::max(nlevel, lv + 1);
    }
    plan.nlevel = nlevel;
    plan.level_ptr.assign((size_t)nlevel + 1, 0);
    for (u32 k = 0; k < nbk; k++)
        plan.level_ptr[level[k] + 1]++;
    for (u32 l = 0; l < nlevel; l++)
        plan.level_ptr[l + 1] += plan.level_ptr[l];
    plan.rows.assign(nbk, pangulu_hip_solve_row_t());
    plan.blk_slots.clear();
    plan.blk_bcol.clear();
    std::vector<pangulu_uint64_t> cur(plan.level_ptr.begin(), plan.level_ptr.end() - 1);
    for (u32 i = 0; i < nbk; i++)
    {
        pangulu_hip_solve_row_t R;
        R.brow = i;
        R.first = plan.blk_slots.size();
        R.diag = sweep.diag[i];
        for (u64 r = sweep.begin[i]; r < sweep.end[i]; r++)
        {
            plan.blk_slots.push_back(S.slot_of[sweep.block_of(r)]);
            plan.blk_bcol.push_back(sweep.neighbour[r]);
        }
        R.nblk = (pangulu_exblock_idx)(plan.blk_slots.size() - R.first);
        plan.rows[cur[level[i]]++] = R;
    }
    if (plan.blk_slots.empty())
    {
        plan.blk_slots.push_back(nullptr);
        plan.blk_bcol.push_back(0);
    }
}

// one rank, a device platform, PANGULU_AMD_DEVICE_SOLVE not 0
static bool device_solve_enabled(const Solver &S, const Platform &plat)
{
    const char *e = getenv("PANGULU_AMD_DEVICE_SOLVE");
    return !(S.nproc != 1 || plat.host_memory || !plat.block_trsv || (e && atoi(e) == 0));
}

// the two sweeps of a direction as the platform operators take them, from the handle's plans (built here on first use)
static void solve_sweeps_of(Solver &S, int trans, pangulu_hip_solve_sweep_t sw[2])
{
    const int d = trans == PANGULU_AMD_TRANS_NONE ? 0 : 1;
    if (!S.solve_plan_ready[d])
    {
        for (int s = 0; s < 2; s++)
            build_sweep_plan(S, sweep_shape(S, d == 1, s), S.solve_plan[d][s]);
        S.solve_plan_ready[d] = true;
    }
    for (int s = 0; s < 2; s++)
    {
        const SolveSweepPlan &pl = S.solve_plan[d][s];
        sw[s].nlevel = pl.nlevel;
        sw[s].level_ptr = pl.level_ptr.data();
        sw[s].rows = pl.rows.data();
        sw[s].blk_slots = pl.blk_slots.data();
        sw[s].blk_bcol = pl.blk_bcol.data();
    }
}

// Single rank on a device: both sweeps on the device-resident factors (no download of the factors), level by level of the block
// dependency graph.  X holds `npanel` panels one after the other, panel p with nbk*nb x w[p] values, right-hand side fastest: one
// pangulu_platform_0201001_block_trsm_multi call; a platform with block_trsv alone takes single columns (w[p] = 1), sweep by sweep.
// The plans of both sweeps are built on first use and kept on the handle.  trans = PANGULU_AMD_TRANS_T / _H: the transposed sweeps
// (U^T forward, L^T backward) on plans of their own through Platform::block_trsm_multi_trans, which the caller has found to be offered.
static void device_solve_panels(Solver &S, Platform &plat, val_t *X, size_t npanel, const int *w, int trans = PANGULU_AMD_TRANS_NONE)
{
    pangulu_hip_solve_sweep_t sw[2];
    solve_sweeps_of(S, trans, sw);
    const pangulu_uint64_t xlen = (pangulu_uint64_t)S.nbk * S.nb;
    if (trans != PANGULU_AMD_TRANS_NONE)
    {
        plat.block_trsm_multi_trans((pangulu_inblock_idx)S.nb, &sw[0], &sw[1], trans == PANGULU_AMD_TRANS_H, X, xlen, (pangulu_uint64_t)npanel, w);
        return;
    }
    if (plat.block_trsm_multi)
    {
        plat.block_trsm_multi((pangulu_inblock_idx)S.nb, &sw[0], &sw[1], X, xlen, (pangulu_uint64_t)npanel, w);
        return;
    }
    for (size_t p = 0; p < npanel; p++)
        for (int s = 0; s < 2; s++)
            plat.block_trsv((pangulu_inblock_idx)S.nb, s, sw[s].nlevel, sw[s].level_ptr, sw[s].rows, sw[s].blk_slots, sw[s].blk_bcol, X + p * xlen, xlen);
}

// One sweep of the host solve across the ranks, segment by segment in the sweep's direction: every rank that owns blocks of the
// segment on the sweep's side (with the subtree mapping these are not confined to the diagonal owner's process row / column) adds the
// products of its own blocks with `spmv`, the diagonal owner sums the partial vectors in rank order, solves with its diagonal half
// (`diag_solve`) and broadcasts the finished segment.  A partial vector of segment i travels under tag_base + (i & 0xfffff):
// 0x100000 for the untransposed sweeps, 0x200000 for the transposed ones.
template <class Spmv, class DiagSolve>
static void host_sweep(Solver &S, const SweepShape &sweep, int tag_base, Spmv spmv, DiagSolve diag_solve, std::vector<val_t> &x)
{
    Comm *comm = world();
    const u32 nb = S.nb, nbk = S.nbk;
    const int me = S.rank;
    std::vector<char> contributes((size_t)S.nproc, 0);
    std::vector<val_t> acc(nb), tmp(nb);
    for (u32 step = 0; step < nbk; step++)
    {
        const u32 i = sweep.segment_at(step, nbk);
        val_t *seg = x.data() + (size_t)i * nb;
        const int diag_rank = S.owner(i, i);
        const int tag = tag_base + (int)(i & 0xfffff);
        std::fill(contributes.begin(), contributes.end(), 0);
        for (u64 r = sweep.begin[i]; r < sweep.end[i]; r++)
            contributes[(size_t)sweep.owner_of(S, i, r)] = 1;
        if (contributes[(size_t)me] || me == diag_rank)
        {
            std::fill(acc.begin(), acc.end(), vmake(0));
            for (u64 r = sweep.begin[i]; r < sweep.end[i]; r++)
                if (sweep.owner_of(S, i, r) == me)
                    spmv(S.slot_of[sweep.block_of(r)], x.data() + (size_t)sweep.neighbour[r] * nb, acc.data());
            if (me == diag_rank)
            {
                for (int r = 0; r < S.nproc; r++)
                {
                    if (r == me || !contributes[(size_t)r])
                        continue;
                    comm->recv_bytes(r, tag, tmp.data(), sizeof(val_t) * nb);
                    for (u32 k = 0; k < nb; k++)
                        acc[k] = vadd(acc[k], tmp[k]);
                }
                for (u32 k = 0; k < nb; k++)
                    seg[k] = vadd(seg[k], acc[k]);
                diag_solve(sweep.diag[i], seg);
            }
            else
            {
                comm->send_bytes(diag_rank, tag, acc.data(), sizeof(val_t) * nb);
            }
        }
        comm->bcast(seg, sizeof(val_t) * nb, diag_rank);
    }
    comm->barrier();
}

// Both sweeps on the host copies of the factors for one vector, everywhere the device solve does not run (collective): L then U
// over block rows, or (transposed) U^T then L^T over block columns with op() = conjugation for A^H.
static void host_solve(Solver &S, val_t *rhs, bool transposed, bool conj)
{
    download_factors(S);
    const u32 nb = S.nb;
    std::vector<val_t> x((size_t)S.nbk * nb, vmake(0));
    std::copy(rhs, rhs + S.n, x.begin());
    for (int s = 0; s < 2; s++)
    {
        const SweepShape sweep = sweep_shape(S, transposed, s);
        if (!transposed)
            host_sweep(
                S, sweep, 0x100000, [&](const slot_t *a, const val_t *xk, val_t *y) { block_spmv(nb, a, xk, y); },
                [&](const slot_t *d, val_t *seg) { s == 0 ? block_lower_solve(nb, d, seg) : block_upper_solve(nb, d, seg); }, x);
        else
            host_sweep(
                S, sweep, 0x200000, [&](const slot_t *a, const val_t *xk, val_t *y) { block_spmv_trans(nb, a, xk, y, conj); },
                [&](const slot_t *d, val_t *seg) { s == 0 ? block_upper_trans_solve(nb, d, seg, conj) : block_lower_trans_solve(nb, d, seg, conj); }, x);
    }
    std::copy(x.begin(), x.begin() + S.n, rhs);
}

void triangular_solve(Solver &S, val_t *rhs)
{
    Platform &plat = active_platform();
    if (device_solve_enabled(S, plat))
    {
        // the block solve with one column
        std::vector<val_t> x((size_t)S.nbk * S.nb, vmake(0));
        std::copy(rhs, rhs + S.n, x.begin());
        const int one = 1;
        device_solve_panels(S, plat, x.data(), 1, &one);
        std::copy(x.begin(), x.begin() + S.n, rhs);
        return;
    }
    host_solve(S, rhs, false, false);
}

// panels for nrhs columns: the widest width while that many columns are left, then the smallest power of two that holds the rest (zero columns pad it)
static std::vector<int> solve_panel_widths(u32 nrhs, int wmax)
{
    std::vector<int> w;
    for (u32 left = nrhs; left;)
    {
        int wp = 1;
        while (wp < wmax && (u32)wp < left)
            wp <<= 1;
        w.push_back(wp);
        left -= std::min(left, (u32)wp);
    }
    return w;
}

// the columns of Bm in panels through the device sweeps (trans: which pair), panels at most wmax wide
static void device_solve_columns(Solver &S, Platform &plat, val_t *Bm, u32 nrhs, int wmax, int trans)
{
    S.last_solve_device_columns = (int)nrhs;
    const u32 nb = S.nb, n = S.n;
    const std::vector<int> w = solve_panel_widths(nrhs, wmax);
    size_t total_w = 0;
    for (int wp : w)
        total_w += (size_t)wp;
    const size_t xlen = (size_t)S.nbk * nb;
    std::vector<val_t> X(xlen * total_w, vmake(0));
    auto each_panel = [&](auto &&f)
    {
        size_t off = 0;
        u32 j0 = 0;
        for (int wp : w)
        {
            const u32 nc = std::min((u32)wp, nrhs - j0);
            f(X.data() + off, wp, j0, nc);
            off += xlen * (size_t)wp;
            j0 += nc;
        }
    };
    each_panel([&](val_t *Xp, int wp, u32 j0, u32 nc)
               {
                   for (u32 r = 0; r < nc; r++)
                   {
                       const val_t *col = Bm + (size_t)(j0 + r) * n;
                       for (u32 i = 0; i < n; i++)
                           Xp[(size_t)i * wp + r] = col[i];
                   } });
    device_solve_panels(S, plat, X.data(), w.size(), w.data(), trans);
    each_panel([&](val_t *Xp, int wp, u32 j0, u32 nc)
               {
                   for (u32 r = 0; r < nc; r++)
                   {
                       val_t *col = Bm + (size_t)(j0 + r) * n;
                       for (u32 i = 0; i < n; i++)
                           col[i] = Xp[(size_t)i * wp + r];
                   } });
    S.last_solve_panel_width = w[0];
    S.last_solve_panels = (int)w.size();
}

// Panels of right-hand sides through pangulu_platform_0201001_block_trsm_multi where the device solve runs, triangular_solve()
// column by column everywhere else (N > 1 ranks, host-memory platforms, PANGULU_AMD_DEVICE_SOLVE=0): collective, same tags.
void triangular_solve_multi(Solver &S, val_t *Bm, u32 nrhs)
{
    Platform &plat = active_platform();
    S.last_solve_device_columns = 0;
    S.last_solve_panel_width = 1;
    S.last_solve_panels = (int)nrhs;
    if (!device_solve_enabled(S, plat) || !plat.block_trsm_multi)
    {
        for (u32 j = 0; j < nrhs; j++)
            triangular_solve(S, Bm + (size_t)j * S.n);
        return;
    }
    const int wmax = plat.block_trsm_multi((pangulu_inblock_idx)S.nb, nullptr, nullptr, nullptr, 0, 0, nullptr);
    device_solve_columns(S, plat, Bm, nrhs, wmax, PANGULU_AMD_TRANS_NONE);
}

void triangular_solve_multi_trans(Solver &S, val_t *Bm, u32 nrhs, bool conjugate)
{
    Platform &plat = active_platform();
    S.last_solve_device_columns = 0;
    S.last_solve_panel_width = 1;
    S.last_solve_panels = (int)nrhs;
    int wmax = 0;
    if (device_solve_enabled(S, plat) && plat.block_trsm_multi_trans)
        wmax = plat.block_trsm_multi_trans((pangulu_inblock_idx)S.nb, nullptr, nullptr, 0, nullptr, 0, 0, nullptr);
    if (wmax < 1)
    {
        for (u32 j = 0; j < nrhs; j++)
            host_solve(S, Bm + (size_t)j * S.n, true, conjugate);
        return;
    }
    device_solve_columns(S, plat, Bm, nrhs, wmax, conjugate ? PANGULU_AMD_TRANS_H : PANGULU_AMD_TRANS_T);
}

// pangulu_amd_gstrs_device: the columns of a device matrix through Platform::block_trsm_multi_device, which packs, sweeps and unpacks
// each panel on the device and keeps what does not depend on the right-hand sides in S.solve_workspace.  Every condition for 4 is
// this rank's own (no exchange), and nothing has been touched when it is returned.
// the widest panel the device-resident solve of this direction takes; 0: no such path for this handle
static int device_solve_widest_panel(Solver &S, int trans, bool reproducible)
{
    Platform &plat = active_platform();
    if (!device_solve_enabled(S, plat) || !plat.block_trsm_multi_device || !plat.solve_workspace_free)
        return 0;
    const pangulu_uint64_t xlen = (pangulu_uint64_t)S.nbk * S.nb;
    const int wmax = plat.block_trsm_multi_device((pangulu_inblock_idx)S.nb, nullptr, nullptr, trans | (reproducible ? PANGULU_HIP_SOLVE_REPRODUCIBLE : 0), nullptr,
                                                  0, 0, 0, nullptr, xlen, nullptr, nullptr, nullptr);
    return wmax < 1 ? 0 : wmax;
}

bool device_solve_offered(Solver &S, int trans, bool reproducible) { return device_solve_widest_panel(S, trans, reproducible) > 0; }

int triangular_solve_device(Solver &S, val_t *d_rhs, u32 nrhs, u64 ldb, int trans, void *stream, bool reproducible)
{
    Platform &plat = active_platform();
    const pangulu_uint64_t xlen = (pangulu_uint64_t)S.nbk * S.nb;
    const int wmax = device_solve_widest_panel(S, trans, reproducible);
    if (wmax < 1)
        return 4;
    const SolveMaps &M = solve_maps(S, trans != PANGULU_AMD_TRANS_NONE);
    pangulu_hip_solve_maps_t maps;
    maps.n = S.n;
    maps.n_user = S.n_user;
    maps.in_idx = M.in_idx.data();
    maps.out_idx = M.out_idx.data();
    maps.s_in = M.s_in.empty() ? nullptr : M.s_in.data();
    maps.s_out = M.s_out.empty() ? nullptr : M.s_out.data();
    pangulu_hip_solve_sweep_t sw[2];
    solve_sweeps_of(S, trans, sw);
    const std::vector<int> w = solve_panel_widths(nrhs, wmax);
    const int rc = plat.block_trsm_multi_device((pangulu_inblock_idx)S.nb, &sw[0], &sw[1], trans | (reproducible ? PANGULU_HIP_SOLVE_REPRODUCIBLE : 0), d_rhs, ldb, nrhs, (pangulu_uint64_t)w.size(), w.data(), xlen,
                                                &maps, &S.solve_workspace, stream);
    if (rc < 0)
        return 2;
    if (rc == 0)
        return 4;
    S.last_solve_device_columns = (int)nrhs;
    S.last_solve_panel_width = w[0];
    S.last_solve_panels = (int)w.size();
    return 0;
}

void drop_solve_workspace(Solver &S)
{
    if (!S.solve_workspace)
        return;
    active_platform().solve_workspace_free(&S.solve_workspace);
    S.solve_workspace = nullptr;
}

} // namespace pg
