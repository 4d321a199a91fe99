// pg_condest.cpp -- can the factorisation be trusted?  pangulu_amd_factor_stats and pangulu_amd_rcond.
//
// The factorisation does no pivoting: a pivot with |Re| < 1e-16 is replaced by 1e-16 where it divides (clamp_pivot,
// solve_clamped_divisor) and the run goes on.  What SuperLU answers with gscon / PivotGrowth and LAPACK with gecon is answered here
// from the factors where they are:
//   factor_stats           one pass over the records this rank owns -- Platform::factor_stats on device-resident records (one launch,
//                          pg_hip_factor_stats.h), the loops below on host records -- one partial per record, combined in block order,
//                          then over the ranks in rank order on rank 0: the same call gives the same bits;
//   reciprocal_condition   Higham's 1-norm estimator as LAPACK's xLACN2 states it, written ONCE over CondestOps: on a device vector
//                          (Platform::condest_vector between triangular_solve_device calls; a few scalars come back per step) where
//                          the device-resident solve exists for A and A^H, on a host vector through collective_column_solve
//                          (pg_api.cpp) everywhere else (rank 0 drives; one word per step tells the other ranks which
//                          solve comes next, or to leave).
#include <algorithm>
#include <cmath>
#include <limits>

#include "pg_host.h"

namespace pg
{

namespace
{

inline double re_of(val_t v)
{
#ifdef PANGULU_COMPLEX
    return (double)v.re;
#else
    return (double)v;
#endif
}
inline double im_of(val_t v)
{
#ifdef PANGULU_COMPLEX
    return (double)v.im;
#else
    (void)v;
    return 0.0;
#endif
}
inline double modulus(double re, double im) { return im == 0.0 ? std::fabs(re) : std::hypot(re, im); }
inline double modulus(val_t v) { return modulus(re_of(v), im_of(v)); }
inline val_t value_of(double re, double im)
{
#ifdef PANGULU_COMPLEX
    return val_t{(calculate_real_type)re, (calculate_real_type)im};
#else
    (void)im;
    return (val_t)re;
#endif
}
#ifdef PANGULU_COMPLEX
constexpr bool kComplex = true;
#else
constexpr bool kComplex = false;
#endif
constexpr double kPivotClamp = 1e-16;

// ---- a product as mantissa and binary exponent ---------------------------------------------------------------------------------------
struct Scaled // (re + i im) 2^e, 0.5 <= max(|re|, |im|) < 1; zero: 0, 0, 0; a non-finite mantissa stays as it is
{
    double re = 0.5, im = 0.0;
    long long e = 1;
};
Scaled normalise(Scaled p)
{
    if (!std::isfinite(p.re) || !std::isfinite(p.im))
        return p;
    const double m = std::max(std::fabs(p.re), std::fabs(p.im));
    if (m == 0.0)
    {
        p.re = p.im = 0.0;
        p.e = 0;
        return p;
    }
    int k = 0;
    (void)std::frexp(m, &k);
    p.re = std::ldexp(p.re, -k);
    p.im = std::ldexp(p.im, -k);
    p.e += k;
    return p;
}
Scaled times(const Scaled &a, const Scaled &b)
{
    Scaled r;
    if (a.im == 0.0 && b.im == 0.0)
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
    return normalise(r);
}
Scaled scaled_of(double re, double im)
{
    Scaled s;
    s.re = re;
    s.im = im;
    s.e = 0;
    return normalise(s);
}

// ---- one record on the host (what factor_stats_kernel does, serially) ----------------------------------------------------------------
inline bool larger(double key, u64 idx, double best_key, u64 best_idx) { return key > best_key || (key == best_key && idx < best_idx); }

void host_record_stats(const slot_t &s, u32 nb, bool upper_diag, const unsigned char *pad, pangulu_factor_stats_partial_t &o)
{
    memset(&o, 0, sizeof(o));
    const u64 nnz = s.columnpointer[nb];
    o.entries = nnz;
    double best = -1.0;
    for (u64 p = 0; p < nnz; p++)
    {
        const double re = re_of(s.value[p]), im = im_of(s.value[p]);
        if (!std::isfinite(re) || !std::isfinite(im))
            o.nonfinite++;
        const double a = modulus(re, im);
        if (a > best) // (a NaN never wins)
        {
            best = a;
            o.max_re = re;
            o.max_im = im;
        }
    }
    o.minp_row = ~0ull;
    o.prod_re = 0.5;
    o.prod_exp = 1;
    if (!upper_diag)
        return;
    Scaled prod;
    double kmin = 0, kmax = -1.0;
    for (u32 r = 0; r < nb; r++)
    {
        const u32 b = s.columnpointer[r], e = s.columnpointer[r + 1];
        const u64 row = (u64)s.brow_pos * nb + r;
        if (b == e || (pad && pad[row]))
            continue;
        const double re = re_of(s.value[b]), im = im_of(s.value[b]);
        const double a = modulus(re, im);
        const double key_max = a == a ? a : -1.0, key_min = a == a ? a : HUGE_VAL;
        if (key_max > kmax)
        {
            kmax = key_max;
            o.maxp_re = re;
            o.maxp_im = im;
        }
        if (o.minp_row == ~0ull || key_min < kmin)
        {
            kmin = key_min;
            o.minp_re = re;
            o.minp_im = im;
            o.minp_row = row;
        }
        o.clamped += std::fabs(re) < kPivotClamp ? 1 : 0;
        o.pivots++;
        prod = times(prod, scaled_of(re, im));
    }
    o.prod_re = prod.re;
    o.prod_im = prod.im;
    o.prod_exp = prod.e;
}

// ---- what a rank knows after its records, and what everybody knows at the end --------------------------------------------------------
struct StatsTotal
{
    double maxl_re = 0, maxl_im = 0, maxu_re = 0, maxu_im = 0;
    u64 nonfinite = 0, entries = 0, clamped = 0, pivots = 0;
    double minp_re = 0, minp_im = 0, maxp_re = 0, maxp_im = 0;
    u64 minp_row = ~0ull;
    Scaled prod;
};
void keep_larger(double &re, double &im, double cre, double cim)
{
    if (modulus(cre, cim) > modulus(re, im))
    {
        re = cre;
        im = cim;
    }
}
void add_pivots(StatsTotal &t, double minp_re, double minp_im, u64 minp_row, double maxp_re, double maxp_im, u64 clamped, u64 pivots, const Scaled &prod)
{
    if (pivots == 0)
        return;
    if (minp_row != ~0ull)
    {
        const double a = modulus(minp_re, minp_im), b = modulus(t.minp_re, t.minp_im);
        if (t.minp_row == ~0ull || a < b || (a == b && minp_row < t.minp_row) || (b != b && a == a))
        {
            t.minp_re = minp_re;
            t.minp_im = minp_im;
            t.minp_row = minp_row;
        }
    }
    if (t.pivots == 0)
    {
        t.maxp_re = maxp_re;
        t.maxp_im = maxp_im;
    }
    else
        keep_larger(t.maxp_re, t.maxp_im, maxp_re, maxp_im);
    t.clamped += clamped;
    t.pivots += pivots;
    t.prod = times(t.prod, prod);
}

} // namespace

void user_matrix_norms(u32 n, const u64 *colptr, const u32 *rowidx, const val_t *value, double &norm_one, double &norm_inf)
{
    std::vector<double> row(n, 0.0);
    norm_one = 0;
    bool nan = false;
    for (u32 j = 0; j < n; j++)
    {
        double col = 0;
        for (u64 p = colptr[j]; p < colptr[j + 1]; p++)
        {
            const double a = modulus(value[p]);
            col += a;
            row[rowidx[p]] += a;
        }
        nan = nan || col != col;
        norm_one = std::max(norm_one, col);
    }
    norm_inf = 0;
    for (u32 i = 0; i < n; i++)
        norm_inf = std::max(norm_inf, row[i]);
    if (nan) // (std::max drops a NaN; the norm of a matrix with one is one)
        norm_one = norm_inf = std::numeric_limits<double>::quiet_NaN();
}

void factor_stats(Solver &S, pangulu_amd_factor_stats_t &out)
{
    Platform &plat = active_platform();
    Comm *comm = world();
    const u32 nb = S.nb;
    const size_t xlen = (size_t)S.nbk * nb;
    // rows of the factors' ordering that are not the user's: the padding rows of an aligned ordering, the tail of the last block
    std::vector<unsigned char> pad(xlen, 1);
    for (u32 i = 0; i < S.n; i++)
        pad[i] = S.perm[i] >= S.n_user ? 1 : 0;
    std::vector<slot_t *> slots;
    std::vector<int> upper_diag, in_u;
    for (auto &s : S.storage.owned)
    {
        const bool diag = s.brow_pos == s.bcol_pos;
        slots.push_back(&s);
        upper_diag.push_back(diag && s.is_upper ? 1 : 0);
        in_u.push_back((diag && s.is_upper) || (!diag && s.brow_pos < s.bcol_pos) ? 1 : 0);
    }
    std::vector<pangulu_factor_stats_partial_t> part(std::max<size_t>(slots.size(), 1));
    // (PANGULU_AMD_DEVICE_SOLVE=0, read per call like the solves do, takes the host loops on downloaded factors here as well)
    const char *ds = getenv("PANGULU_AMD_DEVICE_SOLVE");
    if (!plat.host_memory && plat.factor_stats && !(ds && atoi(ds) == 0))
        plat.factor_stats((pangulu_inblock_idx)nb, slots.size(), slots.data(), upper_diag.data(), pad.data(), xlen, part.data());
    else
    {
        download_factors(S);
        for (size_t i = 0; i < slots.size(); i++)
            host_record_stats(*slots[i], nb, upper_diag[i] != 0, pad.data(), part[i]);
    }
    // this rank's records in storage order
    StatsTotal mine;
    for (size_t i = 0; i < slots.size(); i++)
    {
        const pangulu_factor_stats_partial_t &p = part[i];
        if (in_u[i])
            keep_larger(mine.maxu_re, mine.maxu_im, p.max_re, p.max_im);
        else
            keep_larger(mine.maxl_re, mine.maxl_im, p.max_re, p.max_im);
        mine.nonfinite += p.nonfinite;
        mine.entries += p.entries;
        if (upper_diag[i])
        {
            Scaled pr;
            pr.re = p.prod_re;
            pr.im = p.prod_im;
            pr.e = p.prod_exp;
            add_pivots(mine, p.minp_re, p.minp_im, p.minp_row, p.maxp_re, p.maxp_im, p.clamped, p.pivots, pr);
        }
    }
    // the ranks in rank order on rank 0
    StatsTotal all = mine;
    if (comm->size > 1)
    {
        const int TAG = 0x200001;
        if (comm->rank == 0)
        {
            for (int r = 1; r < comm->size; r++)
            {
                StatsTotal t;
                comm->recv_bytes(r, TAG, &t, sizeof(t));
                keep_larger(all.maxl_re, all.maxl_im, t.maxl_re, t.maxl_im);
                keep_larger(all.maxu_re, all.maxu_im, t.maxu_re, t.maxu_im);
                all.nonfinite += t.nonfinite;
                all.entries += t.entries;
                add_pivots(all, t.minp_re, t.minp_im, t.minp_row, t.maxp_re, t.maxp_im, t.clamped, t.pivots, t.prod);
            }
        }
        else
            comm->send_bytes(0, TAG, &mine, sizeof(mine));
    }
    memset(&out, 0, sizeof(out));
    if (comm->rank == 0)
    {
        // det(A1) = the product of the pivots (the symmetric permutation contributes +1, a padding row exactly 1).  With scaling on
        // A1 = Dr A Q Dc, Q the matching's column permutation: det(A) = det(A1) sign(Q) / (prod dr prod dc)
        Scaled det = all.prod;
        if (!S.scale_row.empty())
        {
            Scaled sc;
            for (u32 i = 0; i < S.n_user; i++)
                sc = times(times(sc, scaled_of(S.scale_row[i], 0.0)), scaled_of(S.scale_col[i], 0.0));
            Scaled q;
            q.re = det.re / sc.re; // (sc.im == 0: the scalings are real)
            q.im = det.im / sc.re;
            q.e = det.e - sc.e;
            det = normalise(q);
            std::vector<char> seen(S.n_user, 0);
            u32 cycles = 0;
            for (u32 i = 0; i < S.n_user; i++)
            {
                if (seen[i])
                    continue;
                cycles++;
                for (u32 k = i; !seen[k]; k = S.match_col[k])
                    seen[k] = 1;
            }
            if ((S.n_user - cycles) & 1u)
            {
                det.re = -det.re;
                det.im = -det.im;
            }
        }
        out.det_mantissa_re = det.re;
        out.det_mantissa_im = det.im;
        out.det_exponent = det.e;
        const double m = modulus(det.re, det.im);
        out.log_abs_det = m == 0.0 ? -HUGE_VAL : std::log(m) + (double)det.e * 0.6931471805599453094;
        out.min_abs_pivot = all.minp_row == ~0ull ? 0.0 : modulus(all.minp_re, all.minp_im);
        out.max_abs_pivot = modulus(all.maxp_re, all.maxp_im);
        // the user's index: row min_pivot_index of the matrix given to pangulu_init (with scaling on its column is the matched one)
        out.min_pivot_index = all.minp_row < S.n ? S.perm[all.minp_row] : 0;
        out.clamped_pivots = all.clamped;
        out.nonfinite_entries = all.nonfinite;
        out.entries = all.entries;
        out.max_abs_l = modulus(all.maxl_re, all.maxl_im);
        out.max_abs_u = modulus(all.maxu_re, all.maxu_im);
        double amax = 0;
        for (const val_t &v : S.Aperm.value)
            amax = std::max(amax, modulus(v));
        out.max_abs_a = amax;
        out.pivot_growth = out.max_abs_u / amax;
    }
    comm->bcast(&out, sizeof(out), 0);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// the estimator
// ---------------------------------------------------------------------------------------------------------------------------------------
namespace
{

// the steps between two solves and the solves, on a vector x of n values and a saved sign vector, wherever they live
struct CondestOps
{
    virtual ~CondestOps() {}
    virtual void fill_inv_n() = 0;
    // sum |x_i|, then x = its sign vector; real types with `compare`: unchanged = every sign equals the saved one; the signs are saved
    virtual void norm1_sign(bool compare, double &norm1, bool &unchanged) = 0;
    virtual void argmax(u64 jprev, u64 &j, double &absmax, double &abs_prev) = 0; // the FIRST largest modulus
    virtual void set_ej(u64 j) = 0;
    virtual void fill_alt() = 0;
    virtual double norm1() = 0;
    virtual void solve(bool adjoint) = 0; // x = inv(M) x, or x = inv(M)^H x
};

// An estimate of || inv(M) ||_1, a lower bound: xLACN2 with the reverse communication unrolled.  At most 5 iterations whatever the
// data: 1 + 1 + 4 * 2 + 1 = 11 solves.  One departure: where xLACN2 leaves its loop because the new estimate is not larger than the
// old one it goes on with the new one; both are || inv(M) x ||_1 for some || x ||_1 = 1, so the larger is kept.
double estimate_inverse_norm1(CondestOps &ops, u64 n, int &solves, bool &saw_nan)
{
    constexpr int ITMAX = 5;
    solves = 0;
    saw_nan = false;
    auto seen = [&](double v)
    {
        saw_nan = saw_nan || v != v;
        return v;
    };
    ops.fill_inv_n();
    ops.solve(false);
    solves++;
    if (n == 1)
        return seen(ops.norm1());
    double est = 0;
    bool unchanged = false;
    ops.norm1_sign(false, est, unchanged);
    seen(est);
    ops.solve(true);
    solves++;
    u64 j = 0;
    double absmax = 0, abs_prev = 0;
    ops.argmax(~0ull, j, absmax, abs_prev);
    for (int iter = 2;; iter++)
    {
        ops.set_ej(j);
        ops.solve(false);
        solves++;
        const double estold = est;
        double now = 0;
        ops.norm1_sign(true, now, unchanged);
        seen(now);
        if (now > est || now != now)
            est = now;
        if (unchanged)
            break; // repeated sign vector: converged
        if (!(now > estold))
            break; // cycling (or a NaN)
        ops.solve(true);
        solves++;
        const u64 jlast = j;
        ops.argmax(jlast, j, absmax, abs_prev);
        if (abs_prev == absmax || iter >= ITMAX)
            break;
    }
    ops.fill_alt();
    ops.solve(false);
    solves++;
    const double alt = 2.0 * (seen(ops.norm1()) / (3.0 * (double)n));
    if (alt > est)
        est = alt;
    return est;
}

// One collective solve of the host path with the user's vector on rank 0: what pangulu_amd_gstrs_multi / _trans do with one column.
// `x` is ignored on the other ranks.  (real values: A^H = A^T)
void collective_host_solve(Solver &S, val_t *x, bool adjoint)
{
    collective_column_solve(S, x, 1, S.n_user, adjoint ? PANGULU_AMD_TRANS_H : PANGULU_AMD_TRANS_NONE);
}

constexpr u64 STEP_LEAVE = 0, STEP_SOLVE = 1, STEP_SOLVE_ADJOINT = 2;

struct HostOps : CondestOps
{
    Solver &S;
    bool swap; // infinity norm: the estimator runs on A^H
    std::vector<val_t> x, save;
    HostOps(Solver &s, bool sw) : S(s), swap(sw), x(s.n_user), save(s.n_user) {}
    void fill_inv_n() override
    {
        for (auto &v : x)
            v = value_of(1.0 / (double)x.size(), 0.0);
    }
    void norm1_sign(bool compare, double &norm1, bool &unchanged) override
    {
        norm1 = 0;
        u64 changed = 0;
        for (size_t i = 0; i < x.size(); i++)
        {
            const double re = re_of(x[i]), im = im_of(x[i]), a = modulus(re, im);
            norm1 += a;
            val_t sg;
            if (kComplex)
                sg = a > std::numeric_limits<double>::min() ? value_of(re / a, im / a) : value_of(1.0, 0.0);
            else
                sg = value_of(std::signbit(re) ? -1.0 : 1.0, 0.0);
            x[i] = sg;
            if (!kComplex)
            {
                changed += memcmp(&save[i], &sg, sizeof(val_t)) != 0 ? 1 : 0;
                save[i] = sg;
            }
        }
        unchanged = !kComplex && compare && changed == 0;
    }
    void argmax(u64 jprev, u64 &j, double &absmax, double &abs_prev) override
    {
        double best = -2.0;
        j = 0;
        for (size_t i = 0; i < x.size(); i++)
        {
            const double a = modulus(x[i]), key = a == a ? a : -1.0;
            if (key > best)
            {
                best = key;
                j = i;
            }
        }
        absmax = modulus(x[j]);
        abs_prev = jprev < x.size() ? modulus(x[jprev]) : 0.0;
    }
    void set_ej(u64 j) override
    {
        for (size_t i = 0; i < x.size(); i++)
            x[i] = value_of(i == j ? 1.0 : 0.0, 0.0);
    }
    void fill_alt() override
    {
        const size_t n = x.size();
        for (size_t i = 0; i < n; i++)
        {
            const double v = 1.0 + (double)i / (double)(n > 1 ? n - 1 : 1);
            x[i] = value_of((i & 1) ? -v : v, 0.0);
        }
    }
    double norm1() override
    {
        double s = 0;
        for (const val_t &v : x)
            s += modulus(v);
        return s;
    }
    void solve(bool adjoint) override
    {
        const bool adj = adjoint != swap;
        Comm *comm = world();
        if (comm->size > 1)
        {
            u64 word = adj ? STEP_SOLVE_ADJOINT : STEP_SOLVE;
            comm->bcast(&word, sizeof(word), 0);
        }
        collective_host_solve(S, x.data(), adj);
    }
};

// x and the saved signs in device memory for the whole call; every solve is triangular_solve_device on x, everything in between a
// kernel of Platform::condest_vector, whose scratch lives in the handle's solve workspace
struct DeviceOps : CondestOps
{
    Solver &S;
    Platform &plat;
    bool swap;
    val_t *d_x = nullptr, *d_save = nullptr;
    DeviceOps(Solver &s, Platform &p, bool sw) : S(s), plat(p), swap(sw)
    {
        plat.malloc_((void **)&d_x, sizeof(val_t) * (size_t)S.n_user);
        if (!kComplex)
            plat.malloc_((void **)&d_save, sizeof(val_t) * (size_t)S.n_user);
    }
    ~DeviceOps() override
    {
        plat.free_(d_x);
        if (d_save)
            plat.free_(d_save);
    }
    pangulu_condest_result_t step(int what, u64 j)
    {
        pangulu_condest_result_t r;
        memset(&r, 0, sizeof(r));
        const int rc = plat.condest_vector(what, d_x, d_save, S.n_user, j, &r, (pangulu_inblock_idx)S.nb, (pangulu_uint64_t)S.nbk * S.nb, S.n, &S.solve_workspace,
                                           nullptr);
        if (rc != 1)
            fatal("pangulu_amd_rcond: the platform refused step %d of the estimator (%d)", what, rc);
        return r;
    }
    void fill_inv_n() override { step(PANGULU_CONDEST_FILL_INV_N, 0); }
    void norm1_sign(bool compare, double &norm1, bool &unchanged) override
    {
        const pangulu_condest_result_t r = step(PANGULU_CONDEST_NORM1_SIGN, compare ? 1 : 0);
        norm1 = r.norm1;
        unchanged = r.unchanged != 0;
    }
    void argmax(u64 jprev, u64 &j, double &absmax, double &abs_prev) override
    {
        const pangulu_condest_result_t r = step(PANGULU_CONDEST_ARGMAX, jprev);
        j = r.argmax;
        absmax = r.absmax;
        abs_prev = r.abs_prev;
    }
    void set_ej(u64 j) override { step(PANGULU_CONDEST_SET_EJ, j); }
    void fill_alt() override { step(PANGULU_CONDEST_FILL_ALT, 0); }
    double norm1() override { return step(PANGULU_CONDEST_NORM1, 0).norm1; }
    void solve(bool adjoint) override
    {
        const int trans = adjoint != swap ? PANGULU_AMD_TRANS_H : PANGULU_AMD_TRANS_NONE;
        const int rc = triangular_solve_device(S, d_x, 1, S.n_user, trans, nullptr, true); // (reproducible: the estimate is the same from call to call)
        if (rc != 0)
            fatal("pangulu_amd_rcond: the device-resident solve answered %d in the middle of the estimator", rc);
    }
};

} // namespace

void reciprocal_condition(Solver &S, int norm, double &rcond, double &anorm, double &ainv_norm, int &solves, int &on_device)
{
    Comm *comm = world();
    Platform &plat = active_platform();
    const bool swap = norm == PANGULU_AMD_NORM_INF; // || inv(A) ||_inf = || inv(A)^H ||_1: the same loop with the two solves swapped
    double res[5] = {0, 0, 0, 0, 0};
    if (comm->rank == 0)
    {
        const bool device = comm->size == 1 && plat.condest_vector && device_solve_offered(S, PANGULU_AMD_TRANS_NONE, true) &&
                            device_solve_offered(S, PANGULU_AMD_TRANS_H, true);
        bool saw_nan = false;
        int nsolve = 0;
        double est;
        if (device)
        {
            DeviceOps ops(S, plat, swap);
            est = estimate_inverse_norm1(ops, S.n_user, nsolve, saw_nan);
        }
        else
        {
            HostOps ops(S, swap);
            est = estimate_inverse_norm1(ops, S.n_user, nsolve, saw_nan);
            if (comm->size > 1)
            {
                u64 word = STEP_LEAVE;
                comm->bcast(&word, sizeof(word), 0);
            }
        }
        const double a = swap ? S.user_norm_inf : S.user_norm_one;
        double rc;
        if (saw_nan || est != est || a != a)
            rc = std::numeric_limits<double>::quiet_NaN();
        else if (std::isinf(est) || a == 0.0 || est == 0.0)
            rc = 0.0;
        else
            rc = (1.0 / est) / a;
        res[0] = rc;
        res[1] = a;
        res[2] = est;
        res[3] = (double)nsolve;
        res[4] = device ? 1.0 : 0.0;
    }
    else
    {
        for (;;)
        {
            u64 word = STEP_LEAVE;
            comm->bcast(&word, sizeof(word), 0);
            if (word == STEP_LEAVE)
                break;
            collective_host_solve(S, nullptr, word == STEP_SOLVE_ADJOINT);
        }
    }
    comm->bcast(res, sizeof(res), 0);
    rcond = res[0];
    anorm = res[1];
    ainv_norm = res[2];
    solves = (int)res[3];
    on_device = (int)res[4];
}

} // namespace pg
