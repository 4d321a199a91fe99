// The kernels of pangulu_amd/csrc/platform/pg_hip_factor_stats.h run on the CPU (tests/test_factor_stats.py), by the method and
// behind the shims of tests/solve_trans_kernel_emulation.cpp (tests/hip_emulation_shims.h): the header is compiled as plain C++, a
// workgroup is 256 threads.  Checked against serial formulas written out here once more: maxima, first indices, counts, sign vectors and
// filled values exactly; sums within n 2^-53 of the sum of moduli; pivot products within 4 n 2^-53 (the tree multiplies in another order
// than the serial loop: n - 1 multiplications of at most one rounding each, four for a complex product).  It checks indexing,
// the reduction trees and the arithmetic, not the device.
#include "hip_emulation_shims.h"

// shims this header is the first to need: a bit-preserving 64-bit shuffle (the double one would convert the words)
unsigned long long g_shfl_u64[4][64];
inline unsigned long long __shfl_down(unsigned long long v, int off, int) {
    int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_shfl_u64[w][l] = v; g_wave_bar[w]->arrive_and_wait();
    unsigned long long r = l + off < 64 ? g_shfl_u64[w][l + off] : v; g_wave_bar[w]->arrive_and_wait(); return r; }

#include "pg_hip_factor_stats.h"

#include <cstdint>
#include <limits>

std::mt19937_64 rng(20261021);
double urand() { return std::uniform_real_distribution<double>(-1, 1)(rng); }
val_t vmk(double re, double im) {
#ifdef PANGULU_COMPLEX
    return val_t{re, im};
#else
    (void)im; return re;
#endif
}
val_t vrand(double scale = 1.0) { return vmk(scale * urand(), scale * urand()); }
double vre(val_t v) { return fs_re(v); }
double vim(val_t v) { return fs_im(v); }
double vmod(val_t v) { return vim(v) == 0.0 ? std::fabs(vre(v)) : std::hypot(vre(v), vim(v)); }
bool same_bits(const val_t &a, const val_t &b) { return memcmp(&a, &b, sizeof(val_t)) == 0; }
const double QNAN = std::numeric_limits<double>::quiet_NaN();
const double EPS = 1.0 / 9007199254740992.0; // 2^-53

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 30) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- records -------------------------------------------------------------------------------------------------------------------------
struct Record { std::vector<val_t> val; std::vector<u32> rowptr; bool diag = false; unsigned long long row0 = 0; };

Record plain_record(size_t nnz, bool with_nan) {
    Record R; R.val.resize(nnz);
    for (auto &v : R.val) v = vrand(3.0);
    if (nnz > 2) R.val[nnz / 2] = vmk(-7.5, 0.0), R.val[nnz - 1] = vmk(7.5, 0.0); // two equal maxima: the modulus is what counts
    if (with_nan && nnz > 4) { R.val[3] = vmk(QNAN, 0.0); R.val[nnz - 2] = vmk(std::numeric_limits<double>::infinity(), 1.0); }
    return R;
}
// an upper diagonal half of order nb at block row `brow`: rows >= live are empty (the tail of the last block); the pivot first in its row
Record diag_record(int nb, int brow, int live, int special) {
    Record R; R.diag = true; R.row0 = (unsigned long long)brow * nb; R.rowptr.assign(nb + 1, 0);
    for (int r = 0; r < nb; r++) {
        if (r < live) {
            R.val.push_back(vmk(1.5 + urand(), 0.7 * urand())); // the pivot
            const int extra = (int)(rng() % 4);
            for (int k = 0; k < extra && r + 1 + k < nb; k++) R.val.push_back(vrand(5.0));
        }
        R.rowptr[r + 1] = (u32)R.val.size();
    }
    auto pivot = [&](int r) -> val_t & { return R.val[r == 0 ? 0 : R.rowptr[r]]; };
    if (special == 1 && live > 9) { pivot(5) = vmk(0.0, 0.0); }                        // an exact zero: the product is 0
    if (special == 2 && live > 9) { pivot(3) = vmk(1e-17, 0.25); pivot(8) = vmk(-3e-17, 0.0); pivot(2) = pivot(9) = vmk(0.125, 0.0); } // clamped ones; a tie for the minimum of the rest
    if (special == 3 && live > 9) { pivot(7) = vmk(QNAN, 0.0); }
    R.rowptr[0] = 0xdeadbeefu; // (entry 0 of a device pointer array is not the kernels' to read: ptr0)
    return R;
}

void check_records(int nb, const std::vector<Record> &recs, const std::vector<unsigned char> &pad, bool use_pad) {
    std::vector<FactorStatsBlkD> blks(recs.size());
    for (size_t i = 0; i < recs.size(); i++)
        blks[i] = FactorStatsBlkD{recs[i].val.data(), recs[i].diag ? recs[i].rowptr.data() : nullptr, recs[i].val.size(), recs[i].row0};
    std::vector<FactorStatsPartialD> out(recs.size());
    memset(out.data(), 0xff, sizeof(FactorStatsPartialD) * out.size());
    const unsigned char *padp = use_pad ? pad.data() : nullptr;
    launch((unsigned)recs.size(), [&] { factor_stats_kernel(blks.data(), nb, padp, out.data()); });
    for (size_t i = 0; i < recs.size(); i++) {
        const Record &R = recs[i]; const FactorStatsPartialD &o = out[i];
        double best = -1; unsigned long long bad = 0;
        for (const val_t &v : R.val) { const double a = vmod(v); if (a > best) best = a; bad += (std::isfinite(vre(v)) && std::isfinite(vim(v))) ? 0 : 1; }
        CHECK(o.entries == R.val.size(), "record %zu (nnz %zu): entries %llu", i, R.val.size(), o.entries);
        CHECK(o.nonfinite == bad, "record %zu (nnz %zu): %llu non-finite entries, %llu expected", i, R.val.size(), o.nonfinite, bad);
        const double got = vmod(vmk(o.max_re, o.max_im));
        CHECK(R.val.empty() ? (o.max_re == 0 && o.max_im == 0) : got == best, "record %zu (nnz %zu): largest modulus %.17g, expected %.17g", i, R.val.size(), got, best);
        if (!R.diag) {
            CHECK(o.pivots == 0 && o.clamped == 0 && o.minp_row == ~0ull && o.prod_re == 0.5 && o.prod_im == 0.0 && o.prod_exp == 1, "record %zu: pivot figures of a record without pivots", i);
            continue;
        }
        unsigned long long piv = 0, cl = 0, minrow = ~0ull; double pmin = 0, pmax = -1;
        double mre = 0.5, mim = 0; long long ex = 1; bool zero = false, nonfinite = false;
        for (int r = 0; r < nb; r++) {
            const u32 b = r == 0 ? 0 : R.rowptr[r], e = R.rowptr[r + 1];
            const unsigned long long row = R.row0 + r;
            if (b == e || (use_pad && pad[row])) continue;
            const val_t p = R.val[b]; const double a = vmod(p);
            piv++; cl += std::fabs(vre(p)) < 1e-16 ? 1 : 0;
            if (a == a) { if (a > pmax) pmax = a; if (minrow == ~0ull || a < pmin) { pmin = a; minrow = row; } }
            if (a == 0) zero = true;
            if (!(a == a)) nonfinite = true;
            // the serial product with the same representation
            const double nre = mre * vre(p) - mim * vim(p), nim = mre * vim(p) + mim * vre(p);
            int k = 0; const double m = std::max(std::fabs(nre), std::fabs(nim));
            if (m > 0 && std::isfinite(m)) { (void)std::frexp(m, &k); mre = std::ldexp(nre, -k); mim = std::ldexp(nim, -k); ex += k; } else { mre = nre; mim = nim; }
        }
        CHECK(o.pivots == piv && o.clamped == cl, "diagonal half %zu: %llu pivots, %llu clamped; expected %llu, %llu", i, o.pivots, o.clamped, piv, cl);
        if (nonfinite) { CHECK(!(o.prod_re == o.prod_re) || !(o.prod_im == o.prod_im), "diagonal half %zu: a NaN pivot left a finite product", i); }
        else if (zero) { CHECK(o.prod_re == 0 && o.prod_im == 0 && o.prod_exp == 0, "diagonal half %zu: zero product as %g %g 2^%lld", i, o.prod_re, o.prod_im, o.prod_exp); }
        else {
            const double sre = std::ldexp(o.prod_re, (int)(o.prod_exp - ex)), sim = std::ldexp(o.prod_im, (int)(o.prod_exp - ex));
            const double err = std::hypot(sre - mre, sim - mim) / std::hypot(mre, mim);
            CHECK(err <= 4.0 * (double)(piv + 1) * EPS, "diagonal half %zu: product differs by %g relative (%llu pivots)", i, err, piv);
            const double top = std::max(std::fabs(o.prod_re), std::fabs(o.prod_im));
            CHECK(top >= 0.5 && top < 1.0, "diagonal half %zu: mantissa %g %g is not normalised", i, o.prod_re, o.prod_im);
        }
        if (piv && minrow != ~0ull) {
            CHECK(o.minp_row == minrow, "diagonal half %zu: smallest pivot at row %llu, expected the first one at %llu", i, o.minp_row, minrow);
            CHECK(vmod(vmk(o.minp_re, o.minp_im)) == pmin && vmod(vmk(o.maxp_re, o.maxp_im)) == pmax, "diagonal half %zu: pivot range %g .. %g, expected %g .. %g", i,
                  vmod(vmk(o.minp_re, o.minp_im)), vmod(vmk(o.maxp_re, o.maxp_im)), pmin, pmax);
        }
    }
    printf("records: nb=%d, %zu records, padding mask %s\n", nb, recs.size(), use_pad ? "on" : "off");
}

void all_records() {
    for (int nb : {16, 64}) {
        std::vector<Record> recs;
        for (size_t nnz : {0u, 1u, 63u, 64u, 65u, 257u, 1000u}) { recs.push_back(plain_record(nnz, false)); recs.push_back(plain_record(nnz, true)); }
        for (int special = 0; special < 4; special++) recs.push_back(diag_record(nb, special, nb, special));
        recs.push_back(diag_record(nb, 4, nb - 5, 2)); // the last block: five tail rows without entries
        recs.push_back(diag_record(nb, 5, 0, 0));      // no stored pivot at all
        std::vector<unsigned char> pad((size_t)6 * nb, 0);
        for (size_t i = 0; i < pad.size(); i += 7) pad[i] = 1;
        pad[(size_t)1 * nb + 5] = 1; // (the zero pivot of special 1 is a padding row under the mask: the product is not zero then)
        check_records(nb, recs, pad, false);
        check_records(nb, recs, pad, true);
    }
}

// ---- vectors -------------------------------------------------------------------------------------------------------------------------
val_t sign_of(val_t v) {
#ifdef PANGULU_COMPLEX
    const double a = std::hypot(v.re, v.im);
    return a > std::numeric_limits<double>::min() ? val_t{v.re / a, v.im / a} : val_t{1.0, 0.0};
#else
    return std::signbit(v) ? -1.0 : 1.0;
#endif
}

CondestResultD run_norm1(std::vector<val_t> &x, std::vector<val_t> *save, bool with_sign, bool compared) {
    const unsigned long long n = x.size(); const unsigned g = condest_groups(n);
    std::vector<CondestPartialD> part(CONDEST_MAX_GROUPS); CondestResultD res; memset(&res, 0xff, sizeof(res));
    launch(g, [&] { condest_norm1_kernel(x.data(), save ? save->data() : nullptr, n, with_sign ? 1 : 0, g, part.data()); });
    launch(1, [&] { condest_last_kernel(CONDEST_LAST_NORM1, part.data(), g, x.data(), n, 0ull, compared ? 1 : 0, &res); });
    return res;
}
CondestResultD run_argmax(const std::vector<val_t> &x, unsigned long long jprev) {
    const unsigned long long n = x.size(); const unsigned g = condest_groups(n);
    std::vector<CondestPartialD> part(CONDEST_MAX_GROUPS); CondestResultD res; memset(&res, 0xff, sizeof(res));
    launch(g, [&] { condest_argmax_kernel(x.data(), n, g, part.data()); });
    launch(1, [&] { condest_last_kernel(CONDEST_LAST_ARGMAX, part.data(), g, x.data(), n, jprev, 0, &res); });
    return res;
}
void run_fill(int what, std::vector<val_t> &x, unsigned long long j) {
    const unsigned long long n = x.size(); const unsigned g = condest_groups(n);
    launch(g, [&] { condest_fill_kernel(what, x.data(), n, j, g); });
}

void check_vector(size_t n, int special) {
    std::vector<val_t> x(n);
    for (auto &v : x) v = vrand(2.0);
    if (special == 1 && n > 2600) { x[700] = vmk(-9.0, 0.0); x[2600] = vmk(9.0, 0.0); } // equal maxima in different workgroups: the first wins
    if (special == 2) x[n - 1] = vmk(QNAN, 0.0);
    if (special == 3) { x[n / 2] = vmk(0.0, 0.0); x[0] = vmk(-0.0, 0.0); }
    const std::vector<val_t> x0 = x;
    // argmax
    unsigned long long want_j = 0; double best = -2;
    for (size_t i = 0; i < n; i++) { const double a = vmod(x0[i]), key = a == a ? a : -1.0; if (key > best) { best = key; want_j = i; } }
    const unsigned long long jprev = n / 3;
    CondestResultD r = run_argmax(x, jprev);
    CHECK(r.argmax == want_j, "n=%zu special %d: argmax %llu, expected the first maximum %llu", n, special, r.argmax, want_j);
    CHECK(r.absmax == vmod(x0[want_j]) && (r.abs_prev == vmod(x0[jprev]) || (special == 2 && jprev == n - 1)), "n=%zu special %d: |x_j| / |x_jprev| %g %g", n, special, r.absmax, r.abs_prev);
    CHECK(memcmp(x.data(), x0.data(), sizeof(val_t) * n) == 0, "n=%zu: argmax wrote to x", n);
    // plain norm
    double sum = 0; for (const val_t &v : x0) sum += vmod(v);
    r = run_norm1(x, nullptr, false, false);
    if (special == 2) CHECK(r.norm1 != r.norm1, "n=%zu: a NaN entry left the norm %g", n, r.norm1);
    else CHECK(std::fabs(r.norm1 - sum) <= (double)n * EPS * sum, "n=%zu special %d: norm %.17g, serial %.17g", n, special, r.norm1, sum);
    CHECK(memcmp(x.data(), x0.data(), sizeof(val_t) * n) == 0, "n=%zu: the plain norm wrote to x", n);
    // norm + signs, first time (nothing to compare), then the same signs again (unchanged), then one sign flipped
    std::vector<val_t> save(n, vmk(QNAN, QNAN));
    CondestResultD r1 = run_norm1(x, &save, true, false);
    CHECK(r1.unchanged == 0, "n=%zu: 'unchanged' without a comparison", n);
    if (special != 2) CHECK(r1.norm1 == r.norm1, "n=%zu: the two norm steps differ in bits: %.17g %.17g", n, r1.norm1, r.norm1);
    for (size_t i = 0; i < n; i++) {
        CHECK(same_bits(x[i], sign_of(x0[i])), "n=%zu special %d: sign of entry %zu", n, special, i);
#ifndef PANGULU_COMPLEX
        CHECK(same_bits(save[i], x[i]), "n=%zu: saved sign %zu", n, i);
#endif
    }
#ifndef PANGULU_COMPLEX
    if (special != 2) {
        x = x0; for (auto &v : x) v = v * 0.5; // other values, the same signs
        CondestResultD r2 = run_norm1(x, &save, true, true);
        CHECK(r2.unchanged == 1, "n=%zu special %d: the same signs were not recognised", n, special);
        x = x0; x[n - 1] = x0[n - 1] == 0 ? -1.0 : -x0[n - 1]; // the last sign flips
        r2 = run_norm1(x, &save, true, true);
        CHECK(r2.unchanged == 0, "n=%zu special %d: a flipped sign at the last index went unnoticed", n, special);
    }
#else
    CondestResultD r2 = run_norm1(x, &save, true, true);
    CHECK(r2.unchanged == 0, "n=%zu: complex types have no sign test", n);
#endif
    // the fills
    const val_t poison = vmk(QNAN, QNAN);
    x.assign(n, poison); run_fill(CONDEST_FILL_INV_N, x, 0);
    for (size_t i = 0; i < n; i++) CHECK(same_bits(x[i], vmk(1.0 / (double)n, 0.0)), "n=%zu: 1/n at %zu", n, i);
    x.assign(n, poison); run_fill(CONDEST_SET_EJ, x, want_j);
    for (size_t i = 0; i < n; i++) CHECK(same_bits(x[i], vmk(i == want_j ? 1.0 : 0.0, 0.0)), "n=%zu: e_j at %zu", n, i);
    x.assign(n, poison); run_fill(CONDEST_FILL_ALT, x, 0);
    for (size_t i = 0; i < n; i++) {
        const double v = 1.0 + (double)i / (double)(n > 1 ? n - 1 : 1);
        CHECK(same_bits(x[i], vmk((i & 1) ? -v : v, 0.0)), "n=%zu: alternating vector at %zu", n, i);
    }
    printf("vector: n=%zu special %d, %u workgroups\n", n, special, condest_groups(n));
}

int main() {
    all_records();
    for (size_t n : {1u, 63u, 64u, 65u, 257u}) check_vector(n, 0);
    check_vector(2744, 1); // (more than one workgroup per grid stride; random values but for the two maxima)
    check_vector(2744, 2);
    check_vector(65, 2);
    check_vector(257, 3);
    printf("%d failures %s\n", failures, failures == 0 ? "OK" : "FAIL");
    return failures == 0 ? 0 : 1;
}
