// The pack / unpack kernels of pangulu_amd/csrc/platform/pg_hip_solve_pack.h run on the CPU (tests/test_solve_device_rhs_kernels_cpu.py),
// by the method and behind the shims of tests/solve_trans_kernel_emulation.cpp (tests/hip_emulation_shims.h): the header is compiled
// as plain C++, a workgroup is 256 threads.  Checked against the two formulas the header states,
//     in:   X[i * W + r] = s_in[i] * rhs[(j0 + r) * ldb + in_idx[i]]   for i < n, a non-padding row and r < nc; 0 everywhere else
//     out:  rhs[(j0 + r) * ldb + out_idx[i]] = s_out[i] * X[i * W + r]  for non-padding rows and r < nc; nothing else is written
// with exact equality: every value is one product rounded once (or a copy).  It checks indexing and arithmetic, not the device.
#include "hip_emulation_shims.h"
#include "pg_hip_solve_pack.h"

#include <cstdint>
#include <limits>
#include <numeric>

std::mt19937_64 rng(20261020);
double urand() { return std::uniform_real_distribution<double>(-1, 1)(rng); }
val_t vrand() {
#ifdef PANGULU_COMPLEX
    return val_t{urand(), urand()};
#else
    return urand();
#endif
}
val_t vnan() {
    const double q = std::numeric_limits<double>::quiet_NaN();
#ifdef PANGULU_COMPLEX
    return val_t{q, q};
#else
    return q;
#endif
}
bool same_bits(const val_t &a, const val_t &b) { return memcmp(&a, &b, sizeof(val_t)) == 0; }
bool defined(const val_t &v) {
#ifdef PANGULU_COMPLEX
    return v.re == v.re && v.im == v.im;
#else
    return v == v;
#endif
}
val_t times(val_t v, double s) { // the formula, written out here once more
#ifdef PANGULU_COMPLEX
    return val_t{v.re * s, v.im * s};
#else
    return v * s;
#endif
}

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

// n rows of which `npad` are padding rows, xlen >= n, nrhs columns with ldb = n_user + 5, the panel takes columns j0 .. j0 + nc - 1
template <int W> void run(int n, int xlen, int npad, int nrhs, int j0, int nc, bool scaled, bool identity) {
    const int n_user = n - npad, ldb = n_user + 5;
    std::vector<u32> in_idx(n), out_idx(n);
    std::vector<u32> pa(n_user), pb(n_user);
    std::iota(pa.begin(), pa.end(), 0u); std::iota(pb.begin(), pb.end(), 0u);
    if (!identity) { std::shuffle(pa.begin(), pa.end(), rng); std::shuffle(pb.begin(), pb.end(), rng); }
    // padding rows spread over the ordering (13 is coprime to both n used below: npad distinct rows)
    std::vector<char> pad(n, 0);
    for (int k = 0; k < npad; k++) pad[(size_t)((k * 13 + 5) % n)] = 1;
    int real = 0;
    for (int i = 0; i < n; i++) {
        if (pad[i]) { in_idx[i] = out_idx[i] = SOLVE_MAP_PAD; continue; }
        in_idx[i] = pa[real]; out_idx[i] = pb[real]; real++; }
    if (real != n_user) { printf("test set-up: %d of %d real rows\n", real, n_user); exit(2); }
    std::vector<double> s_in(n), s_out(n);
    for (int i = 0; i < n; i++) { s_in[i] = identity ? 1.0 : 0.5 + std::fabs(urand()); s_out[i] = identity ? 1.0 : 0.5 + std::fabs(urand()); }
    const double *ps_in = scaled ? s_in.data() : nullptr, *ps_out = scaled ? s_out.data() : nullptr;
    std::vector<val_t> rhs((size_t)ldb * nrhs);
    for (auto &v : rhs) v = vrand();
    const std::vector<val_t> rhs0 = rhs;
    std::vector<val_t> X((size_t)xlen * W, vnan());
    launch(solve_pack_grid((unsigned long long)xlen * W), [&] { solve_pack_panel_kernel<W>(rhs.data(), (unsigned long long)ldb, (u32)j0, (u32)nc, in_idx.data(), ps_in, (u32)n, (unsigned long long)xlen, X.data()); });
    for (int i = 0; i < xlen; i++) for (int r = 0; r < W; r++) {
        const val_t got = X[(size_t)i * W + r];
        CHECK(defined(got), "W=%d pack: X[%d, %d] was not written", W, i, r);
        val_t want = v_make(0);
        if (i < n && r < nc && in_idx[i] != SOLVE_MAP_PAD) { want = rhs0[(size_t)(j0 + r) * ldb + in_idx[i]]; if (scaled) want = times(want, s_in[i]); }
        CHECK(same_bits(got, want), "W=%d pack: X[%d, %d] differs from the formula", W, i, r);
    }
    CHECK(memcmp(rhs.data(), rhs0.data(), sizeof(val_t) * rhs.size()) == 0, "W=%d pack wrote to rhs", W);
    // the panel as a sweep would leave it: other values everywhere, the zero columns and tail rows included
    for (auto &v : X) v = vrand();
    const std::vector<val_t> X0 = X;
    launch(solve_pack_grid((unsigned long long)n * W), [&] { solve_unpack_panel_kernel<W>(rhs.data(), (unsigned long long)ldb, (u32)j0, (u32)nc, out_idx.data(), ps_out, (u32)n, X.data()); });
    std::vector<val_t> want = rhs0;
    for (int i = 0; i < n; i++) for (int r = 0; r < nc; r++) if (out_idx[i] != SOLVE_MAP_PAD)
        want[(size_t)(j0 + r) * ldb + out_idx[i]] = scaled ? times(X0[(size_t)i * W + r], s_out[i]) : X0[(size_t)i * W + r];
    for (int j = 0; j < nrhs; j++) for (int i = 0; i < ldb; i++)
        CHECK(same_bits(rhs[(size_t)j * ldb + i], want[(size_t)j * ldb + i]), "W=%d unpack: rhs[%d, column %d] %s", W, i, j,
              (j < j0 || j >= j0 + nc) ? "lies in a column outside the panel and changed" : i >= n_user ? "is a spare row and changed" : "differs from the formula");
    CHECK(memcmp(X.data(), X0.data(), sizeof(val_t) * X.size()) == 0, "W=%d unpack wrote to the panel", W);
    if (identity) {
        // pack then unpack with identity maps and unit scales gives the columns back bit for bit
        rhs = rhs0;
        launch(solve_pack_grid((unsigned long long)xlen * W), [&] { solve_pack_panel_kernel<W>(rhs.data(), (unsigned long long)ldb, (u32)j0, (u32)nc, in_idx.data(), ps_in, (u32)n, (unsigned long long)xlen, X.data()); });
        for (int r = 0; r < nc; r++) for (int i = 0; i < n_user; i++) rhs[(size_t)(j0 + r) * ldb + i] = vnan();
        launch(solve_pack_grid((unsigned long long)n * W), [&] { solve_unpack_panel_kernel<W>(rhs.data(), (unsigned long long)ldb, (u32)j0, (u32)nc, out_idx.data(), ps_out, (u32)n, X.data()); });
        CHECK(memcmp(rhs.data(), rhs0.data(), sizeof(val_t) * rhs.size()) == 0, "W=%d: the round trip through the panel changed bits", W);
    }
    printf("W=%d n=%d xlen=%d padding=%d columns [%d, %d) of %d scaled=%d identity=%d\n", W, n, xlen, npad, j0, j0 + nc, nrhs, (int)scaled, (int)identity);
}

template <int W> void all() {
    const int n = 77, xlen = 96; // (n no multiple of the workgroup's 256 / W rows; a tail of 19 rows up to the block boundary)
    run<W>(n, xlen, 6, W + 3, 0, W, true, false);                 // a full panel, scaled, padding rows
    run<W>(n, xlen, 6, W + 3, 2, W > 1 ? W - 1 : 1, true, false); // nc < W (where W > 1), j0 > 0
    run<W>(n, xlen, 6, W + 3, 3, W > 2 ? W / 2 + 1 : 1, false, false); // no scale arrays
    run<W>(n, xlen, 0, W + 3, 1, W, true, true);                  // identity maps, unit scales: the round trip
    run<W>(n, xlen, 0, W + 3, 1, W, false, true);
    run<W>(300, 320, 9, W + 1, 1, W, true, false);                // more than one workgroup even at W = 1
}

int main() {
    all<1>(); all<2>(); all<4>(); all<8>();
#ifndef PANGULU_COMPLEX
    all<16>(); // (a tile row is at most 128 bytes: 16 real values, 8 double-complex ones)
#endif
    printf("%d failures %s\n", failures, failures == 0 ? "OK" : "FAIL");
    return failures == 0 ? 0 : 1;
}
