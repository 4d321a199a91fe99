// The transposed sweeps of the panel solve kernels of pangulu_amd/csrc/platform/pg_hip_block_solve_multi.h run on the CPU
// (tests/test_solve_trans_kernels_cpu.py).  Same method and the same shims as tests/solve_multi_kernel_emulation.cpp
// (tests/hip_emulation_shims.h): the header is compiled as plain C++ and a random block-sparse L (unit) and U are swept level by level the way pangulu_platform_0201001_block_trsm_multi_trans does: forward with U^T, then backward with L^T, gather
// launch then level launch.  The result is compared with dense substitution with U^T / L^T (U^H / L^H with CONJ) per right-hand side.
// One row of U holds nothing but a diagonal below PANGULU_SPTRSV_TOL: the kernel must divide by the clamp there.  It checks the
// kernels' indexing and arithmetic; it says nothing about the device.
#include "hip_emulation_shims.h"
#include "pg_hip_solve_arith.h"
#include "pg_hip_block_solve_multi.h"

struct Blk { std::vector<u32> cp; std::vector<u16> ri; std::vector<val_t> val; };
std::mt19937_64 rng(54321);
double urand() { return std::uniform_real_distribution<double>(-1, 1)(rng); }
val_t vrand(double s) {
#ifdef PANGULU_COMPLEX
    return val_t{s * urand(), s * urand()};
#else
    return s * urand();
#endif
}
template <bool CONJ> val_t op(val_t v) { return CONJ ? v_conj(v) : v; }
// the divisor the sweeps use for a diagonal entry: the clamp replaces a diagonal whose real part is within PANGULU_SPTRSV_TOL of zero
inline val_t clamped(val_t d) { return std::fabs(v_realpart(d)) > PANGULU_SPTRSV_TOL ? d : v_make(PANGULU_SPTRSV_TOL); }

template <int W, bool CONJ> double run(int nb, int nbk, double dens) {
    const int n = nb * nbk;
    const int k0 = 1, r0 = 2, g0 = k0 * nb + r0; // the row of U that holds nothing but a diagonal below the clamp; row g0 of L is empty too,
                                                 // so that the huge x[g0] stays where it is and the other values keep their scale
    std::vector<val_t> A((size_t)n * n, v_make(0)); // dense copy, column-major: L strictly lower (unit), U upper
    std::vector<std::vector<Blk>> off(nbk, std::vector<Blk>(nbk));
    std::vector<std::vector<char>> has(nbk, std::vector<char>(nbk, 0));
    for (int br = 0; br < nbk; br++) for (int bc = 0; bc < nbk; bc++) {
        if (br == bc || urand() > 0.3) continue;
        has[br][bc] = 1; Blk &B = off[br][bc]; B.cp.assign(nb + 1, 0);
        // (columns of very different lengths: some empty, some nearly full, so that lane groups of one wavefront run different trip counts)
        for (int c = 0; c < nb; c++) { const double dc = c % 5 == 0 ? 0.0 : c % 7 == 0 ? 0.45 : dens;
            for (int r = 0; r < nb; r++) if (!(br == k0 && r == r0) && urand() > 1 - 2 * dc) { val_t v = vrand(0.3 / (nb * dens + 1)); B.ri.push_back(r); B.val.push_back(v); A[(size_t)(bc * nb + c) * n + br * nb + r] = v; } B.cp[c + 1] = B.ri.size(); }
        B.cp[0] = 0xdeadbeef; // (colptr[0] is treated as 0)
    }
    std::vector<Blk> dl(nbk), du(nbk);
    for (int k = 0; k < nbk; k++) {
        Blk &L = dl[k]; L.cp.assign(nb + 1, 0);
        for (int c = 0; c < nb; c++) { for (int r = c + 1; r < nb; r++) if (!(k == k0 && r == r0) && urand() > 1 - 2 * dens) { val_t v = vrand(0.5 / (nb * dens + 1)); L.ri.push_back(r); L.val.push_back(v); A[(size_t)(k * nb + c) * n + k * nb + r] = v; } L.cp[c + 1] = L.ri.size(); }
        L.cp[0] = 0xdeadbeef;
        Blk &U = du[k]; U.cp.assign(nb + 1, 0); // CSR, diagonal first
        for (int r = 0; r < nb; r++) {
            if (k == nbk - 1 && r == nb - 2) { U.cp[r + 1] = U.ri.size(); A[(size_t)(k * nb + r) * n + k * nb + r] = v_make(1); continue; } // an empty row record: skipped, x stays
            val_t d = vrand(1.0);
#ifdef PANGULU_COMPLEX
            d.re += d.re < 0 ? -1.5 : 1.5;
            if (k == k0 && r == r0) d = val_t{1e-20, 0.3};
#else
            d += d < 0 ? -1.5 : 1.5;
            if (k == k0 && r == r0) d = 1e-20;
#endif
            U.ri.push_back(r); U.val.push_back(d); A[(size_t)(k * nb + r) * n + k * nb + r] = d;
            if (!(k == k0 && r == r0))
                for (int c = r + 1; c < nb; c++) if (urand() > 1 - 2 * dens) { val_t v = vrand(0.5 / (nb * dens + 1)); U.ri.push_back(c); U.val.push_back(v); A[(size_t)(k * nb + c) * n + k * nb + r] = v; }
            U.cp[r + 1] = U.ri.size(); }
    }
    // rhs panel and reference: forward with op(U)^T, backward with op(L)^T (unit), per rhs
    std::vector<val_t> X((size_t)n * W), ref((size_t)n * W);
    for (auto &v : X) v = vrand(1.0);
    for (int i = 0; i < n; i++) X[(size_t)i * W + (W > 1 ? 1 : 0)] = W > 1 ? v_make(0) : X[(size_t)i * W];
    ref = X;
    for (int r = 0; r < W; r++) {
        for (int i = 0; i < n; i++) { val_t acc = ref[(size_t)i * W + r]; for (int k = 0; k < i; k++) acc = v_submul(acc, op<CONJ>(A[(size_t)i * n + k]), ref[(size_t)k * W + r]);
            ref[(size_t)i * W + r] = v_div(acc, clamped(op<CONJ>(A[(size_t)i * n + i]))); }
        for (int i = n - 1; i >= 0; i--) { val_t acc = ref[(size_t)i * W + r]; for (int k = i + 1; k < n; k++) acc = v_submul(acc, op<CONJ>(A[(size_t)i * n + k]), ref[(size_t)k * W + r]); ref[(size_t)i * W + r] = acc; }
    }
    const size_t budget = 96 << 10;
    const int ch = std::min(solve_multi_chunk(nb, W, budget), 3); // (small: several chunks even at small nb)
    if (solve_trans_lds_gather(nb, W) > solve_multi_lds_gather(nb, W)) { printf("the transposed gather asks for more LDS than its twin\n"); exit(1); }
    if (solve_multi_lds_gather(nb, W) > sizeof(smem_raw) || solve_multi_lds_level(nb, W, ch) > sizeof(smem_raw)) { printf("lds too large\n"); exit(1); }
    for (int pass = 0; pass < 2; pass++) {
        const bool forward = pass == 0; // segment i reads the segments k of the blocks (k, i): k < i forward, k > i backward
        std::vector<int> level(nbk, 0); int nlevel = 0;
        for (int s = 0; s < nbk; s++) { int i = forward ? s : nbk - 1 - s, lv = 0; for (int k = 0; k < nbk; k++) if (has[k][i] && (forward ? k < i : k > i)) lv = std::max(lv, level[k] + 1); level[i] = lv; nlevel = std::max(nlevel, lv + 1); }
        for (int l = 0; l < nlevel; l++) {
            std::vector<SolveBlkD> blks; std::vector<SolveRowD> rows;
            for (int i = 0; i < nbk; i++) if (level[i] == l) {
                const Blk &D = forward ? du[i] : dl[i];
                rows.push_back(SolveRowD{(u32)i, 0, 0, D.cp.data(), D.ri.data(), D.val.data()});
                for (int k = 0; k < nbk; k++) if (has[k][i] && (forward ? k < i : k > i)) { const Blk &B = off[k][i]; blks.push_back(SolveBlkD{B.cp.data(), B.ri.data(), B.val.data(), (u32)k, (u32)i}); }
            }
            if (!blks.empty()) launch((unsigned)blks.size(), [&] { block_trsm_gather_trans_kernel<W, CONJ>(blks.data(), nb, X.data()); });
            if (forward) launch((unsigned)rows.size(), [&] { block_trsm_level_kernel<SOLVE_UT, W, CONJ>(rows.data(), nb, X.data(), ch); });
            else launch((unsigned)rows.size(), [&] { block_trsm_level_kernel<SOLVE_LT, W, CONJ>(rows.data(), nb, X.data(), ch); });
        }
    }
    // the clamped row on its own scale (about 1e16), everything else on the scale of the rest
    double err = 0, scale = 0, err0 = 0, scale0 = 0;
    for (size_t i = 0; i < X.size(); i++) {
        const double e = vabs(v_sub(X[i], ref[i])), s = vabs(ref[i]);
        if ((int)(i / W) == g0) { err0 = std::max(err0, e); scale0 = std::max(scale0, s); }
        else { err = std::max(err, e); scale = std::max(scale, s); }
    }
    if (!(scale0 > 1e12)) { printf("the clamped row did not reach the clamp's scale (%g)\n", scale0); return 1; }
    if (W > 1) for (int i = 0; i < n; i++) if (vabs(X[(size_t)i * W + 1]) != 0) { printf("zero column not zero\n"); return 1; }
    return std::max(err / scale, err0 / scale0);
}
int main() {
    double worst = 0;
#define RUN(W, C, nb, nbk) { double e = run<W, C>(nb, nbk, 0.15); printf("W=%d conj=%d nb=%d nbk=%d rel err %.2e\n", W, (int)C, nb, nbk, e); worst = std::max(worst, e); }
    RUN(1, false, 37, 5) RUN(2, false, 37, 5) RUN(4, false, 40, 6) RUN(8, false, 33, 5) RUN(4, false, 7, 4)
#ifdef PANGULU_COMPLEX
    RUN(1, true, 37, 5) RUN(2, true, 37, 5) RUN(4, true, 40, 6) RUN(8, true, 33, 5) RUN(16, true, 37, 5) RUN(4, true, 7, 4)
#endif
    RUN(16, false, 37, 5)
    printf("worst %.2e %s\n", worst, worst < 1e-12 ? "OK" : "FAIL");
    return worst < 1e-12 ? 0 : 1;
}
