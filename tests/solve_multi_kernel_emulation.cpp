// The panel solve kernels of pangulu_amd/csrc/platform/pg_hip_block_solve_multi.h run on the CPU (tests/test_solve_multi_kernels_cpu.py):
// the header is compiled as plain C++ behind a few shims (tests/hip_emulation_shims.h) -- a workgroup is 256 std::threads, __syncthreads /
// wave_lds_fence / __shfl_down are barriers over the workgroup / the wavefront, atomics are compare-and-swap loops, the LDS is one array -- and a random
// block-sparse L (unit) and U are swept level by level, gather launch then level launch, like pangulu_platform_0201001_block_trsm_multi
// does.  The result is compared with dense substitution per right-hand side.  It checks the kernels' indexing and arithmetic for every
// panel width, block orders that are no multiple of anything and several chunks per diagonal half; it says nothing about the device.
// W = 1 is what pangulu_gstrs launches (pangulu_platform_0201001_block_trsv and a width-1 panel of block_trsm_multi alike): the
// default single-vector kernels are tested here too.
#include "hip_emulation_shims.h"
#include "pg_hip_solve_arith.h"
#include "pg_hip_block_solve_multi.h"

struct Blk { std::vector<u32> cp; std::vector<u16> ri; std::vector<val_t> val; };
std::mt19937_64 rng(12345);
double urand() { return std::uniform_real_distribution<double>(-1, 1)(rng); }
val_t vrand(double s) {
#ifdef PANGULU_COMPLEX
    return val_t{s * urand(), s * urand()};
#else
    return s * urand();
#endif
}
template <int W> double run(int nb, int nbk, double dens) {
    const int n = nb * nbk;
    std::vector<val_t> A((size_t)n * n, v_make(0)); // dense copy, column-major: L strictly lower (unit), U upper
    // off-diagonal blocks (CSC), lower: brow > bcol, upper: brow < bcol
    std::vector<std::vector<Blk>> off(nbk, std::vector<Blk>(nbk));
    std::vector<std::vector<char>> has(nbk, std::vector<char>(nbk, 0));
    for (int br = 0; br < nbk; br++) for (int bc = 0; bc < nbk; bc++) {
        if (br == bc || urand() > 0.2) continue;
        has[br][bc] = 1; Blk &B = off[br][bc]; B.cp.assign(nb + 1, 0);
        for (int c = 0; c < nb; c++) { for (int r = 0; r < nb; r++) if (urand() > 1 - 2 * dens) { val_t v = vrand(0.3 / (nb * dens + 1)); B.ri.push_back(r); B.val.push_back(v); A[(size_t)(bc * nb + c) * n + br * nb + r] = v; } B.cp[c + 1] = B.ri.size(); }
        B.cp[0] = 0xdeadbeef; // (colptr[0] is treated as 0)
    }
    std::vector<Blk> dl(nbk), du(nbk);
    for (int k = 0; k < nbk; k++) {
        Blk &L = dl[k]; L.cp.assign(nb + 1, 0);
        for (int c = 0; c < nb; c++) { for (int r = c + 1; r < nb; r++) if (urand() > 1 - 2 * dens) { val_t v = vrand(0.5 / (nb * dens + 1)); L.ri.push_back(r); L.val.push_back(v); A[(size_t)(k * nb + c) * n + k * nb + r] = v; } L.cp[c + 1] = L.ri.size(); }
        L.cp[0] = 0xdeadbeef;
        Blk &U = du[k]; U.cp.assign(nb + 1, 0); // CSR, diagonal first
        for (int r = 0; r < nb; r++) { val_t d = vrand(1.0);
#ifdef PANGULU_COMPLEX
            d.re += d.re < 0 ? -1.5 : 1.5;
#else
            d += d < 0 ? -1.5 : 1.5;
#endif
            U.ri.push_back(r); U.val.push_back(d); A[(size_t)(k * nb + r) * n + k * nb + r] = d;
            for (int c = r + 1; c < nb; c++) if (urand() > 1 - 2 * dens) { val_t v = vrand(0.5 / (nb * dens + 1)); U.ri.push_back(c); U.val.push_back(v); A[(size_t)(k * nb + c) * n + k * nb + r] = v; }
            U.cp[r + 1] = U.ri.size(); }
    }
    // rhs panel and reference (dense forward with unit L, backward with U), per rhs
    std::vector<val_t> X((size_t)n * W), ref((size_t)n * W);
    for (auto &v : X) v = vrand(1.0);
    for (int i = 0; i < n; i++) X[(size_t)i * W + (W > 1 ? 1 : 0)] = W > 1 ? v_make(0) : X[(size_t)i * W];
    ref = X;
    for (int r = 0; r < W; r++) {
        for (int c = 0; c < n; c++) for (int i = c + 1; i < n; i++) ref[(size_t)i * W + r] = v_submul(ref[(size_t)i * W + r], A[(size_t)c * n + i], ref[(size_t)c * W + r]);
        for (int i = n - 1; i >= 0; i--) { val_t acc = ref[(size_t)i * W + r]; for (int c = i + 1; c < n; c++) acc = v_submul(acc, A[(size_t)c * n + i], ref[(size_t)c * W + r]); ref[(size_t)i * W + r] = v_div(acc, A[(size_t)i * n + i]); }
    }
    const size_t budget = 96 << 10;
    const int ch = std::min(solve_multi_chunk(nb, W, budget), 3); // (small: several chunks even at small nb)
    if (solve_multi_lds_gather(nb, W) > sizeof(smem_raw) || solve_multi_lds_level(nb, W, ch) > sizeof(smem_raw)) { printf("lds too large\n"); exit(1); }
    for (int pass = 0; pass < 2; pass++) {
        const bool lower = pass == 0;
        std::vector<int> level(nbk, 0); int nlevel = 0;
        for (int s = 0; s < nbk; s++) { int br = lower ? s : nbk - 1 - s, lv = 0; for (int bc = 0; bc < nbk; bc++) if (has[br][bc] && (lower ? bc < br : bc > br)) lv = std::max(lv, level[bc] + 1); level[br] = lv; nlevel = std::max(nlevel, lv + 1); }
        for (int l = 0; l < nlevel; l++) {
            std::vector<SolveBlkD> blks; std::vector<SolveRowD> rows;
            for (int br = 0; br < nbk; br++) if (level[br] == l) {
                const Blk &D = lower ? dl[br] : du[br];
                rows.push_back(SolveRowD{(u32)br, 0, 0, D.cp.data(), D.ri.data(), D.val.data()});
                for (int bc = 0; bc < nbk; bc++) if (has[br][bc] && (lower ? bc < br : bc > br)) { const Blk &B = off[br][bc]; blks.push_back(SolveBlkD{B.cp.data(), B.ri.data(), B.val.data(), (u32)bc, (u32)br}); }
            }
            if (!blks.empty()) launch((unsigned)blks.size(), [&] { block_trsm_gather_multi_kernel<W>(blks.data(), nb, X.data()); });
            if (lower) launch((unsigned)rows.size(), [&] { block_trsm_level_kernel<SOLVE_LOWER, W, false>(rows.data(), nb, X.data(), ch); });
            else launch((unsigned)rows.size(), [&] { block_trsm_level_kernel<SOLVE_UPPER, W, false>(rows.data(), nb, X.data(), ch); });
        }
    }
    double err = 0, scale = 0;
    for (size_t i = 0; i < X.size(); i++) { err = std::max(err, vabs(v_sub(X[i], ref[i]))); scale = std::max(scale, vabs(ref[i])); }
    if (W > 1) for (int i = 0; i < n; i++) if (vabs(X[(size_t)i * W + 1]) != 0) { printf("zero column not zero\n"); return 1; }
    return err / scale;
}
int main() {
    double worst = 0;
#define RUN(W, nb, nbk) { double e = run<W>(nb, nbk, 0.15); printf("W=%d nb=%d nbk=%d rel err %.2e\n", W, nb, nbk, e); worst = std::max(worst, e); }
    RUN(1, 37, 5) RUN(2, 37, 5) RUN(4, 40, 6) RUN(8, 33, 5)
#ifndef PANGULU_COMPLEX
    RUN(16, 37, 5)
#endif
    RUN(4, 7, 4)
    printf("worst %.2e %s\n", worst, worst < 1e-12 ? "OK" : "FAIL");
    return worst < 1e-12 ? 0 : 1;
}
