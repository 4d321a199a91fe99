// The reproducible gather pair of pangulu_amd/csrc/platform/pg_hip_block_solve_multi.h (solve_gather_part_kernel,
// solve_gather_sum_kernel: what pangulu_amd_rcond's solves use instead of the atomic gathers) run on the CPU
// (tests/test_factor_stats.py), behind the shims of tests/hip_emulation_shims.h: one level with four segments that own 3, 0, 1 and 5
// blocks, blocks with empty, short and full columns, nb = 16, 64 and 100, untransposed and transposed (complex build: conjugated as
// well).  Checked: every value of the partial buffer is written; x_row - sum_b op(B_b) x_src against the serial formula within
// (entries + blocks) 2^-53 of the sum of the terms' moduli; segments that are not destinations keep their bits; and two runs -- 256
// host threads scheduled as they come -- give the same bits.
#include "hip_emulation_shims.h"
#include "pg_hip_solve_arith.h"
#include "pg_hip_block_solve_multi.h"

#include <limits>

std::mt19937_64 rng(20261022);
double urand() { return std::uniform_real_distribution<double>(-1, 1)(rng); }
val_t vrand() {
#ifdef PANGULU_COMPLEX
    return val_t{urand(), urand()};
#else
    return urand();
#endif
}
val_t vnan() { return v_make(std::numeric_limits<double>::quiet_NaN()); }
int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Blk { std::vector<u32> cp; std::vector<u16> ri; std::vector<val_t> val; u32 bcol, brow; };

Blk make_block(int nb, int kind, u32 brow, u32 bcol) {
    Blk B; B.brow = brow; B.bcol = bcol; B.cp.assign(nb + 1, 0);
    for (int c = 0; c < nb; c++) {
        int len = kind == 0 ? (int)(rng() % 4) : kind == 1 ? nb : (c % 3 == 0 ? 0 : (int)(rng() % (unsigned)nb)); // short, full, mixed with empty columns
        std::vector<u16> rows(nb); for (int i = 0; i < nb; i++) rows[i] = (u16)i;
        std::shuffle(rows.begin(), rows.end(), rng); rows.resize(len); std::sort(rows.begin(), rows.end());
        for (u16 r : rows) { B.ri.push_back(r); B.val.push_back(vrand()); }
        B.cp[c + 1] = (u32)B.ri.size();
    }
    if (B.ri.empty()) { B.ri.push_back(0); B.val.push_back(v_make(0)); } // (data() of an empty vector may be null)
    return B;
}

template <bool TRANS, bool CONJ> void run(int nb) {
    const int nseg = 12;                       // segments 0 .. 7 are sources, 8 .. 11 the level's destinations
    const int nblk_of[4] = {3, 0, 1, 5};
    std::vector<Blk> blocks;
    std::vector<SolveRowD> rows(4);
    const unsigned long long level_first = 7; // (the level's blocks do not start the sweep's list)
    for (int r = 0; r < 4; r++) {
        rows[r].brow = 8 + r; rows[r].nblk = nblk_of[r]; rows[r].first = level_first + blocks.size();
        rows[r].dptr = nullptr; rows[r].didx = nullptr; rows[r].dval = nullptr;
        for (int b = 0; b < nblk_of[r]; b++) blocks.push_back(make_block(nb, (int)((blocks.size() + r) % 3), 8 + r, (u32)(rng() % 8)));
    }
    std::vector<SolveBlkD> blks(blocks.size());
    for (size_t b = 0; b < blocks.size(); b++) {
        blocks[b].cp[0] = 0xdeadbeefu; // (entry 0 of a column pointer array is not the kernels' to read)
        blks[b] = SolveBlkD{blocks[b].cp.data(), blocks[b].ri.data(), blocks[b].val.data(), blocks[b].bcol, blocks[b].brow};
    }
    std::vector<val_t> x0((size_t)nseg * nb);
    for (auto &v : x0) v = vrand();
    std::vector<val_t> got[2];
    for (int rep = 0; rep < 2; rep++) {
        std::vector<val_t> x = x0, part(blocks.size() * nb, vnan());
        launch((unsigned)blocks.size(), [&] { solve_gather_part_kernel<TRANS, CONJ>(blks.data(), nb, x.data(), part.data()); });
        for (size_t k = 0; k < part.size(); k++) CHECK(vabs(part[k]) == vabs(part[k]), "nb=%d trans=%d: partial %zu was not written", nb, (int)TRANS, k);
        launch(4, [&] { solve_gather_sum_kernel(rows.data(), level_first, nb, part.data(), x.data()); });
        got[rep] = x;
    }
    CHECK(memcmp(got[0].data(), got[1].data(), sizeof(val_t) * got[0].size()) == 0, "nb=%d trans=%d conj=%d: two runs differ in bits", nb, (int)TRANS, (int)CONJ);
    CHECK(memcmp(got[0].data(), x0.data(), sizeof(val_t) * 8 * nb) == 0, "nb=%d trans=%d: a source segment changed", nb, (int)TRANS);
    // the serial formula with the sum of the terms' moduli as the scale of the error
    double worst = 0;
    for (int r = 0; r < 4; r++) {
        std::vector<val_t> want(x0.begin() + (size_t)(8 + r) * nb, x0.begin() + (size_t)(9 + r) * nb);
        std::vector<double> scale(nb, 0.0), terms(nb, 1.0);
        for (int i = 0; i < nb; i++) scale[i] = vabs(want[i]);
        for (int b = 0; b < nblk_of[r]; b++) {
            const Blk &B = blocks[rows[r].first - level_first + b];
            const val_t *xs = x0.data() + (size_t)B.bcol * nb;
            for (int c = 0; c < nb; c++) for (u32 p = c == 0 ? 0 : B.cp[c]; p < B.cp[c + 1]; p++) {
                const int dst = TRANS ? c : B.ri[p], src = TRANS ? B.ri[p] : c;
                const val_t t = v_mul(CONJ ? v_conj(B.val[p]) : B.val[p], xs[src]);
                want[dst] = v_sub(want[dst], t); scale[dst] += vabs(t); terms[dst] += 2;
            }
        }
        for (int i = 0; i < nb; i++) {
            const double err = vabs(v_sub(got[0][(size_t)(8 + r) * nb + i], want[i]));
            CHECK(err <= 2.0 * terms[i] * 1.1102230246251565e-16 * scale[i], "nb=%d trans=%d conj=%d segment %d row %d: off by %g (scale %g, %g terms)", nb, (int)TRANS, (int)CONJ, 8 + r, i, err, scale[i], terms[i]);
            worst = std::max(worst, scale[i] > 0 ? err / scale[i] : 0.0);
        }
    }
    printf("nb=%d trans=%d conj=%d: %zu blocks, worst error %.2e of the terms' sum\n", nb, (int)TRANS, (int)CONJ, blocks.size(), worst);
}

int main() {
    for (int nb : {16, 64, 100}) {
        run<false, false>(nb);
        run<true, false>(nb);
#ifdef PANGULU_COMPLEX
        run<true, true>(nb);
#endif
    }
    printf("%d failures %s\n", failures, failures == 0 ? "OK" : "FAIL");
    return failures == 0 ? 0 : 1;
}
