// The two kernels of pangulu_amd/csrc/platform/pg_hip_values_refresh.h run on the CPU (tests/test_update_values_device_kernels_cpu.py),
// by the method and behind the shims of tests/solve_device_rhs_kernel_emulation.cpp (tests/hip_emulation_shims.h): the header is
// compiled as plain C++, a workgroup is 256 threads.  An arena of three chunks holds records (32-byte header, values, index arrays)
// of 0, 1, 3, 1000, 16 389 and 65 536 values; value areas are prefilled with NaN, everything else with a sentinel byte.  After
// values_clear_kernel and values_scatter_kernel every value must equal, bit for bit, what the serial statement of the header gives
//     zero everywhere in a value area;  then arena[user_dst[p]] = src[p];  then arena[const_dst[c]] = const_value[c]
// no NaN may be left and no sentinel byte may have changed.  It checks indexing and stores, not the device.
#include "hip_emulation_shims.h"
thread_local dim3e gridDim; // (the shims have threadIdx and blockIdx; these kernels stride by the grid)
#include "pg_hip_values_refresh.h"

#include <cstdint>
#include <limits>

std::mt19937_64 rng(20261021);
double urand() { return std::uniform_real_distribution<double>(-1, 1)(rng); }
val_t vrand() {
#ifdef PANGULU_COMPLEX
    return val_t{urand(), urand()};
#else
    return urand();
#endif
}
val_t vreal(double r) {
#ifdef PANGULU_COMPLEX
    return val_t{r, 0.0};
#else
    return r;
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

int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)
#define SETUP(cond, what) do { if (!(cond)) { printf("test set-up: %s\n", what); exit(2); } } while (0)

// one launch with the grid the kernels read from gridDim
template <class F> void launch_grid(unsigned grid, F f) { launch(grid, [=] { gridDim.x = grid; f(); }); }

constexpr unsigned char SENTINEL = 0xA5;
constexpr size_t V = sizeof(val_t);
struct Rec { u64 first, count; }; // value area: `count` values from arena offset `first`

// `slice_max` values per slice at most; `pow2`: the chunk length in values is a power of two (the shift path) or not (the division)
void run(u64 slice_max, bool pow2, unsigned clear_grid, unsigned scatter_grid) {
    const u64 vpc = pow2 ? (1ull << 17) : (1ull << 17) + 40, nchunk = 3;
    std::vector<std::vector<unsigned char>> mem(nchunk, std::vector<unsigned char>((size_t)vpc * V + 64, SENTINEL));
    std::vector<val_t *> chunks(nchunk);
    for (u64 c = 0; c < nchunk; c++) // (a 64-byte aligned base inside the allocation, as a device allocation has)
        chunks[c] = (val_t *)(((uintptr_t)mem[c].data() + 63) & ~(uintptr_t)63);
    // records one after the other as preprocess() lays them out: 64-byte aligned starts, values 32 bytes in, index arrays behind them,
    // no record across a chunk boundary
    const u64 counts[] = {3, 1000, 0, 65536, 1, 16389, 65536, 1000, 3, 16389, 65536};
    std::vector<Rec> recs;
    u64 chunk = 0, cursor = 0; // (cursor in bytes within the chunk)
    for (u64 count : counts) {
        const u64 bytes = 32 + count * V + 2 * count + 10;
        if (cursor + bytes > vpc * V) { chunk++; cursor = 0; }
        SETUP(chunk < nchunk, "the records do not fit three chunks");
        recs.push_back(Rec{chunk * vpc + (cursor + 32) / V, count});
        cursor = (cursor + bytes + 63) & ~63ull;
    }
    SETUP(chunk == 2, "the third chunk is unused");
    // ... and one value at the very end of chunk 0, so that a place at the last value of a chunk and one at the first value area of the
    // next chunk are both written
    for (const Rec &r : recs) SETUP(r.first / vpc != 0 || r.first + r.count < vpc - 1, "chunk 0 is full to its end");
    recs.push_back(Rec{vpc - 1, 1});
    u64 first_of_chunk1 = ~0ull;
    for (const Rec &r : recs) if (r.first / vpc == 1 && r.count) first_of_chunk1 = std::min(first_of_chunk1, r.first);
    std::vector<char> is_value((size_t)(nchunk * vpc), 0);
    std::vector<unsigned long long> places;
    for (const Rec &r : recs) for (u64 k = 0; k < r.count; k++) { is_value[(size_t)(r.first + k)] = 1; places.push_back(r.first + k); }
    for (unsigned long long o : places) chunks[o / vpc][o % vpc] = vreal(std::numeric_limits<double>::quiet_NaN());
    const std::vector<std::vector<unsigned char>> mem0 = mem;
    // the lists.  Slices of the value areas; of the places two in three are the user's (the two around the chunk boundary among them),
    // seven are constants -- unit diagonals and 1e-8 ones -- and the rest stays zero (fill)
    std::vector<unsigned long long> slice_off, user_dst, const_dst;
    std::vector<u32> slice_count;
    bool boundary_inside = false, odd_count = false;
    for (const Rec &r : recs) for (u64 k = 0; k < r.count; k += slice_max) {
        slice_off.push_back(r.first + k); slice_count.push_back((u32)std::min(slice_max, r.count - k));
        boundary_inside |= k > 0; odd_count |= slice_count.back() % 2 == 1 && slice_count.back() > 2; }
    SETUP(boundary_inside && odd_count, "no slice boundary inside a record, or no slice with a scalar tail");
    for (size_t k = 0; k < places.size(); k++) {
        if (places[k] == vpc - 1 || places[k] == first_of_chunk1 || k % 3 != 2) user_dst.push_back(places[k]);
        else if (const_dst.size() < 7) const_dst.push_back(places[k]);
    }
    std::shuffle(user_dst.begin(), user_dst.end(), rng);
    const size_t nuser = user_dst.size(), nconst = const_dst.size();
    std::vector<val_t> src(nuser), const_value(nconst);
    for (auto &v : src) v = vrand();
    for (size_t c = 0; c < nconst; c++) const_value[c] = vreal(c % 2 ? 1e-8 : 1.0);
    SETUP((unsigned long long)scatter_grid * 256ull < nuser, "one grid stride covers the user's list");
    int shift = -1;
    if ((vpc & (vpc - 1)) == 0) for (shift = 0; (1ull << shift) != vpc; shift++) {}
    launch_grid(clear_grid, [&] { values_clear_kernel(slice_off.data(), slice_count.data(), (unsigned long long)slice_off.size(), chunks.data(), vpc, shift); });
    for (unsigned long long o : places) CHECK(same_bits(chunks[o / vpc][o % vpc], vreal(0.0)), "after the clear kernel value %llu is not zero", o);
    launch_grid(scatter_grid, [&] { values_scatter_kernel(src.data(), user_dst.data(), (unsigned long long)nuser, const_value.data(), const_dst.data(), (unsigned long long)nconst, chunks.data(), vpc, shift); });
    // the serial statement
    std::vector<val_t> want((size_t)(nchunk * vpc), vreal(0.0));
    for (size_t p = 0; p < nuser; p++) want[(size_t)user_dst[p]] = src[p];
    for (size_t c = 0; c < nconst; c++) want[(size_t)const_dst[c]] = const_value[c];
    for (unsigned long long o : places) {
        const val_t got = chunks[o / vpc][o % vpc];
        CHECK(defined(got), "value %llu is still NaN", o);
        CHECK(same_bits(got, want[(size_t)o]), "value %llu differs from the serial formula", o);
    }
    // headers, index arrays and the room between records
    for (u64 c = 0; c < nchunk; c++) {
        const size_t lead = (size_t)((const unsigned char *)chunks[c] - mem[c].data());
        for (size_t b = 0; b < mem[c].size(); b++) {
            const bool in_value = b >= lead && b < lead + vpc * V && is_value[(size_t)(c * vpc + (b - lead) / V)];
            if (!in_value) CHECK(mem[c][b] == mem0[c][b], "byte %zu of chunk %llu is no value and changed", b, c);
        }
    }
    printf("slices of %llu, %s chunk length: %zu slices, %zu user entries, %zu constants, grids %u / %u\n", slice_max, pow2 ? "power-of-two" : "other",
           slice_off.size(), nuser, nconst, clear_grid, scatter_grid);
}

int main() {
    run(16384, true, 5, 3);  // the product's slice length: 65 536 values are four slices, 16 389 two with a tail of five
    run(16384, false, 2, 2); // a chunk length that is no power of two: the division path
    run(4098, true, 64, 4);  // more workgroups than slices of most records; every full slice ends between two 16-byte pairs of the next
    printf("%d failures %s\n", failures, failures == 0 ? "OK" : "FAIL");
    return failures == 0 ? 0 : 1;
}
