// pg_hip_values_refresh.h -- new matrix values on a fixed pattern, written into the device-resident block records
// (pangulu_platform_0201001_values_refresh): what pangulu_amd_update_values does through the host arena -- zero every owned record's
// value area, scatter the permuted matrix into it -- as two streaming kernels over lists the host builds once per handle.
//   values_clear_kernel     the value areas, cut into slices of bounded length, are zeroed;
//   values_scatter_kernel   user entry p goes to its place, then the few values that are not the user's (unit diagonals of padding
//                           rows, inserted diagonals) to theirs.
// A place is an offset into the arena in values; the arena lives in separately allocated chunks of `vpc` values each (the last one
// may be shorter), so the address of offset o is chunks[o / vpc] + o % vpc.  Both kernels only copy: the records hold the bits the
// host path would have put there.  Plain C++: no LDS, no atomics.  Included inside the anonymous namespace of pg_hip_platform.hip and,
// as plain C++, by tests/values_refresh_kernel_emulation.cpp.
#pragma once

// 16 bytes moved by one instruction: the clear kernel's store, and a double-complex value
struct __attribute__((aligned(16), may_alias)) values_vec16_t
{
    unsigned long long lo, hi;
};
typedef unsigned long long __attribute__((may_alias)) values_word8_t;
typedef unsigned int __attribute__((may_alias)) values_word4_t;

template <size_t BYTES>
struct values_word_of;
template <>
struct values_word_of<4>
{
    typedef values_word4_t type;
};
template <>
struct values_word_of<8>
{
    typedef values_word8_t type;
};
template <>
struct values_word_of<16>
{
    typedef values_vec16_t type;
};
// one value as one machine word: both parts of a complex value travel in one load and one store
typedef values_word_of<sizeof(val_t)>::type values_word_t;

// chunk_shift >= 0: vpc == 1 << chunk_shift (the default chunk size is a power of two: no 64-bit division per entry)
__host__ __device__ inline val_t *values_place(val_t *const *__restrict__ chunks, unsigned long long vpc, int chunk_shift, unsigned long long off)
{
    if (chunk_shift >= 0)
        return chunks[off >> chunk_shift] + (off & (vpc - 1ull));
    return chunks[off / vpc] + off % vpc;
}

// One slice per workgroup pass, the workgroups striding over the list: a record of 64 K values is several slices, a record of 3
// values is one, and the lanes of a wavefront store neighbouring 16 bytes either way.  A slice starts on a 16-byte boundary (value
// areas are 32-byte aligned and the slice length is a multiple of 16 bytes); the values behind its last full 16 bytes are stored one
// by one.
constexpr u32 VALUES_VEC = (u32)(16 / sizeof(val_t));
__global__ __launch_bounds__(256) void values_clear_kernel(const unsigned long long *__restrict__ slice_off, const u32 *__restrict__ slice_count,
                                                           unsigned long long nslice, val_t *const *__restrict__ chunks, unsigned long long vpc,
                                                           int chunk_shift)
{
    const values_vec16_t zero16 = {0ull, 0ull};
    for (unsigned long long s = blockIdx.x; s < nslice; s += gridDim.x)
    {
        val_t *p = values_place(chunks, vpc, chunk_shift, slice_off[s]);
        const u32 count = slice_count[s], nvec = count / VALUES_VEC;
        values_vec16_t *pv = (values_vec16_t *)p;
        for (u32 i = threadIdx.x; i < nvec; i += 256u)
            pv[i] = zero16;
        for (u32 i = nvec * VALUES_VEC + threadIdx.x; i < count; i += 256u)
            p[i] = v_make(0);
    }
}

// One work-item per entry, the grid striding over the user's list and then over the constants: src and the destination lists are
// read as contiguous streams, every entry is one store.
__global__ __launch_bounds__(256) void values_scatter_kernel(const val_t *__restrict__ src, const unsigned long long *__restrict__ user_dst,
                                                             unsigned long long nuser, const val_t *__restrict__ const_value,
                                                             const unsigned long long *__restrict__ const_dst, unsigned long long nconst,
                                                             val_t *const *__restrict__ chunks, unsigned long long vpc, int chunk_shift)
{
    const unsigned long long first = (unsigned long long)blockIdx.x * 256ull + threadIdx.x, stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long k = first; k < nuser; k += stride)
        *(values_word_t *)values_place(chunks, vpc, chunk_shift, user_dst[k]) = ((const values_word_t *)src)[k];
    for (unsigned long long k = first; k < nconst; k += stride)
        *(values_word_t *)values_place(chunks, vpc, chunk_shift, const_dst[k]) = ((const values_word_t *)const_value)[k];
}

// workgroups for `items` work-items of 256-thread workgroups, at most `cap`
inline unsigned values_refresh_grid(unsigned long long items, unsigned per_workgroup, unsigned cap)
{
    const unsigned long long want = (items + per_workgroup - 1ull) / per_workgroup;
    return (unsigned)(want < 1ull ? 1ull : want > cap ? cap : want);
}
