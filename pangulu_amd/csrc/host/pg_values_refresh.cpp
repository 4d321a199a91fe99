// pg_values_refresh.cpp -- new values on the handle's pattern, taken from where they are (pangulu_amd_update_values_device).
//
// pangulu_amd_update_values refills the host copy of every record and uploads the whole arena, patterns and index arrays included.
// The device needs zeros in the value areas, the nnz(A) new values at places that depend on the pattern only, and the few values that
// are not the user's.  Those places are a ValuesRefreshMap (pg_host.h), built here once per handle with the lookups of scatter_values
// and of pangulu_amd_update_values; Platform::values_refresh applies it with two kernels (pg_hip_values_refresh.h), the loop below
// applies it on a platform whose memory is host memory.  The host arena is not written.
#include <algorithm>
#include <cstring>

#include "pg_host.h"

namespace pg
{

namespace
{

// records of 64 K values and records of 3 must not share a launch geometry: value areas go to the back-end in slices of at most this
// many values (a multiple of 16 bytes for every value type, so that every slice starts as aligned as its record's value area)
constexpr u64 VALUES_SLICE_MAX = 16384;

// where entry (i, j) of the permuted matrix lives, as an offset into the arena counted in values: the lookups of scatter_values
u64 arena_offset_of_entry(const Solver &S, u32 i, u32 j)
{
    const u32 nb = S.nb, bi = i / nb, bj = j / nb, r = i % nb, c = j % nb;
    const slot_t *s = nullptr;
    bool csr_row_search = false;
    if (bi == bj)
    {
        s = i > j ? S.diag_lower[bj] : S.diag_upper[bj];
        csr_row_search = i <= j;
    }
    else
    {
        const u64 b = S.pat.find(bi, bj);
        if (b == ~0ull)
            fatal("entry (%u,%u) of A outside the symbolic block pattern", i, j);
        s = S.slot_of[b];
    }
    if (!s || !s->value)
        fatal("entry (%u,%u) of A has no record on this rank", i, j);
    const u32 major = csr_row_search ? r : c, minor = csr_row_search ? c : r;
    const pangulu_inblock_idx *b0 = s->rowindex + s->columnpointer[major];
    const pangulu_inblock_idx *b1 = s->rowindex + s->columnpointer[major + 1];
    const pangulu_inblock_idx *hit = std::lower_bound(b0, b1, (pangulu_inblock_idx)minor);
    if (hit == b1 || *hit != minor)
        fatal("entry (%u,%u) of A outside the symbolic pattern", i, j);
    return (u64)((const char *)(s->value + (hit - s->rowindex)) - S.storage.harena) / sizeof(val_t);
}

const ValuesRefreshMap &values_refresh_map(Solver &S)
{
    ValuesRefreshMap &M = S.values_map;
    if (M.ready)
        return M;
    const CscMatrix &B = S.Aperm;
    const u64 nnz = S.info.nnz;
    M.user_dst.assign(nnz, 0);
    std::vector<char> from_user(B.nnz(), 0);
    // the user's entry p of column j sits at (iperm[i], iperm[j]) of the permuted matrix (the loop of pangulu_amd_update_values)
#pragma omp parallel for schedule(dynamic, 512)
    for (i64 j_ = 0; j_ < (i64)S.n_user; j_++)
    {
        const u32 j = (u32)j_, pj = S.iperm[j];
        for (u64 p = S.user_colptr[j]; p < S.user_colptr[j + 1]; p++)
        {
            const u32 pi = S.iperm[S.user_rowidx[p]];
            const u32 *b0 = B.rowidx.data() + B.colptr[pj], *b1 = B.rowidx.data() + B.colptr[pj + 1];
            const u32 *hit = std::lower_bound(b0, b1, pi);
            if (hit == b1 || *hit != pi)
                fatal("pangulu_amd_update_values_device: entry (%u,%u) is not in the pattern the handle was initialised with", S.user_rowidx[p], j);
            from_user[hit - B.rowidx.data()] = 1;
            M.user_dst[p] = arena_offset_of_entry(S, pi, pj);
        }
    }
    // what no user entry maps to keeps the value it has: unit diagonals of padding rows, the diagonals of the zero-diagonal rule
    for (u32 j = 0; j < B.n; j++)
        for (u64 q = B.colptr[j]; q < B.colptr[j + 1]; q++)
            if (!from_user[q])
            {
                M.const_dst.push_back(arena_offset_of_entry(S, B.rowidx[q], j));
                M.const_value.push_back(B.value[q]);
            }
    for (const slot_t &s : S.storage.owned)
    {
        if (!s.value)
            continue;
        const u64 first = (u64)((const char *)s.value - S.storage.harena) / sizeof(val_t), count = s.columnpointer[S.nb];
        for (u64 k = 0; k < count; k += VALUES_SLICE_MAX)
        {
            M.slice_off.push_back(first + k);
            M.slice_count.push_back((u32)std::min(VALUES_SLICE_MAX, count - k));
        }
    }
    M.ready = true;
    return M;
}

} // namespace

int refresh_values_from(Solver &S, const val_t *values, val_t *host_copy, void *stream)
{
    Platform &plat = active_platform();
    Storage &st = S.storage;
    const ValuesRefreshMap &M = values_refresh_map(S);
    if (plat.host_memory)
    {
        val_t *arena = (val_t *)st.darena;
        for (size_t s = 0; s < M.slice_off.size(); s++)
            memset((void *)(arena + M.slice_off[s]), 0, sizeof(val_t) * (size_t)M.slice_count[s]);
        for (size_t p = 0; p < M.user_dst.size(); p++)
            arena[M.user_dst[p]] = values[p];
        for (size_t c = 0; c < M.const_dst.size(); c++)
            arena[M.const_dst[c]] = M.const_value[c];
        std::copy(values, values + M.user_dst.size(), host_copy);
    }
    else
    {
        pangulu_hip_values_map_t m;
        m.nuser = M.user_dst.size();
        m.nconst = M.const_dst.size();
        m.nslice = M.slice_off.size();
        m.user_dst = (const pangulu_uint64_t *)M.user_dst.data();
        m.const_dst = (const pangulu_uint64_t *)M.const_dst.data();
        m.const_value = M.const_value.data();
        m.slice_off = (const pangulu_uint64_t *)M.slice_off.data();
        m.slice_count = M.slice_count.data();
        m.nchunk = st.dchunks.size();
        m.values_per_chunk = st.dchunk_bytes / sizeof(val_t);
        m.arena_values = st.arena_bytes / sizeof(val_t);
        m.chunks = st.dchunks.data();
        if (plat.values_refresh(&m, values, host_copy, &S.values_map_device, stream) < 0)
            return 2;
    }
    // the handle as reload_values leaves it, except that the host copy of the records has not been written
    S.remain = S.remain0;
    S.remain_diag = S.remain_diag0;
    S.rank_remain_task = S.rank_remain_task0;
    S.rank_remain_recv = S.rank_remain_recv0;
    for (auto &s : st.owned)
        s.data_status = PANGULU_DATA_PREPARING;
    for (auto &q : S.pending)
        q.clear();
    S.pending_dirty.clear();
    S.pending_total = 0;
    S.factored = false;
    S.host_values_current = plat.host_memory;
    return 0;
}

void drop_values_refresh(Solver &S)
{
    if (!S.values_map_device)
        return;
    active_platform().values_refresh_free(&S.values_map_device);
    S.values_map_device = nullptr;
}

} // namespace pg
