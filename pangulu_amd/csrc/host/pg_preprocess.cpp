// pg_preprocess.cpp -- block records, storage, dependency counters, receive bins.
//
// Restates the parts of the reference's set-up whose OUTPUT is an input contract of the hot path:
//   record layout        src/pangulu_communication.c:1290-1322, 1340-1393; device mirror src/pangulu_storage.c:295-357
//   dependency counters  src/pangulu_preprocessing.c:132-207 (owned), 443-556 (remote consumers), 209-315 (receives)
//   receive bins         src/pangulu_preprocessing.c:319-366, src/pangulu_storage.c:171-197
// Unlike the reference (rank 0 builds everything and ships it), every rank derives its own records from the
// replicated symbolic pattern, in parallel, and uploads them with one copy.
#include <algorithm>
#include <cmath>
#include <queue>
#include <string>
#include <omp.h>
#include <sys/mman.h>

#include "pg_host.h"

namespace pg
{

static inline size_t pad8(size_t x) { return (x + 7) & ~(size_t)7; }

size_t record_bytes(u32 nb, u64 nnz, bool lower_offdiag)
{
    size_t sz = 32 + sizeof(val_t) * nnz + sizeof(pangulu_inblock_ptr) * (nb + 1) + sizeof(pangulu_inblock_idx) * nnz;
    sz = pad8(sz);
    if (lower_offdiag)
    {
        sz += sizeof(pangulu_inblock_ptr) * nnz + sizeof(pangulu_inblock_ptr) * (nb + 1) + sizeof(pangulu_inblock_idx) * nnz;
        sz = pad8(sz);
    }
    return sz;
}

void bind_record(slot_t &s, u32 nb, u64 nnz, char *hrec, char *drec, bool lower_offdiag, bool diag_upper)
{
    auto lay = [&](char *rec, bool device)
    {
        char *v = rec + 32;
        char *cp = v + sizeof(val_t) * nnz;
        char *ri = cp + sizeof(pangulu_inblock_ptr) * (nb + 1);
        char *csr = rec + pad8(32 + sizeof(val_t) * nnz + sizeof(pangulu_inblock_ptr) * (nb + 1) + sizeof(pangulu_inblock_idx) * nnz);
        if (!device)
        {
            s.value = (val_t *)v;
            s.columnpointer = (pangulu_inblock_ptr *)cp;
            s.rowindex = (pangulu_inblock_idx *)ri;
            if (lower_offdiag)
            {
                s.idx_of_csc_value_for_csr = (pangulu_inblock_ptr *)csr;
                s.rowpointer = (pangulu_inblock_ptr *)(csr + sizeof(pangulu_inblock_ptr) * nnz);
                s.columnindex = (pangulu_inblock_idx *)(csr + sizeof(pangulu_inblock_ptr) * nnz + sizeof(pangulu_inblock_ptr) * (nb + 1));
            }
        }
        else
        {
            s.d_value = (val_t *)v;
            if (diag_upper)
            {
                // the device mirror names the CSR arrays of an upper diagonal half for what they are
                s.d_rowpointer = (pangulu_inblock_ptr *)cp;
                s.d_columnindex = (pangulu_inblock_idx *)ri;
            }
            else
            {
                s.d_columnpointer = (pangulu_inblock_ptr *)cp;
                s.d_rowindex = (pangulu_inblock_idx *)ri;
            }
            if (lower_offdiag)
            {
                s.d_idx_of_csc_value_for_csr = (pangulu_inblock_ptr *)csr;
                s.d_rowpointer = (pangulu_inblock_ptr *)(csr + sizeof(pangulu_inblock_ptr) * nnz);
                s.d_columnindex = (pangulu_inblock_idx *)(csr + sizeof(pangulu_inblock_ptr) * nnz + sizeof(pangulu_inblock_ptr) * (nb + 1));
            }
        }
    };
    lay(hrec, false);
    lay(drec, true);
    BlockHeader *h = (BlockHeader *)hrec;
    h->nnz = nnz;
    h->brow = s.brow_pos;
    h->bcol = s.bcol_pos;
    h->is_upper = (u32)s.is_upper;
}

slot_t *Storage::allocate(size_t bytes)
{
    std::lock_guard<std::mutex> g(mutex);
    for (size_t b = 1; b < bins.size(); b++)
    {
        RecvBin &bin = bins[b];
        if (bin.slot_capacity >= bytes && !bin.free_list.empty())
        {
            i32 idx = bin.free_list.front();
            bin.free_list.pop_front();
            slot_t *s = &bin.slots[idx];
            s->data_status = PANGULU_DATA_PREPARING;
            s->bin_id = (i32)b;
            s->slot_idx = idx;
            return s;
        }
    }
    return nullptr;
}

void Storage::recycle(slot_t *s)
{
    if (!s || s->bin_id <= 0)
        return;
    std::lock_guard<std::mutex> g(mutex);
    RecvBin &bin = bins[s->bin_id];
    i32 idx = s->slot_idx, bid = s->bin_id;
    val_t *v = s->value, *dv = s->d_value;
    memset((void *)s, 0, sizeof(slot_t));
    s->value = v;
    s->d_value = dv;
    s->bin_id = bid;
    s->slot_idx = idx;
    s->data_status = PANGULU_DATA_INVALID;
    bin.free_list.push_back(idx);
}

namespace
{

// transpose an in-block CSC pattern (colptr over nb columns) into CSR order, recording for every CSR
// position the CSC position it came from
void transpose_inblock(u32 nb, const pangulu_inblock_ptr *cp, const pangulu_inblock_idx *ri,
                       pangulu_inblock_ptr *rp, pangulu_inblock_idx *ci, pangulu_inblock_ptr *from)
{
    u32 nnz = cp[nb];
    for (u32 r = 0; r <= nb; r++)
        rp[r] = 0;
    for (u32 p = 0; p < nnz; p++)
        rp[ri[p] + 1]++;
    for (u32 r = 0; r < nb; r++)
        rp[r + 1] += rp[r];
    std::vector<pangulu_inblock_ptr> cur(rp, rp + nb);
    for (u32 c = 0; c < nb; c++)
        for (u32 p = cp[c]; p < cp[c + 1]; p++)
        {
            u32 o = cur[ri[p]]++;
            ci[o] = (pangulu_inblock_idx)c;
            if (from)
                from[o] = p;
        }
}

} // namespace

// Mapping of the block elimination tree onto the ranks (multi-rank runs).  Deterministic: every rank computes the same map
// from the same block pattern and the same structure model.
//
// Weights: col_time[c] of the structure model (pg_model.cpp) -- the T* seconds (max of algorithmic bytes / HBM rate and
// structural flops / MFMA rate per task) of everything that EXECUTES in block column c when a column's panels live on
// one rank: GETRF(c), the solves of column c and row c, and every update whose destination (i, j) has min(i, j) = c.  (Round
// 2 weighed a column by its task COUNT: a 256 x 256 dense update and a five-entry one counted the same.)
//
// PANGULU_AMD_SEPARATOR_MAP=group (default since round 3): PROPORTIONAL mapping with rank GROUPS that shrink down the
// tree (subtree-to-subcube).  The root's group is all ranks; the children of a node share their parent's group in
// proportion to their subtree weights (recursive bisection of the group, heaviest child first to the lighter half); a
// subtree whose group is one rank lives on that rank whole -- diagonal blocks, L columns, U rows -- and runs without any
// exchange.  A block column whose group has several ranks is a separator.  If its own work is heavy (at least
// PANGULU_AMD_DISTRIBUTE_US microseconds of T*, default 1000, or 5 % of a rank's fair share of the whole factorisation)
// its blocks are distributed 2D BLOCK-CYCLIC over the group's p x q grid -- the reference's rule, owner(i, j) =
// (i mod p) q + (j mod q) (src/pangulu.c:83-90, src/pangulu_common.h:135), applied inside the group: on 3D problems the top
// separators ARE the factorisation and have to be shared.  A light separator goes, with its panels, to the least loaded
// rank of its group: every level of a distributed separator costs dependent hops between ranks, which only pays when
// there is work to share.
// Other values: "path" (round 2's default: a separator follows the rank of its heaviest child), "cyclic" (every
// separator 2D block-cyclic over ALL ranks), "rank0".  PANGULU_AMD_SUBTREE_MAP=0: pure 2D block-cyclic, the reference.
void assign_subtrees(Solver &S)
{
    S.home.clear();
    S.grp.clear();
    const char *env = getenv("PANGULU_AMD_SUBTREE_MAP");
    if (S.nproc <= 1 || (env && atoi(env) == 0))
        return;
    const BlockPattern &P = S.pat;
    const u32 nbk = S.nbk, NONE = 0xFFFFFFFFu;
    const int np = S.nproc;
    std::vector<u32> parent(nbk, NONE);
    std::vector<double> own(nbk, 0.0), sub(nbk, 0.0);
    std::vector<std::vector<u32>> kids(nbk);
    const bool have_model = S.smodel.col_time.size() == nbk;
    double total = 0;
    for (u32 k = 0; k < nbk; k++)
    {
        if (have_model)
            own[k] = S.smodel.col_time[k];
        else
        {
            const double nl = (double)(P.colptr[k + 1] - P.first_after_diag[k]);
            const double nu = (double)(P.rowptr[k + 1] - P.first_after_diag_csr[k]);
            own[k] = 1.0 + nl + nu + nl * nu; // (nb > 65535: no structure model; task counts as in round 2)
        }
        total += own[k];
        sub[k] += own[k];
        if (P.first_after_diag[k] < P.colptr[k + 1])
            parent[k] = P.rowidx[P.first_after_diag[k]];
        if (parent[k] != NONE)
        {
            sub[parent[k]] += sub[k]; // (parent > k: its own term is added when the loop gets there)
            kids[parent[k]].push_back(k);
        }
    }
    const char *sm = getenv("PANGULU_AMD_SEPARATOR_MAP");
    const std::string mode = sm ? sm : "group";
    S.home.assign(nbk, -1);
    std::vector<double> load((size_t)np, 0.0);
    std::vector<u32> stack;
    size_t nsub = 0, ndist = 0;
    auto whole_subtree_to = [&](u32 root, int r)
    {
        load[(size_t)r] += sub[root];
        nsub++;
        stack.assign(1, root);
        while (!stack.empty())
        {
            u32 k = stack.back();
            stack.pop_back();
            S.home[k] = r;
            for (u32 c : kids[k])
                stack.push_back(c);
        }
    };
    if (mode == "group")
    {
        const char *de = getenv("PANGULU_AMD_DISTRIBUTE_US");
        const double heavy_abs = have_model ? 1e-6 * (de ? atof(de) : 1000.0) : 1e300;
        const double heavy_rel = 0.05 * total / np;
        S.grp.assign(nbk, Solver::Group{0, 1, 1});
        struct Work
        {
            std::vector<u32> nodes; // roots of the subtrees that share the group
            int lo, cnt;
        };
        std::vector<Work> todo;
        {
            Work w;
            for (u32 k = 0; k < nbk; k++)
                if (parent[k] == NONE)
                    w.nodes.push_back(k);
            w.lo = 0;
            w.cnt = np;
            todo.push_back(std::move(w));
        }
        while (!todo.empty())
        {
            Work w = std::move(todo.back());
            todo.pop_back();
            if (w.nodes.empty())
                continue;
            if (w.cnt == 1)
            {
                for (u32 k : w.nodes)
                    whole_subtree_to(k, w.lo);
                continue;
            }
            if (w.nodes.size() == 1)
            {
                // a separator (or a chain link of one): place its own column, hand the group on to its children
                const u32 k = w.nodes[0];
                if (own[k] >= heavy_abs || own[k] >= heavy_rel)
                {
                    int p = (int)std::sqrt((double)w.cnt);
                    while (w.cnt % p)
                        p--;
                    S.grp[k] = Solver::Group{(unsigned short)w.lo, (unsigned short)p, (unsigned short)(w.cnt / p)};
                    for (int r = w.lo; r < w.lo + w.cnt; r++)
                        load[(size_t)r] += own[k] / w.cnt;
                    ndist++;
                }
                else
                {
                    int best = w.lo;
                    for (int r = w.lo; r < w.lo + w.cnt; r++)
                        if (load[(size_t)r] < load[(size_t)best])
                            best = r;
                    S.home[k] = best;
                    load[(size_t)best] += own[k];
                }
                Work next;
                next.nodes = kids[k];
                next.lo = w.lo;
                next.cnt = w.cnt;
                todo.push_back(std::move(next));
                continue;
            }
            // several subtrees share the group
            std::sort(w.nodes.begin(), w.nodes.end(), [&](u32 a, u32 b)
                      { return sub[a] > sub[b] || (sub[a] == sub[b] && a < b); });
            double wsum = 0;
            for (u32 k : w.nodes)
                wsum += sub[k];
            const double ideal0 = wsum > 0 ? sub[w.nodes[0]] / wsum * w.cnt : 0.0; // ranks the heaviest subtree deserves
            Work h[2];
            if (ideal0 >= (double)w.cnt - 0.5)
            {
                // the rest deserves less than half a rank: whole subtrees on the least loaded ranks of the group, the heavy
                // one keeps the whole group (many tiny trees beside the main one: padding rows, small components)
                for (size_t t = 1; t < w.nodes.size(); t++)
                {
                    int best = w.lo;
                    for (int r = w.lo; r < w.lo + w.cnt; r++)
                        if (load[(size_t)r] < load[(size_t)best])
                            best = r;
                    whole_subtree_to(w.nodes[t], best);
                }
                h[0].nodes.assign(1, w.nodes[0]);
                h[0].lo = w.lo;
                h[0].cnt = w.cnt;
            }
            else if (ideal0 >= 1.0)
            {
                // proportional: the heaviest subtree gets its share of the ranks (rounded), the others share the rest
                const int c0 = std::max(1, std::min(w.cnt - 1, (int)std::floor(ideal0 + 0.5)));
                h[0].nodes.assign(1, w.nodes[0]);
                h[0].lo = w.lo;
                h[0].cnt = c0;
                h[1].nodes.assign(w.nodes.begin() + 1, w.nodes.end());
                h[1].lo = w.lo + c0;
                h[1].cnt = w.cnt - c0;
            }
            else
            {
                // every subtree is worth less than one rank: bisect the group, heaviest first to the half that is lighter
                // per rank
                h[0].lo = w.lo;
                h[0].cnt = (w.cnt + 1) / 2;
                h[1].lo = w.lo + h[0].cnt;
                h[1].cnt = w.cnt - h[0].cnt;
                double wt[2] = {0, 0};
                for (u32 k : w.nodes)
                {
                    const int side = (wt[0] / h[0].cnt <= wt[1] / h[1].cnt) ? 0 : 1;
                    h[side].nodes.push_back(k);
                    wt[side] += sub[k];
                }
            }
            todo.push_back(std::move(h[1]));
            todo.push_back(std::move(h[0]));
        }
    }
    else
    {
        // legacy maps: split the tree from the top until no remaining subtree carries more than 1/(8 nproc) of the work,
        // give every remaining subtree to the least loaded rank, then place the separators split off on the way
        const char *per_env = getenv("PANGULU_AMD_SUBTREES_PER_RANK");
        const double per_rank = per_env ? atof(per_env) : 8.0;
        const double target = total / (per_rank * (double)np);
        auto cmp = [&](u32 a, u32 b)
        { return sub[a] < sub[b] || (sub[a] == sub[b] && a > b); };
        std::priority_queue<u32, std::vector<u32>, decltype(cmp)> pq(cmp);
        for (u32 k = 0; k < nbk; k++)
            if (parent[k] == NONE)
                pq.push(k);
        while (!pq.empty() && sub[pq.top()] > target)
        {
            u32 k = pq.top();
            pq.pop(); // stays block-cyclic
            for (u32 c : kids[k])
                pq.push(c);
        }
        while (!pq.empty())
        {
            u32 root = pq.top();
            pq.pop();
            whole_subtree_to(root, (int)(std::min_element(load.begin(), load.end()) - load.begin()));
        }
        if (mode == "rank0")
        {
            for (u32 k = 0; k < nbk; k++)
                if (S.home[k] < 0)
                    S.home[k] = 0;
        }
        else if (mode == "path")
        {
            for (u32 k = 0; k < nbk; k++) // (children have smaller indices: they are placed by the time k is)
                if (S.home[k] < 0)
                {
                    int best = -1;
                    double w = -1;
                    for (u32 c : kids[k])
                        if (S.home[c] >= 0 && sub[c] > w)
                        {
                            w = sub[c];
                            best = S.home[c];
                        }
                    S.home[k] = best >= 0 ? best : 0;
                }
        }
        else if (mode != "cyclic")
            fatal("PANGULU_AMD_SEPARATOR_MAP must be group, path, cyclic or rank0");
    }
    if (S.rank == 0 && getenv("PANGULU_AMD_TRACE"))
    {
        size_t top = 0;
        for (int h : S.home)
            top += h < 0;
        fprintf(stderr, "[pangulu_amd trace] mapping '%s': %zu whole subtrees over %d ranks, %zu of %u block columns distributed block-cyclic (%zu over rank groups)\n",
                mode.c_str(), nsub, np, top, nbk, ndist);
    }
}

// scatter the permuted A into the owned patterns (zero elsewhere)
// (the reference's pangulu_convert_block_fill_value_to_struct, src/pangulu_conversion.c:241-350)
void scatter_values(Solver &S, const CscMatrix &A)
{
    const BlockPattern &P = S.pat;
    const u32 nb = S.nb, n = S.n;
    const int me = S.rank;
#pragma omp parallel for schedule(dynamic, 256)
    for (i64 j_ = 0; j_ < (i64)n; j_++)
    {
        u32 j = (u32)j_, bj = j / nb, c = j % nb;
        for (u64 p = A.colptr[j]; p < A.colptr[j + 1]; p++)
        {
            u32 i = A.rowidx[p], bi = i / nb, r = i % nb;
            slot_t *s = nullptr;
            bool csr_row_search = false;
            if (bi == bj)
            {
                if (i > j)
                    s = S.diag_lower[bj];
                else
                {
                    s = S.diag_upper[bj];
                    csr_row_search = true;
                }
            }
            else
            {
                if (S.owner(bi, bj) != me)
                    continue;
                u64 b = P.find(bi, bj);
                if (b == ~0ull)
                    fatal("entry (%u,%u) of A outside the symbolic block pattern", i, j);
                s = S.slot_of[b];
            }
            if (!s)
                continue;
            u32 major = csr_row_search ? r : c, minor = csr_row_search ? c : r;
            const pangulu_inblock_idx *b0 = s->rowindex + s->columnpointer[major];
            const pangulu_inblock_idx *b1 = s->rowindex + s->columnpointer[major + 1];
            const pangulu_inblock_idx *hit = std::lower_bound(b0, b1, (pangulu_inblock_idx)minor);
            if (hit == b1 || *hit != minor)
                fatal("entry (%u,%u) of A outside the symbolic pattern", i, j);
            s->value[hit - s->rowindex] = A.value[p];
        }
    }
}

// New values on the same pattern (pangulu_amd_update_values): the records are zeroed, refilled from the permuted matrix and
// uploaded; counters, slots and the recorded schedule of the handle stay as they are.
void reload_values(Solver &S, const CscMatrix &A)
{
    Platform &plat = active_platform();
    Storage &st = S.storage;
    const u32 nb = S.nb;
    for (auto &s : st.owned)
        if (s.value)
            memset((void *)s.value, 0, sizeof(val_t) * (size_t)s.columnpointer[nb]);
    scatter_values(S, A);
    if (!plat.host_memory)
    {
        plat.synchronize();
        for (size_t c = 0; c < st.dchunks.size(); c++)
            plat.memcpy_(st.dchunks[c], st.harena + c * st.dchunk_bytes, st.chunk_len(c), 0);
        plat.synchronize();
    }
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
    S.host_values_current = true;
}

void preprocess(Solver &S, const CscMatrix &A)
{
    assign_subtrees(S);
    const BlockPattern &P = S.pat;
    const Symbolic &sym = S.sym;
    Platform &plat = active_platform();
    u32 nb = S.nb, nbk = S.nbk, n = S.n;
    int me = S.rank;
    u64 nblk = P.colptr[nbk];

    const bool trace_pre = getenv("PANGULU_AMD_TRACE") != nullptr && S.rank == 0;
    double t_mark = wall_seconds();
    auto lap = [&](const char *what)
    {
        const double now = wall_seconds();
        if (trace_pre)
            fprintf(stderr, "[pangulu_amd trace] preprocess: %s %.2f s\n", what, now - t_mark);
        t_mark = now;
    };
    // ---- owned slots: off-diagonal blocks in block-CSC order, then diagonal halves ---------------------
    Storage &st = S.storage;
    st.nb = nb;
    std::vector<u64> owned_bidx;
    for (u32 bc = 0; bc < nbk; bc++)
        for (u64 b = P.colptr[bc]; b < P.colptr[bc + 1]; b++)
            if (S.owner(P.rowidx[b], bc) == me)
                owned_bidx.push_back(b);
    std::vector<u32> owned_diag;
    for (u32 k = 0; k < nbk; k++)
        if (S.owner(k, k) == me)
            owned_diag.push_back(k);
    st.n_owned_nondiag = owned_bidx.size();
    st.owned.assign(owned_bidx.size() + 2 * owned_diag.size(), slot_t());
    for (auto &s : st.owned)
        memset((void *)&s, 0, sizeof(slot_t));

    // record offsets (64-byte aligned starts so value arrays are 32-byte aligned for vector/MFMA loads)
    std::vector<size_t> off(st.owned.size() + 1, 0);
    auto align64 = [](size_t x)
    { return (x + 63) & ~(size_t)63; };
    size_t cursor = 0;
    const char *chunk_env = getenv("PANGULU_AMD_ARENA_CHUNK_MB");
    const size_t chunk = (size_t)(chunk_env ? atol(chunk_env) : 1024) << 20;
    // place a record of `bytes` at the cursor, or at the start of the next chunk if it would straddle a chunk boundary
    auto place = [&](size_t bytes)
    {
        if (bytes > chunk)
            fatal("a block record of %zu bytes does not fit an arena chunk (PANGULU_AMD_ARENA_CHUNK_MB)", bytes);
        if (cursor / chunk != (cursor + bytes - 1) / chunk)
            cursor = (cursor / chunk + 1) * chunk;
        size_t at = cursor;
        cursor = align64(cursor + bytes);
        return at;
    };
    for (size_t i = 0; i < owned_bidx.size(); i++)
    {
        u64 b = owned_bidx[i];
        u32 br = P.rowidx[b];
        // block column of b: recover by binary search over colptr
        u32 bc = (u32)(std::upper_bound(P.colptr.begin(), P.colptr.end(), b) - P.colptr.begin() - 1);
        off[i] = place(record_bytes(nb, P.nnz[b], br > bc));
    }
    for (size_t d = 0; d < owned_diag.size(); d++)
    {
        u32 k = owned_diag[d];
        size_t i = owned_bidx.size() + 2 * d;
        off[i] = place(record_bytes(nb, P.diag_lower_nnz[k], false));
        off[i + 1] = place(record_bytes(nb, P.diag_upper_nnz[k], false));
    }
    st.arena_bytes = cursor ? cursor : 64;
    S.info.nblocks_owned = st.owned.size();
    S.info.owned_bytes = st.arena_bytes;
    const bool analysis_only = S.analysis_only;
    if (analysis_only)
        st.arena_bytes = 64; // no records: mapping, counters and models only (PANGULU_AMD_ANALYSIS_ONLY)
    // (2 MB alignment + MADV_HUGEPAGE, round 6: the first touch of 87 GB in 4 KB pages -- 21 M page faults -- was most of the 12 s this
    //  step took of a 33 s pangulu_init on the default bench matrix, with all threads zeroing; where transparent huge pages are off
    //  the advice is ignored and nothing changes)
    if (posix_memalign((void **)&st.harena, st.arena_bytes >= ((size_t)2 << 20) ? ((size_t)2 << 20) : 64, st.arena_bytes) != 0)
        fatal("host arena allocation of %zu bytes failed", st.arena_bytes);
#ifdef MADV_HUGEPAGE
    if (st.arena_bytes >= ((size_t)2 << 20) && !getenv("PANGULU_AMD_NO_HUGEPAGES"))
        (void)madvise(st.harena, st.arena_bytes, MADV_HUGEPAGE);
#endif
    lap("mapping + slots");
    {
        // zeroed by all threads (first touch included): one thread took 12 of the 60 s of pangulu_init on the default bench matrix's 87 GB
        const size_t piece = (size_t)64 << 20;
        const i64 npiece = (i64)((st.arena_bytes + piece - 1) / piece);
#pragma omp parallel for schedule(static)
        for (i64 k = 0; k < npiece; k++)
            memset(st.harena + (size_t)k * piece, 0, std::min(piece, st.arena_bytes - (size_t)k * piece));
    }
    lap("host arena zeroed");
    if (plat.host_memory || analysis_only)
    {
        st.darena = st.harena;
    }
    else
    {
        st.dchunk_bytes = chunk;
        size_t nchunks = (st.arena_bytes + chunk - 1) / chunk;
        st.dchunks.assign(nchunks, nullptr);
        for (size_t c = 0; c < nchunks; c++)
            plat.malloc_((void **)&st.dchunks[c], st.chunk_len(c));
    }

    S.slot_of.assign(nblk, nullptr);
    S.diag_lower.assign(nbk, nullptr);
    S.diag_upper.assign(nbk, nullptr);
    for (size_t i = 0; i < owned_bidx.size() && !analysis_only; i++)
    {
        u64 b = owned_bidx[i];
        u32 br = P.rowidx[b];
        u32 bc = (u32)(std::upper_bound(P.colptr.begin(), P.colptr.end(), b) - P.colptr.begin() - 1);
        slot_t &s = st.owned[i];
        s.brow_pos = br;
        s.bcol_pos = bc;
        s.is_upper = 0;
        s.bin_id = 0;
        s.slot_idx = (i32)i;
        s.data_status = PANGULU_DATA_PREPARING;
        bind_record(s, nb, P.nnz[b], st.harena + off[i], st.device_ptr(off[i]), br > bc, false);
        S.slot_of[b] = &s;
    }
    for (size_t d = 0; d < owned_diag.size() && !analysis_only; d++)
    {
        u32 k = owned_diag[d];
        size_t i = owned_bidx.size() + 2 * d;
        slot_t &lo = st.owned[i], &up = st.owned[i + 1];
        lo.brow_pos = lo.bcol_pos = up.brow_pos = up.bcol_pos = k;
        lo.is_upper = 0;
        up.is_upper = 1;
        lo.slot_idx = (i32)i;
        up.slot_idx = (i32)(i + 1);
        lo.related_block = &up;
        up.related_block = &lo;
        lo.data_status = up.data_status = PANGULU_DATA_PREPARING;
        bind_record(lo, nb, P.diag_lower_nnz[k], st.harena + off[i], st.device_ptr(off[i]), false, false);
        bind_record(up, nb, P.diag_upper_nnz[k], st.harena + off[i + 1], st.device_ptr(off[i + 1]), false, true);
        S.diag_lower[k] = &lo;
        S.diag_upper[k] = &up;
    }
    lap("device arena + records bound");
    // ---- patterns: one sweep per block column over the symbolic lower pattern ------------------------
    // lower block (br, bc), br > bc, is needed by its owner (CSC + CSR view) and by the owner of the upper
    // block (bc, br), whose CSC is the transpose.
#pragma omp parallel if (!analysis_only)
    {
        std::vector<i64> local_of(nbk, -1);      // block row -> position in this column's lower block list
        std::vector<std::vector<pangulu_inblock_idx>> tmp_ri;
        std::vector<std::vector<pangulu_inblock_ptr>> tmp_cp;
        std::vector<u32> cursor_nnz;
#pragma omp for schedule(dynamic, 2)
        for (i64 bc_ = 0; bc_ < (analysis_only ? (i64)0 : (i64)nbk); bc_++)
        {
            u32 bc = (u32)bc_;
            u64 l0 = P.lcolptr[bc], l1 = P.lcolptr[bc + 1];
            size_t nl = (size_t)(l1 - l0);
            // which of this column's lower blocks do I need?
            std::vector<char> need(nl, 0);
            bool any = false;
            for (size_t t = 0; t < nl; t++)
            {
                u32 br = P.lrowidx[l0 + t];
                bool mine = (br == bc) ? (S.owner(bc, bc) == me) : (S.owner(br, bc) == me || S.owner(bc, br) == me);
                need[t] = mine;
                any |= mine;
                local_of[br] = (i64)t;
            }
            if (any)
            {
                tmp_ri.assign(nl, {});
                tmp_cp.assign(nl, {});
                for (size_t t = 0; t < nl; t++)
                    if (need[t])
                    {
                        tmp_ri[t].reserve(P.lnnz[l0 + t]);
                        tmp_cp[t].assign(nb + 1, 0);
                    }
                u32 j0 = bc * nb, j1 = std::min(n, j0 + nb);
                for (u32 j = j0; j < j1; j++)
                {
                    u32 c = j - j0;
                    for (u64 p = sym.ptr[j]; p < sym.ptr[j + 1]; p++)
                    {
                        u32 i = sym.idx[p];
                        i64 t = local_of[i / nb];
                        if (t >= 0 && need[(size_t)t])
                        {
                            tmp_ri[(size_t)t].push_back((pangulu_inblock_idx)(i % nb));
                        }
                    }
                    for (size_t t = 0; t < nl; t++)
                        if (need[t])
                            tmp_cp[t][c + 1] = (pangulu_inblock_ptr)tmp_ri[t].size();
                }
                for (u32 c = j1 - j0; c < nb; c++)
                    for (size_t t = 0; t < nl; t++)
                        if (need[t])
                            tmp_cp[t][c + 1] = (pangulu_inblock_ptr)tmp_ri[t].size();

                for (size_t t = 0; t < nl; t++)
                {
                    if (!need[t])
                        continue;
                    u32 br = P.lrowidx[l0 + t];
                    const auto &cp = tmp_cp[t];
                    const auto &ri = tmp_ri[t];
                    if (br == bc)
                    {
                        // diagonal block: strictly-lower CSC half + (diagonal first) CSR upper half whose row r
                        // mirrors lower column r
                        slot_t *lo = S.diag_lower[bc], *up = S.diag_upper[bc];
                        u32 ol = 0, ou = 0;
                        lo->columnpointer[0] = 0;
                        up->columnpointer[0] = 0;
                        for (u32 c = 0; c < nb; c++)
                        {
                            for (u32 p = cp[c]; p < cp[c + 1]; p++)
                            {
                                u32 r = ri[p];
                                up->rowindex[ou++] = (pangulu_inblock_idx)r; // r == c first (diagonal), then r > c
                                if (r != c)
                                    lo->rowindex[ol++] = (pangulu_inblock_idx)r;
                            }
                            lo->columnpointer[c + 1] = ol;
                            up->columnpointer[c + 1] = ou;
                        }
                        continue;
                    }
                    u64 bl = P.find(br, bc); // lower block (br, bc)
                    u64 bu = P.find(bc, br); // its mirror, upper block (bc, br)
                    slot_t *sl = S.slot_of[bl], *su = S.slot_of[bu];
                    if (sl)
                    {
                        std::copy(cp.begin(), cp.end(), sl->columnpointer);
                        std::copy(ri.begin(), ri.end(), sl->rowindex);
                        transpose_inblock(nb, sl->columnpointer, sl->rowindex, sl->rowpointer, sl->columnindex, sl->idx_of_csc_value_for_csr);
                    }
                    if (su)
                    {
                        // CSC of U(bc, br) = CSR of L(br, bc) with the roles of row and column swapped
                        transpose_inblock(nb, cp.data(), ri.data(), su->columnpointer, su->rowindex, nullptr);
                    }
                }
            }
            for (size_t t = 0; t < nl; t++)
                local_of[P.lrowidx[l0 + t]] = -1;
        }
    }

    if (!analysis_only)
        scatter_values(S, A);

    lap("patterns + values into the records");
    // ---- dependency counters (src/pangulu_preprocessing.c:132-207, 443-556) ---------------------------
    S.remain.assign(nblk, 0);
    S.remain_diag.assign(nbk, 0);
    // Forwarding rule.  The reference sends a finished L(br,k) to every rank that owns a block of block row br right of
    // column k, and U(k,bc) down its block column (src/pangulu_numeric.c:452-517,535-600) -- whether or not that rank has an
    // update that uses it.  Under 2D block-cyclic ownership nearly every such rank does; under the subtree mapping most do
    // not (the partner operand lives in a sibling subtree, i.e. is structurally absent): two ranks exchanged gigabytes of
    // blocks nobody read.  Every rank therefore computes, for every block, the set of ranks that really consume it, and both
    // the sender (pg_numeric.cpp send_to_consumers) and the receive count below follow that set.
    // PANGULU_AMD_REFERENCE_FORWARDING=1 (or more than 64 ranks) keeps the reference's rule.
    const bool consumer_rule = S.nproc > 1 && S.nproc <= 64 && !getenv("PANGULU_AMD_REFERENCE_FORWARDING");
    S.consumers.clear();
    if (consumer_rule)
        S.consumers.assign(nblk, 0);
    // every structurally possible update L(a,k) * U(k,b) -> (a,b): a in Lcol(k), b in Lcol(k) (mirror)
    // counted on the destination if I own it, and on each remote operand once per update of mine.
    i64 my_ssssm = 0;
#pragma omp parallel
    {
        std::vector<i64> pos(nbk, -1); // block row -> index (block-CSC) within destination column b
#pragma omp for schedule(dynamic, 2) reduction(+ : my_ssssm)
        for (i64 b_ = 0; b_ < (i64)nbk; b_++)
        {
            u32 b = (u32)b_;
            for (u64 t = P.colptr[b]; t < P.colptr[b + 1]; t++)
                pos[P.rowidx[t]] = (i64)t;
            // k runs over the U blocks of column b: U(k,b), k < b
            for (u64 t = P.colptr[b]; t < P.first_after_diag[b]; t++)
            {
                u32 k = P.rowidx[t];
                u64 ukb = t;
                // a runs over the L blocks of column k: L(a,k), a > k
                for (u64 la = P.first_after_diag[k]; la < P.colptr[k + 1]; la++)
                {
                    u32 a = P.rowidx[la];
                    bool dst_mine;
                    if (consumer_rule && (a == b || pos[a] >= 0))
                    {
                        const int od = a == b ? S.owner(b, b) : S.owner(a, b);
                        if (S.owner(a, k) != od)
                        {
#pragma omp atomic
                            S.consumers[la] |= 1ull << od;
                        }
                        if (S.owner(k, b) != od)
                        {
#pragma omp atomic
                            S.consumers[ukb] |= 1ull << od;
                        }
                    }
                    if (a == b)
                    {
                        dst_mine = S.owner(b, b) == me;
                        if (dst_mine)
                        {
#pragma omp atomic
                            S.remain_diag[b]++;
                        }
                    }
                    else
                    {
                        i64 d = pos[a];
                        if (d < 0)
                            continue; // destination block structurally empty: the product is structurally zero
                        dst_mine = S.owner(a, b) == me;
                        if (dst_mine)
                            S.remain[(size_t)d]++; // column b is handled by this thread only
                    }
                    if (dst_mine)
                    {
                        my_ssssm++;
                        if (S.owner(a, k) != me)
                        {
#pragma omp atomic
                            S.remain[la]++;
                        }
                        if (S.owner(k, b) != me)
                        {
#pragma omp atomic
                            S.remain[ukb]++;
                        }
                    }
                }
            }
            for (u64 t = P.colptr[b]; t < P.colptr[b + 1]; t++)
                pos[P.rowidx[t]] = -1;
        }
    }
    // + 1 for the panel operation of every owned block; remote diagonals count my TSTRF/GESSM consumers
    i64 my_tasks = 0, my_getrf = 0, my_tstrf = 0, my_gessm = 0, my_recv = 0;
    // What will be SENT to me follows the owners' forwarding rule (pg_numeric.cpp release_after_L/U, reference
    // src/pangulu_numeric.c:452-517,535-600): a finished L(br,k) goes to every rank owning a block of block row
    // br right of column k (or diagonal (br,br)); a finished U(k,bc) to every rank owning a block of block
    // column bc below row k (or diagonal (bc,bc)) -- whether or not that rank ends up with an update that uses
    // it (the partner operand may be structurally absent).  The receive count must follow the same rule.
    std::vector<i64> last_owned_col(nbk, -1), last_owned_row(nbk, -1);
    for (u32 bc = 0; bc < nbk; bc++)
        for (u64 t = P.colptr[bc]; t < P.colptr[bc + 1]; t++)
            if (S.owner(P.rowidx[t], bc) == me)
            {
                u32 br = P.rowidx[t];
                last_owned_col[br] = std::max<i64>(last_owned_col[br], bc);
                last_owned_row[bc] = std::max<i64>(last_owned_row[bc], br);
            }
    for (u32 k = 0; k < nbk; k++)
        if (S.owner(k, k) == me)
        {
            last_owned_col[k] = std::max<i64>(last_owned_col[k], k);
            last_owned_row[k] = std::max<i64>(last_owned_row[k], k);
        }
    for (u32 bc = 0; bc < nbk; bc++)
    {
        for (u64 t = P.colptr[bc]; t < P.colptr[bc + 1]; t++)
        {
            u32 br = P.rowidx[t];
            if (S.owner(br, bc) == me)
            {
                S.remain[t] += 1;
                my_tasks++;
                u32 level = std::min(br, bc);
                if (br > bc)
                    my_tstrf++;
                else
                    my_gessm++;
                if (S.owner(level, level) != me)
                    S.remain_diag[level]++;
            }
            else
            {
                bool sent_to_me = consumer_rule ? ((S.consumers[t] >> me) & 1ull) != 0
                                                : ((br > bc) ? (last_owned_col[br] > (i64)bc) : (last_owned_row[bc] > (i64)br));
                if (sent_to_me)
                    my_recv++;
            }
        }
    }
    for (u32 k = 0; k < nbk; k++)
    {
        if (S.owner(k, k) == me)
        {
            S.remain_diag[k] += 1;
            my_tasks++;
            my_getrf++;
        }
        else if (S.remain_diag[k] > 0)
        {
            // a remote diagonal arrives as up to two records: the U half if I run TSTRFs below it, the L half
            // if I run GESSMs right of it
            bool need_u = false, need_l = false;
            for (u64 t = P.first_after_diag[k]; t < P.colptr[k + 1] && !need_u; t++)
                need_u = S.owner(P.rowidx[t], k) == me;
            for (u64 t = P.first_after_diag_csr[k]; t < P.rowptr[k + 1] && !need_l; t++)
                need_l = S.owner(k, P.colidx[t]) == me;
            my_recv += (need_u ? 1 : 0) + (need_l ? 1 : 0);
        }
    }
    S.rank_remain_task = my_tasks; // SSSSM updates bypass the heap in this build (see pg_numeric.cpp)
    S.rank_remain_recv = my_recv;
    S.remain0 = S.remain;
    S.remain_diag0 = S.remain_diag;
    S.rank_remain_task0 = S.rank_remain_task;
    S.rank_remain_recv0 = S.rank_remain_recv;
    S.info.ntask_getrf = (u64)my_getrf;
    S.info.ntask_tstrf = (u64)my_tstrf;
    S.info.ntask_gessm = (u64)my_gessm;
    S.info.ntask_ssssm = (u64)my_ssssm;
    S.info.recv_blocks = (u64)my_recv;
    S.heap.reserve((size_t)my_tasks + 1);
    S.pending.assign(st.owned.size(), {});

    lap("dependency counters");
    // ---- receive bins (src/pangulu_preprocessing.c:319-366) -------------------------------------------
    st.bins.clear();
    st.bins.resize(7);
    if (S.nproc > 1 && !analysis_only)
    {
        // six size classes by nnz, as the reference: tiny, one entry per row/col x4, ~1% .. full
        u64 full = (u64)nb * nb;
        u64 cls_nnz[7] = {0,
                          std::max<u64>(5, full / 1024),
                          std::max<u64>(4ull * nb, full / 256),
                          std::max<u64>((u64)nb * std::max<u32>(nb / 100, 8), full / 64),
                          full / 16,
                          full / 4,
                          full};
        for (int b = 1; b <= 6; b++)
            cls_nnz[b] = std::min(cls_nnz[b], full);
        // how many remote blocks of each class will I receive in total?  slots = level * that, floored.  A block is counted in the
        // class Storage::allocate will take its slot from -- the first one whose slot holds the RECORD (an upper block or a
        // diagonal half has no CSR part and may fit a class below the one its entry count suggests) --: with FIFO free lists a
        // bin that is provisioned for its blocks then hands out every slot once per factorisation (multi-rank replay needs that).
        u64 need_cnt[7] = {0, 0, 0, 0, 0, 0, 0};
        size_t cls_cap[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int b = 1; b <= 6; b++)
            cls_cap[b] = (record_bytes(nb, cls_nnz[b], true) + 63) & ~(size_t)63;
        auto classify = [&](u64 nnz, bool lower_offdiag)
        {
            const size_t bytes = record_bytes(nb, nnz, lower_offdiag);
            for (int b = 1; b <= 6; b++)
                if (bytes <= cls_cap[b])
                    return b;
            return 6;
        };
        for (u32 bc = 0; bc < nbk; bc++)
            for (u64 t = P.colptr[bc]; t < P.colptr[bc + 1]; t++)
            {
                u32 br = P.rowidx[t];
                if (S.owner(br, bc) == me)
                    continue;
                bool sent_to_me = consumer_rule ? ((S.consumers[t] >> me) & 1ull) != 0
                                                : ((br > bc) ? (last_owned_col[br] > (i64)bc) : (last_owned_row[bc] > (i64)br));
                if (sent_to_me)
                    need_cnt[classify(P.nnz[t], br > bc)]++;
            }
        for (u32 k = 0; k < nbk; k++)
            if (S.owner(k, k) != me && S.remain_diag[k] > 0)
            {
                need_cnt[classify(P.diag_lower_nnz[k], false)]++;
                need_cnt[classify(P.diag_upper_nnz[k], false)]++;
            }
        // The reference sizes bins as a fraction of block_length (init_options.mpi_recv_buffer_level) and aborts
        // when they run dry (src/pangulu_storage.c:109-132).  With 288 GB of HBM per GPU the safe choice is
        // affordable: provision one slot per block this rank will ever receive as long as that stays within
        // the budget (PANGULU_AMD_RECV_BUDGET_GB, default 48); beyond it fall back to the level-scaled share
        // and let the receiver stop draining its peers while a class is exhausted.
        float level = S.recv_buffer_level > 0 ? S.recv_buffer_level : 0.5f;
        const char *budget_env = getenv("PANGULU_AMD_RECV_BUDGET_GB");
        double budget = (budget_env ? atof(budget_env) : 48.0) * 1e9;
        double full_bytes = 0;
        for (int b = 1; b <= 6; b++)
            full_bytes += (double)((record_bytes(nb, cls_nnz[b], true) + 63) & ~(size_t)63) * (double)(need_cnt[b] + 2);
        bool provision_all = full_bytes <= budget;
        for (int b = 1; b <= 6; b++)
        {
            RecvBin &bin = st.bins[b];
            bin.slot_capacity = (record_bytes(nb, cls_nnz[b], true) + 63) & ~(size_t)63;
            u64 want = (u64)(level * (float)need_cnt[b]) + 64;
            u64 cnt = provision_all ? need_cnt[b] + 2 : std::min<u64>(need_cnt[b] + 2, want);
            if (need_cnt[b] == 0)
                cnt = 0;
            size_t bytes = bin.slot_capacity * cnt;
            bin.slots.assign(cnt, slot_t());
            bin.free_list.clear();
            if (cnt == 0)
                continue;
            if (posix_memalign((void **)&bin.hbuf, 64, bytes) != 0)
                fatal("receive bin allocation failed");
            if (plat.host_memory)
                bin.dbuf = bin.hbuf;
            else
                plat.malloc_((void **)&bin.dbuf, bytes);
            for (u64 i = 0; i < cnt; i++)
            {
                slot_t &s = bin.slots[i];
                memset((void *)&s, 0, sizeof(slot_t));
                s.value = (val_t *)(bin.hbuf + i * bin.slot_capacity + 32);
                s.d_value = (val_t *)(bin.dbuf + i * bin.slot_capacity + 32);
                s.bin_id = b;
                s.slot_idx = (i32)i;
                bin.free_list.push_back((i32)i);
            }
        }
    }

    lap("receive bins");
    // ---- upload -------------------------------------------------------------------------------------------
    if (!plat.host_memory && !analysis_only)
    {
        for (size_t c = 0; c < st.dchunks.size(); c++)
            plat.memcpy_(st.dchunks[c], st.harena + c * st.dchunk_bytes, st.chunk_len(c), 0);
        plat.synchronize();
        lap("upload of the records");
        if (plat.prepare_diag)
            for (u32 k : owned_diag)
                plat.prepare_diag((pangulu_inblock_idx)nb, S.diag_lower[k]);
        if (plat.prepare_blocks && st.n_owned_nondiag)
        {
            std::vector<slot_t *> offdiag(st.n_owned_nondiag);
            for (size_t i = 0; i < st.n_owned_nondiag; i++)
                offdiag[i] = &st.owned[i];
            plat.prepare_blocks((pangulu_inblock_idx)nb, offdiag.size(), offdiag.data());
        }
        lap("back-end preparation (diagonal column views, pattern summaries)");
    }
    if (world()->size > 1 && !analysis_only)
        world()->register_arena(st.dchunks.data(), plat.host_memory ? 0 : st.dchunks.size(), st.dchunk_bytes, st.arena_bytes); // (collective)
    S.host_values_current = true;
}

void download_factors(Solver &S)
{
    if (S.host_values_current)
        return;
    Platform &plat = active_platform();
    if (!plat.host_memory)
    {
        plat.synchronize();
        // values are the only part of a record the numeric phase changes; one pass over the arena is simpler
        // and, with records being value-dominated, barely more traffic than per-block copies
        for (size_t c = 0; c < S.storage.dchunks.size(); c++)
            plat.memcpy_(S.storage.harena + c * S.storage.dchunk_bytes, S.storage.dchunks[c], S.storage.chunk_len(c), 1);
    }
    S.host_values_current = true;
}

Solver::~Solver()
{
    Platform &plat = active_platform();
    drop_solve_workspace(*this);
    drop_values_refresh(*this);
    if (schedule_recorded && plat.schedule)
        plat.schedule(0, this); // the recorded launches point into this handle's arena and mirrors
    for (char *c : snapshot_dchunks)
        if (c)
            plat.free_(c);
    if (arena_snapshot)
    {
        if (plat.host_memory || snapshot_on_host)
            free(arena_snapshot);
        else
            plat.free_(arena_snapshot);
    }
    if (storage.harena)
    {
        for (char *c : storage.dchunks)
            if (c)
                plat.free_(c);
        free(storage.harena);
    }
    for (auto &bin : storage.bins)
    {
        if (bin.hbuf)
        {
            if (!plat.host_memory && bin.dbuf)
                plat.free_(bin.dbuf);
            free(bin.hbuf);
        }
    }
}

} // namespace pg
