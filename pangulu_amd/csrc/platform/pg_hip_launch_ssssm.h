// pg_hip_launch_ssssm.h -- host side of the update launches, one stage after the other: dense / sparse decision per destination,
// descriptors per update, groups per destination, then the work plan (pg_hip_update_plan.h) and the launches of the MFMA and LDS
// update kernels.  Included inside the anonymous namespace of pg_hip_platform.hip.
#pragma once

// ---- SSSSM -----------------------------------------------------------------------------------------------------
// Tasks arrive grouped by destination.  Per group the destination is either dense-mode (updates accumulate in its
// mirror) or sparse; per task the update runs on the matrix cores when destination and both operands have mirrors,
// on the LDS-accumulator kernel otherwise.
// Tasks per launch (PANGULU_HIP_LAUNCH_CHUNK).  The host builds the descriptors of a launch before it can start: a leaf level
// of the bench matrix has 8000 updates and 4000 solves, and the device sat idle for 260 us per level while their mirror
// jobs and descriptors were written.  Cut into chunks, the first kernels run while the rest is being prepared.
size_t launch_chunk_tasks()
{
    static const size_t chunk = []()
    {
        const char *e = getenv("PANGULU_HIP_LAUNCH_CHUNK");
        long v = e ? atol(e) : 0;
        return v > 0 ? (size_t)v : ~(size_t)0;
    }();
    return chunk;
}

// an update of the current destination that goes to the matrix cores: (operand mirrors, live K-slabs per tile)
struct HeavyUpdate
{
    SsssmTaskD T;
    unsigned short live[4];
    unsigned char full; // bit tl: every 16 x 16 piece of both operands that meets tile tl is live (dense front)
};

// what one launch carries from stage to stage.  One object for all calls: its vectors keep their storage
struct UpdateStaging
{
    // descriptor arrays in the launch's staging segment: where the host writes, where the kernels read
    SsssmTaskD *tasks_s, *d_tasks_s, *tasks_d, *d_tasks_d; // (tasks_d, CR64: four real products per update)
    SsssmGroupD *groups_s, *d_groups_s, *groups_d, *d_groups_d;
    SsssmWorkD *work, *d_work, *work_f, *d_work_f; // every workgroup of the MFMA launch, and of the dense-front launch
    size_t take;                                   // tasks of the call in this launch
    size_t ns, nd, gs, gd, nd_updates;             // nd: real MFMA tasks; nd_updates: the updates they stand for
    double bytes_s, bytes_d;
    unsigned ksplit;
    int tiles_per_dim;
    bool bg_hazard;                     // a mirror job of this launch touches a destination of an earlier launch of the same background call
    std::vector<unsigned short> live_k; // per dense task and tile: K-slabs in which both operands have entries
    std::vector<unsigned char> full_t;  // per dense task: tiles on which the update is a dense-front product
    std::vector<HeavyUpdate> heavy;     // the current destination's
    UpdatePlanScratch plan;
};

// Stage 1: where the updates of destination `dst` (tasks [i, j) of the list) accumulate.  Fills G, the descriptor all groups of the
// destination start from -- its mirror, or the sparse views --, and returns the destination's entry count.
inline u32 update_destination(UpdateStaging &U, int nb, slot_t *dst, task_t **list, size_t i, size_t j, bool dense_ok, bool background,
                              const std::unordered_set<const void *> &bg_earlier, SsssmGroupD &G)
{
    const bool diag = dst->brow_pos == dst->bcol_pos;
    memset(&G, 0, sizeof(G));
    u32 nnz_c;
    slot_t *up = nullptr, *lo = dst;
    if (diag)
    {
        diag_halves(dst, &up, &lo);
        nnz_c = host_nnz(lo, nb) + host_nnz(up, nb);
    }
    else
    {
        nnz_c = host_nnz(dst, nb);
    }
    // The destination works on its dense mirror when the mirror is already ahead of the sparse record, or
    // when at least one update of the group is heavy enough for the matrix cores.
    double *cm = nullptr;
    const size_t jobs_before = MP.to_densify.size() + MP.to_sparsify.size() + MP.early.size();
    if (dense_ok)
    {
        bool want = mirror_is_ahead(dst);
        for (size_t t = i; t < j && !want; t++)
            want = is_heavy_update(host_nnz(list[t]->op1, nb), host_nnz(list[t]->op2, nb), nb);
        if (want)
            cm = current_mirror(dst, nb);
        if (cm)
        {
            block_state(dst, nb).sparse_current = false; // from now on the mirror is ahead of the record
            G.cdense = reinterpret_cast<val_t *>(cm);
        }
    }
    if (!cm)
    {
        require_sparse(dst, nb);
        block_state(dst, nb).written = true; // (the sparse kernel updates the record: its first densify is no longer free to move)
    }
    if (background && !bg_earlier.empty() && MP.to_densify.size() + MP.to_sparsify.size() + MP.early.size() != jobs_before &&
        bg_earlier.count(block_key_any(dst)))
        U.bg_hazard = true;
    if (!G.cdense)
    {
        G.c = BlkView{lo->d_columnpointer, lo->d_rowindex, lo->d_value};
        if (diag)
        {
            const DiagAux &aux = get_diag_aux(up, nb);
            G.ucp = aux.d_cp;
            G.uri = aux.d_ri;
            G.uvi = aux.d_vi;
            G.uval = up->d_value;
        }
    }
    return nnz_c;
}

// Stage 2: the task descriptors of the destination's updates [i, j).  Those for the LDS kernel go straight to tasks_s; those for the
// matrix cores are collected in U.heavy with the tiles of the destination they can reach (tile = tm + tiles * tn), per K-slab.
inline void update_descriptors(UpdateStaging &U, int nb, task_t **list, size_t i, size_t j, size_t n, const SsssmGroupD &G, u32 nnz_c)
{
    const int tiles_per_dim = U.tiles_per_dim;
    SsssmTaskD *const tasks_s = U.tasks_s;
    std::vector<HeavyUpdate> &heavy = U.heavy;
    size_t ns = U.ns; // (the counters of the loop in locals: U is a static object the compiler must assume every store may reach)
    double bytes_s = U.bytes_s, bytes_d = U.bytes_d;
    heavy.clear();
    for (size_t t = i; t < j; t++)
    {
        if (t + PREFETCH_SLOTS_AHEAD < n)
            prefetch_task_slots(list[t + PREFETCH_SLOTS_AHEAD]);
        if (t + PREFETCH_DETAILS_AHEAD < n)
            prefetch_task_details(list[t + PREFETCH_DETAILS_AHEAD], nb);
        slot_t *a = list[t]->op1, *b = list[t]->op2;
        SsssmTaskD T;
        memset(&T, 0, sizeof(T));
        T.a = BlkView{a->d_columnpointer, a->d_rowindex, a->d_value};
        T.b = BlkView{b->d_columnpointer, b->d_rowindex, b->d_value};
        T.sign = 1.0;
        T.count = 1;
        u32 na = host_nnz(a, nb), nbz = host_nnz(b, nb);
        double by = (SV + 2) * ((double)na + nbz) + (2 * SV + 2) * (double)nnz_c + 12.0 * (nb + 1);
        bool on_mfma = false;
        if (G.cdense && is_heavy_update(na, nbz, nb))
        {
            double *am = current_mirror(a, nb);
            double *bm = am ? current_mirror(b, nb) : nullptr;
            if (am && bm)
            {
                T.a.val = reinterpret_cast<val_t *>(am); // the pattern pointers stay: the flop counter reads them
                T.b.val = reinterpret_cast<val_t *>(bm);
                on_mfma = true;
            }
        }
        if (!on_mfma)
        {
            tasks_s[ns++] = T;
            bytes_s += by;
            continue;
        }
        HeavyUpdate H;
        H.T = T;
        const BlockState *sa = MP.blocks.find(block_key(a)), *sb = MP.blocks.find(block_key(b));
        for (int tl = 0; tl < 4; tl++)
            H.live[tl] = tl >= tiles_per_dim * tiles_per_dim ? (unsigned short)0
                         : (sa && sb && sa->occ_valid && sb->occ_valid)
                             ? (unsigned short)(sa->occ_a[tl % tiles_per_dim] & sb->occ_b[tl / tiles_per_dim])
                             : (unsigned short)0xFFFF;
        H.full = 0;
        if (sa && sb && sa->occ_valid && sb->occ_valid)
        {
            H.T.has_map = 1;
            memcpy(H.T.amap, sa->occ_map, sizeof(H.T.amap));
            memcpy(H.T.bmap_t, sb->occ_map_t, sizeof(H.T.bmap_t));
            const int nslab = nb / 16;
            const unsigned pm = nb >= 128 ? 0xFFu : ((1u << nslab) - 1u);
            for (int tl = 0; tl < tiles_per_dim * tiles_per_dim; tl++)
            {
                const int tm = tl % tiles_per_dim, tn = tl / tiles_per_dim;
                bool all = true;
                for (int sl = 0; sl < nslab && all; sl++)
                    all = (((unsigned)H.T.amap[sl] >> (8 * tm)) & pm) == pm && (((unsigned)H.T.bmap_t[sl] >> (8 * tn)) & pm) == pm;
                if (all)
                    H.full |= (unsigned char)(1u << tl);
            }
        }
        heavy.push_back(H);
        bytes_d += by;
    }
    U.ns = ns;
    U.nd_updates += heavy.size();
    U.bytes_s = bytes_s;
    U.bytes_d = bytes_d;
}

// Stage 3: the groups of one destination, from its descriptor G (changed in place), its LDS-kernel tasks [s0, U.ns) and U.heavy.
inline void cut_update_groups(UpdateStaging &U, int nb, SsssmGroupD &G, size_t s0)
{
    // cut long queues into chunks that run concurrently and merge with atomics
    // (a launch with few updates cannot fill the chip with whole queues: one update per workgroup then)
    size_t chunk = (size_t)(B.opt_group_chunk > 0 ? B.opt_group_chunk : 1 << 30);
    if (B.opt_group_chunk > 0 && U.take <= (size_t)B.opt_small_launch_tasks)
        chunk = 1;
    const size_t ns = U.ns, nheavy = U.heavy.size();
    // ... and a destination updated by both kernels at once (they run side by side on two streams) must take
    // atomics from both
    const bool split = (ns - s0) > chunk || nheavy > chunk || ((ns > s0) && nheavy && B.opt_two_streams);
    for (size_t c = s0; c < ns; c += chunk)
    {
        G.task_begin = (u32)c;
        G.task_end = (u32)std::min(ns, c + chunk);
        G.atomic = split ? 1u : 0u;
        U.groups_s[U.gs++] = G;
    }
    if (!nheavy)
        return;
    const unsigned ksplit = U.ksplit;
    const int ntiles = U.tiles_per_dim * U.tiles_per_dim;
    unsigned short *const live_k = U.live_k.data();
    size_t nd = U.nd, gd = U.gd;
    // R64: one task per update.  CR64: per destination plane the two real products of every update, consecutive, so
    // that one accumulator pass serves both (C_re -= A_re B_re - A_im B_im;  C_im -= A_re B_im + A_im B_re)
    for (int plane = 0; plane < PG_PLANES; plane++)
    {
        const size_t d0 = nd;
        for (const HeavyUpdate &H : U.heavy)
            for (int term = 0; term < PG_PLANES; term++)
            {
                SsssmTaskD T = H.T;
#if PG_PLANES > 1
                const size_t ps = mirror_plane_stride(nb);
                double *am = reinterpret_cast<double *>(H.T.a.val), *bm = reinterpret_cast<double *>(H.T.b.val);
                // plane 0 (real):  + A_re B_re  - A_im B_im      plane 1 (imaginary):  + A_re B_im  + A_im B_re
                const int a_im = term, b_im = plane ^ term;
                T.a.val = reinterpret_cast<val_t *>(am + (a_im ? ps : 0));
                T.b.val = reinterpret_cast<val_t *>(bm + (b_im ? ps : 0));
                T.sign = (plane == 0 && term == 1) ? -1.0 : 1.0;
                T.count = (plane == 0 && term == 0) ? 1u : 0u;
#endif
                for (int tl = 0; tl < 4; tl++)
                    live_k[nd * 4 + tl] = H.live[tl];
                U.full_t[nd] = H.full;
                U.tasks_d[nd++] = T;
            }
        SsssmGroupD GP = G;
#if PG_PLANES > 1
        GP.cdense = reinterpret_cast<val_t *>(reinterpret_cast<double *>(G.cdense) + (size_t)plane * mirror_plane_stride(nb));
#endif
        const size_t dchunk = chunk >= ((size_t)1 << 28) ? chunk : chunk * PG_PLANES;
        for (size_t c = d0; c < nd; c += dchunk)
        {
            GP.task_begin = (u32)c;
            GP.task_end = (u32)std::min(nd, c + dchunk);
            GP.atomic = (split || ksplit > 1) ? 1u : 0u;
            const unsigned slabs = (unsigned)nb / 16u, per = slabs / ksplit;
            for (unsigned q = 0; q < ksplit; q++)
            {
                GP.slab_mask = ksplit > 1 ? (((1u << per) - 1u) << (q * per)) : 0u;
                unsigned steps[4];
                update_live_steps(GP, live_k, ntiles, steps);
                GP.live_tiles = (steps[0] ? 1u : 0u) | (steps[1] ? 2u : 0u) | (steps[2] ? 4u : 0u) | (steps[3] ? 8u : 0u);
                U.groups_d[gd++] = GP;
            }
        }
    }
    U.nd = nd;
    U.gd = gd;
}

// Stage 4: mirror jobs, then the launches -- the LDS kernel on `ms`, the MFMA kernels beside it.
inline void issue_update_launch(UpdateStaging &U, Segment &seg, int nb, hipStream_t ms, bool background)
{
    const size_t ns = U.ns, nd = U.nd, gs = U.gs, gd = U.gd;
    if (U.bg_hazard)
    {
        pg_event_record(B.ev_bg_done, ms);
        pg_stream_wait(B.stream, B.ev_bg_done);
    }
    // mirrors that have to be (re)built for this launch, and sparse records that must catch up first
    if (!MP.to_sparsify.empty())
        flush_mirror_jobs(nb, MP.to_sparsify, false);
    flush_early_jobs(nb);
    if (!MP.to_densify.empty())
        flush_mirror_jobs(nb, MP.to_densify, true);
    // longest queues first: workgroups are dispatched in grid order, so the big groups start at once and the small
    // ones fill the tail of the launch
    auto by_size = [](const SsssmGroupD &x, const SsssmGroupD &y)
    { return (x.task_end - x.task_begin) > (y.task_end - y.task_begin); };
    std::stable_sort(U.groups_s, U.groups_s + gs, by_size);
    std::stable_sort(U.groups_d, U.groups_d + gd, by_size);
    commit_segment(seg);
    if (background)
    {
        // mirrors are current and the operands final from here on (main stream); the kernels run on the background stream
        pg_event_record(B.ev_bg_fork, B.stream);
        pg_stream_wait(ms, B.ev_bg_fork);
    }
    if (gs && gd && B.opt_two_streams && !background)
        pg_event_record(B.ev_fork, B.stream); // mirrors are current from here on
    if (gs)
    {
        join_records(ms); // operands and destinations of the LDS kernel are sparse records
        LaunchTimer lt(4, ms);
        // columns per wavefront: 1 unless the grid would exceed 2^20 workgroups (more parallel waves beat fewer launches:
        // measured 176 ms vs 181 ms per factorisation of the bench matrix with an 8k-workgroup target)
        int cpw = 1;
        while (cpw < 64 && gs * (size_t)((nb + SSSSM_WAVES * cpw - 1) / (SSSSM_WAVES * cpw)) > ((size_t)1 << 20))
            cpw *= 2;
        int colblocks = (nb + SSSSM_WAVES * cpw - 1) / (SSSSM_WAVES * cpw);
        size_t lds = sizeof(val_t) * (size_t)nb * SSSSM_WAVES;
        if (B.opt_getrf_strict)
            PG_LAUNCH(ssssm_sparse_kernel<true>, dim3((unsigned)(gs * colblocks)), dim3(SSSSM_WAVES * 64), lds, ms,
                               U.d_groups_s, U.d_tasks_s, nb, cpw, B.d_flops + 4);
        else
            PG_LAUNCH(ssssm_sparse_kernel<false>, dim3((unsigned)(gs * colblocks)), dim3(SSSSM_WAVES * 64), lds, ms,
                               U.d_groups_s, U.d_tasks_s, nb, cpw, B.d_flops + 4);
        B.stats.launches[4]++;
        B.stats.tasks[4] += ns;
        B.stats.alg_bytes[4] += U.bytes_s;
    }
    if (gd)
    {
        hipStream_t ds = ms;
        const bool side = B.opt_two_streams && gs && !background;
        if (side)
        {
            // fork: the MFMA kernel starts as soon as the mirrors are ready and runs beside the LDS kernel (both
            // are bound by memory latency and launch tails, not by a shared resource)
            ds = B.stream2;
            pg_stream_wait(ds, B.ev_fork);
        }
        {
            const int tiles = nb / DG_TILE;
            const UpdatePlanOptions opt{nb, B.opt_front_stages, B.opt_tiles_stages, B.opt_front_min_wgs, (int)B.opt_heavy_first};
            const UpdatePlanCounts plan = plan_update_work(U.groups_d, gd, U.live_k.data(), U.full_t.data(), opt, U.work, U.work_f, U.plan);
            const size_t nw = plan.nw, nf = plan.nf, nfm = plan.nfm;
            LaunchTimer lt(5, ds);
            if (B.opt_profile)
            {
                lt.tag[0] = nw + nf;
                lt.tag[1] = nd;
                lt.tag[2] = update_launch_steps(U.groups_d, gd, U.live_k.data(), nb);
            }
            B.front_workgroups += nf + nfm;
            B.general_workgroups += nw - nfm;
            unsigned long long *pc = B.opt_count_flops ? B.d_flops + 6 : nullptr;
            unsigned long long *pc_front = B.opt_count_flops ? B.d_flops + 7 : nullptr; // (the dense-front kernel's products on their own)
            // PANGULU_HIP_FRONT_FORK (on by default since round 6, see Backend::opt_front_fork): the two launches of a call on two streams, so that workgroups of both are resident at once
            // (one bound by the matrix pipes, the other by its per-step latencies) instead of one launch behind the other's tail.
            const bool fork_front = nf && nw && B.opt_front_fork && !B.opt_profile;
            hipStream_t fs = ds;
            if (fork_front)
            {
                fs = B.stream_front;
                pg_event_record(B.ev_front_fork, ds);
                pg_stream_wait(fs, B.ev_front_fork);
            }
            if (nf)
            {
                // the longest-running workgroups first: the front launch, then the general one fills in behind it
                LaunchTimer lk(100, fs);
                const unsigned unit = (unsigned)(tiles * tiles) * (unsigned)std::max<long long>(1, B.opt_front_unit);
                if (B.opt_front_stages >= 4)
                    PG_LAUNCH((ssssm_front_f64_kernel<4, true>), dim3((unsigned)nf), dim3(FR_THREADS), 0, fs, U.d_tasks_d, nb, U.d_work_f, pc_front, unit);
                else if (B.opt_front_stages == 3)
                    PG_LAUNCH((ssssm_front_f64_kernel<3, true>), dim3((unsigned)nf), dim3(FR_THREADS), 0, fs, U.d_tasks_d, nb, U.d_work_f, pc_front, unit);
                else
                    PG_LAUNCH((ssssm_front_f64_kernel<2, true>), dim3((unsigned)nf), dim3(FR_THREADS), 0, fs, U.d_tasks_d, nb, U.d_work_f, pc_front, unit);
            }
            if (fork_front)
                pg_event_record(B.ev_front_join, fs);
            LaunchTimer lk_general(nw ? 101 : 102, ds); // (102: no general launch in this call -- an empty pair, dropped at harvest)
            if (nw && B.opt_tiles_stages >= 1)
            {
                // the general MFMA update kernel: LDS-DMA pipeline of two stages, strided piece ownership, step records a step ahead,
                // DMA issue behind the first products (pg_hip_front.h).  (Round 3's ssssm_tiles_f64_kernel<STAGES> and round 5's
                // piece-indexed ssssm_tilesp_f64_kernel -- option values 1, 3, 4, 5 -- live in tools/experiments/ since round 6:
                // neither won an in-situ comparison, profiles/r03*, r05[a-h]_pieces_*.)
                const unsigned unit = (unsigned)(tiles * tiles) * (unsigned)std::max<long long>(1, B.opt_tiles_unit);
                PG_LAUNCH(ssssm_tilesv_f64_kernel, dim3((unsigned)nw), dim3(FR_THREADS), 0, ds, U.d_tasks_d, nb, U.d_work, pc, unit);
            }
            else if (nw)
                PG_LAUNCH(ssssm_dense_f64_kernel, dim3((unsigned)nw), dim3(DG_THREADS), 0, ds, U.d_tasks_d, nb, pc,
                                   B.opt_debug_ssssm ? B.d_flops + 8 : nullptr, U.d_work);
            if (fork_front)
                pg_stream_wait(ds, B.ev_front_join);
        }
        if (B.opt_count_flops)
            PG_LAUNCH(ssssm_flop_count_kernel, dim3((unsigned)nd), dim3(256), 0, ds, U.d_tasks_d, nb, B.d_flops + 5);
        if (side)
        {
            pg_event_record(B.ev_join, ds);
            pg_stream_wait(B.stream, B.ev_join); // join before anything later on the main stream
        }
        B.stats.launches[5]++;
        B.stats.tasks[5] += U.nd_updates;
        B.stats.alg_bytes[5] += U.bytes_d;
    }
    HIP_CHECK(hipGetLastError());
    release_pending_segments(ms);
}

// `background`: the update kernels of this call go to the background stream (see Backend::stream_bg); their mirror jobs
// stay on the main stream, in front of the fork
void launch_ssssm(int nb, task_t **list, size_t n, bool background = false)
{
    if (n == 0)
        return;
    HostTimer ht(0);
    hipStream_t const ms = background ? B.stream_bg : B.stream; // where the update kernels of this call run
    const bool dense_ok = dense_mode_available(nb);
    // A call that does not fit one descriptor segment is cut into several launches.  On the background stream the mirror jobs
    // of a later launch -- queued on the MAIN stream -- are not ordered behind the kernels of the earlier ones: a destination
    // whose first updates went to its sparse record there and whose mirror is built here would be read before they have
    // landed (found at the end of round 4: poisson3d(48) with a dense threshold of 100 per mille, factor check 4e-3).  The
    // destinations of the earlier launches of this call are kept, and the main stream waits for them when a job touches one.
    static std::unordered_set<const void *> bg_earlier;
    bg_earlier.clear();
    static UpdateStaging U;
    size_t i = 0;
    while (i < n)
    {
        const size_t chunk_begin = i;
        // worst case per task: one group + one task descriptor in each class; fill until the segment is full
        // (per update: a task descriptor in each class -- PG_PLANES^2 real products on the MFMA side --, a group in each, four
        // work items per MFMA group; the K-split of very small launches multiplies groups and work items of <= 64 tasks by four)
        const size_t per_task = sizeof(SsssmTaskD) * (1 + PG_PLANES * PG_PLANES) + sizeof(SsssmGroupD) * (1 + PG_PLANES) +
                                sizeof(SsssmWorkD) * 8 * PG_PLANES;
        const size_t fixed_part = 64 * 4 * PG_PLANES * (sizeof(SsssmGroupD) + 4 * sizeof(SsssmWorkD)) + 4096;
        Segment seg = acquire_segment(std::min(n - i, launch_chunk_tasks()) * per_task + fixed_part + 65536);
        size_t max_tasks = (seg.cap - fixed_part) / per_task;
        const size_t take = U.take = std::min(n - i, std::min(max_tasks, launch_chunk_tasks()));
        U.tasks_s = seg.alloc<SsssmTaskD>(take, &U.d_tasks_s);
        U.tasks_d = seg.alloc<SsssmTaskD>(take * PG_PLANES * PG_PLANES, &U.d_tasks_d);
        U.tiles_per_dim = nb >= DG_TILE ? nb / DG_TILE : 1;
        U.ksplit = (B.opt_ksplit != 0 && nb <= 256 && nb % 64 == 0 && take * (size_t)(U.tiles_per_dim * U.tiles_per_dim) <= 64) ? 4u : 1u;
        U.groups_s = seg.alloc<SsssmGroupD>(take, &U.d_groups_s);
        U.groups_d = seg.alloc<SsssmGroupD>(take * U.ksplit * PG_PLANES, &U.d_groups_d);
        U.live_k.assign(take * 4 * PG_PLANES * PG_PLANES, 0);
        U.full_t.assign(take * PG_PLANES * PG_PLANES, 0);
        U.work = seg.alloc<SsssmWorkD>(take * U.ksplit * 4 * PG_PLANES, &U.d_work);
        U.work_f = seg.alloc<SsssmWorkD>(take * 4 * PG_PLANES, &U.d_work_f);
        if (!U.tasks_s || !U.tasks_d || !U.groups_s || !U.groups_d || !U.work || !U.work_f)
        {
            fprintf(stderr, "[PanguLU-AMD ERROR] descriptor staging segment too small\n");
            exit(EXIT_FAILURE);
        }
        U.ns = U.nd = U.gs = U.gd = U.nd_updates = 0;
        U.bytes_s = U.bytes_d = 0;
        U.bg_hazard = false;
        const size_t end = i + take;
        while (i < end)
        {
            slot_t *dst = canon_dst(list[i]->opdst);
            size_t j = i;
            while (j < end && canon_dst(list[j]->opdst) == dst)
                j++;
            SsssmGroupD G;
            const u32 nnz_c = update_destination(U, nb, dst, list, i, j, dense_ok, background, bg_earlier, G);
            const size_t s0 = U.ns;
            update_descriptors(U, nb, list, i, j, n, G, nnz_c);
            cut_update_groups(U, nb, G, s0);
            i = j;
        }
        issue_update_launch(U, seg, nb, ms, background);
        if (background && i < n)
            for (size_t t = chunk_begin; t < i; t++)
                bg_earlier.insert(block_key_any(list[t]->opdst));
    }
    if (background)
    {
        pg_event_record(B.ev_bg_done, ms);
        B.bg_active = true;
        for (size_t t = 0; t < n; t++)
            B.bg_tiles.insert(block_key_any(list[t]->opdst));
    }
}
