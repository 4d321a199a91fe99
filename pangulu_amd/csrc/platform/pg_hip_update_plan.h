// pg_hip_update_plan.h -- the work plan of one MFMA update launch: which kernel runs each (group, tile) pair and in which order.
// A pure function of the groups, the per-task tile summaries and five option values: no device, no back-end state
// (tests/update_plan_check.cpp runs it on the CPU).  Needs val_t / u32 / u16 from whoever includes it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "pg_hip_update_desc.h"

struct UpdatePlanOptions
{
    int nb;
    long long front_stages, tiles_stages, front_min_wgs; // Backend::opt_front_stages, opt_tiles_stages, opt_front_min_wgs
    int heavy_mode;                                      // Backend::opt_heavy_first
};

struct UpdatePlanScratch // kept between launches so that no launch allocates
{
    std::vector<unsigned char> full_g, g_class;
    std::vector<u32> g_order;
};

struct UpdatePlanCounts
{
    size_t nw, nf, nfm; // items in `work`, items in `work_f`, dense-front items among those in `work` (pad_ = 1)
};

// live_k[4 * t + tl]: K-slabs (16 wide, bit = slab) in which both operands of dense task t have entries that meet tile tl.
// steps[tl]: the slab steps the kernel takes for group G on tile tl -- live slabs of its tasks under the group's slab mask.
// One pass over the group's tasks; steps of tiles >= ntiles stay 0.
inline void update_live_steps(const SsssmGroupD &G, const unsigned short *live_k, int ntiles, unsigned steps[4])
{
    const unsigned kmask = G.slab_mask ? G.slab_mask : 0xFFFFu;
    steps[0] = steps[1] = steps[2] = steps[3] = 0;
    for (u32 t = G.task_begin; t < G.task_end; t++)
        for (int tl = 0; tl < ntiles; tl++)
            steps[tl] += (unsigned)__builtin_popcount(live_k[(size_t)t * 4 + tl] & kmask);
}

// live 128 x 128 x 16 slab steps of a whole launch (the launch log's third tag; profiling only)
inline unsigned long long update_launch_steps(const SsssmGroupD *groups_d, size_t gd, const unsigned short *live_k, int nb)
{
    const int ntiles = (nb / DG_TILE) * (nb / DG_TILE);
    unsigned long long total = 0;
    unsigned steps[4];
    for (size_t gi = 0; gi < gd; gi++)
    {
        update_live_steps(groups_d[gi], live_k, ntiles, steps);
        total += (unsigned long long)steps[0] + steps[1] + steps[2] + steps[3];
    }
    return total;
}

// One workgroup per (group, tile) some update of the group can reach (SsssmGroupD::live_tiles).  Pairs whose whole queue is
// dense-front products (full_t[t] bit tl: every 16 x 16 piece of both operands of task t that meets tile tl is live; no K-split)
// go to the front kernel's list `work_f`, or stay in `work` marked pad_ = 1 when a launch of their own does not pay.
inline UpdatePlanCounts plan_update_work(const SsssmGroupD *groups_d, size_t gd, const unsigned short *live_k, const unsigned char *full_t,
                                         const UpdatePlanOptions &opt, SsssmWorkD *work, SsssmWorkD *work_f, UpdatePlanScratch &scratch)
{
    const int tiles = opt.nb / DG_TILE, ntiles = tiles * tiles;
    UpdatePlanCounts n{0, 0, 0};
    const bool front_on = opt.front_stages >= 1 && (opt.nb == 128 || opt.nb == 256) && (opt.front_stages >= 2 || opt.tiles_stages >= 1);
    // (first pass: which pairs qualify, and how many -- a front launch of its own pays from a few thousand workgroups
    //  on: fem27(112) 883.8 ms with it against 892.1 with the pairs inside the general launch, shell(398) 39.2 against 38.5)
    std::vector<unsigned char> &full_g = scratch.full_g;
    full_g.assign(gd, 0);
    size_t nfull = 0;
    for (size_t gi = 0; gi < gd && front_on; gi++)
    {
        const SsssmGroupD &Gd = groups_d[gi];
        unsigned all_full = Gd.slab_mask ? 0u : 0xFu;
        for (u32 t = Gd.task_begin; t < Gd.task_end && all_full; t++)
            all_full &= full_t[t];
        all_full &= Gd.live_tiles;
        full_g[gi] = (unsigned char)all_full;
        nfull += (size_t)__builtin_popcount(all_full);
    }
    const bool own_launch = opt.front_stages >= 2 && (opt.tiles_stages < 1 || nfull >= (size_t)opt.front_min_wgs);
    // longest queues first (Backend::opt_heavy_first): classes by the live steps of a group's busiest tile, input order inside a class
    std::vector<u32> &g_order = scratch.g_order;
    g_order.resize(gd);
    if (opt.heavy_mode != 0 && gd > 1)
    {
        std::vector<unsigned char> &g_class = scratch.g_class;
        g_class.resize(gd);
        size_t count[16] = {0};
        for (size_t gi = 0; gi < gd; gi++)
        {
            unsigned steps[4];
            update_live_steps(groups_d[gi], live_k, ntiles, steps);
            const unsigned most = std::max(std::max(steps[0], steps[1]), std::max(steps[2], steps[3]));
            if (opt.heavy_mode == 2)
                g_class[gi] = (unsigned char)(15 - std::min(15u, most / 16u));
            else
                g_class[gi] = most >= 96 ? 0 : most >= 48 ? 1 : most >= 24 ? 2 : 3;
            count[g_class[gi]]++;
        }
        size_t at[16];
        at[0] = 0;
        for (int c = 1; c < 16; c++)
            at[c] = at[c - 1] + count[c - 1];
        for (size_t gi = 0; gi < gd; gi++)
            g_order[at[g_class[gi]]++] = (u32)gi;
    }
    else
        for (size_t gi = 0; gi < gd; gi++)
            g_order[gi] = (u32)gi;
    for (size_t go = 0; go < gd; go++)
    {
        const size_t gi = g_order[go];
        const SsssmGroupD &Gd = groups_d[gi];
        const unsigned all_full = full_g[gi];
        for (int tl = 0; tl < ntiles; tl++)
            if ((Gd.live_tiles >> tl) & 1u)
            {
                SsssmWorkD item{Gd.cdense, Gd.task_begin, Gd.task_end, Gd.atomic, Gd.slab_mask, (u32)tl, 0u};
                if (!((all_full >> tl) & 1u))
                    work[n.nw++] = item;
                else if (own_launch)
                    work_f[n.nf++] = item;
                else
                {
                    // same launch as the partly filled tiles: one launch, one tail; the kernel skips the step list
                    item.pad_ = 1u;
                    work[n.nw++] = item;
                    n.nfm++;
                }
            }
    }
    return n;
}
