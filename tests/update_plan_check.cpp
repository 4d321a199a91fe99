// Device-free check of plan_update_work (pangulu_amd/csrc/platform/pg_hip_update_plan.h): which kernel runs each (group, tile) pair
// of an MFMA update launch, and in which order.  Driven by tests/test_update_plan_cpu.py:
//   update_plan_check        properties of the plan over seeded random and hand-made inputs; prints OK
//   update_plan_check plans  the plans of the recorded cases (tests/golden/update_plan_expected.json), whitespace-separated integers:
//                            per case nw nf nfm, then per item of work and of work_f: cdense task_begin task_end atomic slab_mask tile pad_
// (cdense is never dereferenced: a mirror is named by a small number, carried as the pointer value / 8.)
#include "hip_emulation_shims.h"
#include "pg_hip_update_plan.h"

#include <cstdint>
#include <map>
#include <tuple>

struct Case
{
    UpdatePlanOptions opt;
    std::vector<SsssmGroupD> groups;
    std::vector<unsigned short> live_k;
    std::vector<unsigned char> full_t;
};
struct Plan
{
    UpdatePlanCounts n;
    std::vector<SsssmWorkD> work, work_f;
};

static val_t *mirror(unsigned long id) { return reinterpret_cast<val_t *>((uintptr_t)id * 8); }
static unsigned long mirror_id(const val_t *p) { return (unsigned long)(reinterpret_cast<uintptr_t>(p) / 8); }

static Plan run(const Case &c)
{
    Plan p;
    // (the launch code's bound: four work items per group)
    p.work.resize(c.groups.size() * 4 + 1);
    p.work_f.resize(c.groups.size() * 4 + 1);
    UpdatePlanScratch scratch;
    p.n = plan_update_work(c.groups.data(), c.groups.size(), c.live_k.data(), c.full_t.data(), c.opt, p.work.data(), p.work_f.data(), scratch);
    return p;
}

static unsigned kmask_of(const SsssmGroupD &g) { return g.slab_mask ? g.slab_mask : 0xFFFFu; }

// live_tiles as the launch code derives it: tiles on which some task of the group has a live K-slab under the group's mask
static void derive_live_tiles(Case &c)
{
    const int tiles = c.opt.nb / 128;
    for (SsssmGroupD &g : c.groups)
    {
        g.live_tiles = 0;
        for (u32 t = g.task_begin; t < g.task_end; t++)
            for (int tl = 0; tl < tiles * tiles; tl++)
                if (c.live_k[(size_t)t * 4 + tl] & kmask_of(g))
                    g.live_tiles |= 1u << tl;
    }
}

// full_mode: 0 = no task full on any tile, 1 = every task on every tile, 2 = mixed;  mask_mode: 0 = no K-split, 1 = every group one
// of four slab quarters, 2 = mixed
static Case random_case(unsigned seed, int nb, size_t gd, int full_mode, int mask_mode, UpdatePlanOptions opt)
{
    std::mt19937 rng(seed);
    Case c;
    opt.nb = nb;
    c.opt = opt;
    const int tiles = nb / 128, ntiles = tiles * tiles;
    const unsigned slabs = (unsigned)nb / 16u;
    u32 t0 = 0;
    for (size_t gi = 0; gi < gd; gi++)
    {
        SsssmGroupD g;
        memset(&g, 0, sizeof(g));
        const u32 ntask = 1 + rng() % 8;
        g.cdense = mirror(1000 + gi);
        g.task_begin = t0;
        g.task_end = t0 + ntask;
        g.atomic = rng() % 2;
        const bool masked = mask_mode == 1 || (mask_mode == 2 && rng() % 3 == 0);
        const unsigned per = slabs / 4;
        g.slab_mask = masked ? (((1u << per) - 1u) << ((rng() % 4) * per)) : 0u;
        const unsigned density = rng() % 4; // groups of few and of many live slabs: every class of the heavy-first order
        for (u32 t = 0; t < ntask; t++)
        {
            unsigned char full = 0;
            for (int tl = 0; tl < 4; tl++)
            {
                unsigned short live = 0;
                if (tl < ntiles)
                    for (unsigned s = 0; s < slabs; s++)
                        if (rng() % 4 <= density)
                            live |= (unsigned short)(1u << s);
                const bool is_full = tl < ntiles && (full_mode == 1 || (full_mode == 2 && rng() % 4 != 0));
                if (is_full)
                {
                    live = (unsigned short)((1u << slabs) - 1u); // (a dense-front product has every slab live)
                    full |= (unsigned char)(1u << tl);
                }
                c.live_k.push_back(live);
            }
            c.full_t.push_back(full);
        }
        t0 += ntask;
        c.groups.push_back(g);
    }
    derive_live_tiles(c);
    return c;
}

static int g_failures = 0;
#define EXPECT(cond_, ...)                              \
    do                                                  \
    {                                                   \
        if (!(cond_))                                   \
        {                                               \
            if (g_failures++ < 20)                      \
            {                                           \
                printf("FAILED %s: %s -- ", name, #cond_); \
                printf(__VA_ARGS__);                    \
                printf("\n");                           \
            }                                           \
        }                                               \
    } while (0)

// the properties, from the inputs alone
static void check(const char *name, const Case &c)
{
    const Plan p = run(c);
    const UpdatePlanOptions &o = c.opt;
    const size_t gd = c.groups.size();
    const int tiles = o.nb / 128, ntiles = tiles * tiles;
    const bool front_on = o.front_stages >= 1 && (o.nb == 128 || o.nb == 256) && (o.front_stages >= 2 || o.tiles_stages >= 1);
    // which pairs are dense-front pairs, how many there are, and the class of every group
    std::vector<unsigned> front(gd, 0), cls(gd, 0);
    size_t nfull = 0, nlive = 0;
    for (size_t gi = 0; gi < gd; gi++)
    {
        const SsssmGroupD &g = c.groups[gi];
        unsigned most = 0;
        for (int tl = 0; tl < ntiles; tl++)
        {
            bool all = front_on && g.slab_mask == 0;
            unsigned steps = 0;
            for (u32 t = g.task_begin; t < g.task_end; t++)
            {
                all = all && ((c.full_t[t] >> tl) & 1u);
                steps += (unsigned)__builtin_popcount(c.live_k[(size_t)t * 4 + tl] & kmask_of(g));
            }
            most = std::max(most, steps);
            if ((g.live_tiles >> tl) & 1u)
            {
                nlive++;
                if (all)
                {
                    front[gi] |= 1u << tl;
                    nfull++;
                }
            }
        }
        if (o.heavy_mode == 2 && gd > 1)
            cls[gi] = 15 - std::min(15u, most / 16u);
        else if (o.heavy_mode != 0 && gd > 1)
            cls[gi] = most >= 96 ? 0 : most >= 48 ? 1 : most >= 24 ? 2 : 3;
    }
    const bool own_launch = o.front_stages >= 2 && (o.tiles_stages < 1 || nfull >= (size_t)o.front_min_wgs);
    EXPECT(p.n.nw + p.n.nf == nlive, "%zu + %zu items for %zu live pairs", p.n.nw, p.n.nf, nlive);
    EXPECT(p.n.nw <= gd * 4 && p.n.nf <= gd * 4, "more items than pairs");
    EXPECT(p.n.nf == (own_launch ? nfull : 0), "nf %zu, nfull %zu, own_launch %d", p.n.nf, nfull, (int)own_launch);
    EXPECT(p.n.nfm == (own_launch ? 0 : nfull), "nfm %zu, nfull %zu, own_launch %d", p.n.nfm, nfull, (int)own_launch);
    std::map<std::tuple<unsigned long, u32, u32, u32>, size_t> by_key;
    for (size_t gi = 0; gi < gd; gi++)
    {
        const SsssmGroupD &g = c.groups[gi];
        const bool fresh = by_key.emplace(std::make_tuple(mirror_id(g.cdense), g.task_begin, g.task_end, g.slab_mask), gi).second;
        EXPECT(fresh, "test input: groups %zu is a copy of an earlier one", gi);
    }
    std::vector<unsigned> seen(gd, 0);
    size_t padded = 0;
    for (int list = 0; list < 2; list++)
    {
        const std::vector<SsssmWorkD> &w = list ? p.work_f : p.work;
        const size_t nitem = list ? p.n.nf : p.n.nw;
        long prev_cls = -1, prev_g = -1, prev_tile = -1;
        for (size_t k = 0; k < nitem && k < w.size(); k++)
        {
            const SsssmWorkD &it = w[k];
            auto found = by_key.find(std::make_tuple(mirror_id(it.cdense), it.task_begin, it.task_end, it.slab_mask));
            EXPECT(found != by_key.end(), "list %d item %zu belongs to no group", list, k);
            if (found == by_key.end())
                continue;
            const size_t gi = found->second;
            const SsssmGroupD &g = c.groups[gi];
            EXPECT(it.atomic == g.atomic, "list %d item %zu: atomic %u, group's %u", list, k, it.atomic, g.atomic);
            EXPECT(it.tile < (u32)ntiles && ((g.live_tiles >> it.tile) & 1u), "list %d item %zu: tile %u is not live in group %zu", list, k, it.tile, gi);
            if (it.tile >= 4)
                continue;
            EXPECT(!((seen[gi] >> it.tile) & 1u), "list %d item %zu: pair (%zu, %u) twice", list, k, gi, it.tile);
            seen[gi] |= 1u << it.tile;
            const bool is_front = (front[gi] >> it.tile) & 1u;
            EXPECT(it.pad_ <= 1u, "pad_ %u", it.pad_);
            EXPECT((list == 1 || it.pad_ == 1u) == is_front, "list %d item %zu pad_ %u: pair (%zu, %u) front %d", list, k, it.pad_, gi, it.tile, (int)is_front);
            EXPECT(!is_front || (list == 1) == own_launch, "front pair (%zu, %u) in list %d, own_launch %d", gi, it.tile, list, (int)own_launch);
            EXPECT(list == 0 || it.pad_ == 0u, "front list item %zu with pad_ %u", k, it.pad_);
            padded += list == 0 && it.pad_ == 1u;
            // order: classes non-decreasing, input order inside a class, tiles ascending inside a group
            const bool ordered = (long)cls[gi] > prev_cls || ((long)cls[gi] == prev_cls && ((long)gi > prev_g || ((long)gi == prev_g && (long)it.tile > prev_tile)));
            EXPECT(ordered, "list %d item %zu: (class %u, group %zu, tile %u) behind (class %ld, group %ld, tile %ld)", list, k, cls[gi], gi, it.tile, prev_cls, prev_g, prev_tile);
            prev_cls = (long)cls[gi];
            prev_g = (long)gi;
            prev_tile = (long)it.tile;
        }
    }
    EXPECT(padded == p.n.nfm, "%zu items with pad_ = 1, nfm %zu", padded, p.n.nfm);
    for (size_t gi = 0; gi < gd; gi++)
        EXPECT(seen[gi] == (c.groups[gi].live_tiles & ((1u << ntiles) - 1u)), "group %zu: tiles %x planned, %x live", gi, seen[gi], c.groups[gi].live_tiles);
    // the launch log's slab-step total: the sum over every (group, tile), live or not
    unsigned long long steps = 0;
    for (const SsssmGroupD &g : c.groups)
        for (u32 t = g.task_begin; t < g.task_end; t++)
            for (int tl = 0; tl < ntiles; tl++)
                steps += (unsigned long long)__builtin_popcount(c.live_k[(size_t)t * 4 + tl] & kmask_of(g));
    const unsigned long long got = update_launch_steps(c.groups.data(), gd, c.live_k.data(), o.nb);
    EXPECT(got == steps, "steps %llu, expected %llu", got, steps);
}

static UpdatePlanOptions options(long long front_stages, long long tiles_stages, long long front_min_wgs, int heavy_mode)
{
    return UpdatePlanOptions{0, front_stages, tiles_stages, front_min_wgs, heavy_mode};
}

// the hand-made inputs
static Case ksplit_case(int nb) // one destination, three updates, cut four ways along K (the directed small launches)
{
    Case c;
    c.opt = options(2, 2, 2048, 2);
    c.opt.nb = nb;
    const int tiles = nb / 128;
    const unsigned slabs = (unsigned)nb / 16u, per = slabs / 4;
    for (int t = 0; t < 3; t++)
    {
        for (int tl = 0; tl < 4; tl++)
            c.live_k.push_back(tl < tiles * tiles ? (unsigned short)(t == 1 ? 0x0F0Fu & ((1u << slabs) - 1u) : (1u << slabs) - 1u) : (unsigned short)0);
        c.full_t.push_back(t == 1 ? 0 : (unsigned char)((1u << (tiles * tiles)) - 1u));
    }
    for (unsigned q = 0; q < 4; q++)
    {
        SsssmGroupD g;
        memset(&g, 0, sizeof(g));
        g.cdense = mirror(7);
        g.task_begin = 0;
        g.task_end = 3;
        g.atomic = 1;
        g.slab_mask = ((1u << per) - 1u) << (q * per);
        c.groups.push_back(g);
    }
    derive_live_tiles(c);
    return c;
}
static Case arbitrary_live_tiles_case() // live_tiles is followed as given, whatever live_k says
{
    Case c = random_case(77, 256, 9, 2, 0, options(2, 2, 4, 1));
    const unsigned bits[9] = {0x0, 0x1, 0x2, 0x4, 0x8, 0x5, 0xA, 0xF, 0x6};
    for (size_t gi = 0; gi < 9; gi++)
        c.groups[gi].live_tiles = bits[gi];
    return c;
}
static Case all_front_case(size_t gd, long long front_min_wgs, long long tiles_stages) // nb = 128: every group one dense-front pair, nfull = gd
{
    return random_case(5, 128, gd, 1, 0, options(2, tiles_stages, front_min_wgs, 2));
}

// the recorded cases: tests/golden/update_plan_expected.json holds the plans the launch code made of them before the plan was a function
static std::vector<Case> recorded_cases()
{
    std::vector<Case> v;
    v.push_back(random_case(11, 256, 48, 2, 2, options(2, 2, 2048, 2))); // the defaults: front pairs stay in the general launch
    v.push_back(random_case(12, 256, 48, 2, 2, options(2, 2, 16, 2)));   // ... and get a launch of their own
    v.push_back(random_case(13, 256, 40, 2, 2, options(2, 2, 16, 1)));   // four classes
    v.push_back(random_case(14, 256, 40, 2, 2, options(2, 2, 16, 0)));   // the input order
    v.push_back(random_case(15, 128, 40, 2, 0, options(1, 2, 2048, 2))); // one tile; front pairs without a kernel of their own
    v.push_back(random_case(16, 128, 24, 1, 0, options(3, 0, 2048, 2))); // register-staged general kernel: always an own front launch
    v.push_back(random_case(17, 192, 20, 2, 2, options(2, 2, 1, 2)));    // no front path at this block order
    v.push_back(random_case(18, 256, 2, 2, 0, options(2, 2, 1, 2)));
    v.push_back(random_case(19, 256, 1, 1, 0, options(2, 2, 1, 2)));
    v.push_back(random_case(20, 256, 0, 0, 0, options(2, 2, 1, 2)));
    v.push_back(ksplit_case(256));
    v.push_back(ksplit_case(128));
    v.push_back(random_case(21, 256, 30, 2, 2, options(0, 2, 1, 2)));     // front path off
    return v;
}

static void write_plan(FILE *f, const Plan &p)
{
    fprintf(f, "%zu %zu %zu\n", p.n.nw, p.n.nf, p.n.nfm);
    for (int list = 0; list < 2; list++)
        for (size_t k = 0; k < (list ? p.n.nf : p.n.nw); k++)
        {
            const SsssmWorkD &it = (list ? p.work_f : p.work)[k];
            fprintf(f, "%lu %u %u %u %u %u %u\n", mirror_id(it.cdense), it.task_begin, it.task_end, it.atomic, it.slab_mask, it.tile, it.pad_);
        }
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "plans"))
    {
        for (const Case &c : recorded_cases())
            write_plan(stdout, run(c));
        return 0;
    }
    char name[128];
    int k = 0;
    for (const Case &c : recorded_cases())
    {
        snprintf(name, sizeof(name), "recorded case %d", k++);
        check(name, c);
    }
    // every switch combination, block order, queue count, fill and K-split mix
    unsigned seed = 100;
    for (int nb : {128, 256, 192})
        for (size_t gd : {(size_t)0, (size_t)1, (size_t)2, (size_t)7, (size_t)300})
            for (long long fs : {0, 1, 2})
                for (long long ts : {0, 1})
                    for (int hm : {0, 1, 2})
                        for (int full_mode : {0, 1, 2})
                        {
                            const int mask_mode = (int)(seed % 3);
                            const long long fmw = (seed % 2) ? 8 : 2048;
                            snprintf(name, sizeof(name), "random nb=%d gd=%zu front_stages=%lld tiles_stages=%lld heavy=%d full=%d mask=%d min_wgs=%lld seed=%u",
                                     nb, gd, fs, ts, hm, full_mode, mask_mode, fmw, seed);
                            check(name, random_case(seed++, nb, gd, full_mode, mask_mode, options(fs, ts, fmw, hm)));
                        }
    // the threshold of the front kernel's own launch: one below, at, one above
    for (long long ts : {1, 2})
        for (long long fmw : {39, 40, 41})
        {
            snprintf(name, sizeof(name), "40 front pairs, front_min_wgs=%lld tiles_stages=%lld", fmw, ts);
            check(name, all_front_case(40, fmw, ts));
        }
    {
        // ... and with four tiles: nfull counts pairs, not groups
        Case c = random_case(6, 256, 10, 1, 0, options(2, 2, 40, 2));
        for (long long fmw : {39, 40, 41})
        {
            c.opt.front_min_wgs = fmw;
            snprintf(name, sizeof(name), "10 groups of 4 front pairs, front_min_wgs=%lld", fmw);
            check(name, c);
        }
    }
    snprintf(name, sizeof(name), "arbitrary live_tiles");
    check(name, arbitrary_live_tiles_case());
    if (g_failures)
    {
        printf("%d checks failed\n", g_failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
