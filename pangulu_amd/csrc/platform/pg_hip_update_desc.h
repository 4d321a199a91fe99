// pg_hip_update_desc.h -- what the host writes for the update (SSSSM) kernels and the kernels read: block views, task, group and
// work-item descriptors.  Plain C++ over val_t / u32 / u16 (pg_hip_platform.hip, or tests/hip_emulation_shims.h for the
// device-free test of the work plan): nothing of HIP.
#pragma once

#define DG_TILE 128 // edge of the destination tile one workgroup of the MFMA update kernels owns (SsssmWorkD::tile)

struct BlkView // one compressed view of a block: pointer array over the major dimension, minor indices, values
{
    const u32 *ptr;
    const u16 *idx;
    val_t *val;
};

struct SsssmTaskD
{
    BlkView a; // op1 (L block), CSC
    BlkView b; // op2 (U block), CSC
    // MFMA kernel only.  CR64: a complex update is four real products on the planes of the mirrors; `sign` multiplies the A
    // operand (the A_im B_im product ADDS to the real plane), `count` marks the one of the four whose structural flops count
    double sign;
    u32 count;
    // has_map: amap / bmap_t hold the occupancy of the operands (from the host's summaries, BlockState::occ_map):
    //   amap[s]   bit r: A has pattern entries in row slab r of K-slab (column slab) s
    //   bmap_t[s] bit c: B has pattern entries in column slab c of K-slab (row slab) s
    // otherwise (blocks received from another rank) the kernel reads the maps behind the mirrors
    u32 has_map;
    unsigned short amap[16], bmap_t[16];
};
static_assert(sizeof(SsssmTaskD) == 128, "two task descriptors per 256 bytes");

// one workgroup of the MFMA update launch: a 128 x 128 tile of one destination and the queue of updates that reach it
struct SsssmWorkD
{
    val_t *cdense;          // the destination's mirror (CR64: one plane of it)
    u32 task_begin, task_end;
    u32 atomic, slab_mask;  // as in SsssmGroupD
    u32 tile, pad_;
};

struct SsssmGroupD
{
    BlkView c;        // destination CSC (diagonal destination: its strictly-lower half)
    // diagonal destination only: column view of the upper half (built once per diagonal block, see DiagAux)
    const u32 *ucp;
    const u16 *uri;
    const u32 *uvi;
    val_t *uval;
    // dense-mode destination: its nb x nb column-major mirror (see pg_hip_dense.h); the sparse views above are unused
    val_t *cdense;
    u32 task_begin, task_end;
    // a destination with many queued updates is cut into several groups that run concurrently: each then starts
    // from zero and ADDS its partial sum to the destination with floating-point atomics (otherwise the longest
    // queue sets the duration of the whole launch)
    u32 atomic;
    // MFMA kernel, nb <= 256: bit s set = this group works on K-slab s (16 wide) of every task; 0 = all slabs.  A launch
    // with a handful of updates (the diagonal block's update near the root of the tree, on the critical path of
    // every level) is cut four ways along K so that 16 CUs instead of 4 share a 256 x 256 x 256 product.
    u32 slab_mask;
    // host side only: which of the destination's 128 x 128 tiles some update of this group can reach (bit = tile index);
    // the launch leaves the others out (pangulu_platform_0201001_prepare_blocks)
    u32 live_tiles;
    u32 pad_;
};
