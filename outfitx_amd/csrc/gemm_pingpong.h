// The two-wave-group "ping-pong" main loop of the counted-wait 8-wave tile kernels, once (included by gemm_common.h): gemm_w2.hip,
// gemm_x3.hip, gemm_w2f8.hip and the dual-weight branch and the fp8-correction kernel of fused_qkv_attn.hip.  The kernels keep what is theirs - stage layout,
// piece list, wait counts, products - and pass it in as callables; everything here is force-inlined into them.
//
// Waves 0-3 (group 0) and 4-7 (group 1) run the same per-k-step program offset by ONE barrier slot: on every SIMD one wave reads its
// fragments and issues LDS-DMA while the other runs its MFMAs.
//
// BK = 32, NST = 3 or 4 stages; pp_slot below is one iteration = two slots of one group:
//     slot:      0     1         2         3         4         5
//     group 0:  [W0]  [R0 I2]   [M0]      [R1 I3]   [M1]      [R2 I4]  ...   I(s) = issue step s into stage s % NST
//     group 1:  [W0]  [  ]      [R0 I2]   [M0]      [R1 I3]   [M1]     ...
//   Step s is read in slots 2s+1 (group 0) and 2s+2 (group 1); with three stages its stage is refilled with step s+3 in slots 2s+3 /
//   2s+4 (WAR: both groups' reads ended before the barrier that closes slot 2s+2).  Every wave waits for its own pieces of step s+1
//   before the barrier that closes slot 2s+2 - a counted vmcnt(NV), NV = the pieces the iteration itself issued, which stay in flight:
//   group 0 at the end of its MFMA slot, group 1 at the end of its read slot - and step s+1 is first read in slot 2s+3 (RAW).
//   ISSUE comes before the reads: the LDS-DMA issue costs the issuing wave ~100 cycles, which the wave would otherwise spend waiting
//   for its fragments (threaded through the MFMAs it cost 0.3 us of every 0.8 us slot).
//   Group 1 opens with one barrier (slot 1: group 0 reads step 0), group 0 closes with one (group 1's last MFMA slot: behind it every
//   read of the tile's stages is done).
// Persistent blocks (PpWalk): block b runs tiles b, b + grid, ...; the k-steps are numbered across the block's tiles, step g lives in
//   stage g % NST, so the fills that would be redundant at the end of a tile (steps nk, nk + 1, ...) fetch the NEXT tile's first steps:
//   they land under the epilogue, whose staging sits in the stage of the tile's last step (the one stage no such fill targets), and the
//   next main loop starts without a load-latency bubble.  tests/test_gemm_pingpong.py replays the schedule on the integers below.
// BK = 32 LDS image (PpLane32): operand rows of 64 B, a wave-instruction moves 16 rows; the 16-B chunk c of row r sits at slot
//   c ^ f(r >> 2), f(g) = (-g) & 3, applied on the DMA source address and on the ds_read_b128 side: conflict-free for the hardware's
//   lane groups of ds_read_b128 (MI355X_MICROARCH.md, LDS table).
// (The BK = 64 two-stage loops of gemm_pp.hip and of fused_qkv_attn.hip's single-product branch wait with vmcnt(0) and thread
// group 1's pieces through its MFMAs: another protocol, written out in those two files.)
#pragma once
#include "gemm_walk.h"

// Stage arithmetic of a persistent block's walk: plain integers, host-compilable like gemm_walk.h.  `base` = (index, counted over
// the block's tiles, of the current tile's step 0) mod NST; step x of the walk (x >= nk: step x - nk of the next tile) lives in:
template <int NST>
OFX_WALK_FN int pp_stage(int base, int x) { return (base + x) % NST; }
// the epilogue stages in the stage of the tile's last step
template <int NST>
OFX_WALK_FN int pp_epilogue_stage(int base, int nk) { return (base + nk - 1) % NST; }
template <int NST>
OFX_WALK_FN int pp_next_base(int base, int nk) { return (base + nk) % NST; }

#if defined(__HIP__)
#include "ofx_common.h"

namespace {

struct PpNone {
    __device__ __forceinline__ void operator()() const {}
};

// One iteration of group GRP in the counted-wait family; NV reaches the instruction as an immediate.
template <int GRP, int NV, typename Issue, typename Read, typename Mfma, typename Tail = PpNone>
__device__ __forceinline__ void pp_slot(Issue&& issue, Read&& read, Mfma&& mfma, Tail&& tail = Tail()) {
    issue();
    read();
    if (GRP == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NV) : "memory");      // my pieces of the next step landed: group 0 reads them next slot
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    mfma();
    tail();
    if (GRP == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NV) : "memory");      // my pieces of the next step landed (this iteration's stay in flight)
    __builtin_amdgcn_s_barrier();
}
template <int GRP>
__device__ __forceinline__ void pp_group_begin() {
    if (GRP == 1) __builtin_amdgcn_s_barrier();      // slot 1: group 0 reads step 0
}
template <int GRP>
__device__ __forceinline__ void pp_group_end() {
    if (GRP == 0) __builtin_amdgcn_s_barrier();      // closes group 1's last MFMA slot: every read of this tile's stages is done
}

// Lane constants of the BK = 32 image, from an opaque copy of the lane id.  LDS-DMA piece (16 rows x 64 B): lane l -> row l >> 2,
// physical slot l & 3 <- logical chunk (l & 3) ^ f(row >> 2); fragment: row fr, k-quarter fq at byte fchk of the row.
struct PpLane32 {
    int prow, pchk, fr, fq, fchk;
    __device__ __forceinline__ explicit PpLane32(int ln)
        : prow(ln >> 2), pchk((ln & 3) ^ ((4 - (ln >> 4)) & 3)), fr(ln & 15), fq(ln >> 4), fchk((fq ^ ((4 - (fr >> 2)) & 3)) * 16) {}
};

// The persistent walk of a block over TM x TN tiles with NST stages.  Precondition: nk >= 2 (with four stages: a multiple of 4) -
// an iteration fills up to NST - 1 steps ahead, and stage(x) knows the next tile only: a fill must not reach past it (with one
// k-step per tile iteration 0's fill of step 2 would belong two tiles ahead).  The dispatcher admits no shallower problem.
template <int NST, int TM, int TN>
struct PpWalk {
    int nwg, group_m, tiles_m, tiles_n, nk;
    int vb, base, m0, n0;
    bool first;
    __device__ __forceinline__ PpWalk(int nwg_, int group_m_, int tiles_m_, int tiles_n_, int nk_)
        : nwg(nwg_), group_m(group_m_), tiles_m(tiles_m_), tiles_n(tiles_n_), nk(nk_), vb(blockIdx.x), base(0), first(true) {
        origin(vb, m0, n0);
    }
    __device__ __forceinline__ void origin(int v, int& m, int& n) const {
        int tm, tn;
        grouped_tile(xcd_remap(v, nwg), group_m, tiles_m, tiles_n, tm, tn);
        m = tm * TM;
        n = tn * TN;
    }
    __device__ __forceinline__ bool has_next() const { return vb + (int)gridDim.x < nwg; }
    // the next tile's origin; the block's last tile names itself (it re-fills its own first steps: nobody reads them)
    __device__ __forceinline__ void next_origin(int& m1, int& n1) const {
        m1 = m0; n1 = n0;
        if (has_next()) origin(vb + (int)gridDim.x, m1, n1);
    }
    __device__ __forceinline__ int stage(int x) const { return pp_stage<NST>(base, x); }
    __device__ __forceinline__ int epilogue_stage() const { return pp_epilogue_stage<NST>(base, nk); }
    __device__ __forceinline__ void advance() {
        vb += gridDim.x;
        origin(vb, m0, n0);
        base = pp_next_base<NST>(base, nk);
        first = false;
    }
};

// The dual-weight step: 8 A fragments x NJ column tiles x {hi, lo} of a BK = 32 stage whose W_lo part lies `lo_off` bytes behind W_hi.
template <int NJ, typename V8>
__device__ __forceinline__ void pp_w2_read(OFX_LDS char* stg, int a_frag, int w_frag, int lo_off, V8 (&af)[8], V8 (&wh)[NJ], V8 (&wl)[NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) wh[j] = *(OFX_LDS V8*)(stg + w_frag + j * 16 * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) af[i] = *(OFX_LDS V8*)(stg + a_frag + i * 16 * 64);
#pragma unroll
    for (int j = 0; j < NJ; ++j) wl[j] = *(OFX_LDS V8*)(stg + lo_off + w_frag + j * 16 * 64);
}
// 16 NJ MFMAs (per A fragment: NJ hi then NJ lo) and nothing else in the stream
template <typename T, int NJ, typename V8>
__device__ __forceinline__ void pp_w2_mfma(f32x4 (&acc)[8][NJ], const V8 (&af)[8], const V8 (&wh)[NJ], const V8 (&wl)[NJ]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int m = 0; m < 16 * NJ; ++m) {
        const int i = m / (2 * NJ), j = m % NJ;
        acc[i][j] = OpT<T>::mfma16((m % (2 * NJ)) >= NJ ? wl[j] : wh[j], af[i], acc[i][j]);
    }
    __builtin_amdgcn_s_setprio(0);
}

}  // namespace
#endif
