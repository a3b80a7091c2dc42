// How a dense contraction is launched: which kernel, its tiles and grid, the split-K plan and its second pass, and the profile
// record's label - ONE pure function of the problem's shape, the ofx_tune knobs and the device's CU count (gemm_plan), which
// ofx_launch_gemm (gemm.hip) calls after validating its arguments and then only carries out; plus the TN kernel's split plan
// (gemm_tn_splits) and the slab sizes that go with both.  Plain integer and double arithmetic, nothing of HIP, so a host compiler
// builds it alone: tests/test_gemm_plan.py dumps every field over a lattice of shapes and knobs and compares with the transcription
// of the rules in tests/gemm_plan_ref.py.  The cost models switch floating-point contraction off, so a plan does not depend on the
// flags the host code is compiled with.
#pragma once
#include <cstddef>

// The NT GEMM kernels by number.  The same numbers are the values of ofx_tune(2, v) (GemmKnobs::kernel: 0 = the automatic choice; 6
// forces only the kernel of split-weight GEMMs) and the `kind` of the profile records (include/ofx.h), where 7 - no dispatcher kind -
// labels the fused QKV projection + attention launch of fused_qkv_attn.hip.
//   kind   tile      kernel                 notes
//   1      128x128   gemm_128x128_kernel    4 waves; carries the split-K plans and, planned or forced, the 64-row variant
//   2      256x256   gemm_big_kernel        8 waves, two LDS stages
//   3      256x128   gemm_big_kernel        4 waves, register-resident k-tile, two blocks per CU
//   4      256x256   gemm_pp_kernel         ping-pong wave groups (short K)
//   5      64x128    gemm_128x128_kernel    the 64-row variant, forced (ofx_tune only)
//   6      256x256   gemm_w2_kernel         dual weight [hi | lo] against one copy of A
//   8      256x256   gemm_w2f8_kernel       kind 6 with the correction product on the fp8 matrix instruction (never forced: chosen from 6)
//   9      256x128   gemm_x3_kernel         three products with the operand tiles loaded once (never forced: ofx_tune(15, v))
enum GemmKind { GEMM_AUTO = 0, GEMM_128 = 1, GEMM_256 = 2, GEMM_256x128 = 3, GEMM_PP = 4, GEMM_64 = 5, GEMM_W2 = 6, GEMM_W2F8 = 8, GEMM_X3 = 9 };
// the big-tile kernels live in their own translation units behind the ofx_gemm_launch_* functions (gemm_common.h)
inline bool gemm_kind_big_tile(int kind) {
    return kind == GEMM_256 || kind == GEMM_256x128 || kind == GEMM_PP || kind == GEMM_W2 || kind == GEMM_W2F8 || kind == GEMM_X3;
}

// The ofx_tune knobs of the GEMM launch (the one object lives in gemm.hip).
struct GemmKnobs {
    int kernel = GEMM_AUTO;   // ofx_tune(2, v): a GemmKind forces that kernel
    int splitk = 1;           // ofx_tune(5, v): 0 = never split, 1 = plan, >= 2 = forced (experiments: low byte = splits, bit 8 = 64-row tiles)
    int x3_kernel = 1;        // ofx_tune(15, v), three-product GEMMs (k_mult == 3: A rows [hi | lo | hi], W rows [hi | hi | lo]): 1 = the operand-tiles-loaded-once
                              // 256x128 kernel (gemm_x3.hip) from 192 tiles on, 2 = always, 0 = the K-concatenated single-product kernels
    int x3_persist = 1;       // ofx_tune(16, v): 1 gemm_x3_kernel launches one block per CU walking its tiles (when it has more tiles than CUs), 0 = one block per tile
    int w2_persist = -1;      // ofx_tune(11, v), dual-weight kernels: persistent grid size (blocks walk tiles b, b + grid, ...): -1 = one block per CU of the device, 0 = one block per tile
    int epi_direct = 1;       // ofx_tune(18, v): 1 gemm_w2f8_kernel's operand-type outputs leave straight from the accumulator layout (epilogue_direct), 0 = through LDS
};

// What the launch decision reads of a validated GemmArgs (ofx_common.h).
struct GemmShape {
    int M, N, K, lda;
    int a_wrap;          // split weights: K = 2 a_wrap, A's k index wraps; 0 otherwise
    int k_mult;          // 3: three-product K-concatenation
    bool f16;            // operand type f16 (else bf16)
    bool has_w8;         // the fp8 copy of the weights' lo half and its scales are given
    bool has_m_dev;      // device-side live row count
    bool can_split;      // a split-K slab is given and the GEMM has no LayerNorm-fold role
    bool defer;          // the caller takes the slabs of a split plan (GemmArgs::defer_splits)
    bool ln_fusable;     // a LayerNorm follows and the epilogue is plain (fp32 output, no activation, tape or dropout): all of the fused reduce's condition but the width
    int out_kind;        // 0 fp32 | 1 operand type | 2 split3
    bool resid, aux, xlo;
};

// second pass of a split-K plan: none (one launch writes the output), left to the consumer, fused with the following LayerNorm, the plain reduce
enum GemmSecondPass { GEMM_PASS_NONE = 0, GEMM_PASS_DEFERRED = 1, GEMM_PASS_REDUCE_LN = 2, GEMM_PASS_REDUCE = 3 };

struct GemmPlan {
    int kind;                     // GemmKind of the kernel (a planned 64-row launch stays kind 1)
    int tile_m, tile_n;           // the block's output tile
    int tiles_m, tiles_n, nwg;    // tiles of the problem (KArgs)
    int group_m;                  // row panels per L2 group of the tile walk (gemm_walk.h)
    int splits, kt_per_split;     // split-K over blockIdx.y: split y owns k-tiles [y kt_per_split, ...); 1, 0 without
    int grid_x, grid_y;           // the launch's grid: grid_x < nwg = a persistent grid whose blocks walk tiles b, b + grid_x, ...
    int second_pass;              // GemmSecondPass
    int reduce_grid;              // blocks of the plain reduce (GEMM_PASS_REDUCE; 0 otherwise)
    int epi_direct;               // KArgs::epi_direct (kind 8 only)
    // the profile record: executed FLOPs in f16-rate equivalents (the fp8 correction product of kind 8 runs at twice the f16 rate:
    // 1.5 products, not 2), algorithmic HBM bytes, and the logical shape - K without the split-weight / three-product concatenation
    double flops, bytes;
    int kmul, k_logical;
};

// the widths ofx_launch_splitk_reduce_ln (norm_act.hip) has kernels for
inline bool splitk_reduce_ln_width_ok(int D) { return D == 512 || D == 768 || D == 1024 || D == 1536; }

// Grid of a kernel whose blocks can walk tiles b, b + grid, ... over nwg tiles.  persist: -1 = one block per CU, 0 = one block per
// tile, n = n blocks.  A device-side row count (has_m_dev) always takes one block per tile: tiles past the live rows leave at once.
// Never more blocks than tiles.
inline int gemm_persistent_grid(int nwg, int persist, bool has_m_dev, int cu_count) {
    if (persist < 0) persist = cu_count;
    return (persist && !has_m_dev && nwg > persist) ? persist : nwg;
}

// Plan for problems the big-tile kernels cannot fill (small M): tile height (128 rows, 2 blocks per CU = 512 slots; or 64 rows, 3 per
// CU = 768 slots) x deterministic split-K over blockIdx.y.  Cost model (us), measured on these kernels: ~1.06 / ~0.65 us per k-tile
// and round of co-resident 128- / 64-row blocks; a split adds the fp32 slab written once and read once (~5 TB/s) and the reduce
// launch.  M = 2304 x N = 1024 (144 blocks) is faster UNSPLIT (17 vs 26 us); M = 288 (K = 3072) wants the split.
struct GemmSmallPlan { int tile64, splits; double cost; };
inline GemmSmallPlan gemm_plan_small(int M, int N, int K, bool allow_split, bool allow64, int splitk) {
#pragma clang fp contract(off)
    const int nk = K / 64;
    GemmSmallPlan best{0, 1, 1e30};
    if (splitk >= 2) {
        GemmSmallPlan f{(splitk >> 8) & 1, (splitk & 0xff) > 16 ? 16 : (splitk & 0xff), 0.0};      // forced plans: at most 16 slices, as the planner's own
        if (f.tile64 && !allow64) f.tile64 = 0;
        if (!allow_split || f.splits > nk) f.splits = 1;
        const int kps = (nk + f.splits - 1) / f.splits;
        f.splits = (nk + kps - 1) / kps;                       // every split owns at least one k-tile
        return f;
    }
    for (int t64 = 0; t64 <= (allow64 ? 1 : 0); ++t64) {
        const long blocks = (long)((M + (t64 ? 63 : 127)) / (t64 ? 64 : 128)) * (N / 128);
        const long slots = t64 ? 768 : 512;
        const double per = t64 ? 0.65 : 1.06;
        for (int sp = 1; sp <= 16; ++sp) {
            if (sp > 1 && !(allow_split && splitk != 0 && blocks < 256 && nk >= 16 && sp <= nk / 4)) break;
            const int kps = (nk + sp - 1) / sp;
            if ((nk + kps - 1) / kps != sp) continue;
            double t = (double)((blocks * sp + slots - 1) / slots) * kps * per + (t64 ? 1.0 : 0.0);
            if (sp > 1) t += 2.0 * sp * M * N * 4.0 / 5.0e6 + 3.0;
            if (t < best.cost) best = GemmSmallPlan{t64, sp, t};
        }
    }
    return best;
}
// Slab size for ANY plan the launcher may pick for this shape: gemm_plan plans with or without 64-row tiles depending on the kernel
// knob and the grid (can64), so the slab covers the larger slice count of the two tile heights (forced plans: <= 16).
inline size_t gemm_splitk_slab_bytes(int M, int N, int K, const GemmKnobs& kn) {
    const int a = gemm_plan_small(M, N, K, true, true, kn.splitk).splits, b = gemm_plan_small(M, N, K, true, false, kn.splitk).splits;
    const int sp = a > b ? a : b;
    return sp > 1 ? (size_t)sp * M * N * 4 : 0;
}

inline GemmPlan gemm_plan(const GemmShape& g, const GemmKnobs& kn, int cu_count) {
    GemmPlan p{};
    // big tiles when they still fill the chip, else the 128^2 kernel
    int kind = kn.kernel == GEMM_W2 ? GEMM_AUTO : kn.kernel;      // GEMM_W2 only forces the kernel of split-weight GEMMs; every other GEMM keeps the automatic choice
    if (g.a_wrap) {        // split weights: the dual-weight 256x256 kernel when its grid fills the chip, else the 128x128 kernel with a wrapping A index
        const long t2 = (long)((g.M + 255) / 256) * (g.N / 256);
        kind = (g.K == 2 * g.a_wrap && g.a_wrap % 32 == 0 && g.a_wrap >= 64 && g.N % 256 == 0 && (t2 >= 256 || kn.kernel == GEMM_W2) && kn.kernel != GEMM_128) ? GEMM_W2 : GEMM_128;
        // the correction product on the fp8 matrix instruction
        if (kind == GEMM_W2 && g.has_w8 && g.f16 && g.a_wrap % 128 == 0) kind = GEMM_W2F8;
    } else if (kind == GEMM_AUTO) {   // measured crossover points (tools/gemm_bench.py, profiles/r01_gemm_variants.txt)
        const long t2 = (long)((g.M + 255) / 256) * (g.N / 256), t3 = (long)((g.M + 255) / 256) * (g.N / 128);
        if (g.N % 256 == 0 && t2 >= 1024) kind = g.K <= 1024 ? GEMM_PP : GEMM_256;   // 256x256, one block per CU (short K: the ping-pong kernel)
        else if (g.N % 128 == 0 && t3 >= 512) kind = GEMM_256x128;                  // short K / mid-size M: 256x128, two blocks per CU
        else kind = GEMM_128;
    }
    if (g.k_mult == 3 && !g.a_wrap && kn.x3_kernel && (kn.kernel == GEMM_AUTO || kn.kernel == GEMM_W2) && g.K % 96 == 0 && g.N % 128 == 0 && g.lda >= g.K &&
        (kn.x3_kernel >= 2 || (long)((g.M + 255) / 256) * (g.N / 128) >= 192))
        kind = GEMM_X3;            // the three products from ONE copy of each operand tile
    if ((kind == GEMM_256 || kind == GEMM_PP) && g.N % 256) kind = GEMM_128;
    if (kind == GEMM_64 && g.N % 128) kind = GEMM_128;
    p.kind = kind;

    // algorithmic HBM bytes of this launch: A once (its k index wraps over a_wrap columns for split weights), the weight rows as
    // stored, and per output element what the configured epilogue moves: fp32 4 (+4 residual read), operand type 2 (in-place
    // (hi, lo) stream: 4 read + 4 written), [hi | lo | hi] 6, +4 pre-activation tape copy
    p.kmul = g.a_wrap ? g.K / g.a_wrap : (g.k_mult > 0 ? g.k_mult : 1);
    p.k_logical = g.K / p.kmul;
    const double ab = kind == GEMM_X3 ? 2.0 * g.M * (g.K / 3) * 2 : 2.0 * g.M * (g.a_wrap ? g.a_wrap : g.K);
    const double wb = kind == GEMM_W2F8 ? 3.0 * g.N * g.a_wrap : (kind == GEMM_X3 ? 2.0 * g.N * (g.K / 3) * 2 : 2.0 * g.N * g.K);      // GEMM_W2F8 reads the hi rows (2 B) + the fp8 lo rows (1 B)
    double ob = g.out_kind == 0 ? 4.0 : (g.out_kind == 2 ? 6.0 : 2.0);
    if (g.xlo) ob = 8.0;
    else if (g.resid) ob += 4.0;
    if (g.aux) ob += 4.0;
    p.bytes = ab + wb + ob * g.M * g.N;
    p.flops = 2.0 * g.M * g.N * g.K * (kind == GEMM_W2F8 ? 0.75 : 1.0);

    p.splits = 1; p.kt_per_split = 0; p.grid_y = 1; p.second_pass = GEMM_PASS_NONE;
    if (gemm_kind_big_tile(kind)) {
        p.tile_m = 256; p.tile_n = (kind == GEMM_256x128 || kind == GEMM_X3) ? 128 : 256;
        p.group_m = kind == GEMM_256x128 ? 4 : 8;
        p.tiles_n = g.N / p.tile_n; p.tiles_m = (g.M + p.tile_m - 1) / p.tile_m; p.nwg = p.tiles_m * p.tiles_n;
        p.grid_x = p.nwg;
        if (kind == GEMM_W2 || kind == GEMM_W2F8) p.grid_x = gemm_persistent_grid(p.nwg, kn.w2_persist, g.has_m_dev, cu_count);
        // ofx_tune(16, 0): one block per tile (short-lived blocks: a side stream's GEMM then frees its CUs tile by tile)
        if (kind == GEMM_X3) p.grid_x = gemm_persistent_grid(p.nwg, kn.x3_persist == 1 ? kn.w2_persist : 0, g.has_m_dev, cu_count);
        if (kind == GEMM_W2F8) p.epi_direct = kn.epi_direct;
        return p;
    }
    p.tile_m = 128; p.tile_n = 128;
    p.tiles_n = g.N / 128; p.tiles_m = (g.M + 127) / 128;
    // row panels per L2 group: (group_m + 64/group_m) panels of 128 x K operands should fit ~3 MiB of the XCD's L2
    int gm = (int)((3u << 20) / ((size_t)128 * g.K * 2) / 2);
    gm = gm < 1 ? 1 : (gm > 8 ? 8 : gm);
    p.group_m = gm;
    const bool can64 = (kind == GEMM_64) || (kind == GEMM_128 && kn.kernel == GEMM_AUTO && g.M > 64 && (long)p.tiles_m * p.tiles_n <= 384);
    GemmSmallPlan pl = gemm_plan_small(g.M, g.N, g.K, g.can_split, can64, kn.splitk);
    if (kind == GEMM_64) pl.tile64 = 1;
    if (pl.tile64) {        // 64-row tiles, three blocks per CU: grids that would leave CUs idle with 128-row tiles (with or without split-K)
        p.tile_m = 64; p.tiles_m = (g.M + 63) / 64; p.group_m = 2 * gm;
    }
    p.nwg = p.tiles_m * p.tiles_n;
    p.splits = pl.splits;
    p.grid_x = p.nwg; p.grid_y = p.splits > 1 ? p.splits : 1;
    if (p.splits > 1) {
        p.kt_per_split = (g.K / 64 + p.splits - 1) / p.splits;
        p.second_pass = g.defer ? GEMM_PASS_DEFERRED : ((g.ln_fusable && splitk_reduce_ln_width_ok(g.N)) ? GEMM_PASS_REDUCE_LN : GEMM_PASS_REDUCE);
        if (p.second_pass == GEMM_PASS_REDUCE) {
            const size_t tot = (size_t)g.M * (g.N / 4);
            const int rg = (int)((tot + 255) / 256);
            p.reduce_grid = rg > 2048 ? 2048 : rg;
        }
    }
    return p;
}

// ---- TN GEMM (wgrad, gemm_tn.hip): split plan
inline int gemm_tn_splits(int M, int N, int K) {
#pragma clang fp contract(off)
    // cost model (us): waves of blocks x k-tiles per split x ~1.6 us per 256x256x64 k-tile, plus the slab written once and
    // read once at ~4 TB/s.  K is the static upper bound of the live row count, so the plan is shape-only (graph-safe).
    const long tiles = (long)((M + 255) / 256) * (N / 256);
    const int nkt = (K + 63) / 64;
    int best = 1;
    double best_t = 1e30;
    for (int s = 1; s <= 16 && s <= nkt; ++s) {
        const double waves = (double)((tiles * s + 255) / 256);
        const double t = waves * ((nkt + s - 1) / s) * 1.6 + 4.0 + (s > 1 ? 2.0 * s * M * N * 4.0 / 4.0e6 + 3.0 : 0.0);
        if (t < best_t) { best_t = t; best = s; }
    }
    return best;
}
inline size_t gemm_tn_slab_bytes(int M, int N, int K) {
    const int s = gemm_tn_splits(M, N, K);
    return s > 1 ? (size_t)s * M * N * 4 : 0;
}
