// C[M,N] = epilogue( A[M,K] · W[N,K]^T ) on gfx950 matrix cores.
//
// Both operands are K-contiguous (activations row-major, weights in torch Linear layout), bf16 or
// f16, fp32 accumulate (v_mfma_f32_16x16x32_{bf16,f16}).  This one kernel carries every dense
// contraction of the scoring path (reference call sites: the nn.Linear / in_proj GEMMs inside
// nn.TransformerEncoderLayer built at src/models/outfit_x.py:32-45 and inside HF CLIP's
// CLIPAttention / CLIPMLP called from clip_image_encoder.py:74-76, clip_text_encoder.py:56-58).
//
// Tile 128x128x64, 256 threads = 4 waves (2x2), wave tile 64x64 = 4x4 MFMA tiles x 2 k-steps.
//  * global -> LDS by LDS-DMA (global_load_lds_dwordx4), two stages; the LDS image is lane-linear,
//    so the bank swizzle (16-B chunk ^= (row>>1)&7) is applied to the per-lane SOURCE address and
//    again on the ds_read_b128 side (guide rule 21).
//  * operands are swapped in the MFMA (W fragment as A-operand) so a lane ends up holding 4
//    consecutive output COLUMNS of one row; the epilogue goes through LDS once and leaves as
//    whole 128/256-byte row segments with bias / activation / fp32 residual fused.
//  * 1-D grid with an XCD-aware remap: the blocks that share an A row-panel are consecutive on
//    one XCD so the panel is fetched into that XCD's L2 once.
#include "gemm_common.h"

namespace {
// MT = MFMA row tiles per wave: 4 -> the 128x128 block tile, 2 -> 64x128 (twice the blocks for grids that leave CUs idle: the
// training step's M ~ 2k-row GEMMs with N = 1024; 48 KiB of LDS, three blocks per CU)
template <typename T, int MT = 4>
__global__ __launch_bounds__(256, 2) void gemm_128x128_kernel(KArgs p) {
    constexpr int BMT = 32 * MT, STAGE_T = (BMT + BN) * BK * 2, EPI_T = 16 * MT * EPI_STRIDE * 4;
    typedef typename OpT<T>::v8 v8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    OFX_LDS char* lds = (OFX_LDS char*)smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    int tm, tn;
    grouped_tile(xcd_remap(blockIdx.x, p.nwg), p.group_m, p.tiles_m, p.tiles_n, tm, tn);
    const int m0 = tm * BMT, n0 = tn * BN;
    if (clamp_live_rows(p.m_dev, p.M, m0)) return;

    // ---- LDS-DMA source addressing: each wave moves 4 A-chunks and 4 W-chunks of 1 KiB (8 rows) per k-tile
    const int lrow = lane >> 3, lchk = lane & 7;
    const char* a_src[MT];
    const char* w_src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = wave * 4 + i;                     // chunk 0..15 → rows c*8 .. c*8+7
        const int row = c * 8 + lrow;
        const int kch = lchk ^ ((row >> 1) & 7);        // logical 16-B chunk stored at physical slot lchk
        w_src[i] = p.W + ((size_t)(n0 + row) * p.K + kch * 8) * 2;
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int row = (wave * MT + i) * 8 + lrow;
        const int kch = lchk ^ ((row >> 1) & 7);
        int gm = m0 + row; gm = gm < p.M ? gm : p.M - 1;
        a_src[i] = p.A + ((size_t)gm * p.lda + kch * 8) * 2;
    }
    const int a_dst = wave * MT * 1024, w_dst = BMT * BK * 2 + wave * 4 * 1024;

    auto issue = [&](int kt, int stage) {
        OFX_LDS char* base = lds + stage * STAGE_T;
        const size_t koff = (size_t)kt * BK * 2, koff_a = (size_t)(kt % p.ka_tiles) * BK * 2;
#pragma unroll
        for (int i = 0; i < MT; ++i) glds16(a_src[i] + koff_a, base + a_dst + i * 1024);
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16(w_src[i] + koff, base + w_dst + i * 1024);
    };

    // ---- fragment read addressing (swizzled): row = tile*16 + (lane&15), logical chunk = ks*4 + (lane>>4)
    const int fr = lane & 15, fq = lane >> 4, fsw = fr >> 1;
    const int a_frag = (wm * 16 * MT + fr) * 128;
    const int w_frag = BMT * BK * 2 + (wn * 64 + fr) * 128;

    f32x4 acc[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    v8 af[2][MT], wf[2][4];
    const int kt0 = p.splits > 1 ? blockIdx.y * p.kt_per_split : 0;
    const int nk = p.splits > 1 ? min(p.K / BK, kt0 + p.kt_per_split) : p.K / BK;
    // (round 4: a third stage - two k-tiles in flight - for the 64-row variant on small grids was built and measured on the batch-32 set transformer,
    //  whose 21 GEMMs are this kernel: 0.637 vs 0.638 ms per forward, i.e. nothing; the k-tile time of those launches is not prefetch depth. Removed.)
    issue(kt0, kt0 & 1);
    for (int kt = kt0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {
            issue(kt + 1, cur ^ 1);
            if (MT == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        OFX_LDS char* base = lds + cur * STAGE_T;
        // all 16 fragment reads of the k-tile go out first; the MFMAs then wait on counted lgkmcnt
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int chk = ((ks * 4 + fq) ^ fsw) * 16;
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[ks][j] = *(OFX_LDS v8*)(base + w_frag + j * 16 * 128 + chk);
#pragma unroll
            for (int i = 0; i < MT; ++i) af[ks][i] = *(OFX_LDS v8*)(base + a_frag + i * 16 * 128 + chk);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = OpT<T>::mfma16(wf[ks][j], af[ks][i], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    // ---- epilogue: acc[i][j][r] = C[m = wm*64 + i*16 + (lane&15)][n = wn*64 + j*16 + (lane>>4)*4 + r]
    OFX_LDS float* ep = (OFX_LDS float*)(lds + wave * EPI_T);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *(OFX_LDS f32x4*)(ep + (i * 16 + fr) * EPI_STRIDE + j * 16 + fq * 4) = acc[i][j];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (p.splits > 1) {                                  // raw partial sums; bias / activation / residual happen in splitk_reduce
        KArgs q = p;
        q.C = (char*)(p.slab + (size_t)blockIdx.y * p.m_slab * p.N); q.ldc = p.N; q.out_kind = 0; q.bias = nullptr; q.resid = nullptr; q.aux_out = nullptr; q.drop.thresh = 0;
        epilogue<T, OFX_ACT_NONE>(q, ep, m0 + wm * 16 * MT, n0 + wn * 64, lane, 16 * MT);
        return;
    }
    switch (p.act) {
        case OFX_ACT_QUICK_GELU: epilogue<T, OFX_ACT_QUICK_GELU>(p, ep, m0 + wm * 16 * MT, n0 + wn * 64, lane, 16 * MT); break;
        case OFX_ACT_GELU: epilogue<T, OFX_ACT_GELU>(p, ep, m0 + wm * 16 * MT, n0 + wn * 64, lane, 16 * MT); break;
        case OFX_ACT_MISH: epilogue<T, OFX_ACT_MISH>(p, ep, m0 + wm * 16 * MT, n0 + wn * 64, lane, 16 * MT); break;
        case OFX_ACT_MISH_GRAD: epilogue<T, OFX_ACT_MISH_GRAD>(p, ep, m0 + wm * 16 * MT, n0 + wn * 64, lane, 16 * MT); break;
        default: epilogue<T, OFX_ACT_NONE>(p, ep, m0 + wm * 16 * MT, n0 + wn * 64, lane, 16 * MT); break;
    }
}


}  // namespace

// The launch knobs: ofx_tune(2 | 5 | 11 | 15 | 16 | 18, v) (GemmKnobs, gemm_plan.h).  No other file reads them: the plan carries what they decide.
static GemmKnobs g_knobs;
int ofx_gemm_tune(int knob, int value) {
    switch (knob) {
        case 2: g_knobs.kernel = value; return OFX_OK;
        case 5:      // a forced plan (>= 2) names its slice count in the low byte: none would divide by zero in gemm_plan_small
            if (value >= 2 && (value & 0xff) == 0) { ofx_set_error("ofx_tune(5): %d forces a split-K plan of 0 slices (low byte = slices, 1-16)", value); return OFX_EINVAL; }
            g_knobs.splitk = value; return OFX_OK;
        case 11: g_knobs.w2_persist = value; return OFX_OK;
        case 15: g_knobs.x3_kernel = value; return OFX_OK;
        case 16: g_knobs.x3_persist = value != 0; return OFX_OK;
        case 18: if (value != 0 && value != 1) { ofx_set_error("ofx_tune(18): %d is not 0 or 1", value); return OFX_EINVAL; } g_knobs.epi_direct = value; return OFX_OK;
        default: ofx_set_error("ofx_tune: unknown knob %d", knob); return OFX_EINVAL;
    }
}
size_t ofx_gemm_splitk_bytes(int M, int N, int K) { return gemm_splitk_slab_bytes(M, N, K, g_knobs); }

// What gemm_plan reads of a GemmArgs.
static GemmShape gemm_shape(const GemmArgs& g, int op_dtype) {
    const bool producer = g.xb_out || g.stat_part || g.xlo;
    GemmShape sh;
    sh.M = g.M; sh.N = g.N; sh.K = g.K; sh.lda = g.lda; sh.a_wrap = g.a_wrap; sh.k_mult = g.k_mult;
    sh.f16 = op_dtype == OFX_F16; sh.has_w8 = g.W8 && g.w8_scale; sh.has_m_dev = g.m_dev != nullptr;
    sh.can_split = g.slab && !producer && !g.row_stat; sh.defer = g.defer_splits != nullptr;
    sh.ln_fusable = g.ln_gamma && g.out_kind == 0 && g.act == OFX_ACT_NONE && !g.aux_out && !g.drop.thresh;
    sh.out_kind = g.out_kind; sh.resid = g.resid != nullptr; sh.aux = g.aux_out != nullptr; sh.xlo = g.xlo != nullptr;
    return sh;
}
// The GemmKind ofx_launch_gemm would run these arguments as, under the current knobs: callers that choose between a GEMM and a kernel
// that stands in for it (clip_layer: the fused QKV projection + attention with the fp8 correction) ask the plan instead of copying its rules.
int ofx_gemm_plan_kind(const GemmArgs& g, int op_dtype) { return gemm_plan(gemm_shape(g, op_dtype), g_knobs, device_cu_count()).kind; }
// Grid of a kernel outside the dispatcher that walks its nwg tiles as the dual-weight GEMMs do: ofx_tune(11, v) applies.
int ofx_gemm_w2_grid(int nwg) { return gemm_persistent_grid(nwg, g_knobs.w2_persist, false, device_cu_count()); }

// Four steps: validate, describe the problem (GemmShape), plan (gemm_plan: every decision), carry the plan out.
int ofx_launch_gemm(const GemmArgs& g, int op_dtype, hipStream_t s) {
    OFX_REQUIRE(g.M > 0 && g.N > 0 && g.K > 0, OFX_ESHAPE, "gemm: empty problem M=%d N=%d K=%d", g.M, g.N, g.K);
    OFX_REQUIRE(g.N % BN == 0, OFX_ESHAPE, "gemm: N=%d must be a multiple of %d (pad the weight at pack time)", g.N, BN);
    OFX_REQUIRE(g.K % BK == 0, OFX_ESHAPE, "gemm: K=%d must be a multiple of %d", g.K, BK);
    OFX_REQUIRE(g.a_wrap == 0 || (g.a_wrap > 0 && g.a_wrap % BK == 0 && g.K % g.a_wrap == 0), OFX_ESHAPE, "gemm: a_wrap=%d must be a multiple of %d dividing K=%d", g.a_wrap, BK, g.K);
    const int ka = g.a_wrap ? g.a_wrap : g.K;
    OFX_REQUIRE(g.lda >= ka && g.lda % 8 == 0, OFX_ESHAPE, "gemm: lda=%d must be >= K and a multiple of 8", g.lda);
    OFX_REQUIRE(g.ldc % (g.out_kind == 0 ? 4 : 8) == 0 && g.ldc >= (g.out_kind == 2 ? 3 * g.N : g.N), OFX_ESHAPE, "gemm: bad ldc=%d", g.ldc);
    OFX_REQUIRE(!g.resid || (g.ldr % 4 == 0 && g.ldr >= g.N), OFX_ESHAPE, "gemm: bad ldr=%d", g.ldr);
    OFX_REQUIRE(((uintptr_t)g.A % 16 == 0) && ((uintptr_t)g.W % 16 == 0) && ((uintptr_t)g.C % 16 == 0), OFX_EINVAL,
                "gemm: operands must be 16-byte aligned");
    OFX_REQUIRE(op_dtype == OFX_BF16 || op_dtype == OFX_F16, OFX_EINVAL, "gemm: operand dtype must be bf16 or f16");
    if (g.defer_splits) *g.defer_splits = 1;
    if (g.ln_done) *g.ln_done = false;
    const bool producer = g.xb_out || g.stat_part || g.xlo;
    OFX_REQUIRE(!producer || (g.xb_out && g.stat_part && g.xlo && g.C == g.xb_out && g.out_kind == 1 && g.ldc == g.N && g.N % 64 == 0), OFX_EINVAL,
                "gemm: a LayerNorm-fold producer takes xb_out, stat_part and xlo together, with C == xb_out in the operand type");
    OFX_REQUIRE(!g.row_stat || g.col_sum, OFX_EINVAL, "gemm: row_stat needs col_sum");
    OFX_REQUIRE(!(g.row_stat || producer) || (!g.aux_out && !g.drop.thresh && g.act != OFX_ACT_MISH && g.act != OFX_ACT_MISH_GRAD), OFX_EINVAL,
                "gemm: LayerNorm folding does not combine with the training epilogue features");
    OFX_REQUIRE(!(g.row_stat || producer) || !g.resid, OFX_EINVAL, "gemm: LayerNorm folding takes no residual (a producer's stream is (xb_out, xlo))");
    OFX_REQUIRE(!producer || g.act == OFX_ACT_NONE, OFX_EINVAL, "gemm: a LayerNorm-fold producer has no activation");

    const GemmPlan pl = gemm_plan(gemm_shape(g, op_dtype), g_knobs, device_cu_count());
    if (pl.splits > 1) OFX_REQUIRE(g.slab_bytes >= (size_t)pl.splits * g.M * g.N * 4, OFX_EWORKSPACE, "gemm: split-K slab too small");

    // record label: logical shape (K without the split-weight / three-product concatenation), the K multiplier and the GemmKind
    if (g_ofx_prof_on) ofx_prof_set_tag(g.M, g.N, pl.k_logical, pl.kind, pl.kmul, pl.bytes);
    ProfScope prof(PROF_GEMM, s, pl.flops, true);      // events ride on the launches (OFX_PLAUNCH)
    KArgs k;
    k.A = (const char*)g.A; k.W = (const char*)g.W; k.C = (char*)g.C; k.bias = g.bias; k.resid = g.resid; k.aux_out = g.aux_out; k.m_dev = g.m_dev;
    k.M = g.M; k.N = g.N; k.K = g.K; k.lda = g.lda; k.ldc = g.ldc; k.ldr = g.ldr; k.act = g.act; k.out_kind = g.out_kind; k.drop = g.drop; k.n_valid = g.N;
    k.ka_tiles = ka / BK;
    k.xb_out = (char*)g.xb_out; k.stat_part = g.stat_part; k.row_stat = g.row_stat; k.col_sum = g.col_sum; k.stat_ld = g.stat_ld > 0 ? g.stat_ld : 1; k.xlo = (char*)g.xlo;
    k.tiles_m = pl.tiles_m; k.tiles_n = pl.tiles_n; k.nwg = pl.nwg; k.group_m = pl.group_m; k.epi_direct = pl.epi_direct;
    k.splits = pl.splits; k.kt_per_split = pl.kt_per_split; k.slab = (float*)g.slab; k.m_slab = g.M;
    if (gemm_kind_big_tile(pl.kind)) {
        if (pl.kind == GEMM_W2F8) { k.W8 = (const char*)g.W8; k.w8_scale = (const char*)g.w8_scale; TRY(ofx_gemm_launch_w2f8(&k, pl, s)); }
        else if (pl.kind == GEMM_X3) TRY(ofx_gemm_launch_x3(&k, pl, op_dtype, s));
        else if (pl.kind == GEMM_W2) TRY(ofx_gemm_launch_w2(&k, pl, op_dtype, s));
        else if (pl.kind == GEMM_PP) TRY(ofx_gemm_launch_pp(&k, pl, op_dtype, s));
        else TRY(ofx_gemm_launch_big(&k, pl, op_dtype, s));
        OFX_LAUNCH_CHECK();
        return OFX_OK;
    }
    // the 128x128 / 64x128 kernel (64-row tiles, three blocks per CU: grids that would leave CUs idle with 128-row tiles), with or without split-K
    static DeviceOnce attr_set;
    TRY(attr_set.run([]() -> int {
        OFX_HIP(hipFuncSetAttribute((const void*)gemm_128x128_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES));
        OFX_HIP(hipFuncSetAttribute((const void*)gemm_128x128_kernel<f16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES));
        OFX_HIP(hipFuncSetAttribute((const void*)gemm_128x128_kernel<bf16_t, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM64_LDS_BYTES));
        OFX_HIP(hipFuncSetAttribute((const void*)gemm_128x128_kernel<f16_t, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM64_LDS_BYTES));
        return OFX_OK;
    }));
    const dim3 grid(pl.grid_x, pl.grid_y);
    const bool one = pl.second_pass == GEMM_PASS_NONE || pl.second_pass == GEMM_PASS_DEFERRED;      // the launch that carries the profile record's stop event
    if (pl.tile_m == 64) {
        if (op_dtype == OFX_F16) OFX_PLAUNCH(one, (gemm_128x128_kernel<f16_t, 2>), grid, dim3(256), GEMM64_LDS_BYTES, s, k);
        else OFX_PLAUNCH(one, (gemm_128x128_kernel<bf16_t, 2>), grid, dim3(256), GEMM64_LDS_BYTES, s, k);
    } else if (op_dtype == OFX_F16) OFX_PLAUNCH(one, gemm_128x128_kernel<f16_t>, grid, dim3(256), GEMM_LDS_BYTES, s, k);
    else OFX_PLAUNCH(one, gemm_128x128_kernel<bf16_t>, grid, dim3(256), GEMM_LDS_BYTES, s, k);
    // second pass of a split-K plan: left to the consumer (defer_splits), fused with the following LayerNorm (ln_gamma), or the plain reduce
    if (pl.second_pass == GEMM_PASS_DEFERRED) *g.defer_splits = pl.splits;
    else if (pl.second_pass == GEMM_PASS_REDUCE_LN) {
        SplitKLnArgs a{(const float*)g.slab, (size_t)g.M * g.N, pl.splits, g.bias, g.resid, g.ldr, (float*)g.C, g.ldc,
                       g.ln_gamma, g.ln_beta, g.ln_out, g.ln_ld, g.ln_kind, g.ln_eps, g.M, g.N, g.m_dev};
        TRY(ofx_launch_splitk_reduce_ln(a, op_dtype, s, true));
        if (g.ln_done) *g.ln_done = true;
    } else if (pl.second_pass == GEMM_PASS_REDUCE) {
        if (op_dtype == OFX_F16) OFX_PLAUNCH(true, splitk_reduce_kernel<f16_t>, dim3(pl.reduce_grid), dim3(256), 0, s, k);
        else OFX_PLAUNCH(true, splitk_reduce_kernel<bf16_t>, dim3(pl.reduce_grid), dim3(256), 0, s, k);
    }
    OFX_LAUNCH_CHECK();
    return OFX_OK;
}
