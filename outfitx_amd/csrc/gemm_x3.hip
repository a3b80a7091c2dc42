// Three-product GEMM with every operand tile loaded ONCE: C = A_hi . W_hi^T + A_lo . W_hi^T + A_hi . W_lo^T.
//
// The K-concatenated form of the same sum ([hi | lo | hi] x [hi | hi | lo], K' = 3 K on a single-product kernel) stages A_hi and
// W_hi twice: 6 operand tiles per three products.  This kernel reads the SAME buffers - activation rows [hi | lo | hi] (lda = 3 K,
// the LayerNorm / epilogue split3 output), weight rows [hi | hi | lo] (ofx_launch_pack_rows mode 2) - but stages the four distinct
// tiles of a k-step once and runs the three products from registers: 48 KiB through LDS per 32-deep k-step of a 256 x 128 tile for
// 3 x 2.1 MFLOP = 131 FLOP per staged byte, against 64 (128 x 128 tiles) / 85 (256 x 128) for the K-concatenated GEMMs - and these loops
// run at the rate their LDS fill sustains.
//
// 256 x 128 tile, 8 waves as 4 x 2 of 64 x 64 wave tiles (64 accumulator VGPRs), BK = 32, three 48 KiB stages
// [A_hi 256 rows | A_lo 256 rows | W_hi 128 rows | W_lo 128 rows] x 64 B; per k-step and wave 6 LDS-DMA pieces (2 + 2 + 1 + 1), 16
// fragment reads and 48 MFMAs.  Schedule, swizzle and persistence: gemm_pingpong.h (counted-wait family) - step t + 2 issued in
// iteration t, counted vmcnt(6), the next tile's first two steps fetched under the epilogue; LDS-DMA through buffer resources
// (bload16 / make_rsrc, gemm_common.h: rows past M read zeros).
#include "gemm_common.h"

namespace {

template <typename T>
__global__ __launch_bounds__(512, 2) void gemm_x3_kernel(KArgs p) {
    typedef typename OpT<T>::v8 v8;
    constexpr int TM = 256, TN = 128, BK2 = 32, PA = TM * BK2 * 2, PW = TN * BK2 * 2, STAGE = 2 * PA + 2 * PW, NST = 3;      // 16 + 16 + 8 + 8 KiB
    extern __shared__ __attribute__((aligned(16))) char smem[];
    OFX_LDS char* lds = (OFX_LDS char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;            // 4 x 2 waves of 64 x 64; waves 0-3 (rows 0-127) are ping-pong group 0
    int grp = wave >> 2;
    asm volatile("" : "+s"(grp));
    const int Kl = p.K / 3;                             // logical depth; A rows are [hi | lo | hi] (3 Kl), W rows [hi | hi | lo]
    p.K = Kl;
    clamp_live_rows(p.m_dev, p.M);                      // device-side live row count: the launcher runs one block per tile then
    const int nk = Kl / BK2;
    const unsigned a_lo_off = (unsigned)Kl * 2, w_lo_off = (unsigned)Kl * 4;      // byte offsets of the lo column blocks in a row

    PpWalk<NST, TM, TN> w(p.nwg, p.group_m, p.tiles_m, p.tiles_n, nk);
    if (w.m0 >= p.M) return;
    for (;;) {
        const bool has_next = w.has_next();
        const int m0 = w.m0, n0 = w.n0;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const PpLane32 L(ln);
        unsigned a_off[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a_off[i] = ((unsigned)((wave * 2 + i) * 16 + L.prow) * p.lda + L.pchk * 8) * 2;
        const unsigned w_off = ((unsigned)(wave * 16 + L.prow) * (3 * Kl) + L.pchk * 8) * 2;
        const int a_frag = (wr * 64 + L.fr) * 64 + L.fchk;
        const int w_frag = 2 * PA + (wc * 64 + L.fr) * 64 + L.fchk;
        int m1, n1;
        w.next_origin(m1, n1);
        const size_t a_row = (size_t)p.lda * 2, w_row = (size_t)Kl * 6;
        const __amdgpu_buffer_rsrc_t r_a = make_rsrc(p.A + (size_t)m0 * a_row, (size_t)(p.M - m0) * a_row), r_w = make_rsrc(p.W + (size_t)n0 * w_row);
        const __amdgpu_buffer_rsrc_t r_a1 = make_rsrc(p.A + (size_t)m1 * a_row, (size_t)(p.M - m1) * a_row), r_w1 = make_rsrc(p.W + (size_t)n1 * w_row);
        // k-step x of the tile walk (x >= nk: step x - nk of the next tile): A_hi, A_lo (2 pieces each), W_hi, W_lo (1 each)
        auto issue_step = [&](int x) {
            OFX_LDS char* stg = lds + w.stage(x) * STAGE;
            const bool nx = x >= nk;
            const __amdgpu_buffer_rsrc_t ra = nx ? r_a1 : r_a, rw = nx ? r_w1 : r_w;
            const unsigned koff = (unsigned)(nx ? x - nk : x) * BK2 * 2;
            bload16(ra, a_off[0], koff, stg + wave * 2048); bload16(ra, a_off[1], koff, stg + wave * 2048 + 1024);
            bload16(ra, a_off[0], koff + a_lo_off, stg + PA + wave * 2048); bload16(ra, a_off[1], koff + a_lo_off, stg + PA + wave * 2048 + 1024);
            bload16(rw, w_off, koff, stg + 2 * PA + wave * 1024);
            bload16(rw, w_off, koff + w_lo_off, stg + 2 * PA + PW + wave * 1024);
        };

        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        v8 ah[4], al[4], wh[4], wl[4];

        auto read = [&](int step) {
            OFX_LDS char* stg = lds + w.stage(step) * STAGE;
#pragma unroll
            for (int j = 0; j < 4; ++j) { wh[j] = *(OFX_LDS v8*)(stg + w_frag + j * 1024); wl[j] = *(OFX_LDS v8*)(stg + PW + w_frag + j * 1024); }
#pragma unroll
            for (int i = 0; i < 4; ++i) { ah[i] = *(OFX_LDS v8*)(stg + a_frag + i * 1024); al[i] = *(OFX_LDS v8*)(stg + PA + a_frag + i * 1024); }
        };
        // 48 MFMAs: per (activation fragment, weight fragment) hi.hi, lo.hi, hi.lo
        auto mfma = [&]() {
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[i][j] = OpT<T>::mfma16(wh[j], ah[i], acc[i][j]);
                    acc[i][j] = OpT<T>::mfma16(wh[j], al[i], acc[i][j]);
                    acc[i][j] = OpT<T>::mfma16(wl[j], ah[i], acc[i][j]);
                }
            __builtin_amdgcn_s_setprio(0);
        };
        if (w.first) {
            issue_step(0); issue_step(1);
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");        // step 0 landed (my pieces)
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // steps 0 and 1 (fetched under the previous epilogue) and that epilogue's stores
        }
        __builtin_amdgcn_s_barrier();                               // ---- end of slot 0
        // iteration t: issue step t + 2, read and multiply step t; the wait leaves the 6 pieces of step t + 2 in flight
        auto run = [&](auto G) {
            pp_group_begin<G.value>();
            int t = 0;
            do {
                pp_slot<G.value, 6>([&] { issue_step(t + 2); }, [&] { read(t); }, mfma);
            } while (++t < nk);
            pp_group_end<G.value>();
        };
        if (grp == 0) run(std::integral_constant<int, 0>());
        else run(std::integral_constant<int, 1>());
        // Epilogue staging: the stage of this tile's LAST step (8 x 4 KiB + the LayerNorm-fold statistics slots behind them); the fills of
        // steps nk, nk + 1 (the next tile's first steps, still landing) target the other two stages.
        OFX_LDS char* estage = lds + w.epilogue_stage() * STAGE;
        OFX_LDS char* ep = estage + wave * EPI2_BYTES_PER_WAVE;
        OFX_LDS float* st = nullptr;
        if (p.row_stat && p.out_kind != 0) st = (OFX_LDS float*)(estage + 8 * EPI2_BYTES_PER_WAVE + wave * 1024);
        epilogue2_dispatch<T, 4, 4, 0>(p, ep, acc, m0 + wr * 64, n0 + wc * 64, ln, st);
        if (!has_next) break;
        w.advance();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // the last tile's redundant fills have landed before the wave ends
}

template <typename T>
static int launch_x3(const KArgs& k, const GemmPlan& plan, hipStream_t s) {
    constexpr int LDSB = 3 * (2 * 256 + 2 * 128) * 32 * 2;          // 144 KiB
    static DeviceOnce attr;
    TRY(set_max_dynamic_lds(attr, gemm_x3_kernel<T>, LDSB));
    OFX_PLAUNCH(true, (gemm_x3_kernel<T>), dim3(plan.grid_x), dim3(512), LDSB, s, k);
    return OFX_OK;
}

}  // namespace

int ofx_gemm_launch_x3(void* kargs, const GemmPlan& plan, int op_dtype, hipStream_t s) {
    const KArgs& k = *(const KArgs*)kargs;
    return op_dtype == OFX_F16 ? launch_x3<f16_t>(k, plan, s) : launch_x3<bf16_t>(k, plan, s);
}
