// Dual-weight ("W2") 256x256 tile kernel: C = A . (W_hi + W_lo)^T with ONE copy of A.
//
// The weight matrix is stored split, row n = [hi(K) | lo(K)] (hi = round(w), lo = round(w - hi), both in the operand type), so
// the product keeps ~22 significant weight bits (f16: about 18 at |w| ~ 0.02, where the lo half is subnormal with an absolute step of
// 2^-24; bf16: 16) at two MFMAs per (A fragment, column tile) while the activation tile is loaded
// and its fragments are read ONCE: per 32-deep k-step and wave 8 A + 4 W_hi + 4 W_lo fragment reads feed 64 MFMAs (the
// single-product kernels read 12 fragments per 32 MFMAs), so the loop is bound by the matrix pipe, not by the LDS port.
// Used for the CLIP GEMMs whose weight rounding dominates the end-to-end error (fc2, out-proj, patch embedding: DESIGN.md §2).
//
// Structure: the counted-wait ping-pong of gemm_pingpong.h at BK = 32 with three 48 KiB stages [A 256 rows | W_hi 256 rows | W_lo 256
// rows] x 64 B, persistent over tiles (one block per CU; ofx_tune(11, 0) = one block per tile).  Per step and wave 6 LDS-DMA pieces
// (counted vmcnt(6): the youngest step stays in flight), 16 fragment reads, 64 MFMAs; iteration t issues step t + 2, so the fills of
// steps nk and nk + 1 fetch the next tile's first two steps under the current epilogue (see the kernel body).
#include "gemm_common.h"

namespace {

template <typename T>
__global__ __launch_bounds__(512, 2) void gemm_w2_kernel(KArgs p) {
    typedef typename OpT<T>::v8 v8;
    constexpr int TM = 256, TN = 256, BK2 = 32, PART = TM * BK2 * 2, STAGE = 3 * PART, NST = 3;      // 16 KiB per operand, 48 KiB per stage
    extern __shared__ __attribute__((aligned(16))) char smem[];
    OFX_LDS char* lds = (OFX_LDS char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int Kh = p.K >> 1;                           // logical K; 2 Kh is the row stride of W = [hi | lo]
    p.K = Kh;                                          // the epilogues never read K; keep the logical value anyway
    clamp_live_rows(p.m_dev, p.M);                     // device-side live row count: the launcher runs one block per tile then

    const unsigned lo_bytes = (unsigned)Kh * 2;
    const int nk = Kh / BK2;
    const int dst0 = wave * 2 * 1024;

    PpWalk<NST, TM, TN> w(p.nwg, p.group_m, p.tiles_m, p.tiles_n, nk);
    if (w.m0 >= p.M) return;                            // only with m_dev (one block per tile)
    for (;;) {
        const bool has_next = w.has_next();             // its first two steps are fetched by this tile's last two fills
        const int m0 = w.m0, n0 = w.n0;
        // Lane constants are re-derived per tile from an opaque copy of the lane id: kept live across the epilogue they cost more
        // registers than the kernel has (spills), recomputing them costs a few dozen VALU operations per ~50 us tile.
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const PpLane32 L(ln);
        const int prow = L.prow, pchk = L.pchk;
        unsigned w_off[2];                                  // tile-independent
#pragma unroll
        for (int i = 0; i < 2; ++i) w_off[i] = ((unsigned)((wave * 2 + i) * 16 + prow) * (2 * Kh) + pchk * 8) * 2;
        auto a_offset = [&](int mt, int i) {                // rows past M re-read the last live row
            const int row = (wave * 2 + i) * 16 + prow;
            const int rr = mt + row < p.M ? row : p.M - 1 - mt;
            return ((unsigned)rr * p.lda + pchk * 8) * 2;
        };
        const int a_frag = (wr * 128 + L.fr) * 64 + L.fchk;
        const int w_frag = PART + (wc * 64 + L.fr) * 64 + L.fchk;
        const char* a_base = p.A + (size_t)m0 * p.lda * 2;
        const char* w_base = p.W + (size_t)n0 * (2 * Kh) * 2;
        unsigned a_off[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a_off[i] = a_offset(m0, i);

#define OFX_W2_PIECE(Q, AK, A0, A1, WK, BASE)                                                          \
    {                                                                                                  \
        if ((Q) < 2) glds16((AK) + ((Q) ? (A1) : (A0)), (BASE) + dst0 + (Q) * 1024);                    \
        else if ((Q) < 4) glds16((WK) + w_off[(Q) - 2], (BASE) + PART + dst0 + ((Q) - 2) * 1024);       \
        else glds16((WK) + lo_bytes + w_off[(Q) - 4], (BASE) + 2 * PART + dst0 + ((Q) - 4) * 1024);     \
    }
        auto issue_cur = [&](int step) {                // a step of the current tile (step < nk)
            OFX_LDS char* sbase = lds + w.stage(step) * STAGE;
            const char* ak = a_base + (size_t)step * BK2 * 2;
            const char* wk = w_base + (size_t)step * BK2 * 2;
#pragma unroll
            for (int q = 0; q < 6; ++q) OFX_W2_PIECE(q, ak, a_off[0], a_off[1], wk, sbase)
        };
        auto issue_next = [&](int j) {                  // step nk + j: the next tile's step j, in the stage of this tile's step nk + j - 3
            OFX_LDS char* sbase = lds + w.stage(nk + j) * STAGE;
            if (has_next) {
                int m1, n1;
                w.next_origin(m1, n1);
                const char* ak = p.A + (size_t)m1 * p.lda * 2 + (size_t)j * BK2 * 2;
                const char* wk = p.W + (size_t)n1 * (2 * Kh) * 2 + (size_t)j * BK2 * 2;
                const unsigned n0_ = a_offset(m1, 0), n1_ = a_offset(m1, 1);
#pragma unroll
                for (int q = 0; q < 6; ++q) OFX_W2_PIECE(q, ak, n0_, n1_, wk, sbase)
            } else {                                    // the block's last tile: a redundant re-fill with the last step (keeps the counted waits uniform; nobody reads it)
                const char* ak = a_base + (size_t)(nk - 1) * BK2 * 2;
                const char* wk = w_base + (size_t)(nk - 1) * BK2 * 2;
#pragma unroll
                for (int q = 0; q < 6; ++q) OFX_W2_PIECE(q, ak, a_off[0], a_off[1], wk, sbase)
            }
        };

        f32x4 acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        v8 af[8], wh[4], wl[4];

        auto read = [&](int step) { pp_w2_read<4>(lds + w.stage(step) * STAGE, a_frag, w_frag, PART, af, wh, wl); };
        auto mfma = [&] { pp_w2_mfma<T, 4>(acc, af, wh, wl); };

        if (w.first) {
            issue_cur(0); issue_cur(1);
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");        // step 0 landed (my pieces)
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // steps 0 and 1 (fetched under the previous epilogue) and that epilogue's stores
        }
        __builtin_amdgcn_s_barrier();                               // ---- end of slot 0
        // Iteration t refills the stage of step t-1 (both groups have read it) with step t+2; the last two iterations of a tile are
        // peeled so that the steady-state body carries no next-tile logic.  (The two groups are written out: one generic lambda over the
        // group, as gemm_x3 has it, laid the peeled fills out once more here.)
        if (wr == 0) {
            for (int t = 0; t < nk - 2; ++t) pp_slot<0, 6>([&] { issue_cur(t + 2); }, [&] { read(t); }, mfma);
            pp_slot<0, 6>([&] { issue_next(0); }, [&] { read(nk - 2); }, mfma);
            pp_slot<0, 6>([&] { issue_next(1); }, [&] { read(nk - 1); }, mfma);
            pp_group_end<0>();
        } else {
            pp_group_begin<1>();
            for (int t = 0; t < nk - 2; ++t) pp_slot<1, 6>([&] { issue_cur(t + 2); }, [&] { read(t); }, mfma);
            pp_slot<1, 6>([&] { issue_next(0); }, [&] { read(nk - 2); }, mfma);
            pp_slot<1, 6>([&] { issue_next(1); }, [&] { read(nk - 1); }, mfma);
        }
#undef OFX_W2_PIECE
        // Epilogue staging: the stage of this tile's LAST step - read by everybody before the barriers above, and the one stage
        // the fills of steps nk, nk + 1 (the next tile's first steps, still landing) do not target.
        OFX_LDS char* estage = lds + w.epilogue_stage() * STAGE;
        OFX_LDS char* ep = estage + wave * EPI2_BYTES_PER_WAVE;
        const int gm0 = m0 + wr * 128, gn0 = n0 + wc * 64;
        OFX_LDS float* st = nullptr;
        if (p.row_stat && p.out_kind != 0) st = (OFX_LDS float*)(estage + 8 * EPI2_BYTES_PER_WAVE + wave * 1024);
        epilogue2_dispatch<T>(p, ep, acc, gm0, gn0, ln, st);
        if (!has_next) break;
        w.advance();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // the last tile's redundant fills have landed before the wave ends
}

template <typename T>
static int launch_w2(const KArgs& k, const GemmPlan& plan, hipStream_t s) {
    constexpr int LDSB = 3 * 3 * 256 * 32 * 2;          // 144 KiB
    static DeviceOnce attr;
    TRY(set_max_dynamic_lds(attr, gemm_w2_kernel<T>, LDSB));
    OFX_PLAUNCH(true, (gemm_w2_kernel<T>), dim3(plan.grid_x), dim3(512), LDSB, s, k);
    return OFX_OK;
}

}  // namespace

int ofx_gemm_launch_w2(void* kargs, const GemmPlan& plan, int op_dtype, hipStream_t s) {
    const KArgs& k = *(const KArgs*)kargs;
    return op_dtype == OFX_F16 ? launch_w2<f16_t>(k, plan, s) : launch_w2<bf16_t>(k, plan, s);
}
