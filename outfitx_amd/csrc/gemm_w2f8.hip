// Split-weight 256x256 tile kernel with the weight-correction product on the block-scaled fp8 matrix instruction:
//
//     C = A . W_hi^T  (f16 x f16, v_mfma_f32_16x16x32_f16)  +  fp8(A) . fp8(W_lo)^T  (v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 x e5m2)
//
// W = W_hi + W_lo with W_hi = f16(W) as in gemm_w2.hip.  The correction term A . W_lo^T is 2^-11 of the product, so 4 significant
// bits of each of its operands keep the result at ~2^-15 - below the activation rounding the scheme leaves anyway (DESIGN.md section 2,
// tests/studies/fp8_correction_cpu.py) - and the fp8 instruction runs at twice the f16 rate: per 128-deep super-step and wave
// 4 x 32 f16 MFMAs (16 cycles each) + 32 fp8 MFMAs (32 cycles each) = 3,072 matrix-pipe cycles against gemm_w2's 4,096.
//
// What makes it fit (tools/mx_probe.hip pins the instruction semantics used here):
//   * the fp8 copy of the ACTIVATIONS never exists in memory: each wave converts the f16 A fragments it has just read for the f16
//     product (2 elements per instruction) and keeps them for the four k-steps of a super-step: fragment i's 8 VGPRs collect bytes
//     8 s + j <- k = 32 s + 8 g + j (s = k-step, g = lane >> 4) - a k-permutation inside the 128-block, harmless because the packed
//     fp8 weights carry the same one (ofx_launch_pack_lo8);
//   * round 4: the activation image is E5M2 (v_cvt_scalef32_pk_bf8_f16, the instruction's second operand read as bf8: blgp = 1), not
//     E4M3.  e5m2 has f16's exponent field, so the image follows WHATEVER the f16 operand holds - massive residual-stream channels in
//     the hundreds (trained CLIP ViTs have them, and with LayerNorm folding the raw stream is the A operand of qkv and fc1), values
//     down to f16's subnormals - at 3 significant bits, with no scale to choose and nothing that saturates below 57,344 (MODE.
//     FP16_OVFL = 1 clamps the f16 values above that instead of producing infinities).  The e4m3 image of rounds 3 (4 significant
//     bits, x4 scale) saturated at |a| > 112 and then corrected only part of such a channel.  Price: the activation side of the
//     2^-11 correction term is kept to 2^-4 instead of 2^-5 relative - still far below the f16 rounding of the main product
//     (tests/studies/fp8_correction_cpu.py); same instruction rate (tools/mfma_power_probe.hip).
//   * the wave tile is 64 x 128 (8 waves as 4 x 2), so only 4 activation fragments = 32 VGPRs are held; the 8 weight fragments of the
//     fp8 step stream through a 3-deep register ring loaded two fragments ahead of their use (128 accumulators + 32 + 24, in the
//     registers the f16 fragments have just left);
//   * per-row weight scales (E8M0, max |lo| 2^sw in [128, 256)) ride in as the instruction's per-lane scale operand, the activation
//     scale (2^0: the e5m2 image needs none) as the other one.
//
// Structure: the counted-wait ping-pong of gemm_pingpong.h (two wave groups one barrier slot apart, BK = 32, persistent over tiles) with FOUR
// 32 KiB stages [A | W_hi] and ONE 32 KiB buffer for the current super-step's fp8 weights (160 KiB in all).  The kernels of this
// family take time in proportion to the bytes they stage through LDS (~16-20 B/clk/CU: gemm_w2 with 48 KiB per k-step, this kernel
// with 40 KiB, the single-product kernels with 32 KiB; DESIGN.md section 3.1: the fill itself needs that long, and every LDS-DMA
// instruction costs the SIMD's multiplying wave ~65 cycles of issue), so what matters is that the fill never idles:
// the MFMA slot that carries a super-step's fp8 product is three times as long as the others, and the read slot of the partner group
// that runs beside it issues TWO k-steps of LDS-DMA (the fourth stage makes room: an iteration t may fill steps t + 2 and t + 3):
//   group 0:  R0: steps t+2, t+3 (beside group 1's fp8 slot)   R1: the super-step's 4 fp8 quarters   R2: t+2   R3: t+2
//   group 1:  R0: t+3   R1: the 4 fp8 quarters   R2: t+2   R3: t+2, t+3 (beside group 0's fp8 slot)
// i.e. 8 KiB per wave beside a long slot and 4 KiB beside a short one.
// The fp8 buffer is refilled after both groups' fp8 slots of the previous super-step and complete (waited for + a barrier) before
// the next ones; the counted wait of an iteration leaves exactly the pieces that iteration issued in flight.
//   LDS image of the fp8 buffer: row n (256) x 128 B; 16-byte chunk c of row r at slot c ^ x(r & 15),
//   x(c) = (((c >> 1) & 3) << 1) | (c >> 3): conflict-free for ds_read_b128's lane groups with 128-byte rows (each lane reads the two
//   chunks 2 g, 2 g + 1 of row lane & 15).
// Epilogue staging: the stage of the tile's last k-step (8 x 4 KiB; the other three hold the next tile's first steps); the
// waves' slots of epilogue constants (8 x 2 KiB: row statistics, bias, column sums) sit in the fp8 buffer, which is idle between the
// tile's last fp8 slot and the next tile's refill.
#include "gemm_common.h"

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(512, 2) void gemm_w2f8_kernel(KArgs p) {
    typedef f16_t T;
    typedef OpT<T>::v8 v8;
    constexpr int TM = 256, TN = 256, BK2 = 32, PART = TM * BK2 * 2, STAGE = 2 * PART, NST = 4;      // 16 KiB per operand, 32 KiB per stage
    constexpr int W8BASE = NST * STAGE;                                                                 // 32 KiB behind the stages
    extern __shared__ __attribute__((aligned(16))) char smem[];
    OFX_LDS char* lds = (OFX_LDS char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;           // 4 x 2 waves of 64 x 128; waves 0-3 (rows 0-127) are ping-pong group 0
    int grp = wave >> 2;
    asm volatile("" : "+s"(grp));            // an opaque scalar: re-deriving it from threadIdx.x later costs a scratch reload, which drains the DMA queue
    const int Kh = p.K >> 1;                           // logical K; 2 Kh is the row stride (elements) of W = [hi | lo]
    p.K = Kh;
    clamp_live_rows(p.m_dev, p.M);
    const int nk = Kh / BK2, nsup = nk >> 2;
    const int dst0 = wave * 2 * 1024;
    const float a_scale = 1.0f;                        // the e5m2 activation image: f16's exponent range, unscaled (E8M0 byte 127 = 2^0)
    const int a_e8 = 127;

    PpWalk<NST, TM, TN> w(p.nwg, p.group_m, p.tiles_m, p.tiles_n, nk);
    if (w.m0 >= p.M) return;
    bool full_prev = false;
    // per-row E8M0 scale bytes of this wave's 128 columns: 8 bytes per lane (fragment j -> byte j); the NEXT tile's are requested before
    // the epilogue, so that their latency is not paid at the top of every tile
    unsigned long long sc8 = *(const unsigned long long*)(p.w8_scale + ((size_t)((w.n0 >> 7) + wc) * 16 + (lane & 15)) * 8);
    for (;;) {
        const bool has_next = w.has_next();
        const int m0 = w.m0, n0 = w.n0;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        // f16 pieces: 16 rows x 64 B; lane l -> row l >> 2, physical slot l & 3 <- logical chunk (l & 3) ^ f(row >> 2) - the kernel's own
        // copy of PpLane32 (gemm_pingpong.h): built through the struct it takes 244 VGPRs instead of 242
        const int prow = ln >> 2, pchk = (ln & 3) ^ ((4 - (ln >> 4)) & 3);
        unsigned w_off[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) w_off[i] = ((unsigned)((wave * 2 + i) * 16 + prow) * (2 * Kh) + pchk * 8) * 2;
        // fp8 piece q: 8 rows x 128 B, rows (wave * 4 + q) * 8 + (l >> 3); physical chunk l & 7 <- logical (l & 7) ^ x(row & 15),
        // row & 15 = (q & 1) * 8 + (l >> 3)  =>  x = (((l >> 4) & 3) << 1) | (q & 1)
        const unsigned w8_off = (unsigned)(wave * 32 + (ln >> 3)) * Kh + (((ln & 7) ^ (((ln >> 4) & 3) << 1)) << 4);
        const int fr = ln & 15, fq = ln >> 4;
        const int fchk = (fq ^ ((4 - (fr >> 2)) & 3)) * 16;
        const int a_frag = (wr * 64 + fr) * 64 + fchk;
        const int w_frag = PART + (wc * 128 + fr) * 64 + fchk;
        // fp8 weight fragment j: row wc * 128 + j * 16 + fr, logical chunks 2 fq, 2 fq + 1
        const int x8 = (((fr >> 1) & 3) << 1) | (fr >> 3);
        const int w8_frag0 = (wc * 128 + fr) * 128 + (((2 * fq) ^ x8) << 4), w8_frag1 = (wc * 128 + fr) * 128 + (((2 * fq + 1) ^ x8) << 4);
        const char* a_base = p.A + (size_t)m0 * p.lda * 2;
        const char* w_base = p.W + (size_t)n0 * (2 * Kh) * 2;
        const char* w8_base = p.W8 + (size_t)n0 * Kh;
        unsigned a_off[2];                                  // tile-independent too: rows past M read zeros through the sized resource
#pragma unroll
        for (int i = 0; i < 2; ++i) a_off[i] = ((unsigned)((wave * 2 + i) * 16 + prow) * p.lda + pchk * 8) * 2;
        int m1, n1;
        w.next_origin(m1, n1);
        int sc_lo = (int)(unsigned)sc8, sc_hi = (int)(unsigned)(sc8 >> 32);
        // The epilogue's constants of this wave's 64 x 128 sub-tile, requested HERE: lane l takes row l's (mean, rstd), lanes 0-31 four biases
        // each, lanes 32-63 four column sums each (six registers).  A load at the epilogue's own top is waited for with everything older in
        // the vector-memory queue - the next tile's first k-steps of LDS-DMA, issued just before - and one per 64-column half also with the
        // stores of the half before.  From inline assembly, so that the compiler plants no vmcnt(0) of its own where the values are used: in
        // issue order they are older than every piece of iteration 0, whose counted wait (the first tile: the wait below) retires them.
        f32x2 ep_ms = {0.f, 1.f};
        f32x4 ep_c4 = {0.f, 0.f, 0.f, 0.f};
        {
            const float* sp = p.row_stat + 2 * (size_t)min(m0 + wr * 64 + ln, p.M - 1) * p.stat_ld;
            if (p.row_stat) asm volatile("global_load_dwordx2 %0, %1, off" : "+v"(ep_ms) : "v"(sp) : "memory");
            const float* cb = p.row_stat && ln >= 32 ? p.col_sum : p.bias;
            const float* cp = cb + n0 + wc * 128 + (ln & 31) * 4;
            if (cb) asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(ep_c4) : "v"(cp) : "memory");
        }

        // LDS-DMA pieces: the two A and two W_hi pieces of a k-step (KOFF = its byte offset in the k-contiguous rows) and quarter Q of
        // this wave's rows of super-step SUP's fp8 weights
#define OFX_F8_ISSUE_AW(RA, RW, A0, A1, KOFF, STG)                                                                         \
    {                                                                                                                      \
        bload16(RA, A0, KOFF, (STG) + dst0); bload16(RA, A1, KOFF, (STG) + dst0 + 1024);                                    \
        bload16(RW, w_off[0], KOFF, (STG) + PART + dst0); bload16(RW, w_off[1], KOFF, (STG) + PART + dst0 + 1024);          \
    }
#define OFX_F8_ISSUE_W8(SUP, Q)                                                                                            \
    bload16(r_w8, w8_off ^ (((Q) & 1) << 4), (unsigned)(SUP) * 128u + (unsigned)(Q) * 8u * (unsigned)Kh, lds + W8BASE + (wave * 4 + (Q)) * 1024);
        const size_t a_row = (size_t)p.lda * 2;
        const __amdgpu_buffer_rsrc_t r_a = make_rsrc(a_base, (size_t)(p.M - m0) * a_row), r_w = make_rsrc(w_base), r_w8 = make_rsrc(w8_base);
        const __amdgpu_buffer_rsrc_t r_a1 = make_rsrc(p.A + (size_t)m1 * a_row, (size_t)(p.M - m1) * a_row), r_w1 = make_rsrc(p.W + (size_t)n1 * (2 * Kh) * 2);
        // k-step x of the tile walk: a step of this tile, or (x >= nk) step x - nk of the next one - a scalar select of resource and offset
        auto issue_step = [&](int x) {
            OFX_LDS char* stg = lds + w.stage(x) * STAGE;
            const bool nx = x >= nk;
            const __amdgpu_buffer_rsrc_t ra = nx ? r_a1 : r_a, rw = nx ? r_w1 : r_w;
            OFX_F8_ISSUE_AW(ra, rw, a_off[0], a_off[1], (unsigned)(nx ? x - nk : x) * BK2 * 2, stg)
        };

        f32x4 acc[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        v8 af[4], wh[8];
        i32x8 a8[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a8[i] = i32x8{0, 0, 0, 0, 0, 0, 0, 0};

        auto read = [&](int step) {
            OFX_LDS char* stg = lds + w.stage(step) * STAGE;
#pragma unroll
            for (int j = 0; j < 8; ++j) wh[j] = *(OFX_LDS v8*)(stg + w_frag + j * 16 * 64);
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *(OFX_LDS v8*)(stg + a_frag + i * 16 * 64);
        };
        // 32 f16 MFMAs + the conversion of the four A fragments into bytes 8 S .. 8 S + 7 of their fp8 images (S = step & 3, static)
#define OFX_F8_CVT1(I, S)                                                                                      \
    {                                                                                                         \
        i16x2 lo_ = __builtin_bit_cast(i16x2, a8[I][2 * (S)]), hi_ = __builtin_bit_cast(i16x2, a8[I][2 * (S) + 1]); \
        lo_ = __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(lo_, f16x2{af[I][0], af[I][1]}, a_scale, false);       \
        lo_ = __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(lo_, f16x2{af[I][2], af[I][3]}, a_scale, true);        \
        hi_ = __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(hi_, f16x2{af[I][4], af[I][5]}, a_scale, false);       \
        hi_ = __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(hi_, f16x2{af[I][6], af[I][7]}, a_scale, true);        \
        a8[I][2 * (S)] = __builtin_bit_cast(int, lo_); a8[I][2 * (S) + 1] = __builtin_bit_cast(int, hi_);      \
    }
// f16 MFMA order: the weight fragment (the instruction's FIRST operand) stays over 4 consecutive MFMAs while the activation fragment cycles.
// Bit-identical to the activation-outer order (every accumulator sees the same sequence); 242 VGPRs and no scratch instead of 256 + 16 B; in
// back-to-back launches qkv 560 -> 536 us, fc1 760 -> 740 (the part is power-limited and a changing first operand costs more:
// tools/mfma_power_probe.hip), level in the step.
#define OFX_F8_MFMA16(S)                                                                                      \
    {                                                                                                         \
        __builtin_amdgcn_s_setprio(1);                                                                        \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                       \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) acc[i][j] = OpT<T>::mfma16(wh[j], af[i], acc[i][j]); \
            if (j & 1) OFX_F8_CVT1(j >> 1, S)                                                                 \
        }                                                                                                     \
        __builtin_amdgcn_s_setprio(0);                                                                        \
    }
        // the super-step's 32 fp8 MFMAs: weight fragment j (two 16-byte reads per lane) against the four activation images; the
        // fragments go through a 3-deep register ring (24 VGPRs: two in flight beside the one being multiplied); the scale-byte
        // selector of the instruction is an immediate, hence one expansion per fragment
#define OFX_F8_LD(J)                                                                                           \
    {                                                                                                         \
        const i32x4 c0_ = *(OFX_LDS i32x4*)(b8_ + w8_frag0 + (J) * 16 * 128), c1_ = *(OFX_LDS i32x4*)(b8_ + w8_frag1 + (J) * 16 * 128); \
        w8_[(J) % 3] = i32x8{c0_[0], c0_[1], c0_[2], c0_[3], c1_[0], c1_[1], c1_[2], c1_[3]};                 \
    }
#define OFX_F8_MF(J, SEL, SC)                                                                                 \
    if ((J) + 2 < 8) { OFX_F8_LD((J) + 2) __builtin_amdgcn_sched_barrier(0); }     /* keep the load two fragments ahead of its use */ \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                             \
        acc[i][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w8_[(J) % 3], a8[i], acc[i][J], 0, 1, SEL, SC, 0, a_e8);
#define OFX_F8_MFMA8()                                                                                        \
    {                                                                                                         \
        __builtin_amdgcn_sched_barrier(0);      /* the fp8 fragments take the registers the f16 fragments leave: no hoisting above */ \
        OFX_LDS char* b8_ = lds + W8BASE;                                                                     \
        i32x8 w8_[3];                                                                                         \
        OFX_F8_LD(0) OFX_F8_LD(1)                                                                             \
        __builtin_amdgcn_s_setprio(1);                                                                        \
        OFX_F8_MF(0, 0, sc_lo) OFX_F8_MF(1, 1, sc_lo) OFX_F8_MF(2, 2, sc_lo) OFX_F8_MF(3, 3, sc_lo)           \
        OFX_F8_MF(4, 0, sc_hi) OFX_F8_MF(5, 1, sc_hi) OFX_F8_MF(6, 2, sc_hi) OFX_F8_MF(7, 3, sc_hi)           \
        __builtin_amdgcn_s_setprio(0);                                                                        \
    }

        if (w.first) {                                                // group 1 runs one step further ahead (see the schedule below)
            issue_step(0); issue_step(1);
            if (grp == 0) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");        // step 0 landed (my pieces)
            else { issue_step(2); asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); }
        } else if (full_prev) {
            // the next tile's first steps were issued BEFORE the previous epilogue, whose every variant issues at least 16 vector-memory
            // operations per wave on a full tile (two or more 16-byte stores per 16-row pass, 8 passes; + the scale-byte load): all but the
            // 16 youngest done = those steps have landed, while the stores drain under this tile's first slots (the counted waits of
            // iteration 0 retire them in order)
            asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // a ragged previous tile skipped stores: wait for everything
        }
        asm volatile("" : "+v"(sc_lo), "+v"(sc_hi));                  // the scale load is waited for HERE, not inside the counted-vmcnt loop
        asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1");     // MODE.FP16_OVFL: the f16 -> fp8 conversion clamps at the format's largest finite value (e5m2: 57,344; e4m3: 448) instead of inf / NaN
        __builtin_amdgcn_s_barrier();                               // ---- end of slot 0
        // One iteration of a group = pp_slot (gemm_pingpong.h); NV = the LDS-DMA pieces the iteration issues: its counted wait leaves
        // exactly those in flight (everything issued by earlier iterations has landed: an iteration t fills steps t + 2 / t + 3, read
        // from iteration t + 2 on, and the fp8 quarters are read two iterations later at the earliest).  The fp8 product of a
        // super-step runs at the end of the MFMA slot of its fourth k-step.
        auto run = [&](auto G) {
            constexpr int g = G.value;
            pp_group_begin<g>();
            int u = 0;
            do {                                                    // nsup >= 1: no trip-count guard (its flag ended up spilled, and a scratch reload drains the DMA queue)
                const int t = 4 * u;
                pp_slot<g, g ? 4 : 8>([&] { if (g == 0) issue_step(t + 2); issue_step(t + 3); }, [&] { read(t); }, [&] { OFX_F8_MFMA16(0) });
                pp_slot<g, 4>([&] { OFX_F8_ISSUE_W8(u, 0) OFX_F8_ISSUE_W8(u, 1) OFX_F8_ISSUE_W8(u, 2) OFX_F8_ISSUE_W8(u, 3) }, [&] { read(t + 1); }, [&] { OFX_F8_MFMA16(1) });
                pp_slot<g, 4>([&] { issue_step(t + 4); }, [&] { read(t + 2); }, [&] { OFX_F8_MFMA16(2) });
                pp_slot<g, g ? 8 : 4>([&] { issue_step(t + 5); if (g == 1) issue_step(t + 6); }, [&] { read(t + 3); }, [&] { OFX_F8_MFMA16(3) }, [&] { OFX_F8_MFMA8() });
            } while (++u < nsup);
            pp_group_end<g>();
        };
        if (grp == 0) run(std::integral_constant<int, 0>());
        else run(std::integral_constant<int, 1>());
#undef OFX_F8_MFMA16
#undef OFX_F8_MFMA8
#undef OFX_F8_MF
#undef OFX_F8_LD
#undef OFX_F8_CVT1
#undef OFX_F8_ISSUE_AW
#undef OFX_F8_ISSUE_W8
        asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 0");     // the epilogue's f32 -> f16 casts keep the default overflow behaviour
        // Epilogue staging: the stage of this tile's LAST k-step (every read of it is over, no fill targets it); the slots of epilogue
        // constants: the fp8 buffer (idle until the next tile's first iterations refill it, behind the barrier of its slot 0).
        OFX_LDS char* estage = lds + w.epilogue_stage() * STAGE;
        OFX_LDS char* ep = estage + wave * EPI2_BYTES_PER_WAVE;
        const int gm0 = m0 + wr * 64, gn0 = n0 + wc * 128;
        OFX_LDS float* cst = (OFX_LDS float*)(lds + W8BASE + wave * EPI_CONST_BYTES_PER_WAVE);
        *(OFX_LDS f32x2*)(cst + 2 * ln) = ep_ms;                       // row ln
        *(OFX_LDS f32x4*)(cst + EPI_CONST_BIAS + 4 * ln) = ep_c4;      // lanes 32-63 land at EPI_CONST_CSUM + 4 (ln - 32)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        sc8 = *(const unsigned long long*)(p.w8_scale + ((size_t)((n1 >> 7) + wc) * 16 + (ln & 15)) * 8);     // the next tile's scale bytes (this tile's own again on the last one)
        OFX_LDS float* st = (p.row_stat && p.out_kind != 0) ? cst : nullptr;
        if (!epilogue_direct_dispatch<T, 4, 8>(p, acc, gm0, gn0, ln, cst)) {
            epilogue2_dispatch<T, 4, 8, 0>(p, ep, acc, gm0, gn0, ln, st, cst);
            epilogue2_dispatch<T, 4, 8, 4>(p, ep, acc, gm0, gn0 + 64, ln, st, cst);
        }
        if (!has_next) break;
        full_prev = m0 + TM <= p.M;
        w.advance();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // the last tile's redundant fills have landed before the wave ends
}

// fp8 copy of the lo half of split-weight rows: src row n = [hi(K) | lo(K)] in f16 (row stride 2 K); dst row n = K bytes, e4m3 of
// lo 2^sw(n) with max |lo| 2^sw in [128, 256), the 128-blocks k-permuted (byte 32 g + 8 s + j <- k = 32 s + 8 g + j); scale byte
// 127 - sw(n) at scale[((n >> 7) * 16 + (n & 15)) * 8 + ((n >> 4) & 7)].  One wave per row.
__global__ __launch_bounds__(256) void pack_lo8_kernel(const f16_t* src, unsigned char* dst, unsigned char* scale, int N, int K) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    const f16_t* lo = src + (size_t)n * 2 * K + K;
    float mx = 0.f;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, fabsf((float)lo[k]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    int sw = 0;
    if (mx > 0.f) { int e; (void)frexpf(mx, &e); sw = 8 - e; }          // mx = m 2^e, m in [0.5, 1): mx 2^(8 - e) in [128, 256)
    sw = sw > 127 ? 127 : (sw < -127 ? -127 : sw);
    const float mul = ldexpf(1.0f, sw);
    for (int p = lane; p < K; p += 64) {
        const int blk = p >> 7, q = p & 127, g = q >> 5, s_ = (q >> 3) & 3, j = q & 7;
        const float v = (float)lo[blk * 128 + 32 * s_ + 8 * g + j] * mul;
        // e4m3 (OCP, round to nearest even) of |v| <= 256 by hand: exact for the values above, no dependence on library conversions
        const float a = fabsf(v);
        unsigned char b = 0;
        if (a > 0.f) {
            int e; const float m = frexpf(a, &e);                      // a = m 2^e, m in [0.5, 1)
            int E = e - 1 + 7;                                          // biased exponent of 1.xxx 2^(e - 1)
            if (E >= 1) {
                int q3 = (int)rintf((m * 2.0f - 1.0f) * 8.0f);         // 3 mantissa bits, ties to even
                if (q3 == 8) { q3 = 0; ++E; }
                b = (unsigned char)((E << 3) | q3);
            } else {
                const int q3 = (int)rintf(a * 512.0f);                 // subnormal step 2^-9
                b = (unsigned char)(q3 > 7 ? 8 : q3);                  // 8 = the smallest normal
            }
        }
        dst[(size_t)n * K + p] = (unsigned char)(b | (v < 0.f ? 0x80 : 0));
    }
    if (lane == 0) scale[((size_t)(n >> 7) * 16 + (n & 15)) * 8 + ((n >> 4) & 7)] = (unsigned char)(127 - sw);
}

}  // namespace

int ofx_gemm_launch_w2f8(void* kargs, const GemmPlan& plan, hipStream_t s) {
    const KArgs& k = *(const KArgs*)kargs;
    constexpr int LDSB = 4 * 2 * 256 * 32 * 2 + 256 * 128;              // 128 KiB of stages + the 32 KiB fp8 weight buffer = 160 KiB
    static DeviceOnce attr;
    TRY(set_max_dynamic_lds(attr, gemm_w2f8_kernel, LDSB));
    OFX_PLAUNCH(true, gemm_w2f8_kernel, dim3(plan.grid_x), dim3(512), LDSB, s, k);
    return OFX_OK;
}

int ofx_launch_pack_lo8(const void* w2_rows, void* dst8, void* scale8, int N, int K, hipStream_t s) {
    OFX_REQUIRE(N % 128 == 0 && K % 128 == 0, OFX_ESHAPE, "pack_lo8: N and K must be multiples of 128");
    hipLaunchKernelGGL(pack_lo8_kernel, dim3((N + 3) / 4), dim3(256), 0, s, (const f16_t*)w2_rows, (unsigned char*)dst8, (unsigned char*)scale8, N, K);
    OFX_LAUNCH_CHECK();
    return OFX_OK;
}
