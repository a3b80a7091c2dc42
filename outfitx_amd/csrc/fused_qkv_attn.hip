// Fused QKV projection + scaled-dot-product attention of a CLIP ViT layer (the kernel BASELINE.json's north star names).
//
// Replaces, per layer, the pair [QKV GEMM -> q|k|v in HBM -> attention kernel] (HF CLIPAttention reached from
// src/models/encoders/image_encoders/clip_image_encoder.py:74-76: q/k/v_proj, softmax(q k^T / 8) v; out_proj stays a GEMM).
// q | k | v never touch HBM: 2 x 472 MB per ViT layer at 2048 images.
//
// One block = G images (G = 256 / S rounded down = 5 for S = 50: 250 of the 256 tile rows live) x ONE head:
//   1. [256 x 192] = X_blk [256 x W] . W_h^T, W_h = the head's 64 q, 64 k and 64 v weight rows (K = W = 768, 12 k-tiles of 64):
//      the ping-pong main loop of gemm_pp.hip (LDS-DMA into two 56 KiB stages, XOR-swizzled 128-byte rows, the two wave groups
//      offset by one barrier slot), 8 waves x (128 x 48) accumulators;
//   2. epilogue INTO LDS: (LayerNorm-fold row statistics, column sums,) bias, rounding to the operand type; Q and K as 144-byte
//      rows, V as 160-byte rows (conflict-free for ds_read_b128 / ds_read_b64_tr_b16) over the now idle stages: "LDS-staged K/V";
//   3. waves 0 .. G-1 each run one image's attention - the wave-level core of attn_wave.h, the one attention_mfma_kernel runs - with
//      every fragment read from LDS, and store the image's [S x 64] output slice.
// Block order (bijective XCD remap, then units of 6 image groups x half the heads): the blocks resident on an XCD share six 384 KB
// activation tiles and six heads' weights (4.1 MB, the size of that XCD's L2).
#include "attn_wave.h"
#include "gemm_common.h"

namespace {

struct FusedK {
    const char* X;          // [n_img * S, ldx] operand type: LayerNorm output, or the raw stream copy when row_stat (LayerNorm folding)
    const char* Wqkv;       // [3 Wm, Wm] operand type, rows q | k | v
    char* out;              // [n_img * S, ldo] operand type: attention output (heads concatenated)
    const float* bias;      // [3 Wm]
    const float* row_stat;  // optional [rows, 2] (mean, rstd): LayerNorm-fold consumer
    const float* col_sum;   // [3 Wm] with row_stat
    int n_img, S, Wm, heads, ldx, ldo, G, nwg;
    float scale;
    // fp8-correction variant: Wqkv rows are [hi | lo]; W8 [3 Wm, Wm] bytes = the e4m3 copy of the lo half, scale8 its E8M0 row scales (ofx_launch_pack_lo8)
    const char* W8 = nullptr; const char* scale8 = nullptr;
};

constexpr int FQ_TM = 256, FQ_TN = 192, FQ_STAGE = (FQ_TM + FQ_TN) * BK * 2;      // 57344
constexpr int FQ_QK_ROW = 144;                                                    // bytes per Q / K row in LDS; V rows: ATTN_V_ROW
constexpr int FQ_NT = 4;                                                          // 16-row key / query tiles of the attention tail (S <= 64)
static_assert(FQ_TN == 3 * ATTN_D && 16 * FQ_NT == ATTN_D, "the tail runs the attention core at NT = 4 on one head's 64 q, 64 k and 64 v columns");
constexpr int FQ_Q_OFF = 0, FQ_K_OFF = FQ_TM * FQ_QK_ROW, FQ_V_OFF = 2 * FQ_TM * FQ_QK_ROW;      // 0, 36864, 73728; V ends at 114688 = 2 stages
constexpr int FQ_LDS = 2 * FQ_STAGE + 16 * ATTN_V_ROW;                             // + 16 zeroed V rows behind the last image (keys S .. 63 of image G-1)
// Dual-weight variant (W2 = true: Wqkv rows are [hi(Wm) | lo(Wm)], the split weights of DESIGN.md section 2): the counted-wait
// ping-pong of gemm_pingpong.h, as gemm_w2.hip runs it - BK = 32, three stages [A 256 rows | W_hi 192 rows | W_lo 192 rows] x 64 B,
// the two wave groups offset by one barrier slot, 48 MFMAs (8 A fragments x 3 column tiles x {hi, lo}) per wave and step against 14
// fragment reads - then the same epilogue and attention.  The q | k | v image (117,248 B incl. the V pad rows) lies inside the
// three stages (122,880 B).
constexpr int FQ2_BK = 32, FQ2_A = FQ_TM * FQ2_BK * 2, FQ2_W = FQ_TN * FQ2_BK * 2, FQ2_STAGE = FQ2_A + 2 * FQ2_W, FQ2_NST = 3;   // 16384, 12288, 40960
constexpr int FQ2_LDS = FQ2_NST * FQ2_STAGE;
static_assert(FQ2_LDS >= FQ_LDS, "q | k | v image must fit the dual-weight stages");
// fp8-correction variant (fused_qkv_attn_w2f8_kernel below): gemm_w2f8_kernel's main loop on the 256 x 192 tile - BK = 32, FOUR stages [A 256 rows |
// W_hi 192 rows] x 64 B and one buffer of the current super-step's fp8 weights (192 rows x 128 B).  width % 128 == 0 makes the k-steps of a tile a
// multiple of four, so step x of EVERY tile lives in stage x & 3: the q | k | v image starts behind stage 0 (over stages 1 - 3, the fp8 buffer and
// 6,656 B more), and stage 0 receives the next tile's first k-step while the block runs its epilogue and attention.  Behind the image: the waves'
// slots of epilogue constants (64 rows x (mean, rstd), 96 biases, 96 column sums), filled one tile ahead.
constexpr int FQ8_A = FQ_TM * 32 * 2, FQ8_W = FQ_TN * 32 * 2, FQ8_STAGE = FQ8_A + FQ8_W, FQ8_NST = 4;      // 16384, 12288, 28672
constexpr int FQ8_W8BASE = FQ8_NST * FQ8_STAGE, FQ8_W8 = FQ_TN * 128;                                        // 114688, 24576
constexpr int FQ8_IMG = FQ8_STAGE, FQ8_CST = FQ8_IMG + FQ_LDS, FQ8_CST_WAVE = (2 * 64 + 2 * 96) * 4;          // 28672, 145920, 1280
constexpr int FQ8_LDS = FQ8_CST + 8 * FQ8_CST_WAVE;                                                          // 156160
static_assert(FQ8_CST >= FQ8_W8BASE + FQ8_W8 && FQ8_IMG + 2 * FQ_STAGE >= FQ8_W8BASE + FQ8_W8, "the V pad rows and the constants lie behind everything LDS-DMA fills");
static_assert(FQ8_LDS <= 160 * 1024, "one block per CU");

template <typename T>
__device__ __forceinline__ void fq_attention(OFX_LDS char* lds, const FusedK& p, int wave, int lane, int m0, int head);

template <typename T, bool W2 = false>
__global__ __launch_bounds__(512, 2) void fused_qkv_attn_kernel(FusedK p) {
    typedef typename OpT<T>::v8 v8;
    typedef typename OpT<T>::v4 v4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    OFX_LDS char* lds = (OFX_LDS char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    const int bid = xcd_remap(blockIdx.x, p.nwg);
    // L2 working set (4 MiB per XCD, 32 resident blocks): a unit of 36 consecutive blocks = 6 image groups x HALF the heads
    // (6 activation tiles 2.3 MB + 6 heads' weights 1.8 MB), the next unit the same groups x the other half - the activation
    // tiles are fetched once, the weight halves once per 6 groups (head-fastest over all 12 heads needed all 3.5 MB of weights
    // plus the tiles at once and re-fetched the weights per group: 985 MB of fabric traffic per launch against 318 MB algorithmic)
    const int hh = p.heads % 2 == 0 ? p.heads / 2 : p.heads, halves = p.heads / hh, per_unit = 6 * hh;
    const int unit = bid / per_unit, in_unit = bid % per_unit;
    const int grp = (unit / halves) * 6 + in_unit / hh, head = (unit % halves) * hh + in_unit % hh;
    if (grp * p.G >= p.n_img) return;                 // ragged last group batch (block-uniform, before any barrier)
    const int M = p.n_img * p.S;
    const int m0 = grp * p.G * p.S;
    const int n_live_img = min(p.G, p.n_img - grp * p.G);

    f32x4 acc[8][3];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;

    if constexpr (W2) {
    // ------------------------------------------------------------------ dual-weight main loop (gemm_pingpong.h: the slot schedule)
    const PpLane32 L(lane);
    const int prow = L.prow, pchk = L.pchk;
    const char* a_base = p.X + (size_t)m0 * p.ldx * 2;
    const char* w_base = p.Wqkv + (size_t)head * 64 * (2 * p.Wm) * 2;          // row stride 2 Wm elements: [hi | lo]
    unsigned a_off[2], w_off[3];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (wave * 2 + i) * 16 + prow;
        const int rr = m0 + row < M ? row : M - 1 - m0;
        a_off[i] = ((unsigned)rr * p.ldx + pchk * 8) * 2;
    }
    int w_dst[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int q = wave * 3 + i;                                            // 24 weight pieces: 0..11 hi, 12..23 lo (16 tile rows each)
        const int row = (q % 12) * 16 + prow;                                  // tile row 0..191 = which * 64 + r
        const unsigned grow = (unsigned)(row >> 6) * p.Wm + (row & 63);
        w_off[i] = (grow * (2 * p.Wm) + (q >= 12 ? p.Wm : 0) + pchk * 8) * 2;
        w_dst[i] = FQ2_A + (q >= 12 ? FQ2_W : 0) + (q % 12) * 1024;
    }
    const int a_dst = wave * 2 * 1024;
    const int nk = p.Wm / FQ2_BK;
    auto issue_all = [&](int step) {
        const int sc = step < nk ? step : nk - 1;
        OFX_LDS char* base = lds + (step % FQ2_NST) * FQ2_STAGE;
        const char* ak = a_base + (size_t)sc * FQ2_BK * 2;
        const char* wk = w_base + (size_t)sc * FQ2_BK * 2;
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(ak + a_off[i], base + a_dst + i * 1024);
#pragma unroll
        for (int i = 0; i < 3; ++i) glds16(wk + w_off[i], base + w_dst[i]);
    };
    const int a_frag = (wr * 128 + fr) * 64 + L.fchk;
    const int w_frag = FQ2_A + (wc * 48 + fr) * 64 + L.fchk;
    v8 af[8], wh[3], wl[3];
    auto read = [&](int t) { pp_w2_read<3>(lds + (t % FQ2_NST) * FQ2_STAGE, a_frag, w_frag, FQ2_W, af, wh, wl); };
    auto mfma = [&] { pp_w2_mfma<T, 3>(acc, af, wh, wl); };
    issue_all(0); issue_all(1);
    asm volatile("s_waitcnt vmcnt(5)" ::: "memory");            // step 0 landed (my pieces)
    __builtin_amdgcn_s_barrier();
    // iteration t issues step t + 2 (5 pieces per wave: they stay in flight over the counted wait), reads and multiplies step t
    if (wr == 0) {
        for (int t = 0; t < nk; ++t) pp_slot<0, 5>([&] { issue_all(t + 2); }, [&] { read(t); }, mfma);
        pp_group_end<0>();
    } else {
        pp_group_begin<1>();
        for (int t = 0; t < nk; ++t) pp_slot<1, 5>([&] { issue_all(t + 2); }, [&] { read(t); }, mfma);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                           // every stage read and every (clamped) fill is done: the stages become q | k | v
    // the V pad rows lie inside stage 2 here: zero them now (the barrier before the attention publishes them)
    if (tid < 16 * ATTN_V_ROW / 16) *(OFX_LDS f32x4*)(lds + 2 * FQ_STAGE + tid * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
    // ------------------------------------------------------------------ single-product main loop (ping-pong, BK = 64, two stages)
    // zero the V pad rows once (never touched by the stages)
    if (tid < 16 * ATTN_V_ROW / 16) *(OFX_LDS f32x4*)(lds + 2 * FQ_STAGE + tid * 16) = f32x4{0.f, 0.f, 0.f, 0.f};

    const int lrow = lane >> 3, lchk = lane & 7;
    const char* a_base = p.X + (size_t)m0 * p.ldx * 2;
    const char* w_base = p.Wqkv + (size_t)head * 64 * p.Wm * 2;
    unsigned a_off[4], w_off[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + lrow;
        const int rr = m0 + row < M ? row : M - 1 - m0;
        a_off[i] = ((unsigned)rr * p.ldx + (lchk ^ ((row >> 1) & 7)) * 8) * 2;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int row = (wave * 3 + i) * 8 + lrow;                         // tile row 0..191 = which * 64 + r
        const unsigned grow = (unsigned)(row >> 6) * p.Wm + (row & 63);    // + head * 64 (in w_base)
        w_off[i] = (grow * p.Wm + (lchk ^ ((row >> 1) & 7)) * 8) * 2;
    }
    const int a_dst = wave * 4 * 1024, w_dst = FQ_TM * BK * 2 + wave * 3 * 1024;
    auto issue_all = [&](int kt, int stage) {
        OFX_LDS char* base = lds + stage * FQ_STAGE;
        const char* ak = a_base + (size_t)kt * BK * 2;
        const char* wk = w_base + (size_t)kt * BK * 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16(ak + a_off[i], base + a_dst + i * 1024);
#pragma unroll
        for (int i = 0; i < 3; ++i) glds16(wk + w_off[i], base + w_dst + i * 1024);
    };

    const int fsw = fr >> 1;
    const int a_frag = (wr * 128 + fr) * 128;
    const int w_frag = FQ_TM * BK * 2 + (wc * 48 + fr) * 128;
    v8 af[2][8], wf[2][3];

#define FQ_READ_FRAGS(STG)                                                                                    \
    {                                                                                                         \
        OFX_LDS char* base_ = lds + (STG) * FQ_STAGE;                                                         \
        _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                    \
            const int chk = ((ks * 4 + fq) ^ fsw) * 16;                                                       \
            _Pragma("unroll") for (int j = 0; j < 3; ++j) wf[ks][j] = *(OFX_LDS v8*)(base_ + w_frag + j * 16 * 128 + chk); \
            _Pragma("unroll") for (int i = 0; i < 8; ++i) af[ks][i] = *(OFX_LDS v8*)(base_ + a_frag + i * 16 * 128 + chk); \
        }                                                                                                     \
    }

    const int nk = p.Wm / BK;
    issue_all(0, 0);
    issue_all(nk > 1 ? 1 : 0, 1);
    asm volatile("s_waitcnt vmcnt(7)" ::: "memory");        // k-tile 0 landed (my pieces)
    __builtin_amdgcn_s_barrier();                           // ---- end of slot 0
    if (wr == 0) {
        for (int t = 0; t < nk; ++t) {
            if (t >= 1 && t + 1 < nk) issue_all(t + 1, (t + 1) & 1);
            FQ_READ_FRAGS(t & 1)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int m = 0; m < 48; ++m) {
                const int ks = m / 24, i = (m % 24) / 3, j = m % 3;
                acc[i][j] = OpT<T>::mfma16(wf[ks][j], af[ks][i], acc[i][j]);
            }
            __builtin_amdgcn_s_setprio(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        __builtin_amdgcn_s_barrier();
    } else {
        __builtin_amdgcn_s_barrier();
        for (int t = 0; t < nk; ++t) {
            FQ_READ_FRAGS(t & 1)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            OFX_LDS char* nbase = lds + (t & 1) * FQ_STAGE;
            const int kn = t + 2 < nk ? t + 2 : nk - 1;
            const char* ak = a_base + (size_t)kn * BK * 2;
            const char* wk = w_base + (size_t)kn * BK * 2;
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int m = 0; m < 48; ++m) {
                if (m % 6 == 0 && m / 6 < 7) {
                    const int q = m / 6;
                    if (q < 4) glds16(ak + a_off[q], nbase + a_dst + q * 1024);
                    else glds16(wk + w_off[q - 4], nbase + w_dst + (q - 4) * 1024);
                }
                const int ks = m / 24, i = (m % 24) / 3, j = m % 3;
                acc[i][j] = OpT<T>::mfma16(wf[ks][j], af[ks][i], acc[i][j]);
            }
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_s_barrier();
        }
    }
#undef FQ_READ_FRAGS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                           // every stage read and every (clamped) fill is done: the stages become q | k | v
    }

    // ---- epilogue into LDS: acc[i][j][r] = C[row wr*128 + i*16 + fr][col wc*48 + j*16 + fq*4 + r]
    {
        float mu[8], rs[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            mu[i] = 0.f; rs[i] = 1.f;
            if (p.row_stat) {
                const int gm = min(m0 + wr * 128 + i * 16 + fr, M - 1);
                const f32x2 ms = *(const f32x2*)(p.row_stat + 2 * (size_t)gm);
                mu[i] = ms[0]; rs[i] = ms[1];
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int c = wc * 48 + j * 16 + fq * 4, which = c >> 6, d = c & 63;
            const int gn = which * p.Wm + head * 64 + d;
            const f32x4 b4 = *(const f32x4*)(p.bias + gn);
            f32x4 cs4 = {0.f, 0.f, 0.f, 0.f};
            if (p.row_stat) cs4 = *(const f32x4*)(p.col_sum + gn);
            OFX_LDS char* reg = lds + (which == 0 ? FQ_Q_OFF : which == 1 ? FQ_K_OFF : FQ_V_OFF);
            const int stride = which == 2 ? ATTN_V_ROW : FQ_QK_ROW;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = wr * 128 + i * 16 + fr;
                const f32x4 v = (acc[i][j] - cs4 * mu[i]) * rs[i] + b4;
                v4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (T)v[e];
                *(OFX_LDS v4*)(reg + row * stride + d * 2) = o;
            }
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    // ---- attention: wave w < n_live_img owns image w of the group (rows w*S ..), head `head`
    if (wave >= n_live_img) return;
    fq_attention<T>(lds, p, wave, lane, m0, head);
}

// The attention tail of every variant: `wave` runs image `wave` of the block's group on the q | k | v image at `lds` (FQ_*_OFF) and stores
// the image's [S x 64] output slice of head `head`; m0 = the group's first row.
template <typename T>
__device__ __forceinline__ void fq_attention(OFX_LDS char* lds, const FusedK& p, int wave, int lane, int m0, int head) {
    typedef typename OpT<T>::v8 v8;
    constexpr int NT = FQ_NT;
    const int S = p.S, r0 = wave * S;
    const int r16 = lane & 15, q4 = lane >> 4;
    OFX_LDS char* ql = lds + FQ_Q_OFF + r0 * FQ_QK_ROW;
    OFX_LDS char* kl = lds + FQ_K_OFF + r0 * FQ_QK_ROW;
    OFX_LDS char* vl = lds + FQ_V_OFF + r0 * ATTN_V_ROW;
    v8 kf[NT][2], qf[NT][2];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int row = 16 * t + r16;
        row = row < S ? row : S - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kf[t][ks] = *(OFX_LDS v8*)(kl + row * FQ_QK_ROW + (q4 * 8 + ks * 32) * 2);
            qf[t][ks] = *(OFX_LDS v8*)(ql + row * FQ_QK_ROW + (q4 * 8 + ks * 32) * 2);
        }
    }
    float neg[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) neg[t][r] = (16 * t + 4 * q4 + r >= S) ? -INFINITY : 0.f;
    // the wave-level core (attn_wave.h): every query tile live, no dropout, plain output rows
    f32x4 st[NT][NT];
    attn_scores<T, NT>(st, kf, qf, neg, NT);
    v8 pf[NT][attn_ksteps(NT)];
    attn_softmax_p<T, NT, false>(pf, st, p.scale, NT);
    attn_pv_store<T, NT>(vl, pf, NT, true, (T*)p.out, m0 + r0, p.ldo, head * 64, S, 0);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// fp8-correction variant (the default scheme's split weights with their fp8 pair, f16 operands): gemm_w2f8_kernel's main loop on the 256 x 192 tile,
// 8 waves as 4 x 2 of 64 x 96 (acc[4][6]: that kernel's per-wave code with six weight fragments instead of eight).  Per 128-deep super-step every
// accumulator gets the four v_mfma_f32_16x16x32_f16 products of its k-steps in k order (weight fragment first) and then ONE
// v_mfma_scale_f32_16x16x128_f8f6f4 of the e4m3 weight fragment against the e5m2 activation image made in registers from the A fragments just
// read (MODE.FP16_OVFL = 1 inside the loop) - the instruction sequence gemm_w2f8_kernel runs per accumulator, so q | k | v are its bits.
// Pieces of a k-step: 16 A + 12 W_hi of 1 KiB; waves 0-3 (ping-pong group 0) issue 2 + 2, waves 4-7 2 + 1; the super-step's 24 fp8 pieces 3 per wave.
// The slots and their counted waits are gemm_w2f8_kernel's with these piece counts (group 0: 8, 3, 4, 4 in flight; group 1: 3, 3, 3, 6).
// Persistent: block b runs the live tiles b, b + grid, ... of the one-block-per-tile order above.  A tile's redundant fill of step nk (stage 0)
// fetches the NEXT tile's first k-step; the later redundant fills re-read the tile's own last step into stages every read of which is over, and
// have landed before the epilogue turns those stages into q | k | v.  The next tile's epilogue constants and scale bytes are requested before
// the epilogue and stashed (LDS slots, two registers) after it, so no load latency stands between the attention and the next main loop.
// Scale bytes: the E8M0 bytes of a 128-row block lie as scale8[((n >> 7) 16 + (n & 15)) 8 + ((n >> 4) & 7)]; a head's 64 q (k, v) rows are HALF of
// such a block - the word's bytes 0-3 for an even head, 4-7 for an odd one (the loaded word is shifted by the head's parity) - and the six
// fragments of a wave span two of q | k | v: the wave's bytes are gathered into two registers so that fragment j's selector stays an immediate.
typedef int fq_i32x8 __attribute__((ext_vector_type(8)));
typedef int fq_i32x4 __attribute__((ext_vector_type(4)));
typedef short fq_i16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 fq_f16x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(512, 2) void fused_qkv_attn_w2f8_kernel(FusedK p) {
    typedef f16_t T;
    typedef OpT<T>::v8 v8;
    typedef OpT<T>::v4 v4;
    constexpr int BK2 = 32, PART = FQ8_A, STAGE = FQ8_STAGE;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    OFX_LDS char* lds = (OFX_LDS char*)smem;
    OFX_LDS char* img = lds + FQ8_IMG;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;           // 4 x 2 waves of 64 x 96; waves 0-3 (rows 0-127) are ping-pong group 0
    int grp = wave >> 2;
    asm volatile("" : "+s"(grp));
    const int Kh = p.Wm, nk = Kh / BK2, nsup = nk >> 2;
    const int M = p.n_img * p.S;
    const float a_scale = 1.0f;                        // the e5m2 activation image is unscaled (E8M0 byte 127 = 2^0)
    const int a_e8 = 127;

    // the one-block-per-tile order of fused_qkv_attn_kernel (units of 6 image groups x half the heads), walked b, b + grid, ...; tiles of the
    // ragged last unit that lie past the last group are skipped
    const int hh = p.heads % 2 == 0 ? p.heads / 2 : p.heads, halves = p.heads / hh, per_unit = 6 * hh;
    auto decode = [&](int v, int& g, int& h) {
        const int bid = xcd_remap(v, p.nwg), unit = bid / per_unit, in_unit = bid % per_unit;
        g = (unit / halves) * 6 + in_unit / hh;
        h = (unit % halves) * hh + in_unit % hh;
    };
    auto next_live = [&](int v) {
        for (; v < p.nwg; v += (int)gridDim.x) {
            int g, h;
            decode(v, g, h);
            if (g * p.G < p.n_img) break;
        }
        return v;
    };
    int vb = next_live(blockIdx.x);
    if (vb >= p.nwg) return;                           // block-uniform, before any barrier

    int ln = lane;
    asm volatile("" : "+v"(ln));
    OFX_LDS float* cst = (OFX_LDS float*)(lds + FQ8_CST + wave * FQ8_CST_WAVE);      // this wave's constants: [64 x (mean, rstd) | 96 biases | 96 column sums]

    // A tile's epilogue constants and scale bytes: lane l requests row l's (mean, rstd), lanes 0-23 four biases each, lanes 32-55 four column
    // sums each, and per q | k | v the scale word of row l & 15 ...
    auto load_consts = [&](int m0_, int head_, f32x2& ms, f32x4& c4, unsigned long long (&sw)[3]) {
        ms = f32x2{0.f, 1.f};
        c4 = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.row_stat) ms = *(const f32x2*)(p.row_stat + 2 * (size_t)min(m0_ + wr * 64 + ln, M - 1));
        const float* cb = ln >= 32 ? (p.row_stat ? p.col_sum : nullptr) : p.bias;
        const int c = wc * 96 + (ln & 31) * 4;
        if (cb && (ln & 31) < 24) c4 = *(const f32x4*)(cb + (c >> 6) * Kh + head_ * 64 + (c & 63));
#pragma unroll
        for (int w = 0; w < 3; ++w) sw[w] = *(const unsigned long long*)(p.scale8 + ((size_t)(w * (Kh >> 7) + (head_ >> 1)) * 16 + (ln & 15)) * 8);
    };
    // ... and, once they are there, puts them where the tile reads them: the wave's LDS slot, and the six fragments' scale bytes in (sa, sb):
    // fragment j < 4 -> byte j of sa, fragment 4 + j -> byte j of sb (columns wc 96 + 16 j: q 0-3 | k 0-1 for wc = 0, k 2-3 v 0-1 | v 2-3 for wc = 1)
    auto stash_consts = [&](int head_, f32x2 ms, f32x4 c4, const unsigned long long (&sw)[3], int& sa, int& sb) {
        *(OFX_LDS f32x2*)(cst + 2 * ln) = ms;
        if ((ln & 31) < 24) *(OFX_LDS f32x4*)(cst + 128 + (ln >> 5) * 96 + (ln & 31) * 4) = c4;
        const int sh = (head_ & 1) * 32;
        const unsigned q_ = (unsigned)(sw[0] >> sh), k_ = (unsigned)(sw[1] >> sh), v_ = (unsigned)(sw[2] >> sh);
        sa = (int)(wc == 0 ? q_ : (k_ >> 16) | (v_ << 16));
        sb = (int)(wc == 0 ? k_ : v_ >> 16);
    };

    const size_t a_row = (size_t)p.ldx * 2;
    const unsigned w_head = 64u * (2 * Kh) * 2;
    const __amdgpu_buffer_rsrc_t r_w = make_rsrc(p.Wqkv), r_w8 = make_rsrc(p.W8);
    int grp_t, head, sc_a, sc_b;
    decode(vb, grp_t, head);
    {
        f32x2 ms; f32x4 c4; unsigned long long sw[3];
        load_consts(grp_t * p.G * p.S, head, ms, c4, sw);
        stash_consts(head, ms, c4, sw, sc_a, sc_b);
    }
    // the 16 zeroed V rows behind the image (keys S .. 63 of the group's last image): no fill ever reaches them
    if (tid < 16 * ATTN_V_ROW / 16) *(OFX_LDS f32x4*)(img + 2 * FQ_STAGE + tid * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
    bool first = true;

    for (;;) {
        const int vn = next_live(vb + (int)gridDim.x);
        const bool has_next = vn < p.nwg;
        int grp_n = grp_t, head_n = head;               // the block's last tile names itself (it re-fills its own first step: nobody reads it)
        if (has_next) decode(vn, grp_n, head_n);
        const int m0 = grp_t * p.G * p.S, m1 = grp_n * p.G * p.S;
        const int n_live_img = min(p.G, p.n_img - grp_t * p.G);
        // lane constants from an opaque copy of the lane id, per tile: kept across the epilogue and the attention they would not fit the registers
        int l2 = ln;
        asm volatile("" : "+v"(l2));
        const PpLane32 L(l2);
        const int fr = L.fr, fq = L.fq;
        // LDS-DMA pieces (tile-independent offsets; the tile's rows and the head's weight rows ride in the buffer resources)
        const int wp0 = grp == 0 ? wave * 2 : 4 + wave;    // W_hi pieces 2 w, 2 w + 1 (group 0) | 8 + (w - 4) (group 1)
        unsigned a_off[2], w_off[2], w8_off[3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a_off[i] = ((unsigned)((wave * 2 + i) * 16 + L.prow) * p.ldx + L.pchk * 8) * 2;
            const int row = ((wp0 + i) * 16 + L.prow) % FQ_TN;                  // tile row = which * 64 + r  (group 1 uses piece 0 only)
            w_off[i] = (((unsigned)(row >> 6) * Kh + (row & 63)) * (2 * Kh) + L.pchk * 8) * 2;
        }
        // fp8 piece P = 3 wave + q: 8 rows x 128 B, tile rows 8 P + (l >> 3); physical chunk l & 7 <- logical (l & 7) ^ x(row & 15),
        // row & 15 = (P & 1) 8 + (l >> 3)  =>  x = (((l >> 4) & 3) << 1) | (P & 1)   (gemm_w2f8_kernel's buffer image)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int P = wave * 3 + q;
            w8_off[q] = (unsigned)((P >> 3) * Kh + (P & 7) * 8 + (l2 >> 3)) * Kh + ((((l2 & 7) ^ (((l2 >> 4) & 3) << 1)) ^ (P & 1)) << 4);
        }
        const int a_dst = wave * 2 * 1024, w_dst = PART + wp0 * 1024, w8_dst = FQ8_W8BASE + wave * 3 * 1024;
        const int a_frag = (wr * 64 + fr) * 64 + L.fchk;
        const int w_frag = PART + (wc * 96 + fr) * 64 + L.fchk;
        const int x8 = (((fr >> 1) & 3) << 1) | (fr >> 3);
        const int w8_frag0 = (wc * 96 + fr) * 128 + (((2 * fq) ^ x8) << 4), w8_frag1 = (wc * 96 + fr) * 128 + (((2 * fq + 1) ^ x8) << 4);
        // the tile's rows through a resource that ends with the matrix: rows past M read zeros (the hardware's range check covers the per-lane offset,
        // not the scalar one: the tile's origin is the resource's base); the head's weight rows and the k offset ride in the scalar offset
        const __amdgpu_buffer_rsrc_t r_a = make_rsrc(p.X + (size_t)m0 * a_row, (size_t)(M - m0) * a_row), r_a1 = make_rsrc(p.X + (size_t)m1 * a_row, (size_t)(M - m1) * a_row);
        // k-step x of the walk into stage x & 3 (nk % 4 == 0): a step of this tile; x == nk: the next tile's step 0; past it the tile's own last step again
        auto issue_step = [&](int x, bool two_w) {
            OFX_LDS char* stg = lds + (x & 3) * STAGE;
            const bool nx = x == nk;
            const __amdgpu_buffer_rsrc_t ra = nx ? r_a1 : r_a;
            const unsigned koff = (unsigned)(nx ? 0 : (x > nk ? nk - 1 : x)) * BK2 * 2;
            const unsigned sw = (unsigned)(nx ? head_n : head) * w_head + koff;
            bload16(ra, a_off[0], koff, stg + a_dst); bload16(ra, a_off[1], koff, stg + a_dst + 1024);
            bload16(r_w, w_off[0], sw, stg + w_dst);
            if (two_w) bload16(r_w, w_off[1], sw, stg + w_dst + 1024);
        };
#define FQ8_ISSUE_W8(SUP, Q) bload16(r_w8, w8_off[Q], (unsigned)head * 64u * (unsigned)Kh + (unsigned)(SUP) * 128u, lds + w8_dst + (Q) * 1024);

        f32x4 acc[4][6];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        v8 af[4], wh[6];
        fq_i32x8 a8[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a8[i] = fq_i32x8{0, 0, 0, 0, 0, 0, 0, 0};
        auto read = [&](int step) {
            OFX_LDS char* stg = lds + (step & 3) * STAGE;
#pragma unroll
            for (int j = 0; j < 6; ++j) wh[j] = *(OFX_LDS v8*)(stg + w_frag + j * 16 * 64);
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *(OFX_LDS v8*)(stg + a_frag + i * 16 * 64);
        };
        // 24 f16 MFMAs + the conversion of the four A fragments into bytes 8 S .. 8 S + 7 of their fp8 images (S = step & 3, static)
#define FQ8_CVT1(I, S)                                                                                        \
    {                                                                                                         \
        fq_i16x2 lo_ = __builtin_bit_cast(fq_i16x2, a8[I][2 * (S)]), hi_ = __builtin_bit_cast(fq_i16x2, a8[I][2 * (S) + 1]); \
        lo_ = __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(lo_, fq_f16x2{af[I][0], af[I][1]}, a_scale, false);    \
        lo_ = __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(lo_, fq_f16x2{af[I][2], af[I][3]}, a_scale, true);     \
        hi_ = __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(hi_, fq_f16x2{af[I][4], af[I][5]}, a_scale, false);    \
        hi_ = __builtin_amdgcn_cvt_scalef32_pk_bf8_f16(hi_, fq_f16x2{af[I][6], af[I][7]}, a_scale, true);     \
        a8[I][2 * (S)] = __builtin_bit_cast(int, lo_); a8[I][2 * (S) + 1] = __builtin_bit_cast(int, hi_);      \
    }
#define FQ8_MFMA16(S)                                                                                         \
    {                                                                                                         \
        __builtin_amdgcn_s_setprio(1);                                                                        \
        _Pragma("unroll") for (int j = 0; j < 6; ++j) {                                                       \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) acc[i][j] = OpT<T>::mfma16(wh[j], af[i], acc[i][j]); \
            if (j >= 2) FQ8_CVT1(j - 2, S)                                                                    \
        }                                                                                                     \
        __builtin_amdgcn_s_setprio(0);                                                                        \
    }
        // the super-step's 24 fp8 MFMAs: weight fragment j (two 16-byte reads per lane) against the four activation images, through a 3-deep
        // register ring; the scale-byte selector is an immediate, hence one expansion per fragment
#define FQ8_LD(J)                                                                                             \
    {                                                                                                         \
        const fq_i32x4 c0_ = *(OFX_LDS fq_i32x4*)(b8_ + w8_frag0 + (J) * 16 * 128), c1_ = *(OFX_LDS fq_i32x4*)(b8_ + w8_frag1 + (J) * 16 * 128); \
        w8_[(J) % 3] = fq_i32x8{c0_[0], c0_[1], c0_[2], c0_[3], c1_[0], c1_[1], c1_[2], c1_[3]};              \
    }
#define FQ8_MF(J, SEL, SC)                                                                                    \
    if ((J) + 2 < 6) { FQ8_LD((J) + 2) __builtin_amdgcn_sched_barrier(0); }                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                             \
        acc[i][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w8_[(J) % 3], a8[i], acc[i][J], 0, 1, SEL, SC, 0, a_e8);
#define FQ8_MFMA8()                                                                                           \
    {                                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        OFX_LDS char* b8_ = lds + FQ8_W8BASE;                                                                 \
        fq_i32x8 w8_[3];                                                                                      \
        FQ8_LD(0) FQ8_LD(1)                                                                                   \
        __builtin_amdgcn_s_setprio(1);                                                                        \
        FQ8_MF(0, 0, sc_a) FQ8_MF(1, 1, sc_a) FQ8_MF(2, 2, sc_a) FQ8_MF(3, 3, sc_a)                           \
        FQ8_MF(4, 0, sc_b) FQ8_MF(5, 1, sc_b)                                                                 \
        __builtin_amdgcn_s_setprio(0);                                                                        \
    }

        if (first) {                                                  // group 1 runs one step further ahead
            issue_step(0, grp == 0); issue_step(1, grp == 0);
            if (grp == 0) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");        // step 0 landed (my pieces)
            else { issue_step(2, false); asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); }
        } else {
            // step 0 arrived under the previous tile's tail (complete before its epilogue); iteration 0's counted waits cover what is issued here
            issue_step(1, grp == 0);
            if (grp != 0) issue_step(2, false);
        }
        asm volatile("" : "+v"(sc_a), "+v"(sc_b));
        asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1");     // MODE.FP16_OVFL: the f16 -> e5m2 conversion clamps at 57,344 instead of inf / NaN
        __builtin_amdgcn_s_barrier();                               // ---- end of slot 0
        auto run = [&](auto G) {
            constexpr int g = G.value;
            constexpr bool w2 = g == 0;
            pp_group_begin<g>();
            int u = 0;
            do {
                const int t = 4 * u;
                pp_slot<g, g ? 3 : 8>([&] { if (g == 0) issue_step(t + 2, w2); issue_step(t + 3, w2); }, [&] { read(t); }, [&] { FQ8_MFMA16(0) });
                pp_slot<g, 3>([&] { FQ8_ISSUE_W8(u, 0) FQ8_ISSUE_W8(u, 1) FQ8_ISSUE_W8(u, 2) }, [&] { read(t + 1); }, [&] { FQ8_MFMA16(1) });
                pp_slot<g, g ? 3 : 4>([&] { issue_step(t + 4, w2); }, [&] { read(t + 2); }, [&] { FQ8_MFMA16(2) });
                pp_slot<g, g ? 6 : 4>([&] { issue_step(t + 5, w2); if (g == 1) issue_step(t + 6, w2); }, [&] { read(t + 3); }, [&] { FQ8_MFMA16(3) }, [&] { FQ8_MFMA8() });
            } while (++u < nsup);
            pp_group_end<g>();
        };
        if (grp == 0) run(std::integral_constant<int, 0>());
        else run(std::integral_constant<int, 1>());
#undef FQ8_MFMA16
#undef FQ8_MFMA8
#undef FQ8_MF
#undef FQ8_LD
#undef FQ8_CVT1
#undef FQ8_ISSUE_W8
        asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 0");     // the epilogue's f32 -> f16 casts keep the default overflow behaviour
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                           // every stage read and every fill is done: stages 1-3 and the fp8 buffer become q | k | v

        // the next tile's constants: requested before the epilogue, stashed after it
        f32x2 ms_n; f32x4 c4_n; unsigned long long sw_n[3];
        load_consts(m1, head_n, ms_n, c4_n, sw_n);

        // ---- epilogue into LDS: acc[i][j][r] = C[row wr*64 + i*16 + fr][col wc*96 + j*16 + fq*4 + r], the value chain of the GEMM epilogues (epi_value)
        {
            const KArgs none{};
            auto emit = [&](auto FOLD) {
                constexpr bool fold = FOLD.value;
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const int c = wc * 96 + j * 16 + fq * 4, which = c >> 6, d = c & 63;
                    const f32x4 b4 = *(OFX_LDS const f32x4*)(cst + 128 + j * 16 + fq * 4);
                    f32x4 cs4 = {0.f, 0.f, 0.f, 0.f};
                    if (fold) cs4 = *(OFX_LDS const f32x4*)(cst + 224 + j * 16 + fq * 4);
                    OFX_LDS char* reg = img + (which == 0 ? FQ_Q_OFF : which == 1 ? FQ_K_OFF : FQ_V_OFF);
                    const int stride = which == 2 ? ATTN_V_ROW : FQ_QK_ROW;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = wr * 64 + i * 16 + fr;
                        float mu = 0.f, rs = 1.f;
                        if (fold) { const f32x2 ms = *(OFX_LDS const f32x2*)(cst + 2 * (i * 16 + fr)); mu = ms[0]; rs = ms[1]; }
                        const f32x4 v = epi_value(none, acc[i][j], OFX_ACT_NONE, fold, mu, rs, cs4, b4, false);
                        v4 o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (T)v[e];
                        *(OFX_LDS v4*)(reg + row * stride + d * 2) = o;
                    }
                }
            };
            if (p.row_stat) emit(std::true_type());
            else emit(std::false_type());
        }
        stash_consts(head_n, ms_n, c4_n, sw_n, sc_a, sc_b);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();

        // ---- attention: wave w < n_live_img owns image w of the group
        if (wave < n_live_img) fq_attention<T>(img, p, wave, ln, m0, head);
        if (!has_next) break;
        __builtin_amdgcn_s_barrier();                           // every read of the image is done: the next tile's fills may land in stages 1-3
        vb = vn; grp_t = grp_n; head = head_n;
        first = false;
    }
}

}  // namespace

// X [n_img * S, ldx], Wqkv [3 Wm, Wm] (q | k | v rows; split forms: [3 Wm, 2 Wm], row = [hi | lo]), out [n_img * S, ldo]; non-causal, no key mask (the ViT's
// attention).  FUSED_QKV_W2F8: W8 / scale8 = the fp8 copy of the lo half (ofx_launch_pack_lo8), f16 operands, Wm a multiple of 128 (the fp8 super-step)
int ofx_launch_fused_qkv_attn(const void* X, const void* Wqkv, const float* bias, const float* row_stat, const float* col_sum, void* out,
                              int n_img, int S, int Wm, int heads, int ldx, int ldo, float scale, int op_dtype, hipStream_t s, FusedQkvForm form,
                              const void* W8, const void* scale8) {
    const bool w2 = form != FUSED_QKV_PLAIN, f8 = form == FUSED_QKV_W2F8;
    OFX_REQUIRE(X && Wqkv && bias && out && n_img > 0, OFX_EINVAL, "fused_qkv_attn: NULL argument");
    OFX_REQUIRE(!f8 || (W8 && scale8), OFX_EINVAL, "fused_qkv_attn: the fp8 form needs W8 and scale8");
    OFX_REQUIRE(!f8 || op_dtype == OFX_F16, OFX_EINVAL, "fused_qkv_attn: the fp8 form takes f16 operands");
    OFX_REQUIRE(S >= 33 && S <= 64 && Wm == heads * 64 && Wm % BK == 0 && Wm / BK >= 2, OFX_ESHAPE, "fused_qkv_attn: S=%d must be in [33,64], width %d = heads * 64", S, Wm);
    OFX_REQUIRE(!f8 || Wm % 128 == 0, OFX_ESHAPE, "fused_qkv_attn: the fp8 form needs a width that is a multiple of 128, not %d", Wm);
    // a head's weight rows ride in the 32-bit scalar offset of the buffer loads, a tile's 256 rows of X in the per-lane one
    OFX_REQUIRE(!f8 || ((size_t)FQ_TM * ldx * 2 < 0x7fffffff && (size_t)3 * Wm * Wm * 4 < 0x7fffffff), OFX_ESHAPE, "fused_qkv_attn: the fp8 form takes weights below 2 GiB");
    // the last image of a block reads keys up to tile row (G - 1) S + 63; only 16 zeroed V pad rows sit behind row 255
    OFX_REQUIRE((FQ_TM / S - 1) * S + 64 - FQ_TM <= 16, OFX_ESHAPE, "fused_qkv_attn: S=%d would read %d key rows past the tile's 16 pad rows (supported: 33, 34, 37..41, 43..64)", S,
                (FQ_TM / S - 1) * S + 64 - FQ_TM);
    OFX_REQUIRE(ldx >= Wm && ldx % 8 == 0 && ldo >= Wm && ldo % 8 == 0, OFX_ESHAPE, "fused_qkv_attn: bad strides");
    OFX_REQUIRE(!row_stat || col_sum, OFX_EINVAL, "fused_qkv_attn: row_stat needs col_sum");
    FusedK k;
    k.X = (const char*)X; k.Wqkv = (const char*)Wqkv; k.out = (char*)out; k.bias = bias; k.row_stat = row_stat; k.col_sum = col_sum;
    k.n_img = n_img; k.S = S; k.Wm = Wm; k.heads = heads; k.ldx = ldx; k.ldo = ldo; k.G = FQ_TM / S; k.scale = scale;
    k.W8 = (const char*)W8; k.scale8 = (const char*)scale8;
    const int groups = (n_img + k.G - 1) / k.G;
    k.nwg = ((groups + 5) / 6) * 6 * heads;            // whole units of 6 groups (blocks of the ragged tail exit at once)
    static DeviceOnce attr;
    TRY(attr.run([]() -> int {
        OFX_HIP(hipFuncSetAttribute((const void*)fused_qkv_attn_kernel<bf16_t, false>, hipFuncAttributeMaxDynamicSharedMemorySize, FQ_LDS));
        OFX_HIP(hipFuncSetAttribute((const void*)fused_qkv_attn_kernel<f16_t, false>, hipFuncAttributeMaxDynamicSharedMemorySize, FQ_LDS));
        OFX_HIP(hipFuncSetAttribute((const void*)fused_qkv_attn_kernel<bf16_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize, FQ2_LDS));
        OFX_HIP(hipFuncSetAttribute((const void*)fused_qkv_attn_kernel<f16_t, true>, hipFuncAttributeMaxDynamicSharedMemorySize, FQ2_LDS));
        OFX_HIP(hipFuncSetAttribute((const void*)fused_qkv_attn_w2f8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FQ8_LDS));
        return OFX_OK;
    }));
    // algorithmic bytes: X read once, the weight rows once (split: hi and lo, 4 B per weight; fp8 form: hi + the fp8 lo, 3 B), the attention output
    // [rows, Wm] written once in the operand type.  FLOPs in f16-rate equivalents: the fp8 correction product counts half (the plan's 0.75 of two products)
    const double wbytes = f8 ? 3.0 : (w2 ? 4.0 : 2.0), products = f8 ? 1.5 : (w2 ? 2.0 : 1.0);
    if (g_ofx_prof_on) ofx_prof_set_tag(n_img * S, 3 * Wm, Wm, 7, w2 ? 2 : 1, 2.0 * n_img * S * Wm + wbytes * 3.0 * Wm * Wm + 2.0 * n_img * S * Wm);
    ProfScope prof(PROF_GEMM, s, products * 2.0 * n_img * S * 3.0 * Wm * Wm + 4.0 * n_img * S * S * Wm, true);
    if (f8) {
        // persistent over the tiles as the dual-weight GEMMs are: ofx_tune(11, v)
        OFX_PLAUNCH(true, fused_qkv_attn_w2f8_kernel, dim3(ofx_gemm_w2_grid(k.nwg)), dim3(512), FQ8_LDS, s, k);
    } else if (w2) {
        if (op_dtype == OFX_F16) OFX_PLAUNCH(true, (fused_qkv_attn_kernel<f16_t, true>), dim3(k.nwg), dim3(512), FQ2_LDS, s, k);
        else OFX_PLAUNCH(true, (fused_qkv_attn_kernel<bf16_t, true>), dim3(k.nwg), dim3(512), FQ2_LDS, s, k);
    } else {
        if (op_dtype == OFX_F16) OFX_PLAUNCH(true, (fused_qkv_attn_kernel<f16_t, false>), dim3(k.nwg), dim3(512), FQ_LDS, s, k);
        else OFX_PLAUNCH(true, (fused_qkv_attn_kernel<bf16_t, false>), dim3(k.nwg), dim3(512), FQ_LDS, s, k);
    }
    OFX_LAUNCH_CHECK();
    return OFX_OK;
}
