// Single-tile attention of ONE wavefront on the matrix core: one (sequence, head), S <= 16 NT rows, head_dim 64.  The one
// definition behind attention_mfma_kernel (attention.hip: CLIP text and ViT towers, varlen outfit sets) and the tail of
// fused_qkv_attn_kernel (fused_qkv_attn.hip); set_attention_bwd_mfma_kernel shares the LDS row image and its transposed reads.
//
//   S^T = K . Q^T on v_mfma_f32_16x16x32 (K the A operand, Q the B operand, k = feature): with r16 = lane & 15, q4 = lane >> 4,
//     st[t][u][r] = score(query 16u + r16, key 16t + 4q4 + r), so all scores of one query sit in one lane quad {r16, r16 + 16,
//     r16 + 32, r16 + 48}.  The additive key mask (0 or -inf per key, independent of the query) rides in as the accumulator.
//   softmax per query column on the RAW scores: p = exp2(s * c - max(s) * c), c = scale * log2 e > 0: in-lane + 2 shuffles for
//     the max and the sum, one fma + v_exp_f32 + add per element, v_rcp_f32 for the normalisation.
//   P operand in place: the S^T accumulators ARE the B operand of O^T = V^T . P^T once the k index is permuted (guide section 3) -
//     P fragment element j of k-step ks <-> key 16 (2ks + (j >> 2)) + 4q4 + (j & 3).  The A operand is gathered with the same
//     permutation: V goes through LDS once as a row image (ATTN_V_ROW bytes per key) and is read back transposed with
//     ds_read_b64_tr_b16, the 4 x 4 blocks of keys 16 (2ks + h2) + 4q4 .. + 3.
//   d <-> MFMA row permutation: row m = r16 of output tile nd carries d = 16 (m >> 2) + 4 nd + (m & 3), so after the MFMA a lane's
//     16 outputs of one query, ot[0..3][u][0..3], are 16 CONSECUTIVE columns d = 16 q4 .. + 15: two 16-byte stores per lane and
//     query, 128 B per lane quad.
//
// The callers load the K / Q fragments (rows clamped to S - 1) and build the key mask: that is where they differ (global memory,
// key-padding and causal masks in attention.hip; 144-byte LDS rows and the key >= S mask in fused_qkv_attn.hip).  Every piece is
// force-inlined with its caller's constants: nu (live query tiles), the dropout switch and split3_w fold where they are literals.
// The pieces take the lane from threadIdx.x (one-dimensional blocks of 64-lane waves).
//
// The tile grid is rectangular: NT key tiles by NU query tiles, NU = NT (the whole sequence in one wave) unless the caller says
// otherwise.  attention_mfma_long_kernel (attention.hip, 65 .. 256 rows) runs the same pieces with NU = 1: one 16-query tile against
// all NT <= 16 key tiles, the whole score row still in registers, so the softmax is the same two-pass one over the whole key row.
#pragma once
#include "ofx_common.h"

constexpr int ATTN_D = 64;                      // head_dim
constexpr int ATTN_V_ROW = 160;                 // bytes per row of an LDS row image (64 x 2 B + 32 pad): tr-read conflict-free
constexpr int attn_ksteps(int NT) { return (NT + 1) / 2; }      // k-steps of 32 rows over 16 NT keys

// 8-element A fragment of one k-step from a row image, by two ds_read_b64_tr_b16 (EXEC must be all ones): element 4 h2 + e <->
// image row k0 + 16 h2 + 4q4 + e.  A lane addresses the 4 columns col .. col + 3 of row k0 + 16 h2 + 4q4 + (r16 >> 2); the read
// transposes within the 16-lane row: lane m receives column (m & 3) of the four lanes with r16 & 3 == m >> 2.  col is the caller's
// map of (r16 & 3, output tile nd) to a column quad: forward V 16 (r16 & 3) + 4 nd (see above), backward products 16 nd + 4 (r16 & 3).
template <typename T>
__device__ __forceinline__ typename OpT<T>::v8 attn_tr_frag(OFX_LDS char* img, int k0, int col) {
    typedef typename OpT<T>::v4 v4;
    const int lane = threadIdx.x & 63, r16 = lane & 15, q4 = lane >> 4;
    typename OpT<T>::v8 f;
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
        OFX_LDS s16x4* ap = (OFX_LDS s16x4*)(img + (k0 + 16 * h2 + 4 * q4 + (r16 >> 2)) * ATTN_V_ROW + col * 2);
        const v4 trv = __builtin_bit_cast(v4, __builtin_amdgcn_ds_read_tr16_b64_v4i16(ap));
#pragma unroll
        for (int e = 0; e < 4; ++e) f[4 * h2 + e] = trv[e];
    }
    return f;
}

// S^T[key][query] for the query tiles u < nu; neg[t][r] = 0 or -inf for key 16t + 4q4 + r (-inf + finite = -inf)
template <typename T, int NT, int NU = NT>
__device__ __forceinline__ void attn_scores(f32x4 (&st)[NT][NU], const typename OpT<T>::v8 (&kf)[NT][2], const typename OpT<T>::v8 (&qf)[NU][2],
                                            const float (&neg)[NT][4], int nu) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (u >= nu) continue;
            f32x4 c = {neg[t][0], neg[t][1], neg[t][2], neg[t][3]};
            c = OpT<T>::mfma16(kf[t][0], qf[u][0], c);
            st[t][u] = OpT<T>::mfma16(kf[t][1], qf[u][1], c);
        }
}

// Wavefront softmax of the raw scores, P written back normalised as the B operand pf[u][ks] (st is consumed).  A fully masked
// query gets probabilities 0.  DROP: dropout on the probabilities (training), element (pair, query * 32 + key) as in the fp32 set
// kernel, behind the wave-uniform drop.thresh test.
template <typename T, int NT, bool DROP, int NU = NT>
__device__ __forceinline__ void attn_softmax_p(typename OpT<T>::v8 (&pf)[NU][attn_ksteps(NT)], f32x4 (&st)[NT][NU], float scale, int nu,
                                               const DropArgs& drop = DropArgs(), int pair = 0) {
    const int lane = threadIdx.x & 63, r16 = lane & 15, q4 = lane >> 4;
    const float sc = scale * 1.4426950408889634f;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (u >= nu) continue;
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) m = fmaxf(m, st[t][u][r]);
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        if (m == -INFINITY) m = 0.f;
        const float mb = -m * sc;
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(st[t][u][r], sc, mb));      // arguments <= 0: no range fix-up needed
                st[t][u][r] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = sum > 0.f ? __builtin_amdgcn_rcpf(sum) : 0.f;      // a fully masked query: every e is 0, and 0 * rcp(0) would be NaN
        if constexpr (DROP) {
            if (drop.thresh) {
                const int query = 16 * u + r16;
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) st[t][u][r] *= drop_mul(drop, pair, query * 32 + 16 * t + 4 * q4 + r);
            }
        }
        // P fragment of k-step ks: element j <-> key 16(2ks + (j>>2)) + 4q4 + (j&3); keys >= 16 NT (odd NT) are zero
#pragma unroll
        for (int ks = 0; ks < attn_ksteps(NT); ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[u][ks][j] = 2 * ks + (j >> 2) < NT ? (T)(st[(2 * ks + (j >> 2)) % NT][u][j & 3] * inv) : (T)0.0f;
    }
}

// O^T[d][query] = V^T . P^T from the row image vl (rows >= S zero: 0 * garbage must stay 0), ot[nd][u][r] = O[query 16u + r16][d = 16 q4 + 4 nd + r],
// then, if store (wave-uniform), queries < n_rows of the tiles u < nu -> out[row_first + query][col0 + d]: two 16-byte stores per lane
// and query.  split3_w > 0 (wave-uniform): the row is [hi(W) | lo(W) | hi(W)], W = split3_w, lo = the rounding residual.
template <typename T, int NT, int NU = NT>
__device__ __forceinline__ void attn_pv_store(OFX_LDS char* vl, const typename OpT<T>::v8 (&pf)[NU][attn_ksteps(NT)], int nu, bool store,
                                              T* out, int row_first, int ldo, int col0, int n_rows, int split3_w) {
    typedef typename OpT<T>::v8 v8;
    const int lane = threadIdx.x & 63, r16 = lane & 15, q4 = lane >> 4;
    f32x4 ot[4][NU];
#pragma unroll
    for (int nd = 0; nd < 4; ++nd) {
        v8 vf[attn_ksteps(NT)];
#pragma unroll
        for (int ks = 0; ks < attn_ksteps(NT); ++ks) vf[ks] = attn_tr_frag<T>(vl, 32 * ks, 16 * (r16 & 3) + 4 * nd);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (u >= nu) continue;
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < attn_ksteps(NT); ++ks) c = OpT<T>::mfma16(vf[ks], pf[u][ks], c);
            ot[nd][u] = c;
        }
    }
    if (!store) return;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (u >= nu) continue;
        const int query = 16 * u + r16;
        if (query < n_rows) {
            T* op = out + (size_t)(row_first + query) * ldo + col0 + 16 * q4;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                v8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (T)ot[2 * h + (e >> 2)][u][e & 3];
                *(v8*)(op + 8 * h) = o;
                if (split3_w) {
                    v8 lo;
#pragma unroll
                    for (int e = 0; e < 8; ++e) lo[e] = (T)(ot[2 * h + (e >> 2)][u][e & 3] - (float)o[e]);
                    *(v8*)(op + split3_w + 8 * h) = lo;
                    *(v8*)(op + 2 * split3_w + 8 * h) = o;
                }
            }
        }
    }
}
