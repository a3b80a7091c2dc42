// SetWiseRankingLoss (src/losses/set_wise_ranking_loss.py:15-36), fp32: loss value and upstream * d loss / d y_hat from ONE pass over
// the negatives.  The CIR trainer's loss (complementary_item_retrieval_trainer.py:79-88); gfx950 only.
//
//   d_pos = ||y_hat - y + 1e-6||   (F.pairwise_distance adds eps to the difference)      d_k = ||y_hat - neg_k||
//   L_all  = sum over valid (b, k) of relu(d_pos - d_k + margin) / max(#valid in the whole batch, 1)
//   L_hard = mean_b relu(d_pos - min over valid k of d_k + margin)                        (a row without a valid negative adds 0)
//   d/d y_hat = sum_valid [h_k > 0] (u_pos - u_k) / n_valid + [h_hard > 0] (u_pos - u_k*) / B,   u = difference / distance,
//   k* = lowest index attaining the minimum, relu'(0) = 0, a zero distance contributes a zero direction (torch's norm subgradient).
//   No gradient into y or the negatives (the trainer feeds precomputed embeddings).
//
// Two launches:
//   1. rank_loss_count_kernel (one block): n_valid = number of zero bytes of neg_mask - it depends on the mask only - and the reset of
//      the block counter below.
//   2. set_rank_loss_kernel, one 256-thread workgroup per query row b.  y_hat[b] and y_hat[b] - y[b] + eps live in registers (thread t owns
//      the 16-byte column groups t, t + 256, ...: D <= 4096 is at most four of them).  Every valid negative row is read from HBM once with
//      16-byte loads, up to ten rows in flight per thread; padded rows are not read at all.  ||.||^2 goes lane -> wave (shuffles) -> one LDS
//      step across the four waves.  The gradient needs every d_k of the row (the minimum, the hinge signs) before it can weight any
//      direction, so
//        K * D <= 10240 floats (40 KB of LDS; K <= 10 at D = 1024, K <= 40 at D = 256): the row's negatives stay in LDS between the
//                    distance pass and the gradient pass - each thread re-reads exactly the 16-byte groups it stored itself;
//        larger K * D: the gradient pass re-reads them from global memory (L2-resident by then: one row's negatives are K * D * 4 bytes).
//      The distances themselves go to d_neg (or to the workspace when the caller does not want them; the first 256 of a row also stay in
//      LDS): padded entries read +inf there.
//   Deterministic: each row writes its two partial losses to the workspace; the block that finishes last (an integer counter, the
//   only atomic) adds them up in a fixed order.  No floating-point atomics anywhere, so two runs are bit-identical.
//
// Where the rows come from is a template parameter (SRC) of both kernels - ONE body:
//   DenseRows   y [B, D], neg [B, K, D], one mask byte per negative (ofx_set_rank_loss).  Its instances are, instruction for instruction, the
//               kernels this file had before SRC existed: every line SRC touches is an `if constexpr` around the dense expression.
//   TableRows   y[b] = table[pos_index[b]], neg[b, k] = table[neg_index[b, k]], a negative index = padded (ofx_set_rank_loss_indexed); `y` and
//               `neg` both carry the table, `mask` the index array, and pos_index / ld / n_table follow the common arguments.
//               A chunk's <= 32 indices are ONE coalesced load per wave ahead of the burst of row loads (lane i keeps the index of negative
//               k0 + i in a register); a row's base is a v_readlane of that register - wave-uniform, no index load per row and none between
//               the rows in flight.  The gradient pass that re-reads rows (K * D > 10240) fetches indices the same way, 32 at a time.
//               Indices are clamped into the table as they are fetched (pos into [0, n_table), a non-negative neg to <= n_table - 1): a
//               wrong index gives a wrong result, never an access outside the table.
//   Same arithmetic in the same order on the same values: both forms return the same bits for the same rows.
#include <math.h>

#include "ofx_common.h"

namespace {

constexpr int RL_THREADS = 256;
constexpr int RL_KC = 32;                   // negatives per distance chunk (one LDS step across the waves per chunk)
constexpr int RL_SD = 256;                  // distances of the row's first RL_SD negatives are also kept in LDS (no global round trip)
constexpr int RL_LDS_FLOATS = 10240;        // negatives kept in LDS when K * D fits: 40 KB
constexpr size_t RL_HDR_BYTES = 16;         // workspace: int n_valid, unsigned blocks_done, pad | float partial[B][2] | float d[B][K]

struct DenseRows {
    static constexpr bool indexed = false;
    using Pad = uint8_t;                               // per negative: non-zero = padded
};
struct TableRows {
    static constexpr bool indexed = true;
    using Pad = int;                                   // per negative: its table row, negative = padded
    // a wave's copy of the <= RL_KC indices of negatives [k0, k0 + kc), lane i holding negative k0 + i: one coalesced load, clamped to the
    // table's last row; padded entries and lanes >= kc read -1
    static __device__ __forceinline__ int fetch(const int* irow, int k0, int kc, int last) {
        const int lane = threadIdx.x & 63;
        const int t = lane < kc ? irow[k0 + lane] : -1;
        return t < 0 ? -1 : min(t, last);
    }
    // block b's positive row (index clamped into the table), the row stride and the last row, from the arguments this source appends
    static __device__ __forceinline__ void open(const float* table, int b, const float*& prow, int& ld, int& last, const int* pos_index, int ld_,
                                                int n_table) {
        ld = ld_;
        last = n_table - 1;
        prow = table + (size_t)min(max(pos_index[b], 0), last) * ld;
    }
    static __device__ __forceinline__ int at(int held, int i) { return __builtin_amdgcn_readlane(held, i); }      // i is wave-uniform
};

template <class SRC>
__global__ __launch_bounds__(1024) void rank_loss_count_kernel(const typename SRC::Pad* __restrict__ mask, size_t n, int* hdr) {
    __shared__ int red[16];
    int c = 0;
    if constexpr (SRC::indexed) {                      // indices >= 0, 4 per load (a NULL array comes with n = 0)
        const size_t n4 = ((uintptr_t)mask & 15) == 0 ? n / 4 : 0;
        for (size_t i = threadIdx.x; i < n4; i += 1024) {
            const int4 v = ((const int4*)mask)[i];
            c += (v.x >= 0) + (v.y >= 0) + (v.z >= 0) + (v.w >= 0);
        }
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 1024) c += mask[i] >= 0;
    } else if (!mask) {
        c = threadIdx.x == 0 ? (int)n : 0;
    } else {
        const size_t n16 = ((uintptr_t)mask & 15) == 0 ? n / 16 : 0;          // 16 mask bytes per load
        for (size_t i = threadIdx.x; i < n16; i += 1024) {
            const uint4 v = ((const uint4*)mask)[i];
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) c += ((w[q] >> (8 * e)) & 0xffu) == 0u;
        }
        for (size_t i = n16 * 16 + threadIdx.x; i < n; i += 1024) c += mask[i] == 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < 16; ++w) t += red[w];
        hdr[0] = t;
        hdr[1] = 0;
    }
}

__device__ __forceinline__ float dot4(f32x4 v) { return v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }

// NV: 16-byte column groups per thread (D <= 1024 * NV); RES: the row's negatives are kept in LDS for the gradient pass; SRC: the row source,
// X: what it appends to the common arguments (TableRows: pos_index, ld, n_table; DenseRows: nothing)
template <int NV, bool RES, class SRC, class... X>
__global__ __launch_bounds__(RL_THREADS) void set_rank_loss_kernel(const float* __restrict__ y, const float* __restrict__ y_hat,
                                                                   const float* __restrict__ neg, const typename SRC::Pad* __restrict__ mask, int B,
                                                                   int K, int D, float margin, float up, float* loss, float* dy_hat, float* d_pos_out,
                                                                   float* d_all, int* hdr, float* partial, X... extra) {
    extern __shared__ float sneg[];                    // RES: [K][D]
    __shared__ float sred[RL_KC * 4], sd[RL_SD];
    constexpr int U = NV == 1 ? 10 : NV == 2 ? 5 : 2;      // negative rows in flight per thread (the reference config's K = 10 in one burst)
    __shared__ float spos[4], ssum[4], smin[4];
    __shared__ int sact[4], sarg[4], slast;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)b * D;
    const float* nrow = neg + (size_t)b * K * D;
    const typename SRC::Pad* mrow = mask ? mask + (size_t)b * K : nullptr;
    float* drow = d_all + (size_t)b * K;
    [[maybe_unused]] const float* prow = nullptr;      // TableRows: the positive's row, the row stride, the last row, this wave's chunk of indices
    [[maybe_unused]] int ld = 0, last = 0, held = -1;
    if constexpr (SRC::indexed) SRC::open(y, b, prow, ld, last, extra...);

    f32x4 h[NV], pd[NV];
    float pp = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = (tid + j * RL_THREADS) * 4;
        h[j] = pd[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < D) {
            h[j] = *(const f32x4*)(y_hat + row + c);
            if constexpr (SRC::indexed) pd[j] = h[j] - *(const f32x4*)(prow + c) + 1e-6f;
            else pd[j] = h[j] - *(const f32x4*)(y + row + c) + 1e-6f;
            pp += dot4(pd[j]);
        }
    }
    pp = wave_sum(pp);
    if (lane == 0) spos[wave] = pp;

    // ---- distance pass: every valid negative once from HBM, U rows in flight
    for (int k0 = 0; k0 < K; k0 += RL_KC) {
        const int kc = min(RL_KC, K - k0);
        if constexpr (SRC::indexed) held = SRC::fetch(mrow, k0, kc, last);
        for (int kk = 0; kk < kc; kk += U) {
            f32x4 v[U][NV];
            bool on[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = k0 + kk + u;
                [[maybe_unused]] int t = 0;
                if constexpr (SRC::indexed) { t = SRC::at(held, kk + u); on[u] = t >= 0; }           // lanes >= kc hold -1
                else on[u] = kk + u < kc && !(mrow && mrow[k]);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const int c = (tid + j * RL_THREADS) * 4;
                    if constexpr (SRC::indexed) v[u][j] = (on[u] && c < D) ? *(const f32x4*)(neg + (size_t)max(t, 0) * ld + c) : h[j];
                    else v[u][j] = (on[u] && c < D) ? *(const f32x4*)(nrow + (size_t)k * D + c) : h[j];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!on[u]) continue;
                float p = 0.f;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const int c = (tid + j * RL_THREADS) * 4;
                    if (c < D) {
                        if (RES) *(f32x4*)(sneg + (size_t)(k0 + kk + u) * D + c) = v[u][j];
                        p += dot4(h[j] - v[u][j]);
                    }
                }
                p = wave_sum(p);
                if (lane == 0) sred[(kk + u) * 4 + wave] = p;
            }
        }
        __syncthreads();
        if (tid < kc) {
            const int k = k0 + tid;
            bool padded;
            if constexpr (SRC::indexed) padded = held < 0;                     // tid < kc <= RL_KC: thread tid is lane tid of wave 0
            else padded = mrow && mrow[k];
            const float d = padded ? INFINITY : sqrtf((sred[tid * 4] + sred[tid * 4 + 1]) + (sred[tid * 4 + 2] + sred[tid * 4 + 3]));
            drow[k] = d;
            if (k < RL_SD) sd[k] = d;
        }
        __syncthreads();                               // also orders this block's drow stores before its loads below
    }
    if (K == 0) __syncthreads();                       // spos
    const float dpos = sqrtf((spos[0] + spos[1]) + (spos[2] + spos[3]));

    // ---- hinges of the row: sum and count of the active ones, the hardest negative (lowest index on a tie)
    float hs = 0.f, dm = INFINITY;
    int na = 0, km = K;
    for (int k = tid; k < K; k += RL_THREADS) {
        const float d = k < RL_SD ? sd[k] : drow[k];
        if (d < INFINITY) {
            const float hk = dpos - d + margin;
            if (hk > 0.f) { hs += hk; ++na; }
            if (d < dm) { dm = d; km = k; }
        }
    }
    hs = wave_sum(hs);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        na += __shfl_xor(na, o, 64);
        const float od = __shfl_xor(dm, o, 64);
        const int ok = __shfl_xor(km, o, 64);
        if (od < dm || (od == dm && ok < km)) { dm = od; km = ok; }
    }
    if (lane == 0) { ssum[wave] = hs; sact[wave] = na; smin[wave] = dm; sarg[wave] = km; }
    __syncthreads();
    hs = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
    na = sact[0] + sact[1] + sact[2] + sact[3];
    dm = smin[0]; km = sarg[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (smin[w] < dm || (smin[w] == dm && sarg[w] < km)) { dm = smin[w]; km = sarg[w]; }
    const float hh = km < K ? fmaxf(dpos - dm + margin, 0.f) : 0.f;
    const bool hard = hh > 0.f;

    // ---- gradient pass
    if (dy_hat) {
        const float inv_nv = 1.0f / (float)max(hdr[0], 1), inv_b = 1.0f / (float)B;
        const float cp = dpos > 0.f ? ((float)na * inv_nv + (hard ? inv_b : 0.f)) / dpos : 0.f;
        f32x4 acc[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[j] = pd[j] * cp;
        for (int k = 0; k < K; ++k) {
            if constexpr (SRC::indexed && !RES)
                if (k % RL_KC == 0) held = SRC::fetch(mrow, k, min(RL_KC, K - k), last);
            const float d = k < RL_SD ? sd[k] : drow[k];
            if (!(d < INFINITY) || !(d > 0.f)) continue;
            const float w = (dpos - d + margin > 0.f ? inv_nv : 0.f) + (hard && k == km ? inv_b : 0.f);
            if (w == 0.f) continue;
            const float s = w / d;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c = (tid + j * RL_THREADS) * 4;
                if (c < D) {
                    f32x4 v;
                    if constexpr (SRC::indexed && !RES) v = *(const f32x4*)(neg + (size_t)max(SRC::at(held, k % RL_KC), 0) * ld + c);
                    else v = RES ? *(const f32x4*)(sneg + (size_t)k * D + c) : *(const f32x4*)(nrow + (size_t)k * D + c);
                    acc[j] -= (h[j] - v) * s;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = (tid + j * RL_THREADS) * 4;
            if (c < D) *(f32x4*)(dy_hat + row + c) = acc[j] * up;
        }
    }

    // ---- the row's partial losses; the block that finishes last adds all of them up in a fixed order
    if (tid == 0) {
        partial[2 * (size_t)b] = hs;
        partial[2 * (size_t)b + 1] = hh;
        if (d_pos_out) d_pos_out[b] = dpos;
        __threadfence();
        slast = atomicAdd((unsigned*)&hdr[1], 1u) == (unsigned)(B - 1);
    }
    __syncthreads();
    if (!slast) return;
    __threadfence();
    float a = 0.f, g = 0.f;
    const unsigned* pu = (const unsigned*)partial;     // loads that bypass this CU's vector cache (written by other CUs during this launch)
    for (int r = tid; r < B; r += RL_THREADS) {
        a += __builtin_bit_cast(float, __hip_atomic_load(pu + 2 * (size_t)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        g += __builtin_bit_cast(float, __hip_atomic_load(pu + 2 * (size_t)r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    a = wave_sum(a); g = wave_sum(g);
    __syncthreads();
    if (lane == 0) { ssum[wave] = a; smin[wave] = g; }
    __syncthreads();
    if (tid == 0)
        *loss = ((ssum[0] + ssum[1]) + (ssum[2] + ssum[3])) / (float)max(hdr[0], 1) + ((smin[0] + smin[1]) + (smin[2] + smin[3])) / (float)B;
}

template <int NV, class SRC, class... X>
void launch_rows(bool res, size_t lds, hipStream_t s, const float* y, const float* y_hat, const float* neg, const typename SRC::Pad* mask, int B, int K,
                 int D, float margin, float up, float* loss, float* dy_hat, float* d_pos, float* d_all, int* hdr, float* partial, X... extra) {
    if (res)
        hipLaunchKernelGGL((set_rank_loss_kernel<NV, true, SRC, X...>), dim3(B), dim3(RL_THREADS), lds, s, y, y_hat, neg, mask, B, K, D, margin, up, loss,
                           dy_hat, d_pos, d_all, hdr, partial, extra...);
    else
        hipLaunchKernelGGL((set_rank_loss_kernel<NV, false, SRC, X...>), dim3(B), dim3(RL_THREADS), 0, s, y, y_hat, neg, mask, B, K, D, margin, up, loss,
                           dy_hat, d_pos, d_all, hdr, partial, extra...);
}

template <class SRC, class... X>
int launch_set_rank_loss(const float* y, const float* y_hat, const float* neg, const typename SRC::Pad* mask, int B, int K, int D, float margin,
                         float upstream, float* loss, float* dy_hat, float* d_pos, float* d_neg, void* ws, hipStream_t s, X... extra) {
    int* hdr = (int*)ws;
    float* partial = (float*)((char*)ws + RL_HDR_BYTES);
    float* d_all = d_neg ? d_neg : partial + (size_t)B * 2;
    hipLaunchKernelGGL(rank_loss_count_kernel<SRC>, dim3(1), dim3(1024), 0, s, mask, (size_t)B * (size_t)K, hdr);
    OFX_LAUNCH_CHECK();
    const bool res = K > 0 && (size_t)K * (size_t)D <= (size_t)RL_LDS_FLOATS;
    const size_t lds = res ? (size_t)K * D * sizeof(float) : 0;
    if (D <= 1024) launch_rows<1, SRC>(res, lds, s, y, y_hat, neg, mask, B, K, D, margin, upstream, loss, dy_hat, d_pos, d_all, hdr, partial, extra...);
    else if (D <= 2048) launch_rows<2, SRC>(res, lds, s, y, y_hat, neg, mask, B, K, D, margin, upstream, loss, dy_hat, d_pos, d_all, hdr, partial, extra...);
    else launch_rows<4, SRC>(res, lds, s, y, y_hat, neg, mask, B, K, D, margin, upstream, loss, dy_hat, d_pos, d_all, hdr, partial, extra...);
    OFX_LAUNCH_CHECK();
    return OFX_OK;
}

}  // namespace

size_t ofx_set_rank_loss_ws(int B, int K) {
    const size_t n = RL_HDR_BYTES + (size_t)B * 2 * sizeof(float) + (size_t)B * (size_t)K * sizeof(float);
    return (n + 255) / 256 * 256;
}

int ofx_launch_set_rank_loss(const float* y, const float* y_hat, const float* neg, const uint8_t* mask, int B, int K, int D, float margin, float upstream,
                             float* loss, float* dy_hat, float* d_pos, float* d_neg, void* ws, hipStream_t s) {
    return launch_set_rank_loss<DenseRows>(y, y_hat, neg, mask, B, K, D, margin, upstream, loss, dy_hat, d_pos, d_neg, ws, s);
}

int ofx_launch_set_rank_loss_indexed(const float* table, int ld, int n_table, const int* pos_index, const int* neg_index, const float* y_hat, int B, int K,
                                     int D, float margin, float upstream, float* loss, float* dy_hat, float* d_pos, float* d_neg, void* ws, hipStream_t s) {
    return launch_set_rank_loss<TableRows>(table, y_hat, table, neg_index, B, K, D, margin, upstream, loss, dy_hat, d_pos, d_neg, ws, s, pos_index, ld,
                                           n_table);
}
