// CIR training batches drawn on the device (ofx_cir_sample_batch, include/ofx.h): per query the positive, the shuffled and truncated
// remainder of its outfit and K negatives from the positive's pool - the reference's __getitem__ + __get_negative_sample
// (polyvore_complementary_item_retrieval_dataset.py:50-67, 94-109) for a whole batch, from the split and the pools resident in HBM.
//
// Two launches: cir_scan_kernel (one block) turns the remainder lengths min(n - 1, max_len) into cu_seqlens [B + 1]; cir_draw_kernel runs
// one wave per query, four queries per block.  Everything a wave decides is a function of (seed, draw, stream, b, counter) through
// ofx_draw_u32, so no state is kept and nothing is ordered between waves.  Inside the wave:
//   - the shuffle is a ranking: lane j holds the key of remainder item j and counts the lanes whose (key, j) is smaller - n - 1 <= 63 lane
//     reads, no serial Fisher-Yates; a rank below the truncated length is the item's place in the output;
//   - Floyd's K-subset has one serial dependency (was v chosen before?): lane s holds slot s, the K steps are one lane read and one ballot each.
// The query index is made wave-uniform (readfirstlane), so the table walks are loads on the scalar unit; every result leaves through a
// vector store of the lanes that hold it (no store is issued on the scalar unit).
// Contents of the device arrays are trusted but clamped into their arrays by the counts the host passed: wrong tables draw wrongly, inside bounds.
#include "ofx_common.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }      // hi >= lo

struct Span { int o, lo, n; };       // outfit o = outfit_rows[lo .. lo + n), n <= 64 (what one wave ranks)
__device__ __forceinline__ Span outfit_span(const CirSampleArgs& a, int b) {
    const int o = clampi(a.outfit_ids[b], 0, a.n_outfits - 1);
    const int lo = clampi(a.outfit_cu[o], 0, a.n_outfit_rows);
    const int hi = clampi(a.outfit_cu[o + 1], lo, a.n_outfit_rows);
    return {o, lo, min(hi - lo, 64)};
}
__device__ __forceinline__ int remainder_len(int n, int max_len) { return clampi(n - 1, 0, max_len); }

// cu_seqlens[b] = sum over b' < b of the remainder lengths; thread t owns the contiguous slots [t * per, (t + 1) * per).  One block: B is a
// batch size (3072 in the reference's config: three slots per thread), and a second block would need a third launch or a cross-block wait.
constexpr int SCAN_T = 1024;
__global__ __launch_bounds__(SCAN_T) void cir_scan_kernel(CirSampleArgs a) {
    __shared__ int wave_tot[SCAN_T / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int per = (a.B + SCAN_T - 1) / SCAN_T;
    const int b0 = (int)min((long long)t * per, (long long)a.B), b1 = min(b0 + per, a.B);
    int sum = 0;
    for (int b = b0; b < b1; ++b) sum += remainder_len(outfit_span(a, b).n, a.max_len);
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    int run = inc - sum;
    for (int i = 0; i < w; ++i) run += wave_tot[i];
    for (int b = b0; b < b1; ++b) {
        a.cu_seqlens[b] = run;
        run += remainder_len(outfit_span(a, b).n, a.max_len);
    }
    if (t == SCAN_T - 1) a.cu_seqlens[a.B] = run;      // the last thread's running sum ends at the total
}

constexpr int DRAW_WAVES = 4;
__global__ __launch_bounds__(64 * DRAW_WAVES) void cir_draw_kernel(CirSampleArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * DRAW_WAVES + (threadIdx.x >> 6)));
    if (b >= a.B) return;
    const Span sp = outfit_span(a, b);
    const int n = sp.n;

    // 1. the positive: a uniform choice among the eligible positions
    int p = 0;
    {
        const int plo = clampi(a.pos_cu[sp.o], 0, a.n_pos_slots);
        const int P = clampi(a.pos_cu[sp.o + 1], plo, a.n_pos_slots) - plo;
        if (P > 0) p = a.pos_slots[plo + (int)ofx_draw_below(ofx_draw_u32(a.seed, a.draw, 0u, (unsigned)b, 0u), (unsigned)P)];
        p = clampi(p, 0, max(n - 1, 0));
    }
    const int t = clampi(n > 0 ? a.outfit_rows[sp.lo + p] : 0, 0, a.n_table - 1);
    if (lane == 0) a.target_item_index[b] = t;

    // 2. the remainder: lane j < n - 1 holds file-order item j of the outfit without position p; its rank under (key, j) is its place
    {
        const int r = max(n - 1, 0), len = remainder_len(n, a.max_len);
        const int base = a.cu_seqlens[b];
        unsigned key = 0xFFFFFFFFu;
        int row = 0;
        if (lane < r) {
            key = ofx_draw_u32(a.seed, a.draw, 1u, (unsigned)b, (unsigned)lane);
            row = a.outfit_rows[sp.lo + lane + (lane >= p ? 1 : 0)];             // <= sp.lo + n - 1
        }
        int rank = 0;
        for (int j = 0; j < r; ++j) {
            const unsigned kj = (unsigned)__builtin_amdgcn_readlane((int)key, j);
            rank += (kj < key || (kj == key && j < lane)) ? 1 : 0;
        }
        if (lane < r && rank < len) a.item_index[(size_t)base + rank] = row;     // base + rank < cu_seqlens[b + 1] <= B * max_len
    }

    // 3. the negatives: K of the m - 1 other rows of the target's pool
    if (a.K > 0) {
        const int K = a.K, g = a.row_pool[t];
        int glo = 0, m = 0;
        if (g >= 0 && g < a.n_pools) {
            glo = clampi(a.pool_cu[g], 0, a.n_pool_rows);
            m = clampi(a.pool_cu[g + 1], glo, a.n_pool_rows) - glo;
        }
        const int m1 = m - 1;                                                     // the others; <= 0: none
        const int st = m > 0 ? clampi(a.row_slot[t], 0, m - 1) : 0;
        int c = -1;                                                               // this lane's value of [0, m1); -1 = an empty slot
        if (m1 >= K) {
            const int j0 = m1 - K;
            const int v = lane < K ? (int)ofx_draw_below(ofx_draw_u32(a.seed, a.draw, 2u, (unsigned)b, (unsigned)lane), (unsigned)(j0 + lane + 1)) : 0;
            for (int s = 0; s < K; ++s) {
                const int vs = __builtin_amdgcn_readlane(v, s);
                const bool taken = __ballot(lane < s && c == vs) != 0ull;
                if (lane == s) c = taken ? j0 + s : vs;                           // j0 + s exceeds every earlier choice
            }
        } else if (lane < m1) {
            c = lane;
        }
        if (lane < K) a.neg_items_index[(size_t)b * K + lane] = c < 0 ? -1 : a.pool_rows[glo + c + (c >= st ? 1 : 0)];   // <= glo + m - 1
    }
}

}  // namespace

int ofx_launch_cir_sample_batch(const CirSampleArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(cir_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, a);
    hipLaunchKernelGGL(cir_draw_kernel, dim3((a.B + DRAW_WAVES - 1) / DRAW_WAVES), dim3(64 * DRAW_WAVES), 0, s, a);
    OFX_LAUNCH_CHECK();
    return OFX_OK;
}
