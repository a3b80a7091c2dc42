// The accumulation boundary of the training step over the flat gradient arena, fp32: clip_grad_norm_(max_norm) -> AdamW -> zero the
// gradient (torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, amsgrad off, maximize off; what cp_trainer:70-80 runs).  gfx950 only.
//
//   g = grad_scale * grad over the WHOLE arena;  norm = ||g||_2;  non-finite norm: grad := 0 and nothing else moves (*skipped = 1)
//   t = *step + 1;  g *= min(max_norm / (norm + 1e-6), 1);  p *= 1 - lr wd;  m += (g - m)(1 - b1);  v = b2 v + (1 - b2) g g
//   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps);  grad := 0
//
// The gradient and the two moments are arenas of n_arena floats (trainer.FlatGrads' layout: every tensor starts on a 64-float granule,
// the gaps are zero padding); the parameters stay where the caller keeps them, and a device table of (param, offset, numel), sorted by
// offset, says which arena floats belong to which tensor.
//
// Two launches, each at most OPT_MAX_GRID workgroups of 256 threads striding over the arena in steps of OPT_WG_FLOATS floats
// (OPT_UNROLL 16-byte loads in flight per thread and stream, in both kernels: checked in the ISA):
//   1. adamw_norm_kernel: sum of (grad_scale * g)^2, squared and accumulated in DOUBLE from the first element on (the norm's error does
//      not depend on the arena's size, and finite fp32 gradients cannot overflow it) -> one double per workgroup in the workspace.
//      Workgroup 0 also copies *step to the workspace, so that the second launch can read the old value while it writes the new one.
//   2. adamw_update_kernel: every workgroup adds up the same partials in the same order (thread t takes t, t + 256, ...; lanes, then
//      waves), so all of them hold the same norm bits; thread 0 works out the per-step constants in double - 1 - lr wd, 1 - b^t by
//      repeated squaring, the clip coefficient from the fp32 norm it reports - and hands them to the workgroup as floats.  Then one
//      pass, OPT_UNROLL float4s per lane and stride step: the g, m, v loads of all of them go out first (the arenas need no segment);
//      while they fly, a 16-lane group of float4 lanes finds its granule's segment by binary search over the table's offsets (at most
//      11 steps, no LDS; the OPT_UNROLL searches advance side by side, one wait per step); then the OPT_UNROLL parameter loads go out
//      together, and p, m, v are rewritten and g zeroed with 16-byte stores.  The one float4 that straddles the end of a tensor whose
//      numel is no multiple of 4 touches the parameter with scalar accesses and keeps the moments' padding as it was.  Granules (or
//      float4s) past a tensor's end only have their gradient zeroed.
// No floating-point atomics and no atomics at all: two calls from the same state give the same bits.  Nothing is allocated, copied
// or waited for; both launches go to the caller's stream and can be captured.
//
// ofx_adamw_step_scaled: the same boundary behind a dynamic loss scale, torch.amp.GradScaler's unscale_ -> step -> update (what the
// reference's trainers wrap the sequence above in), still two launches, the same loads and stores per arena float, and no atomics.  The
// arena holds loss_scale x the gradient; the scale and its growth tracker are device scalars that this call reads AND rewrites:
//   1. adamw_norm_kernel<true>: every element times c = grad_scale * inv in fp32, inv = (float)(1.0 / (double)*loss_scale), then the
//      same double sum.  Workgroup 0 also copies *loss_scale and *growth_tracker into the workspace header, next to *step.
//   2. adamw_update_kernel<true>: thread 0 of EVERY workgroup rebuilds c from the header's copy of the scale; workgroup 0 writes the
//      new scale and tracker to *loss_scale / *growth_tracker.  That is the hazard the header's step copy exists for: workgroups of
//      one launch run in no defined order, so a workgroup that read *loss_scale itself could see the value workgroup 0 has already
//      replaced, and unscale its share of the arena by another factor than the norm was taken with.  Nobody writes the header in
//      launch 2 and nobody writes *loss_scale in launch 1, so every read is of a value that is final.
//      The scaler: skipped (non-finite norm) -> scale *= backoff, tracker = 0; else tracker += 1 and, when it equals growth_interval,
//      scale *= growth (kept if that is not finite, as torch does) and tracker = 0.  Products in double, stored as float.
// For a power-of-two scale S, (g S) * (grad_scale / S) and g * grad_scale are the same real number: the scaled call on S x the arena
// returns the bits of the plain call (tests/test_gpu_loss_scale.py).  The plain kernels' code is what it was before the scaled ones
// were added: each kernel is one template, and its SCALED = false instance never reads the scaler's arguments.
#include <math.h>

#include "ofx_common.h"

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_UNROLL = 4;
constexpr long long OPT_WG_FLOATS = (long long)OPT_THREADS * 4 * OPT_UNROLL;      // 4096 floats per workgroup and stride step
constexpr int OPT_MAX_GRID = 2048;
constexpr size_t OPT_HDR_BYTES = 256;             // workspace: float step_old, float scale_old, int tracker_old, pad | double partial[OPT_MAX_GRID]

struct OptConsts {                                 // per-step constants, fp32 images of values computed in double
    float clip, decay, w1, beta2, w2, step_size, bc2_sqrt, eps;
    int skip;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the workgroup, the same bits in every thread: lanes -> waves in a fixed order
__device__ __forceinline__ double block_sum_f64(double v, double* sred) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sred[0] + sred[1]) + (sred[2] + sred[3]);
}

struct OptHeader { float step_old, scale_old; int tracker_old; };      // the first words of the workspace

// the factor a scaled gradient element is multiplied by, in fp32: grad_scale / loss_scale
__device__ __forceinline__ float unscale_factor(float grad_scale, float loss_scale) { return grad_scale * (float)(1.0 / (double)loss_scale); }

struct ScalerArgs {                                // ofx_adamw_step_scaled's additions; all zero and never read when !SCALED
    float* loss_scale;
    int* growth_tracker;
    double growth, backoff;
    int interval;
};

template <bool SCALED>
__global__ __launch_bounds__(OPT_THREADS) void adamw_norm_kernel(const float* __restrict__ grad, long long n, float grad_scale,
                                                                 const float* __restrict__ step, OptHeader* hdr, double* partial, ScalerArgs sa) {
    __shared__ double sred[4];
    const int tid = threadIdx.x;
    if constexpr (SCALED) grad_scale = unscale_factor(grad_scale, *sa.loss_scale);
    double acc[OPT_UNROLL];
#pragma unroll
    for (int u = 0; u < OPT_UNROLL; ++u) acc[u] = 0.0;
    for (long long base = (long long)blockIdx.x * OPT_WG_FLOATS; base < n; base += (long long)gridDim.x * OPT_WG_FLOATS) {
        f32x4 g[OPT_UNROLL];
#pragma unroll
        for (int u = 0; u < OPT_UNROLL; ++u) {
            const long long f = base + (long long)u * (OPT_THREADS * 4) + tid * 4;
            g[u] = f < n ? *(const f32x4*)(grad + f) : f32x4{0.f, 0.f, 0.f, 0.f};       // n % 64 == 0: a float4 is inside or outside
        }
#pragma unroll
        for (int u = 0; u < OPT_UNROLL; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)(g[u][e] * grad_scale);
                acc[u] = fma(d, d, acc[u]);
            }
    }
    const double s = block_sum_f64((acc[0] + acc[1]) + (acc[2] + acc[3]), sred);
    if (tid == 0) {
        partial[blockIdx.x] = s;
        if (blockIdx.x == 0) {
            hdr->step_old = *step;
            if constexpr (SCALED) { hdr->scale_old = *sa.loss_scale; hdr->tracker_old = *sa.growth_tracker; }
        }
    }
}

__device__ __forceinline__ double pow_int(double b, long long t) {
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

template <bool SCALED>
__global__ __launch_bounds__(OPT_THREADS) void adamw_update_kernel(const ofx_opt_segment* __restrict__ seg, int n_seg, float* __restrict__ grad,
                                                                   float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, long long n,
                                                                   float grad_scale, double lr, double beta1, double beta2, double eps, double wd,
                                                                   double max_norm, int n_partial, const double* __restrict__ partial,
                                                                   const OptHeader* __restrict__ hdr, float* step, float* grad_norm, int* skipped,
                                                                   ScalerArgs sa) {
    __shared__ double sred[4];
    __shared__ OptConsts sc;
    __shared__ float s_unscale;
    const int tid = threadIdx.x;
    double a = 0.0;
    for (int i = tid; i < n_partial; i += OPT_THREADS) a += partial[i];
    const double sumsq = block_sum_f64(a, sred);
    if (tid == 0) {
        const float norm = (float)sqrt(sumsq);
        const bool ok = isfinite(norm);
        const float t = hdr->step_old + 1.0f;
        const double bc1 = 1.0 - pow_int(beta1, (long long)t), bc2 = 1.0 - pow_int(beta2, (long long)t);
        sc.skip = !ok;
        sc.clip = (float)fmin(max_norm / ((double)norm + 1e-6), 1.0);
        sc.decay = (float)(1.0 - lr * wd);
        sc.w1 = (float)(1.0 - beta1);
        sc.beta2 = (float)beta2;
        sc.w2 = (float)(1.0 - beta2);
        sc.step_size = (float)(lr / bc1);
        sc.bc2_sqrt = (float)sqrt(bc2);
        sc.eps = (float)eps;
        if (blockIdx.x == 0) {
            *grad_norm = norm;
            *skipped = ok ? 0 : 1;
            if (ok) *step = t;
        }
        if constexpr (SCALED) {
            const float scale = hdr->scale_old;
            s_unscale = unscale_factor(grad_scale, scale);
            if (blockIdx.x == 0) {                                         // GradScaler.update(); everyone else reads the header's copy
                const int grown = hdr->tracker_old + 1;
                if (!ok) {
                    *sa.loss_scale = (float)((double)scale * sa.backoff);
                    *sa.growth_tracker = 0;
                } else if (grown == sa.interval) {
                    const float up = (float)((double)scale * sa.growth);
                    if (isfinite(up)) *sa.loss_scale = up;
                    *sa.growth_tracker = 0;
                } else {
                    *sa.growth_tracker = grown;
                }
            }
        }
    }
    __syncthreads();
    const OptConsts c = sc;
    if constexpr (SCALED) grad_scale = s_unscale;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    if (c.skip) {                                                          // non-finite norm: drop the gradient, touch nothing else
        for (long long base = (long long)blockIdx.x * OPT_WG_FLOATS; base < n; base += (long long)gridDim.x * OPT_WG_FLOATS)
#pragma unroll
            for (int u = 0; u < OPT_UNROLL; ++u) {
                const long long f = base + (long long)u * (OPT_THREADS * 4) + tid * 4;
                if (f < n) *(f32x4*)(grad + f) = zero;
            }
        return;
    }
    const int search_steps = 32 - __builtin_clz((unsigned)n_seg);          // halvings of [0, n_seg] until it is empty: <= 11
    for (long long base = (long long)blockIdx.x * OPT_WG_FLOATS; base < n; base += (long long)gridDim.x * OPT_WG_FLOATS) {
        long long f[OPT_UNROLL];
        bool in[OPT_UNROLL];
        f32x4 g[OPT_UNROLL], m0[OPT_UNROLL], v0[OPT_UNROLL], w[OPT_UNROLL];
        // ---- the arenas need no segment: their 3 x OPT_UNROLL loads go out first and fly while the table is searched
#pragma unroll
        for (int u = 0; u < OPT_UNROLL; ++u) {
            f[u] = base + (long long)u * (OPT_THREADS * 4) + tid * 4;
            in[u] = f[u] < n;
            const long long fc = in[u] ? f[u] : 0;
            g[u] = *(const f32x4*)(grad + fc);
            m0[u] = *(const f32x4*)(exp_avg + fc);
            v0[u] = *(const f32x4*)(exp_avg_sq + fc);
        }
        // ---- largest i with seg[i].offset <= the float4's granule (or -1): OPT_UNROLL binary searches side by side, one wait per step
        int lo[OPT_UNROLL], hi[OPT_UNROLL];                                 // first i in [lo, hi) with offset > granule
#pragma unroll
        for (int u = 0; u < OPT_UNROLL; ++u) { lo[u] = 0; hi[u] = n_seg; }
        for (int it = 0; it < search_steps; ++it) {
            long long off[OPT_UNROLL];
#pragma unroll
            for (int u = 0; u < OPT_UNROLL; ++u) off[u] = seg[min((lo[u] + hi[u]) >> 1, n_seg - 1)].offset;
#pragma unroll
            for (int u = 0; u < OPT_UNROLL; ++u) {                          // selects, no branches: the searches stay in lock step
                const int mid = (lo[u] + hi[u]) >> 1;
                const bool open = lo[u] < hi[u], below = off[u] <= (f[u] & ~63LL);
                lo[u] = open && below ? mid + 1 : lo[u];
                hi[u] = open && !below ? mid : hi[u];
            }
        }
        long long live[OPT_UNROLL];                                         // floats of the float4 that belong to a tensor (<= 0: none)
        float OFX_GLB* p[OPT_UNROLL];                                       // device memory: global_*, not flat_*, accesses
#pragma unroll
        for (int u = 0; u < OPT_UNROLL; ++u) {
            const ofx_opt_segment sg = seg[max(lo[u] - 1, 0)];
            const long long rel = f[u] - sg.offset;
            live[u] = in[u] && lo[u] > 0 ? sg.numel - rel : 0;
            p[u] = (float OFX_GLB*)sg.param + rel;
        }
        // ---- the parameters: OPT_UNROLL 16-byte loads in flight.  A float4 that is not wholly inside a tensor loads its own gradient
        // again instead (a valid address, an L2 hit, and no branch between the loads); the one that straddles a tensor's end then
        // reads the parameter float by float
#pragma unroll
        for (int u = 0; u < OPT_UNROLL; ++u)
            w[u] = *(live[u] >= 4 ? (const f32x4 OFX_GLB*)p[u] : (const f32x4 OFX_GLB*)(grad + (in[u] ? f[u] : 0)));
#pragma unroll
        for (int u = 0; u < OPT_UNROLL; ++u)
            if (live[u] > 0 && live[u] < 4) {
                w[u] = zero;
                for (int e = 0; e < 3; ++e)
                    if (e < live[u]) w[u][e] = p[u][e];
            }
#pragma unroll
        for (int u = 0; u < OPT_UNROLL; ++u) {
            if (!in[u]) continue;
            if (live[u] <= 0) { *(f32x4*)(grad + f[u]) = zero; continue; }
            f32x4 m1, v1, w1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gc = (g[u][e] * grad_scale) * c.clip;
                const float pw = w[u][e] * c.decay;
                m1[e] = m0[u][e] + (gc - m0[u][e]) * c.w1;
                v1[e] = c.beta2 * v0[u][e] + (c.w2 * gc) * gc;
                const float denom = sqrtf(v1[e]) / c.bc2_sqrt + c.eps;
                w1[e] = pw - c.step_size * (m1[e] / denom);
            }
            if (live[u] >= 4) {
                *(f32x4 OFX_GLB*)p[u] = w1;
            } else {
                for (int e = 0; e < 3; ++e)
                    if (e < live[u]) p[u][e] = w1[e]; else { m1[e] = m0[u][e]; v1[e] = v0[u][e]; }
                m1[3] = m0[u][3]; v1[3] = v0[u][3];
            }
            *(f32x4*)(exp_avg + f[u]) = m1;
            *(f32x4*)(exp_avg_sq + f[u]) = v1;
            *(f32x4*)(grad + f[u]) = zero;
        }
    }
}

int opt_grid(long long n) { return (int)((n + OPT_WG_FLOATS - 1) / OPT_WG_FLOATS < OPT_MAX_GRID ? (n + OPT_WG_FLOATS - 1) / OPT_WG_FLOATS : OPT_MAX_GRID); }

template <bool SCALED>
int launch_step(const ofx_opt_segment* segments, int n_segments, float* grad, float* exp_avg, float* exp_avg_sq, long long n_arena, float* step,
                double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm, double grad_scale, const ScalerArgs& sa,
                float* grad_norm, int* skipped, void* ws, hipStream_t s) {
    static_assert(sizeof(OptHeader) <= OPT_HDR_BYTES, "the workspace header holds the step, the scale and the tracker");
    OptHeader* hdr = (OptHeader*)ws;
    double* partial = (double*)((char*)ws + OPT_HDR_BYTES);
    const int grid = opt_grid(n_arena);
    hipLaunchKernelGGL(adamw_norm_kernel<SCALED>, dim3(grid), dim3(OPT_THREADS), 0, s, grad, n_arena, (float)grad_scale, step, hdr, partial, sa);
    OFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(adamw_update_kernel<SCALED>, dim3(grid), dim3(OPT_THREADS), 0, s, segments, n_segments, grad, exp_avg, exp_avg_sq, n_arena,
                       (float)grad_scale, lr, beta1, beta2, eps, weight_decay, max_norm, grid, partial, hdr, step, grad_norm, skipped, sa);
    OFX_LAUNCH_CHECK();
    return OFX_OK;
}

}  // namespace

size_t ofx_adamw_step_ws(long long n_arena) { return OPT_HDR_BYTES + (size_t)opt_grid(n_arena) * sizeof(double); }

int ofx_launch_adamw_step(const ofx_opt_segment* segments, int n_segments, float* grad, float* exp_avg, float* exp_avg_sq, long long n_arena,
                          float* step, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm, double grad_scale,
                          float* grad_norm, int* skipped, void* ws, hipStream_t s) {
    return launch_step<false>(segments, n_segments, grad, exp_avg, exp_avg_sq, n_arena, step, lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale,
                              ScalerArgs{}, grad_norm, skipped, ws, s);
}

int ofx_launch_adamw_step_scaled(const ofx_opt_segment* segments, int n_segments, float* grad, float* exp_avg, float* exp_avg_sq, long long n_arena,
                                 float* step, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                                 double grad_scale, float* loss_scale, int* growth_tracker, double growth_factor, double backoff_factor,
                                 int growth_interval, float* grad_norm, int* skipped, void* ws, hipStream_t s) {
    return launch_step<true>(segments, n_segments, grad, exp_avg, exp_avg_sq, n_arena, step, lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale,
                             ScalerArgs{loss_scale, growth_tracker, growth_factor, backoff_factor, growth_interval}, grad_norm, skipped, ws, s);
}
