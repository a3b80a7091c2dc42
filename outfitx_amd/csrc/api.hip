// C ABI of libofx_hip.so: handle, weight packing and the launch sequences of the scoring path.
// Everything here is host code; it only enqueues work on the caller's stream (no syncs, no
// allocation on the launch path — a pack call sizes its weight arena by walking the layout (ofx_weights.h), allocates it once and
// reuses it, pointers unchanged, on every re-pack).
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <vector>
#include <mutex>
#include <cstring>

#include "ofx_weights.h"

static thread_local char g_err[512] = "";
void ofx_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* ofx_last_error(void) { return g_err; }
extern "C" int ofx_abi_version(void) { return OFX_ABI_VERSION; }
extern "C" int ofx_stream_create_low_priority(int device, ofx_stream* out) {
    OFX_REQUIRE(out, OFX_EINVAL, "stream_create_low_priority: NULL argument");
    int prev = 0, least = 0, greatest = 0;
    OFX_HIP(hipGetDevice(&prev));
    OFX_HIP(hipSetDevice(device));
    hipStream_t s = nullptr;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);          // numerically larger = lower priority
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least);
    (void)hipSetDevice(prev);
    OFX_HIP(e);
    *out = (ofx_stream)s;
    return OFX_OK;
}
extern "C" int ofx_stream_destroy(ofx_stream stream) {
    OFX_REQUIRE(stream, OFX_EINVAL, "stream_destroy: NULL stream");
    OFX_HIP(hipStreamDestroy((hipStream_t)stream));
    return OFX_OK;
}

// ------------------------------------------------------------------------------- grids
int device_cu_count() {
    static int cus[64] = {0};                          // per device ordinal; a benign race writes the same value
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    int& c = cus[dev & 63];
    if (c == 0) { int v = 0; c = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256; }
    return c;
}

// ------------------------------------------------------------------------------- profiling
bool g_ofx_prof_on = false;
int g_ofx_prof_mask = 0xf;
namespace {
struct ProfRec { hipEvent_t a, b; int cat; double flops; int tag[5]; double bytes; };      // tag: {M, N, logical K, kernel kind, K multiplier} of a GEMM launch; bytes: its algorithmic HBM bytes
std::vector<ProfRec> g_prof;
int g_prof_next_tag[5] = {0, 0, 0, 0, 0};
double g_prof_next_bytes = 0.0;
size_t g_prof_used = 0;
bool g_prof_over = false;
void fill_record(ProfRec& r, int cat, double flops) {        // takes the pending label (ofx_prof_set_tag), which is then cleared
    r.cat = cat; r.flops = flops;
    for (int i = 0; i < 5; ++i) { r.tag[i] = g_prof_next_tag[i]; g_prof_next_tag[i] = 0; }
    r.bytes = g_prof_next_bytes; g_prof_next_bytes = 0.0;
}
}
void ofx_prof_begin(int cat, hipStream_t s, double flops) {
    if (g_prof_used == g_prof.size()) {              // pool exhausted: stop recording rather than stall the launch path
        g_prof_over = true;
        return;
    }
    g_prof_over = false;
    ProfRec& r = g_prof[g_prof_used];
    fill_record(r, cat, flops);
    (void)hipEventRecord(r.a, s);
}
void ofx_prof_set_tag(int M, int N, int K, int kind, int kmul, double bytes) { g_prof_next_tag[0] = M; g_prof_next_tag[1] = N; g_prof_next_tag[2] = K; g_prof_next_tag[3] = kind; g_prof_next_tag[4] = kmul; g_prof_next_bytes = bytes; }
void ofx_prof_end(hipStream_t s) {
    if (!g_prof_over && g_prof_used < g_prof.size()) { (void)hipEventRecord(g_prof[g_prof_used].b, s); ++g_prof_used; }
}
hipEvent_t g_ofx_launch_e0 = nullptr, g_ofx_launch_e1 = nullptr;
bool ofx_prof_ext_begin(int cat, double flops) {
    if (g_prof_used == g_prof.size()) return false;
    ProfRec& r = g_prof[g_prof_used];
    fill_record(r, cat, flops);
    g_ofx_launch_e0 = r.a; g_ofx_launch_e1 = r.b;
    return true;
}
void ofx_prof_ext_end() {
    // a scope that returned before its last launch (error path) leaves its stop event unrecorded: drop the record
    if (g_ofx_launch_e1 == nullptr && g_ofx_launch_e0 == nullptr) ++g_prof_used;
    g_ofx_launch_e0 = g_ofx_launch_e1 = nullptr;
}
// on: 0 off; otherwise a bit mask of categories to time (1 GEMM, 2 norm/embed, 4 attention, 8 other; 15 = all)
static unsigned g_config_generation = 0;     // bumped by every ofx_tune call: a captured launch sequence is stale when it differs
extern "C" unsigned ofx_config_generation(void) { return g_config_generation; }
extern "C" int ofx_profile_enabled(void) { return g_ofx_prof_on ? 1 : 0; }
extern "C" void ofx_profile_enable(int on) {
    // create the event pool up front (never inside a timed region): room for 4096 bracketed launches
    while (on && g_prof.size() < 4096) {
        ProfRec r; r.cat = 0; r.flops = 0; r.bytes = 0; r.tag[0] = r.tag[1] = r.tag[2] = r.tag[3] = r.tag[4] = 0;
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) break;
        g_prof.push_back(r);
    }
    if (on) g_prof_used = 0;               // turning recording ON clears; turning it off keeps the records for read()
    g_ofx_prof_on = on != 0;
    if (on) g_ofx_prof_mask = on;
}
// Per-launch records of the last recording (call BEFORE ofx_profile_read, which clears them): waits for the events.
extern "C" int ofx_profile_records(ofx_prof_record* out, int cap) {
    int n = 0;
    for (size_t i = 0; i < g_prof_used && n < cap; ++i, ++n) {
        ProfRec& r = g_prof[i];
        OFX_HIP(hipEventSynchronize(r.b));
        float t = 0;
        OFX_HIP(hipEventElapsedTime(&t, r.a, r.b));
        out[n].cat = r.cat; out[n].M = r.tag[0]; out[n].N = r.tag[1]; out[n].K = r.tag[2]; out[n].kind = r.tag[3]; out[n].kmul = r.tag[4]; out[n].ms = t; out[n].flops = r.flops; out[n].bytes = r.bytes;
    }
    return n;
}
// Waits for the recorded events (host sync: call outside the timed region) and sums per category.
extern "C" int ofx_profile_read(double* ms, double* flops, long long* launches) {
    for (int c = 0; c < PROF_NCAT; ++c) { ms[c] = 0; flops[c] = 0; launches[c] = 0; }
    for (size_t i = 0; i < g_prof_used; ++i) {
        ProfRec& r = g_prof[i];
        OFX_HIP(hipEventSynchronize(r.b));
        float t = 0;
        OFX_HIP(hipEventElapsedTime(&t, r.a, r.b));
        ms[r.cat] += t; flops[r.cat] += r.flops; launches[r.cat] += 1;
    }
    g_prof_used = 0;
    return OFX_OK;
}

extern "C" void ofx_default_desc(ofx_model_desc* d) {
    memset(d, 0, sizeof(*d));
    d->d_model = 1024; d->n_head = 16; d->d_ffn = 2024; d->n_layers = 6; d->max_items = 16;
    d->outfit_act = OFX_ACT_MISH; d->outfit_precision = OFX_PREC_BF16X3;
    d->vit_width = 768; d->vit_layers = 12; d->vit_heads = 12; d->vit_mlp = 3072; d->vit_patch = 32; d->vit_image = 224;
    d->vit_act = OFX_ACT_QUICK_GELU;
    d->txt_width = 512; d->txt_layers = 12; d->txt_heads = 8; d->txt_mlp = 2048; d->txt_vocab = 49408; d->txt_max_pos = 77;
    d->txt_act = OFX_ACT_QUICK_GELU; d->txt_eos_id = 49407;
    d->proj_dim = 512; d->tower_precision = OFX_PREC_BF16; d->ln_eps = 1e-5f;
}

extern "C" ofx_handle* ofx_create(int device, const ofx_model_desc* desc) {
    if (!desc) { ofx_set_error("ofx_create: desc is NULL"); return nullptr; }
    ofx_handle* h = new ofx_handle();
    const char* why = ofx_configure(*h, *desc);
    if (!why && hipSetDevice(device) != hipSuccess) why = "hipSetDevice failed";
    if (why) { ofx_set_error("ofx_create: %s", why); delete h; return nullptr; }
    h->device = device;
    return h;
}

extern "C" void ofx_destroy(ofx_handle* h) {
    if (!h) return;
    h->a_out.release(); h->a_vis.release(); h->a_txt.release();
    delete h;
}

// ------------------------------------------------------------------------------------------ pack
// The ~60 small fp32 tensors of a pack (biases, LayerNorm parameters, tokens) travel in ONE kernel launch instead of one
// hipMemcpyAsync each: training re-packs after every optimizer step, and 60 x 3 us of copy launches were 0.2 ms of a 4 ms step.
// Entries are collected while a CopyBatch is active on this thread and flushed at the end of the pack call.
namespace {
struct CopyEntry { const float* src; float* dst; long long n; };
struct CopyBatch;
thread_local CopyBatch* g_copy_batch = nullptr;
struct CopyBatch {
    std::vector<CopyEntry> e;
    CopyBatch() { g_copy_batch = this; }
    ~CopyBatch() { g_copy_batch = nullptr; }
    int flush(hipStream_t s) {          // the table rides in the kernel arguments: nothing is staged, nothing is waited for
        g_copy_batch = nullptr;
        if (e.empty()) return OFX_OK;
        return ofx_launch_multi_copy(e.data(), (int)e.size(), s);
    }
};
}  // namespace
static int copy_f32(float* dst, const void* src, size_t n, hipStream_t s) {
    if (g_copy_batch) { g_copy_batch->e.push_back({(const float*)src, dst, (long long)n}); return OFX_OK; }
    OFX_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return OFX_OK;
}

// Sizes the arena by the layout walk over a counting arena, then places the handle's pointers by the same walk over the real one.
// When this returns OFX_OK the arena holds the whole layout, and only then does a pack call enqueue anything against those pointers.
// An arena that is large enough is reused, so a re-pack leaves every pointer where it was (captured graphs, the training loop).
static int place(ofx_handle* h, Arena& A, size_t (*layout)(ofx_handle&, Arena&)) {
    Arena count;
    TRY(A.reserve(layout(*h, count)));
    layout(*h, A);
    return OFX_OK;
}

extern "C" int ofx_pack_outfit_weights(ofx_handle* h, const void* const* P, int n, ofx_stream stream) {
    OFX_REQUIRE(h, OFX_EINVAL, "pack_outfit: NULL handle");
    const ofx_model_desc& d = h->d;
    OFX_REQUIRE(n == 5 + 12 * d.n_layers, OFX_EINVAL, "pack_outfit: expected %d tensors, got %d", 5 + 12 * d.n_layers, n);
    for (int i = 0; i < n; ++i) OFX_REQUIRE(P[i], OFX_EINVAL, "pack_outfit: tensor %d is NULL", i);
    hipStream_t s = (hipStream_t)stream;
    const size_t D = d.d_model, F = d.d_ffn, Fp = h->ot_ffn_pad;
    Arena& A = h->a_out;
    h->out_ready = false;                           // until the walk below has placed the pointers and the fill is enqueued
    TRY(place(h, A, layout_outfit));
    const bool zero_pad = A.fresh;                  // padding written once per allocation
    CopyBatch copies;
    const int dt = h->ot_dtype, mode = pack_rows_mode(h->ot_form);
    const bool both = h->ot_form == W_PLAIN;        // single-product precisions: a layer weight's row-major copy and its W^T come out of ONE pass
    TRY(copy_f32(h->outfit_token, P[0], D, s)); TRY(copy_f32(h->tgt_img_emb, P[1], D / 2, s));
    TRY(copy_f32(h->cp_w, P[2], D, s)); TRY(copy_f32(h->cp_b, P[3], 1, s));
    TRY(ofx_launch_pack_rows((const float*)P[4], h->cir.w, D, D, D, D, D, mode, dt, s));
    if (h->cir.wt) TRY(ofx_launch_transpose_cast((const float*)P[4], h->cir.wt, (int)D, (int)D, (int)D, dt, s));
    for (int l = 0; l < d.n_layers; ++l) {
        const void* const* q = P + 5 + 12 * l;
        OutfitLayer& L = h->ol[l];
        if (!both) TRY(ofx_launch_pack_rows((const float*)q[0], L.in.w, 3 * D, 3 * D, D, D, D, mode, dt, s));
        TRY(copy_f32(L.in.bias, q[1], 3 * D, s));
        if (!both) TRY(ofx_launch_pack_rows((const float*)q[2], L.out.w, D, D, D, D, D, mode, dt, s));
        TRY(copy_f32(L.out.bias, q[3], D, s));
        if (!both) TRY(ofx_launch_pack_rows((const float*)q[4], L.l1.w, F, Fp, D, D, D, mode, dt, s));
        else if (zero_pad) OFX_HIP(hipMemsetAsync(L.l1.w, 0, 2 * Fp * D, s));                       // rows F.. stay zero
        if (zero_pad) OFX_HIP(hipMemsetAsync(L.l1.bias, 0, Fp * 4, s));
        TRY(copy_f32(L.l1.bias, q[5], F, s));
        if (!both) TRY(ofx_launch_pack_rows((const float*)q[6], L.l2.w, D, D, F, Fp, F, mode, dt, s));
        else if (zero_pad) OFX_HIP(hipMemsetAsync(L.l2.w, 0, 2 * D * Fp, s));                       // columns F.. stay zero
        TRY(copy_f32(L.l2.bias, q[7], D, s));
        TRY(copy_f32(L.g1, q[8], D, s)); TRY(copy_f32(L.be1, q[9], D, s));
        TRY(copy_f32(L.g2, q[10], D, s)); TRY(copy_f32(L.be2, q[11], D, s));
        if (both) {         // W^T copies for the backward dgrad GEMMs: [K_w, N_w] operand, zero padded
            TRY(ofx_launch_transpose_cast((const float*)q[0], L.in.wt, (int)(3 * D), (int)D, (int)(3 * D), dt, s, L.in.w, (int)D));
            TRY(ofx_launch_transpose_cast((const float*)q[2], L.out.wt, (int)D, (int)D, (int)D, dt, s, L.out.w, (int)D));
            if (zero_pad) OFX_HIP(hipMemsetAsync(L.l1.wt, 0, 2 * D * Fp, s));      // [D, Fp], columns F.. stay zero
            TRY(ofx_launch_transpose_cast((const float*)q[4], L.l1.wt, (int)F, (int)D, (int)Fp, dt, s, L.l1.w, (int)D));
            if (zero_pad) OFX_HIP(hipMemsetAsync(L.l2.wt, 0, 2 * Fp * D, s));      // [Fp, D], rows F.. stay zero
            TRY(ofx_launch_transpose_cast((const float*)q[6], L.l2.wt, (int)D, (int)F, (int)D, dt, s, L.l2.w, (int)Fp));
        }
    }
    TRY(copies.flush(s));
    A.fresh = false;
    h->out_ready = true;
    return OFX_OK;
}

// fp8 copy of a split weight's lo halves, where the layout gave the record one
static int pack_f8(const PackedGemm& c, size_t N, size_t K, hipStream_t s) {
    return c.f8.w8 ? ofx_launch_pack_lo8(c.w, c.f8.w8, c.f8.s8, (int)N, (int)K, s) : OFX_OK;
}
// Fills the one copy of a tower GEMM that its launch reads, in the record's form.  `q` points at the 16 per-layer tensors in HF order:
// k.w,k.b,v.w,v.b,q.w,q.b,out.w,out.b,ln1.w,ln1.b,fc1.w,fc1.b,fc2.w,fc2.b,ln2.w,ln2.b; `blocks` lists the weights (their biases follow
// them) stacked as row blocks of Nb rows each (q | k | v: {4, 0, 2}).  A record with column sums is folded (plain or split): the
// LayerNorm whose gamma / beta sit at q[ln], q[ln + 1] goes into the weight.
static int pack_clip_gemm(const PackedGemm& c, const void* const* q, std::initializer_list<int> blocks, size_t Nb, size_t K, int ln, int dt, hipStream_t s) {
    const size_t km = w_kmul(c.form);
    char* w = (char*)c.w;
    size_t r = 0;
    for (int i : blocks) {
        const float* src = (const float*)q[i];
        if (c.col_sum)
            TRY(ofx_launch_fold_pack(src, (const float*)q[ln], (const float*)q[ln + 1], (const float*)q[i + 1], w + 2 * km * r * K, c.col_sum + r, c.bias + r,
                                     (int)Nb, (int)K, dt, s, c.form == W_SPLIT));
        else {
            TRY(ofx_launch_pack_rows(src, w + 2 * km * r * K, (int)Nb, (int)Nb, (int)K, (int)K, (int)K, pack_rows_mode(c.form), dt, s));
            TRY(copy_f32(c.bias + r, q[i + 1], Nb, s));
        }
        r += Nb;
    }
    return pack_f8(c, r, K, s);       // one [N, K] matrix: q | k | v row blocks
}
static int pack_clip_layer(const ClipLayer& L, const void* const* q, size_t W, size_t MLP, int dt, hipStream_t s) {
    TRY(pack_clip_gemm(L.qkv, q, {4, 0, 2}, W, W, 8, dt, s));
    TRY(pack_clip_gemm(L.o, q, {6}, W, W, -1, dt, s));
    TRY(pack_clip_gemm(L.fc1, q, {10}, MLP, W, 14, dt, s));
    TRY(pack_clip_gemm(L.fc2, q, {12}, W, MLP, -1, dt, s));
    TRY(copy_f32(L.g1, q[8], W, s)); TRY(copy_f32(L.be1, q[9], W, s));
    TRY(copy_f32(L.g2, q[14], W, s)); TRY(copy_f32(L.be2, q[15], W, s));
    return OFX_OK;
}

extern "C" int ofx_pack_vision_weights(ofx_handle* h, const void* const* P, int n, ofx_stream stream) {
    OFX_REQUIRE(h, OFX_EINVAL, "pack_vision: NULL handle");
    const ofx_model_desc& d = h->d;
    OFX_REQUIRE(n == 5 + 16 * d.vit_layers + 3, OFX_EINVAL, "pack_vision: expected %d tensors, got %d", 8 + 16 * d.vit_layers, n);
    for (int i = 0; i < n; ++i) OFX_REQUIRE(P[i], OFX_EINVAL, "pack_vision: tensor %d is NULL", i);
    hipStream_t s = (hipStream_t)stream;
    const size_t W = d.vit_width, MLP = d.vit_mlp, KP = 3 * (size_t)d.vit_patch * d.vit_patch, g = d.vit_image / d.vit_patch, S = g * g + 1, PD = d.proj_dim;
    const int dt = h->tw_dtype;
    h->vis_ready = false;
    TRY(place(h, h->a_vis, layout_vision));
    CopyBatch copies;
    TRY(copy_f32(h->v_cls, P[0], W, s));
    TRY(ofx_launch_pack_rows((const float*)P[1], h->v_patch.w, W, W, KP, KP, KP, pack_rows_mode(h->v_patch.form), dt, s));
    TRY(pack_f8(h->v_patch, W, KP, s));
    TRY(copy_f32(h->v_pos, P[2], S * W, s)); TRY(copy_f32(h->v_pre_g, P[3], W, s)); TRY(copy_f32(h->v_pre_b, P[4], W, s));
    for (int l = 0; l < d.vit_layers; ++l) TRY(pack_clip_layer(h->vl[l], P + 5 + 16 * l, W, MLP, dt, s));
    const void* const* t = P + 5 + 16 * d.vit_layers;
    TRY(copy_f32(h->v_post_g, t[0], W, s)); TRY(copy_f32(h->v_post_b, t[1], W, s));
    TRY(ofx_launch_pack_rows((const float*)t[2], h->v_proj.w, PD, PD, W, W, W, pack_rows_mode(h->v_proj.form), dt, s));
    TRY(copies.flush(s));
    h->vis_ready = true;
    return OFX_OK;
}

extern "C" int ofx_pack_text_weights(ofx_handle* h, const void* const* P, int n, ofx_stream stream) {
    OFX_REQUIRE(h, OFX_EINVAL, "pack_text: NULL handle");
    const ofx_model_desc& d = h->d;
    OFX_REQUIRE(n == 2 + 16 * d.txt_layers + 3, OFX_EINVAL, "pack_text: expected %d tensors, got %d", 5 + 16 * d.txt_layers, n);
    for (int i = 0; i < n; ++i) OFX_REQUIRE(P[i], OFX_EINVAL, "pack_text: tensor %d is NULL", i);
    hipStream_t s = (hipStream_t)stream;
    const size_t W = d.txt_width, MLP = d.txt_mlp, V = d.txt_vocab, NP = d.txt_max_pos, PD = d.proj_dim;
    const int dt = h->tw_dtype;
    h->txt_ready = false;
    TRY(place(h, h->a_txt, layout_text));
    CopyBatch copies;
    TRY(copy_f32(h->t_tok, P[0], V * W, s)); TRY(copy_f32(h->t_pos, P[1], NP * W, s));
    for (int l = 0; l < d.txt_layers; ++l) TRY(pack_clip_layer(h->tl[l], P + 2 + 16 * l, W, MLP, dt, s));
    const void* const* t = P + 2 + 16 * d.txt_layers;
    TRY(copy_f32(h->t_fin_g, t[0], W, s)); TRY(copy_f32(h->t_fin_b, t[1], W, s));
    TRY(ofx_launch_pack_rows((const float*)t[2], h->t_proj.w, PD, PD, W, W, W, pack_rows_mode(h->t_proj.form), dt, s));
    TRY(copies.flush(s));
    h->txt_ready = true;
    return OFX_OK;
}

// ------------------------------------------------------------------------------------- workspace
namespace {
struct SetWs { int* cu; float* X; char* H; float* QKV; char* U; char* HP; char* UP; char* slab; size_t slab_bytes; };
size_t carve_set(const ofx_handle* h, Bump& b, int B, int L, SetWs* w) {
    const size_t M = (size_t)B * (L + 1), D = h->d.d_model, km = a_kmul(h->ot_form), Fp = h->ot_ffn_pad, wk = w_kmul(h->ot_form);
    SetWs t;
    t.cu = b.take<int>(B + 1);
    t.X = b.take<float>(M * D);
    t.H = b.take<char>(M * km * D * 2);
    t.QKV = b.take<float>(M * 3 * D);
    t.U = b.take<char>(M * km * Fp * 2);
    t.HP = b.take<char>((size_t)B * km * D * 2);   // last layer: prefix rows only
    t.UP = b.take<char>((size_t)B * km * Fp * 2);
    // split-K scratch for the under-filled GEMMs of small batches (largest need over the shapes used)
    t.slab_bytes = 0;
    for (int m : {(int)M, B}) {
        t.slab_bytes = std::max(t.slab_bytes, ofx_gemm_splitk_bytes(m, 3 * (int)D, (int)(wk * D)));
        t.slab_bytes = std::max(t.slab_bytes, ofx_gemm_splitk_bytes(m, (int)D, (int)(wk * D)));
        t.slab_bytes = std::max(t.slab_bytes, ofx_gemm_splitk_bytes(m, (int)Fp, (int)(wk * D)));
        t.slab_bytes = std::max(t.slab_bytes, ofx_gemm_splitk_bytes(m, (int)D, (int)(wk * Fp)));
    }
    t.slab = b.take<char>(t.slab_bytes);
    if (w) *w = t;
    return b.off;
}
struct ClipWs { float* X; char* H; char* QKV; char* U; int* idx; char* PL; float* E; float* XP; char* HP; char* UP; char* slab; size_t slab_bytes;
                char* XB; float* P; float* S; char* XLO; };   // LayerNorm folding: the (hi, lo) residual stream XB / XLO, per-segment partial stats, (mean, rstd)
// km = 3: the three-product towers keep their GEMM operands K-concatenated ([hi | lo | hi] rows of 3 W / 3 MLP elements), their residual
// stream in the fp32 X; the folded towers (km = 1) keep it in XB / XLO.  x: the fp32 rows X are carved for the folded tower too (the text
// embedding writes them).  A buffer a tower does not use stays null.
// kk = K multiplier of the pooled-row GEMMs' split-K plans (2 with split weights, 3 in three-product mode)
size_t carve_clip(Bump& b, size_t rows, size_t n, size_t W, size_t MLP, size_t PD, size_t u_min_bytes, size_t qkv_min_bytes, ClipWs* w, size_t km, size_t kk, bool x) {
    ClipWs t{};
    if (km == 3 || x) t.X = b.take<float>(rows * W);
    t.H = b.take<char>(rows * km * W * 2);
    t.QKV = b.take<char>(std::max(rows * 3 * W * (km == 3 ? 4 : 2), qkv_min_bytes));      // three-product towers keep q | k | v in fp32
    t.U = b.take<char>(std::max(rows * km * MLP * 2, u_min_bytes));
    t.idx = b.take<int>(n);
    t.PL = b.take<char>(n * 3 * W * 2);   // pooled LayerNorm output, [hi | lo | hi] when the projection runs three products
    t.E = b.take<float>(n * PD);
    t.XP = b.take<float>(n * W);          // last layer runs on the pooled rows only
    t.HP = b.take<char>(n * km * W * 2);
    t.UP = b.take<char>(n * km * MLP * 2);
    t.slab_bytes = 0;
    for (size_t k : {(size_t)1, kk, (size_t)3})
        t.slab_bytes = std::max(std::max(std::max(ofx_gemm_splitk_bytes((int)n, (int)W, (int)(k * W)), ofx_gemm_splitk_bytes((int)n, (int)MLP, (int)(k * W))),
                                         std::max(ofx_gemm_splitk_bytes((int)n, (int)W, (int)(k * MLP)), ofx_gemm_splitk_bytes((int)n, (int)PD, (int)(k * W)))), t.slab_bytes);
    t.slab = b.take<char>(t.slab_bytes);
    if (km != 3) {
        t.XB = b.take<char>(rows * W * 2);
        t.P = b.take<float>(rows * (W / 64) * 2);
        t.S = b.take<float>(rows * 2);
        t.XLO = b.take<char>(rows * W * 2);
    }
    if (w) *w = t;
    return b.off;
}
size_t vit_bytes(const ofx_handle* h, int n, ClipWs* w, void* ws, size_t cap) {
    const ofx_model_desc& d = h->d;
    const size_t g = d.vit_image / d.vit_patch, S = g * g + 1, KP = 3 * (size_t)d.vit_patch * d.vit_patch;
    Bump b(ws, cap);
    // the patch matrix aliases U and the fp32 patch-GEMM output aliases QKV (both dead before the layers start)
    size_t r = carve_clip(b, (size_t)n * S, n, d.vit_width, d.vit_mlp, d.proj_dim, (size_t)n * g * g * KP * 2, (size_t)n * g * g * d.vit_width * 4, w, h->vit_x3 ? 3 : 1, h->vit_x3 ? 3 : 2, false);
    return align_up(r, 256);
}
size_t txt_bytes(const ofx_handle* h, int n, int Tc, ClipWs* w, void* ws, size_t cap) {
    const ofx_model_desc& d = h->d;
    Bump b(ws, cap);
    size_t r = carve_clip(b, (size_t)n * Tc, n, d.txt_width, d.txt_mlp, d.proj_dim, 0, 0, w, h->txt_x3 ? 3 : 1, h->txt_x3 ? 3 : (h->txt_w2_mask ? 2 : 1), true);
    return align_up(r, 256);
}
constexpr int VIT_CHUNK_MAX = 2048;
}  // namespace

extern "C" size_t ofx_workspace_bytes(ofx_handle* h, int op, int n, int len) {
    if (!h || n <= 0) return 0;
    switch (op) {
        case OFX_OP_SET_ENCODER: { Bump b(nullptr, ~(size_t)0); return align_up(carve_set(h, b, n, len, nullptr), 256); }
        case OFX_OP_VIT: return vit_bytes(h, std::min(n, VIT_CHUNK_MAX), nullptr, nullptr, ~(size_t)0);
        case OFX_OP_TEXT: return txt_bytes(h, n, len, nullptr, nullptr, ~(size_t)0);
        case OFX_OP_TOPK: return ofx_l2_topk_ws(n, len);
        default: return 0;
    }
}

// --------------------------------------------------------------------------- outfit transformer
// The set input in either form: a padded [B, L, D] tensor + mask, or (indexed / varlen) item rows of a device-resident table.
int g_set_fuse = 3;          // ofx_tune(10, v): bit 0 / bit 1 = small-batch outfit transformer lets the consumers do the split-K second passes (attention sums q | k | v slabs, reduce + LayerNorm in one launch)
int g_train_mfma_attn = 1;   // ofx_tune(7, v): single-product precisions (training; scoring in bf16 / f16) use the MFMA varlen attention (1) or the fp32 set kernels (0)

struct SetInput {
    const float* x = nullptr; const uint8_t* pad_mask = nullptr;                                   // dense
    const float* table = nullptr; int ld = 0; long long n_table = 0; const int* item_index = nullptr; const int* cu_items = nullptr;   // indexed
};
static SetInput dense_set(const float* x, const uint8_t* pad_mask) { SetInput in; in.x = x; in.pad_mask = pad_mask; return in; }
static SetInput indexed_set(const float* table, int ld, long long n_table, const int* item_index, const int* cu_items) {
    SetInput in; in.table = table; in.ld = ld; in.n_table = n_table; in.item_index = item_index; in.cu_items = cu_items;
    return in;
}
static int build_set(const ofx_handle* h, const SetInput& in, const float* prefix, int prefix_stride, int* cu, float* X, int B, int L, hipStream_t s) {
    const int D = h->d.d_model;
    if (in.table) return ofx_launch_set_build_indexed(in.table, in.ld, in.n_table, in.item_index, in.cu_items, prefix, prefix_stride, cu, X, B, D, s);
    return ofx_launch_set_build(in.x, in.pad_mask, prefix, prefix_stride, cu, X, B, L, D, s);
}
static int set_encoder_core(ofx_handle* h, const SetInput& in, const float* prefix, int prefix_stride, int B, int L, float* out_row0, void* ws,
                            size_t ws_bytes, hipStream_t s);
// softmax scale of the outfit transformer, 1 / sqrt(head_dim): 0.125f exactly at heads of 64
static float set_attn_scale(const ofx_model_desc& d) { return 1.0f / sqrtf((float)(d.d_model / d.n_head)); }
// The training step (MFMA attention forward and backward, ofx_layernorm_bwd) exists for heads of 64 and the widths layernorm_bwd takes;
// every training entry point asks before it launches anything.
static bool ln_bwd_d_ok(int D);
static bool train_shape_ok(const ofx_model_desc& d) { return d.d_model == d.n_head * 64 && ln_bwd_d_ok(d.d_model); }
#define OFX_REQUIRE_TRAIN_SHAPE(h, who) \
    OFX_REQUIRE(!(h) || train_shape_ok((h)->d), OFX_ESHAPE, who ": training needs heads of 64 and d_model in {512, 768, 1024} (d_model=%d, n_head=%d scores only)", (h)->d.d_model, (h)->d.n_head)

extern "C" int ofx_set_encoder_fwd(ofx_handle* h, const float* x, const uint8_t* pad_mask, const float* prefix,
                                   int prefix_stride, int B, int L, float* out_row0, void* ws, size_t ws_bytes,
                                   ofx_stream stream) {
    OFX_REQUIRE(h && h->out_ready, OFX_ESTATE, "set_encoder_fwd: outfit weights not packed");
    OFX_REQUIRE(B > 0 && L >= 0 && L <= 63, OFX_ESHAPE, "set_encoder_fwd: B=%d L=%d (L must be in [0,63])", B, L);
    OFX_REQUIRE((x || L == 0) && (pad_mask || L == 0) && out_row0 && ws, OFX_EINVAL, "set_encoder_fwd: NULL argument");
    return set_encoder_core(h, dense_set(x, pad_mask), prefix, prefix_stride, B, L, out_row0, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int ofx_set_encoder_fwd_indexed(ofx_handle* h, const float* table, int ld, long long n_table, const int* item_index, const int* cu_items,
                                           const float* prefix, int prefix_stride, int B, int max_len, float* out_row0, void* ws, size_t ws_bytes,
                                           ofx_stream stream) {
    OFX_REQUIRE(h && h->out_ready, OFX_ESTATE, "set_encoder_fwd_indexed: outfit weights not packed");
    OFX_REQUIRE(B > 0 && max_len >= 0 && max_len <= 63, OFX_ESHAPE, "set_encoder_fwd_indexed: B=%d max_len=%d (must be in [0,63])", B, max_len);
    OFX_REQUIRE(table && item_index && cu_items && out_row0 && ws && n_table > 0, OFX_EINVAL, "set_encoder_fwd_indexed: NULL argument");
    return set_encoder_core(h, indexed_set(table, ld, n_table, item_index, cu_items), prefix, prefix_stride, B, max_len, out_row0, ws, ws_bytes, (hipStream_t)stream);
}
static int set_encoder_core(ofx_handle* h, const SetInput& in, const float* prefix, int prefix_stride, int B, int L, float* out_row0, void* ws,
                            size_t ws_bytes, hipStream_t s) {
    const ofx_model_desc& d = h->d;
    Bump bump(ws, ws_bytes);
    SetWs w;
    carve_set(h, bump, B, L, &w);
    OFX_REQUIRE(bump.ok, OFX_EWORKSPACE, "set_encoder_fwd: workspace %zu < %zu bytes", ws_bytes, bump.off);
    const int D = d.d_model, km = a_kmul(h->ot_form), Fp = h->ot_ffn_pad, dt = h->ot_dtype, M = B * (L + 1);
    const int okind = km == 3 ? OFX_OUT_SPLIT3 : OFX_OUT_OP;
    const float scale = set_attn_scale(d);
    auto slab_gemm = [&](const PackedGemm& c, int K) { GemmArgs g{}; use_gemm(g, c, K); g.slab = w.slab; g.slab_bytes = w.slab_bytes; return g; };
    if (!prefix) { prefix = h->outfit_token; prefix_stride = 0; }
    TRY(build_set(h, in, prefix, prefix_stride, w.cu, w.X, B, L, s));
    const int* m_dev = w.cu + B;
    // Small batches (split-K plans): the GEMMs' second passes ride on their consumers - the set attention sums the q | k | v slabs,
    // the out-proj / linear2 reduce also emits the LayerNorm that follows it - 8 launches per layer instead of 11 (g_set_fuse)
    const bool fuse_att = (g_set_fuse & 1) != 0 && L + 1 <= 32, fuse = (g_set_fuse & 2) != 0;      // (the attention kernel sums split-K slabs for sets of <= 32 rows)
    bool ln1_done = false;                              // layer l's norm1 output already written by layer l-1's linear2 reduce
    for (int l = 0; l < d.n_layers; ++l) {
        const OutfitLayer& Ly = h->ol[l];
        const bool last = l + 1 == d.n_layers;          // only row 0 of every outfit feeds the heads (outfit_x.py:142,170)
        if (!ln1_done) {
            LnArgs ln{w.X, nullptr, Ly.g1, Ly.be1, w.H, M, D, km * D, okind, d.ln_eps};
            TRY(ofx_launch_layernorm_dev(ln, m_dev, dt, s));
        }
        ln1_done = false;
        GemmArgs g1 = slab_gemm(Ly.in, D);
        g1.A = w.H; g1.C = w.QKV; g1.m_dev = m_dev; g1.M = M; g1.N = 3 * D; g1.ldc = 3 * D;
        // single-product precisions: q|k|v stay in the operand type and the varlen MFMA attention runs (as in the training forward);
        // bf16x3 keeps fp32 q|k|v and the fp32 set attention (1e-5 parity)
        // (heads of 96 have no MFMA attention: their single-product precisions take the fp32 set attention too)
        const bool mfma_attn = h->ot_form == W_PLAIN && g_train_mfma_attn && D == d.n_head * 64;       // f16w2 keeps fp32 q | k | v and the fp32 set attention, as bf16x3 does
        g1.out_kind = mfma_attn ? OFX_OUT_OP : OFX_OUT_F32;
        int qkv_splits = 1;
        if (fuse_att && !mfma_attn) g1.defer_splits = &qkv_splits;
        TRY(ofx_launch_gemm(g1, dt, s));
        if (mfma_attn) {
            AttnArgs at{w.QKV, w.H, nullptr, B, L + 1, d.n_head, 3 * D, D, D, 2 * D, 0, 0, scale};
            at.cu_seqlens = w.cu; at.only_row0 = last ? 1 : 0;
            TRY(ofx_launch_attention_mfma(at, dt, s));
        } else {
            SetAttnArgs sa{w.QKV, w.H, w.cu, B, d.n_head, D, km * D, okind, L + 1, last ? 1 : 0, scale};
            if (qkv_splits > 1) { sa.qkv = w.slab; sa.splits = qkv_splits; sa.plane = (size_t)M * 3 * D; sa.bias = g1.bias; }
            TRY(ofx_launch_set_attention(sa, dt, s));
        }
        float* X = w.X; char* H = w.H; char* U = w.U; int Ml = M; const int* md = m_dev;
        if (last) {
            TRY(ofx_launch_gather_rows(w.H, w.cu, w.HP, B, km * D * 2, km * D * 2, s));
            TRY(ofx_launch_gather_rows(w.X, w.cu, out_row0, B, D * 4, D * 4, s));
            X = out_row0; H = w.HP; U = w.UP; Ml = B; md = nullptr;
        }
        GemmArgs g2 = slab_gemm(Ly.out, D);
        g2.A = H; g2.C = X; g2.resid = X; g2.m_dev = md; g2.M = Ml; g2.N = D; g2.ldc = D; g2.ldr = D; g2.out_kind = OFX_OUT_F32;
        bool ln2_done = false;
        if (fuse) { g2.ln_gamma = Ly.g2; g2.ln_beta = Ly.be2; g2.ln_out = H; g2.ln_ld = km * D; g2.ln_kind = okind; g2.ln_eps = d.ln_eps; g2.ln_done = &ln2_done; }
        TRY(ofx_launch_gemm(g2, dt, s));
        if (!ln2_done) {
            LnArgs ln2{X, nullptr, Ly.g2, Ly.be2, H, Ml, D, km * D, okind, d.ln_eps};
            TRY(ofx_launch_layernorm_dev(ln2, md, dt, s));
        }
        GemmArgs g3 = slab_gemm(Ly.l1, D);
        g3.A = H; g3.C = U; g3.m_dev = md; g3.M = Ml; g3.N = Fp; g3.ldc = km * Fp; g3.act = d.outfit_act; g3.out_kind = okind;
        TRY(ofx_launch_gemm(g3, dt, s));
        GemmArgs g4 = slab_gemm(Ly.l2, Fp);
        g4.A = U; g4.C = X; g4.resid = X; g4.m_dev = md; g4.M = Ml; g4.N = D; g4.ldc = D; g4.ldr = D; g4.out_kind = OFX_OUT_F32;
        if (fuse && !last) {                            // ... and the next layer's norm1
            const OutfitLayer& Nx = h->ol[l + 1];
            g4.ln_gamma = Nx.g1; g4.ln_beta = Nx.be1; g4.ln_out = w.H; g4.ln_ld = km * D; g4.ln_kind = okind; g4.ln_eps = d.ln_eps; g4.ln_done = &ln1_done;
        }
        TRY(ofx_launch_gemm(g4, dt, s));
    }
    return OFX_OK;
}

extern "C" int ofx_cp_head(ofx_handle* h, const float* row0, int B, float* logits, ofx_stream stream) {
    OFX_REQUIRE(h && h->out_ready, OFX_ESTATE, "cp_head: outfit weights not packed");
    OFX_REQUIRE(row0 && logits && B > 0, OFX_EINVAL, "cp_head: bad argument");
    return ofx_launch_cp_head(row0, h->cp_w, h->cp_b, logits, B, h->d.d_model, (hipStream_t)stream);
}

extern "C" int ofx_cir_head(ofx_handle* h, const float* row0, int B, float* emb, void* ws, size_t ws_bytes, ofx_stream stream) {
    OFX_REQUIRE(h && h->out_ready, OFX_ESTATE, "cir_head: outfit weights not packed");
    OFX_REQUIRE(row0 && emb && B > 0 && ws, OFX_EINVAL, "cir_head: bad argument");
    const int D = h->d.d_model, km = a_kmul(h->ot_form);
    OFX_REQUIRE(ws_bytes >= (size_t)B * km * D * 2, OFX_EWORKSPACE, "cir_head: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    TRY(ofx_launch_pack_rows(row0, ws, B, B, D, D, D, km == 3 ? 1 : 0, h->ot_dtype, s));
    GemmArgs g{};
    use_cir_head(g, *h);
    g.A = ws; g.C = emb; g.M = B; g.N = D; g.ldc = D; g.out_kind = OFX_OUT_F32;
    return ofx_launch_gemm(g, h->ot_dtype, s);
}

extern "C" int ofx_cir_prefix(ofx_handle* h, const float* txt, int B, float* out, ofx_stream stream) {
    OFX_REQUIRE(h && h->out_ready, OFX_ESTATE, "cir_prefix: outfit weights not packed");
    OFX_REQUIRE(txt && out && B > 0, OFX_EINVAL, "cir_prefix: bad argument");
    return ofx_launch_cir_prefix(h->tgt_img_emb, txt, out, B, h->d.d_model, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------ CLIP towers
// One CLIP encoder layer on `rows` rows.  When `pool_idx` is given (last layer) everything after the attention
// runs only on the n pooled rows (CLS / EOS): they are the only ones the tower's output depends on.
int g_fuse_qkv = 1;     // ofx_tune(9, v): bit 0 (default on) = ViT layers with single-product q | k | v weights run the fused QKV-projection + attention kernel
                        // (q | k | v stay in LDS); bit 1 (default OFF) = so do layers with split (hi, lo) weights, through its dual-weight variant: level with the
                        // persistent GEMM + attention-kernel pair in time, same error distribution, but on the 100-seed sweep it re-rolls two borderline small-logit weight draws from 8.0e-4 /
                        // 8.9e-4 to 1.05e-3 / 1.12e-3, so the default scheme keeps the dual-weight GEMM + attention-kernel pair
int g_fuse_qkv_w2f8 = 1;     // ofx_tune(22, v): 1 (default) = ViT layers with split q | k | v weights and their fp8 pair run the fused kernel's fp8-correction variant wherever the
                            // plan would run the qkv GEMM as gemm_w2f8_kernel (>= 256 tiles): the same instruction sequence per accumulator, hence the same bits as the pair;
                            // 0 = the GEMM + attention-kernel pair.  A knob of its own: knob 9 keeps its two bits
int g_x3_vit_f32_attn = 0;   // ofx_tune(20, v), experiment: 1 = the three-product ViT keeps q | k | v in fp32 and runs the fp32 set attention (as the text tower does) instead of
                            // the MFMA attention on operand-rounded q | k | v - what the attention core's operand rounding costs under peaked attention
int g_prune_q = 1;      // ofx_tune(8, v): 1 = the ViT's last layer computes queries for the CLS rows only

// One CLIP encoder layer with its LayerNorms folded into the GEMM epilogues.  On entry w.XB / w.XLO hold the residual stream as an
// operand-type (hi, lo) pair and w.S the (mean, rstd) of its rows; the out-proj / fc2 epilogues add into the pair in place and leave
// per-segment statistics for the next folded consumer, so no LayerNorm kernel runs on the full rows.  The pooled last layer
// (`pool_idx`) gathers the pooled rows into the fp32 w.XP and runs its tail there, LayerNorm 2 materialised.
static int clip_layer(const ClipLayer& L, const ClipWs& w, int rows, int nseq, int S, int W, int MLP, int heads, int act,
                      float eps, int causal, const int64_t* key_mask, int mask_ld, int dt, const int* pool_idx, hipStream_t s, bool pool_first) {
    // fused QKV projection + attention (non-pooled ViT layers: one 33..64-token tile per sequence, no mask): q | k | v never reach HBM;
    // split q | k | v weights: its dual-weight variant (ofx_tune(9, 3)), else the dual-weight GEMM + the attention kernel
    const bool fits = !pool_idx && !causal && !key_mask && S >= 33 && S <= 64 && (256 / S - 1) * S + 64 - 256 <= 16;   // (the kernel's key-row overshoot fits its 16 pad rows)
    const bool fused = (g_fuse_qkv & (L.qkv.form == W_SPLIT ? 2 : 1)) && fits;
    GemmArgs g1{}; g1.A = w.XB; g1.C = w.QKV; g1.row_stat = w.S; g1.M = rows; g1.N = 3 * W;
    g1.ldc = 3 * W; g1.act = OFX_ACT_NONE; g1.out_kind = OFX_OUT_OP;
    use_gemm(g1, L.qkv, W);
    // split weights with their fp8 pair, where the plan would run this call's qkv GEMM as gemm_w2f8_kernel: the fused kernel's variant with the
    // same correction product - q | k | v, and with them the layer's output, keep the bits of the GEMM + attention pair
    const bool fused8 = !fused && g_fuse_qkv_w2f8 && fits && L.qkv.form == W_SPLIT && L.qkv.f8.w8 && L.qkv.f8.s8 && dt == OFX_F16 && W % 128 == 0 &&
                        ofx_gemm_plan_kind(g1, dt) == GEMM_W2F8;
    if (fused8) {
        TRY(ofx_launch_fused_qkv_attn(w.XB, L.qkv.w, L.qkv.bias, w.S, L.qkv.col_sum, w.H, nseq, S, W, heads, W, W, 0.125f, dt, s, FUSED_QKV_W2F8, L.qkv.f8.w8, L.qkv.f8.s8));
    } else if (fused) {
        TRY(ofx_launch_fused_qkv_attn(w.XB, L.qkv.w, L.qkv.bias, w.S, L.qkv.col_sum, w.H, nseq, S, W, heads, W, W, 0.125f, dt, s, L.qkv.form == W_SPLIT ? FUSED_QKV_W2 : FUSED_QKV_PLAIN));
    } else {
        const bool prune = pool_idx && pool_first && g_prune_q;
        if (prune) {
            // last layer, pooled row = first row of every sequence (ViT CLS): only those rows' queries are ever used.  K | V for all
            // rows (weight rows W .. 3W), then Q for the nseq pooled rows through strided A / C / statistics.  The other rows' Q
            // columns keep stale workspace bytes; their attention outputs are never read (the tail gathers the pooled rows only).
            GemmArgs kv = g1;
            kv.W = (const char*)g1.W + (size_t)W * g1.K * 2; kv.bias = g1.bias + W; kv.col_sum = g1.col_sum + W; kv.C = (char*)w.QKV + (size_t)W * 2; kv.N = 2 * W;
            if (g1.W8) { kv.W8 = (const char*)g1.W8 + (size_t)W * W; kv.w8_scale = (const char*)g1.w8_scale + W; }      // weight rows W .. 3W: fp8 rows of W bytes, scale bytes 128 per 128-row block
            TRY(ofx_launch_gemm(kv, dt, s));
            GemmArgs q = g1;
            q.M = nseq; q.N = W; q.lda = S * W; q.ldc = S * 3 * W; q.stat_ld = S;
            TRY(ofx_launch_gemm(q, dt, s));
        } else
            TRY(ofx_launch_gemm(g1, dt, s));
        AttnArgs at{w.QKV, w.H, key_mask, nseq, S, heads, 3 * W, W, W, 2 * W, mask_ld, causal, 0.125f};
        at.only_row0 = prune ? 1 : 0;       // pruned last layer of the ViT: only the CLS query row is read afterwards
        TRY(ofx_launch_attention_mfma(at, dt, s));
    }
    char* H = w.H; char* U = w.U; int M = rows;
    if (pool_idx) {
        TRY(ofx_launch_gather_rows(w.H, pool_idx, w.HP, nseq, W * 2, W * 2, s));
        TRY(ofx_launch_gather_hilo(w.XB, w.XLO, pool_idx, w.XP, nseq, W, dt, s));
        H = w.HP; U = w.UP; M = nseq;
    }
    // out-proj and fc2 add into the residual stream: the (hi, lo) pair in place, or the pooled fp32 rows
    auto to_stream = [&](GemmArgs& g) {
        g.M = M; g.N = W; g.ldc = W; g.ldr = W; g.act = OFX_ACT_NONE;
        if (pool_idx) { g.C = w.XP; g.resid = w.XP; g.out_kind = OFX_OUT_F32; g.slab = w.slab; g.slab_bytes = w.slab_bytes; }
        else { g.C = w.XB; g.xb_out = w.XB; g.xlo = w.XLO; g.stat_part = w.P; g.out_kind = OFX_OUT_OP; }
    };
    GemmArgs g2{}; g2.A = H;
    use_gemm(g2, L.o, W); to_stream(g2);
    TRY(ofx_launch_gemm(g2, dt, s));
    GemmArgs g3{}; g3.C = U; g3.M = M; g3.N = MLP; g3.ldc = MLP; g3.act = act; g3.out_kind = OFX_OUT_OP;
    if (pool_idx) {
        LnArgs ln2{w.XP, nullptr, L.g2, L.be2, H, M, W, W, OFX_OUT_OP, eps};
        TRY(ofx_launch_layernorm(ln2, dt, s));
        g3.A = H; g3.slab = w.slab; g3.slab_bytes = w.slab_bytes;
    } else {
        TRY(ofx_launch_stats_finalize(w.P, W / 64, W, eps, w.S, M, s));
        g3.A = w.XB; g3.row_stat = w.S;
    }
    use_gemm(g3, L.fc1, W);
    TRY(ofx_launch_gemm(g3, dt, s));
    GemmArgs g4{}; g4.A = U;
    use_gemm(g4, L.fc2, MLP); to_stream(g4);
    TRY(ofx_launch_gemm(g4, dt, s));
    if (!pool_idx) TRY(ofx_launch_stats_finalize(w.P, W / 64, W, eps, w.S, M, s));
    return OFX_OK;
}

// Three-product layer (hi*hi + lo*hi + hi*lo as ONE K-concatenated GEMM, K' = 3K): fp32 residual stream, materialised LayerNorms
// writing [hi | lo | hi] rows, weights packed [hi | hi | lo] (the outfit transformer's bf16x3 scheme in the towers' operand type).
// q | k | v leave the projection rounded once to the operand type for the MFMA attention, whose output is again (hi, lo).
static int clip_layer_x3(const ClipLayer& L, const ClipWs& w, int rows, int nseq, int S, int W, int MLP, int heads, int act,
                         float eps, int causal, const int64_t* key_mask, int mask_ld, int dt, const int* pool_idx, hipStream_t s, bool mfma_attn = false,
                         int shared_first = 0) {
    LnArgs ln{w.X, nullptr, L.g1, L.be1, w.H, rows, W, 3 * W, OFX_OUT_SPLIT3, eps};
    TRY(ofx_launch_layernorm(ln, dt, s));
    GemmArgs g1{}; g1.A = w.H; g1.C = w.QKV; g1.M = rows; g1.N = 3 * W;
    use_gemm(g1, L.qkv, W);
    // q | k | v stay fp32 and the attention runs in fp32 arithmetic (the outfit transformer's set kernel with HF's causal AND
    // key-padding mask, up to 64 rows per sequence): rounding q, k, v, P to the operand type alone leaves 3.5e-4 at the text embedding
    // (tests/studies/operand_scheme_cpu.py); the MFMA attention stays as the fallback beyond 64 rows (never reached by the text tower:
    // ofx_clip_text_fwd caps the computed tokens at 64; a three-product ViT-B/16, 197 rows, asks for it by mfma_attn anyway)
    // (the ViT in its three-product mode keeps the MFMA attention: 2,048 images x 12 heads of 50 tokens in fp32 VALU arithmetic would
    // cost more than the layer's GEMMs, and the attention core's operand rounding is the smallest term of its budget, 6e-5)
    const bool f32_attn = S <= 64 && !mfma_attn;
    // shared_first (text tower): `rows` = 1 + nseq * (S - 1) in the shared-first-row map; only the attention knows (everything else is row-wise)
    OFX_REQUIRE(!shared_first || f32_attn, OFX_EINVAL, "clip_layer_x3: a shared first row needs the fp32 set attention");
    g1.ldc = 3 * W; g1.act = OFX_ACT_NONE; g1.out_kind = f32_attn ? OFX_OUT_F32 : OFX_OUT_OP;
    TRY(ofx_launch_gemm(g1, dt, s));
    if (f32_attn) {
        SetAttnArgs sa{w.QKV, w.H, nullptr, nseq, heads, W, 3 * W, OFX_OUT_SPLIT3, S, 0, 0.125f};
        sa.fixed_len = S; sa.causal = causal; sa.key_mask = key_mask; sa.mask_ld = mask_ld; sa.shared_first = shared_first;
        TRY(ofx_launch_set_attention(sa, dt, s));
    } else {
        AttnArgs at{w.QKV, w.H, key_mask, nseq, S, heads, 3 * W, 3 * W, W, 2 * W, mask_ld, causal, 0.125f};
        at.split3_w = W;
        TRY(ofx_launch_attention_mfma(at, dt, s));
    }
    float* X = w.X; char* H = w.H; char* U = w.U; int M = rows;
    if (pool_idx) {
        TRY(ofx_launch_gather_rows(w.H, pool_idx, w.HP, nseq, 3 * W * 2, 3 * W * 2, s));
        TRY(ofx_launch_gather_rows(w.X, pool_idx, w.XP, nseq, W * 4, W * 4, s));
        X = w.XP; H = w.HP; U = w.UP; M = nseq;
    }
    GemmArgs g2{}; g2.A = H; g2.C = X; g2.resid = X; g2.M = M; g2.N = W; g2.ldc = W; g2.ldr = W; g2.act = OFX_ACT_NONE; g2.out_kind = OFX_OUT_F32;
    use_gemm(g2, L.o, W);
    if (pool_idx) { g2.slab = w.slab; g2.slab_bytes = w.slab_bytes; }          // the split-K scratch is sized for the pooled rows
    TRY(ofx_launch_gemm(g2, dt, s));
    LnArgs ln2{X, nullptr, L.g2, L.be2, H, M, W, 3 * W, OFX_OUT_SPLIT3, eps};
    TRY(ofx_launch_layernorm(ln2, dt, s));
    GemmArgs g3{}; g3.A = H; g3.C = U; g3.M = M; g3.N = MLP; g3.ldc = 3 * MLP; g3.act = act; g3.out_kind = OFX_OUT_SPLIT3;
    use_gemm(g3, L.fc1, W);
    if (pool_idx) { g3.slab = w.slab; g3.slab_bytes = w.slab_bytes; }
    TRY(ofx_launch_gemm(g3, dt, s));
    GemmArgs g4{}; g4.A = U; g4.C = X; g4.resid = X; g4.M = M; g4.N = W; g4.ldc = W; g4.ldr = W; g4.act = OFX_ACT_NONE; g4.out_kind = OFX_OUT_F32;
    use_gemm(g4, L.fc2, MLP);
    if (pool_idx) { g4.slab = w.slab; g4.slab_bytes = w.slab_bytes; }
    return ofx_launch_gemm(g4, dt, s);
}

// All layers; the pooled rows end up compacted in w.XP [nseq, W].  On entry the residual stream sits in w.X (x3) or, with its row
// statistics, in w.XB / w.XLO / w.S.
static int clip_layers(const std::vector<ClipLayer>& Ls, const ClipWs& w, int rows, int nseq, int S, int W, int MLP,
                       int heads, int act, float eps, int causal, const int64_t* key_mask, int mask_ld, int dt,
                       const int* pool_idx, hipStream_t s, bool pool_first, bool x3, int shared_first = 0) {
    OFX_REQUIRE(!shared_first || x3, OFX_EINVAL, "clip_layers: a shared first row exists in the three-product path only");
    if (x3) {
        for (size_t l = 0; l < Ls.size(); ++l)
            TRY(clip_layer_x3(Ls[l], w, rows, nseq, S, W, MLP, heads, act, eps, causal, key_mask, mask_ld, dt, l + 1 == Ls.size() ? pool_idx : nullptr, s, !causal && !key_mask && !g_x3_vit_f32_attn,
                              shared_first));
        return OFX_OK;
    }
    for (size_t l = 0; l < Ls.size(); ++l)
        TRY(clip_layer(Ls[l], w, rows, nseq, S, W, MLP, heads, act, eps, causal, key_mask, mask_ld, dt,
                       l + 1 == Ls.size() ? pool_idx : nullptr, s, pool_first));
    return OFX_OK;
}

// Raw decoded images for the fused preprocess -> patch-embedding route (ofx_vit_b32_fwd_u8)
struct RawImages {
    const uint8_t* src; const long long* offsets; const int* heights; const int* widths; int channels; const float* mean; const float* stdv;
    void* ws; size_t ws_bytes;
};

static int vit_core(ofx_handle* h, const float* pixels, const RawImages* raw, int N, float* emb, int emb_ld, int emb_col,
                    int normalize, void* ws, size_t ws_bytes, ofx_stream stream) {
    OFX_REQUIRE(h && h->vis_ready, OFX_ESTATE, "vit_b32_fwd: vision weights not packed");
    OFX_REQUIRE((pixels || raw) && emb && ws && N > 0, OFX_EINVAL, "vit_b32_fwd: bad argument");
    const ofx_model_desc& d = h->d;
    OFX_REQUIRE(emb_ld >= emb_col + d.proj_dim && emb_ld % 4 == 0 && emb_col % 4 == 0, OFX_ESHAPE, "vit_b32_fwd: bad emb_ld/emb_col");
    hipStream_t s = (hipStream_t)stream;
    const int g = d.vit_image / d.vit_patch, S = g * g + 1, W = d.vit_width, KP = 3 * d.vit_patch * d.vit_patch, dt = h->tw_dtype;
    // largest chunk of images the workspace holds
    int chunk = std::min(N, VIT_CHUNK_MAX);
    while (chunk > 1 && vit_bytes(h, chunk, nullptr, nullptr, ~(size_t)0) > ws_bytes) chunk = (chunk + 1) / 2;
    OFX_REQUIRE(vit_bytes(h, chunk, nullptr, nullptr, ~(size_t)0) <= ws_bytes, OFX_EWORKSPACE, "vit_b32_fwd: workspace %zu bytes cannot hold one image", ws_bytes);
    const size_t px_per_img = (size_t)3 * d.vit_image * d.vit_image;
    for (int n0 = 0; n0 < N; n0 += chunk) {
        const int n = std::min(chunk, N - n0);
        ClipWs w;
        vit_bytes(h, n, &w, ws, ws_bytes);
        const int rows = n * S;
        if (raw)      // resample + normalise straight into the GEMM operand: no fp32 pixel tensor, no patchify pass
            TRY(ofx_preprocess_to(raw->src, raw->offsets + n0, raw->heights + n0, raw->widths + n0, n, raw->channels, d.vit_image, raw->mean, raw->stdv,
                                  nullptr, w.U, d.vit_patch, dt, raw->ws, raw->ws_bytes, s));
        else
            TRY(ofx_launch_patchify(pixels + (size_t)n0 * px_per_img, w.U, n, d.vit_image, d.vit_patch, dt, s));
        GemmArgs gp{}; gp.A = w.U; gp.C = w.QKV; gp.M = n * g * g; gp.N = W; gp.ldc = W;
        gp.act = OFX_ACT_NONE; gp.out_kind = OFX_OUT_F32;
        use_gemm(gp, h->v_patch, KP);
        TRY(ofx_launch_gemm(gp, dt, s));
        // the pre-LN kernel writes the stream the layers start from: X (three-product ViT), or the (hi, lo) pair + row statistics
        // (the carve leaves the other form's buffers null)
        TRY(ofx_launch_vit_embed_ln((const float*)w.QKV, h->v_cls, h->v_pos, h->v_pre_g, h->v_pre_b, w.X, n, S, W, d.ln_eps, s, w.XB, w.S, dt, w.XLO));
        TRY(ofx_launch_iota_rows(w.idx, n, S, s));                        // CLS rows
        TRY(clip_layers(h->vl, w, rows, n, S, W, d.vit_mlp, d.vit_heads, d.vit_act, d.ln_eps, 0, nullptr, 0, dt, w.idx, s, true, h->vit_x3 != 0));
        const int pk = h->proj_x3 ? 3 : 1;            // the output tail in three products: post-LayerNorm rows [hi | lo | hi] x [hi | hi | lo]
        LnArgs ln{w.XP, nullptr, h->v_post_g, h->v_post_b, w.PL, n, W, pk * W, pk == 3 ? OFX_OUT_SPLIT3 : OFX_OUT_OP, d.ln_eps};
        TRY(ofx_launch_layernorm(ln, dt, s));
        GemmArgs gj{}; gj.A = w.PL; gj.C = w.E; gj.M = n; gj.N = d.proj_dim; gj.ldc = d.proj_dim;
        use_gemm(gj, h->v_proj, W);
        gj.act = OFX_ACT_NONE; gj.out_kind = OFX_OUT_F32; gj.slab = w.slab; gj.slab_bytes = w.slab_bytes;
        TRY(ofx_launch_gemm(gj, dt, s));
        TRY(ofx_launch_l2norm_store(w.E, emb + (size_t)n0 * emb_ld, n, d.proj_dim, emb_ld, emb_col, normalize, s));
    }
    return OFX_OK;
}

extern "C" int ofx_vit_b32_fwd(ofx_handle* h, const float* pixels, int N, float* emb, int emb_ld, int emb_col,
                               int normalize, void* ws, size_t ws_bytes, ofx_stream stream) {
    OFX_REQUIRE(pixels, OFX_EINVAL, "vit_b32_fwd: pixels is NULL");
    return vit_core(h, pixels, nullptr, N, emb, emb_ld, emb_col, normalize, ws, ws_bytes, stream);
}

extern "C" size_t ofx_vit_b32_u8_ws_bytes(ofx_handle* h, const int* heights, const int* widths, int N, int channels) {
    if (!h || N <= 0) return 0;
    const size_t pre = ofx_clip_preprocess_ws(heights, widths, N, channels, h->d.vit_image);
    return pre ? align_up(pre, 256) + vit_bytes(h, std::min(N, VIT_CHUNK_MAX), nullptr, nullptr, ~(size_t)0) : 0;
}

extern "C" int ofx_vit_b32_fwd_u8(ofx_handle* h, const uint8_t* src, const long long* offsets, const int* heights, const int* widths, int N, int channels,
                                  const float* mean, const float* stdv, float* emb, int emb_ld, int emb_col, int normalize, void* ws, size_t ws_bytes,
                                  ofx_stream stream) {
    OFX_REQUIRE(h && src && offsets && heights && widths && mean && stdv && N > 0, OFX_EINVAL, "vit_b32_fwd_u8: bad argument");
    const size_t pre = align_up(ofx_clip_preprocess_ws(heights, widths, N, channels, h->d.vit_image), 256);
    OFX_REQUIRE(pre > 0 && pre < ws_bytes, OFX_EWORKSPACE, "vit_b32_fwd_u8: workspace %zu bytes, the preprocessor alone needs %zu", ws_bytes, pre);
    RawImages raw{src, offsets, heights, widths, channels, mean, stdv, ws, pre};       // [preprocess scratch | ViT workspace]
    return vit_core(h, nullptr, &raw, N, emb, emb_ld, emb_col, normalize, (char*)ws + pre, ws_bytes - pre, stream);
}

int g_text_shared_first = 1;      // ofx_tune(21, v): 1 (default) ofx_clip_text_fwd_shared computes the texts' common first-position row once, 0 = it runs the full rows

// shared_first: the caller vouches that every text starts with the same token and no text masks position 0.  The text tower is causal, so
// position 0 sees itself only and carries the same bits for every text in every layer: the three-product path then computes it once.  Row 0
// is that row, position t >= 1 of text i is row 1 + i * (Tc - 1) + (t - 1), rows = 1 + N * (Tc - 1) instead of N * Tc; the LayerNorms, GEMMs
// and gathers are row-wise and only see fewer rows, the embedding, the EOS index and the attention know the map.  Same bits as the full rows
// wherever the GEMMs' summation order does not depend on M (no split-K plan on the full rows: every batch beyond a few texts).
static int clip_text_core(ofx_handle* h, const int64_t* ids, const int64_t* attn_mask, const int* lengths_host,
                          int N, int T, float* emb, int emb_ld, int emb_col, int normalize, int shared_first, void* ws,
                          size_t ws_bytes, ofx_stream stream) {
    OFX_REQUIRE(h && h->txt_ready, OFX_ESTATE, "clip_text_fwd: text weights not packed");
    OFX_REQUIRE(ids && emb && ws && N > 0 && T > 0, OFX_EINVAL, "clip_text_fwd: bad argument");
    const ofx_model_desc& d = h->d;
    OFX_REQUIRE(T <= d.txt_max_pos, OFX_ESHAPE, "clip_text_fwd: T=%d exceeds max_position_embeddings=%d", T, d.txt_max_pos);
    OFX_REQUIRE(emb_ld >= emb_col + d.proj_dim && emb_ld % 4 == 0 && emb_col % 4 == 0, OFX_ESHAPE, "clip_text_fwd: bad emb_ld/emb_col");
    int Tc = T;
    if (lengths_host) {
        Tc = 1;
        for (int i = 0; i < N; ++i) Tc = std::max(Tc, std::min(lengths_host[i], T));
    }
    OFX_REQUIRE(Tc <= 64, OFX_ESHAPE, "clip_text_fwd: %d tokens per text exceed the 64-token attention tile", Tc);
    hipStream_t s = (hipStream_t)stream;
    ClipWs w;
    const size_t need = txt_bytes(h, N, Tc, &w, ws, ws_bytes);
    OFX_REQUIRE(need <= ws_bytes, OFX_EWORKSPACE, "clip_text_fwd: workspace %zu < %zu bytes", ws_bytes, need);
    const bool x3 = h->txt_x3 != 0, x3p = x3 || h->proj_x3;
    // (the single-product / MFMA-attention path keeps the full rows; one token per text has no other rows to share with)
    const int sf = shared_first && g_text_shared_first && x3 && Tc >= 2 ? 1 : 0;
    const int W = d.txt_width, dt = h->tw_dtype, rows = sf ? 1 + N * (Tc - 1) : N * Tc;        // fewer rows in the same workspace
    TRY(ofx_launch_text_embed(ids, h->t_tok, h->t_pos, w.X, N, T, Tc, W, d.txt_vocab, sf, s));
    TRY(ofx_launch_text_eos_index(ids, w.idx, N, T, Tc, d.txt_eos_id, sf, s));      // EOS rows
    const int pk = x3p ? 3 : 1;
    if (!x3) TRY(ofx_launch_row_stats_cast(w.X, w.XB, w.XLO, w.S, rows, W, d.ln_eps, dt, s));      // layer 0's (hi, lo) stream + LayerNorm-1 statistics
    TRY(clip_layers(h->tl, w, rows, N, Tc, W, d.txt_mlp, d.txt_heads, d.txt_act, d.ln_eps, 1, attn_mask, T, dt, w.idx, s, false, x3, sf));
    LnArgs ln{w.XP, nullptr, h->t_fin_g, h->t_fin_b, w.PL, N, W, pk * W, x3p ? OFX_OUT_SPLIT3 : OFX_OUT_OP, d.ln_eps};
    TRY(ofx_launch_layernorm(ln, dt, s));
    GemmArgs gj{}; gj.A = w.PL; gj.C = w.E; gj.M = N; gj.N = d.proj_dim; gj.ldc = d.proj_dim;
    use_gemm(gj, h->t_proj, W);
    gj.act = OFX_ACT_NONE; gj.out_kind = OFX_OUT_F32; gj.slab = w.slab; gj.slab_bytes = w.slab_bytes;
    TRY(ofx_launch_gemm(gj, dt, s));
    return ofx_launch_l2norm_store(w.E, emb, N, d.proj_dim, emb_ld, emb_col, normalize, s);
}

extern "C" int ofx_clip_text_fwd(ofx_handle* h, const int64_t* ids, const int64_t* attn_mask, const int* lengths_host,
                                 int N, int T, float* emb, int emb_ld, int emb_col, int normalize, void* ws,
                                 size_t ws_bytes, ofx_stream stream) {
    return clip_text_core(h, ids, attn_mask, lengths_host, N, T, emb, emb_ld, emb_col, normalize, 0, ws, ws_bytes, stream);
}
extern "C" int ofx_clip_text_fwd_shared(ofx_handle* h, const int64_t* ids, const int64_t* attn_mask, const int* lengths_host,
                                        int N, int T, float* emb, int emb_ld, int emb_col, int normalize, int shared_first, void* ws,
                                        size_t ws_bytes, ofx_stream stream) {
    return clip_text_core(h, ids, attn_mask, lengths_host, N, T, emb, emb_ld, emb_col, normalize, shared_first, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------- scoring
extern "C" int ofx_fitb_argmin(const float* y, const float* cand, int B, int C, int D, int64_t* idx, float* dist, ofx_stream stream) {
    OFX_REQUIRE(y && cand && idx && B > 0 && C > 0 && D > 0 && D % 4 == 0, OFX_EINVAL, "fitb_argmin: bad argument");
    return ofx_launch_fitb(y, cand, B, C, D, idx, dist, (hipStream_t)stream);
}
extern "C" int ofx_fitb_argmin_indexed(const float* table, int ld, long long n_table, const int* cand_index, const float* y_hat, int B, int C, int D,
                                       const int64_t* answer, int64_t* idx, float* dist, int* n_correct, ofx_stream stream) {
    OFX_REQUIRE(table && cand_index && y_hat && idx, OFX_EINVAL, "fitb_argmin_indexed: NULL argument");
    OFX_REQUIRE((answer != nullptr) == (n_correct != nullptr), OFX_EINVAL, "fitb_argmin_indexed: answer and n_correct go together");
    OFX_REQUIRE((((uintptr_t)table | (uintptr_t)y_hat) & 15) == 0, OFX_EINVAL, "fitb_argmin_indexed: table and y_hat must be 16-byte aligned");
    OFX_REQUIRE(B >= 1 && C >= 1 && D >= 4 && D % 4 == 0, OFX_ESHAPE, "fitb_argmin_indexed: B = %d, C = %d, D = %d; needs B >= 1, C >= 1, D %% 4 == 0, D >= 4",
                B, C, D);
    OFX_REQUIRE(ld >= D && ld % 4 == 0 && n_table >= 1 && n_table <= INT_MAX, OFX_ESHAPE,
                "fitb_argmin_indexed: ld = %d, n_table = %lld; needs ld >= D = %d, ld %% 4 == 0, 1 <= n_table <= INT_MAX", ld, n_table, D);
    return ofx_launch_fitb_indexed(table, ld, (int)n_table, cand_index, y_hat, B, C, D, answer, idx, dist, n_correct, (hipStream_t)stream);
}
extern "C" int ofx_l2_topk(ofx_handle*, const float* Q, const float* P, int nq, int np, int D, int k, int64_t index_base,
                           int64_t* idx, float* dist, void* ws, size_t ws_bytes, ofx_stream stream) {
    return ofx_launch_l2_topk(Q, P, nq, np, D, k, index_base, idx, dist, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int ofx_l2_topk_grouped(ofx_handle*, const float* Q, const float* P, int nq, int np, int D, int k, const int* panels, int n_panels,
                                   int max_group_rows, const int64_t* gt, int64_t* idx, float* dist, int* gt_pos, void* ws, size_t ws_bytes, ofx_stream stream) {
    return ofx_launch_l2_topk_grouped(Q, P, nq, np, D, k, panels, n_panels, max_group_rows, gt, idx, dist, gt_pos, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int ofx_topk_merge(const int64_t* idx_in, const float* dist_in, int parts, int nq, int k, int64_t* idx, float* dist, ofx_stream stream) {
    return ofx_launch_topk_merge(idx_in, dist_in, parts, nq, k, idx, dist, (hipStream_t)stream);
}

// ====================================================================================== training step (N1)
// Forward with a tape + backward of the CP path on precomputed embeddings.  Single-product operand precisions only
// (bf16 / f16, like the reference's AMP training); dropout is NOT applied (the caller must use dropout = 0).
namespace {
struct TapeLayer { float* Xin; float* st1; char* H1; char* QKV; char* O; float* Xmid; float* st2; char* H2; float* Upre; char* A; };
struct Tape { int* cu; float* row0; float* prefix; char* row0b; char* pO; float* pX; std::vector<TapeLayer> L; size_t bytes; };
size_t carve_tape(const ofx_handle* h, Bump& b, int B, int Lq, Tape* t) {
    const size_t M = (size_t)B * (Lq + 1), D = h->d.d_model, Fp = h->ot_ffn_pad, Mp = align_up(M, 64);   // operand copies: rows readable up to Mp (TN GEMM)
    Tape tp;
    tp.cu = b.take<int>(B + 1);
    tp.row0 = b.take<float>((size_t)B * D);
    tp.prefix = b.take<float>((size_t)B * D);                              // CIR: per-outfit prefix [img_emb | target text]
    tp.row0b = b.take<char>(align_up((size_t)B, 64) * D * 2);             // CIR: operand copy of row0 (dW of cir_ffn)
    tp.pO = b.take<char>(align_up((size_t)B, 64) * D * 2);                // last layer: attention output of the prefix rows
    tp.pX = b.take<float>((size_t)B * D);                                 // last layer: layer input at the prefix rows (residual)
    tp.L.resize(h->d.n_layers);
    for (TapeLayer& l : tp.L) {
        l.Xin = b.take<float>(M * D); l.st1 = b.take<float>(M * 2); l.H1 = b.take<char>(Mp * D * 2); l.QKV = b.take<char>(M * 3 * D * 2);
        l.O = b.take<char>(Mp * D * 2); l.Xmid = b.take<float>(M * D); l.st2 = b.take<float>(M * 2); l.H2 = b.take<char>(Mp * D * 2);
        l.Upre = b.take<float>(M * Fp); l.A = b.take<char>(Mp * Fp * 2);
    }
    tp.bytes = align_up(b.off, 256);
    if (t) *t = tp;
    return tp.bytes;
}
struct BwdWs { float *dXa, *dXb_f, *dH, *dO, *part, *d_row0; char *gXb, *dU, *gQb, *dyb; int* rowmap; char* slab; size_t slab_bytes; };
size_t carve_bwd(const ofx_handle* h, Bump& b, int B, int Lq, BwdWs* w) {
    const size_t M = (size_t)B * (Lq + 1), D = h->d.d_model, Fp = h->ot_ffn_pad, Mp = align_up(M, 64);
    BwdWs t;
    t.dXa = b.take<float>(M * D); t.dXb_f = b.take<float>(M * D); t.dH = b.take<float>(M * D); t.dO = b.take<float>(M * D);
    t.part = b.take<float>(std::max(ofx_ln_bwd_part_floats((int)D), ofx_colsum_part_floats((int)(3 * D))));
    t.gXb = b.take<char>(Mp * D * 2); t.dU = b.take<char>(Mp * Fp * 2); t.gQb = b.take<char>(Mp * 3 * D * 2);
    t.d_row0 = b.take<float>((size_t)B * D); t.dyb = b.take<char>(align_up((size_t)B, 64) * D * 2);      // CIR head
    t.rowmap = b.take<int>(M);
    t.slab_bytes = 0;
    const int m = (int)M, Di = (int)D, Fi = (int)Fp;
    for (auto s : {ofx_gemm_tn_slab_bytes(Di, Di, B), ofx_gemm_splitk_bytes(B, Di, Di), ofx_gemm_tn_slab_bytes(Di, Fi, B), ofx_gemm_tn_slab_bytes(Fi, Di, B),
                   ofx_gemm_splitk_bytes(B, Fi, Di), ofx_gemm_splitk_bytes(B, Di, Fi),
                   ofx_gemm_tn_slab_bytes(Di, Fi, m), ofx_gemm_tn_slab_bytes(Fi, Di, m), ofx_gemm_tn_slab_bytes(Di, Di, m), ofx_gemm_tn_slab_bytes(3 * Di, Di, m),
                   ofx_gemm_splitk_bytes(m, Fi, Di), ofx_gemm_splitk_bytes(m, Di, Fi), ofx_gemm_splitk_bytes(m, Di, Di), ofx_gemm_splitk_bytes(m, Di, 3 * Di)})
        t.slab_bytes = std::max(t.slab_bytes, s);
    t.slab = b.take<char>(t.slab_bytes);
    if (w) *w = t;
    return align_up(b.off, 256);
}
// gradient buffer layout (floats), pack order, padded shapes: [outfit_token D][tgt_img D/2][cp_w D][cp_b 1][cir_w D*D] then per layer
// [Win 3D*D][bin 3D][Wo D*D][bo D][W1 Fp*D][b1 Fp][W2 D*Fp][b2 D][g1 D][be1 D][g2 D][be2 D]
void grad_offsets(const ofx_handle* h, std::vector<size_t>& off, size_t* total) {
    const size_t D = h->d.d_model, Fp = h->ot_ffn_pad;
    size_t o = 0;
    auto add = [&](size_t n) { off.push_back(o); o += (n + 63) / 64 * 64; };
    add(D); add(D / 2); add(D); add(1); add(D * D);
    for (int l = 0; l < h->d.n_layers; ++l) { add(3 * D * D); add(3 * D); add(D * D); add(D); add(Fp * D); add(Fp); add(D * Fp); add(D); add(D); add(D); add(D); add(D); }
    *total = o;
}
}  // namespace

extern "C" size_t ofx_cp_train_tape_bytes(ofx_handle* h, int B, int L) { Bump b(nullptr, ~(size_t)0); return h ? carve_tape(h, b, B, L, nullptr) : 0; }
extern "C" size_t ofx_cp_train_ws_bytes(ofx_handle* h, int B, int L) {
    if (!h) return 0;
    Bump b(nullptr, ~(size_t)0);
    const size_t bw = carve_bwd(h, b, B, L, nullptr);
    Bump f(nullptr, ~(size_t)0);
    return std::max(bw, align_up(carve_set(h, f, B, L, nullptr), 256));
}
extern "C" size_t ofx_cp_train_grad_floats(ofx_handle* h, size_t* offsets, int n) {
    if (!h) return 0;
    std::vector<size_t> off; size_t total;
    grad_offsets(h, off, &total);
    if (offsets) for (int i = 0; i < n && i < (int)off.size(); ++i) offsets[i] = off[i];
    return total;
}

// dropout sites: layer l -> 4l + {0 attention probabilities, 1 dropout1 (out_proj output), 2 FFN inner, 3 dropout2 (linear2 output)};
// 4 * n_layers = the head's Dropout (cp_ffn[0]).  torch: nn.TransformerEncoderLayer._sa_block / _ff_block, MultiheadAttention dropout.
// head: 0 = CP (logits [B,1] = Dropout(row0) . w + b), 1 = CIR (y [B,D] = row0 Wc^T; prefix = [target_item_image_emb | target text])
static int cp_train_fwd_core(ofx_handle* h, const SetInput& in, int B, int L, float* logits, void* tape_mem, size_t tape_bytes, void* ws,
                             size_t ws_bytes, float dropout_p, unsigned seed, hipStream_t s, int head = 0, const float* target_text = nullptr);
extern "C" int ofx_cp_train_fwd(ofx_handle* h, const float* x, const uint8_t* pad_mask, int B, int L, float* logits, void* tape_mem,
                                size_t tape_bytes, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream) {
    OFX_REQUIRE(B > 0 && L >= 0 && L <= 31 && (x || L == 0) && (pad_mask || L == 0) && logits && tape_mem, OFX_EINVAL, "cp_train_fwd: bad argument");
    return cp_train_fwd_core(h, dense_set(x, pad_mask), B, L, logits, tape_mem, tape_bytes, ws, ws_bytes, dropout_p, seed, (hipStream_t)stream);
}
extern "C" int ofx_cp_train_fwd_indexed(ofx_handle* h, const float* table, int ld, long long n_table, const int* item_index, const int* cu_items,
                                        int B, int max_len, float* logits, void* tape_mem, size_t tape_bytes, void* ws, size_t ws_bytes,
                                        float dropout_p, unsigned seed, ofx_stream stream) {
    OFX_REQUIRE(B > 0 && max_len >= 0 && max_len <= 31 && table && item_index && cu_items && logits && tape_mem && n_table > 0, OFX_EINVAL,
                "cp_train_fwd_indexed: bad argument");
    return cp_train_fwd_core(h, indexed_set(table, ld, n_table, item_index, cu_items), B, max_len, logits, tape_mem, tape_bytes, ws, ws_bytes, dropout_p, seed, (hipStream_t)stream);
}
extern "C" int ofx_cir_train_fwd(ofx_handle* h, const float* x, const uint8_t* pad_mask, const float* table, int ld, long long n_table,
                                 const int* item_index, const int* cu_items, const float* target_text, int B, int L, float* y, void* tape_mem,
                                 size_t tape_bytes, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream) {
    OFX_REQUIRE(B > 0 && L >= 0 && L <= 31 && target_text && y && tape_mem, OFX_EINVAL, "cir_train_fwd: bad argument");
    OFX_REQUIRE((x && pad_mask) || L == 0 || (table && item_index && cu_items && n_table > 0), OFX_EINVAL, "cir_train_fwd: give (x, pad_mask) or (table, item_index, cu_items)");
    const SetInput in = table ? indexed_set(table, ld, n_table, item_index, cu_items) : dense_set(x, pad_mask);
    return cp_train_fwd_core(h, in, B, L, y, tape_mem, tape_bytes, ws, ws_bytes, dropout_p, seed, (hipStream_t)stream, 1, target_text);
}
static int cp_train_fwd_core(ofx_handle* h, const SetInput& in, int B, int L, float* logits, void* tape_mem, size_t tape_bytes, void* ws,
                             size_t ws_bytes, float dropout_p, unsigned seed, hipStream_t s, int head, const float* target_text) {
    OFX_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, OFX_EINVAL, "cp_train_fwd: dropout_p=%g", dropout_p);
    OFX_REQUIRE_TRAIN_SHAPE(h, "cp_train_fwd");       // a width that scores only is refused whatever the handle's state
    OFX_REQUIRE(h && h->out_ready, OFX_ESTATE, "cp_train_fwd: outfit weights not packed");
    OFX_REQUIRE(h->ot_form == W_PLAIN, OFX_ESTATE, "cp_train_fwd: training uses a single-product precision (bf16 / f16), not bf16x3 / f16w2");
    const ofx_model_desc& d = h->d;
    Bump tb(tape_mem, tape_bytes);
    Tape T;
    carve_tape(h, tb, B, L, &T);
    OFX_REQUIRE(tb.ok, OFX_EWORKSPACE, "cp_train_fwd: tape %zu < %zu bytes", tape_bytes, T.bytes);
    Bump wb(ws, ws_bytes);
    SetWs w;
    carve_set(h, wb, B, L, &w);
    OFX_REQUIRE(wb.ok, OFX_EWORKSPACE, "cp_train_fwd: workspace too small");
    const int D = d.d_model, Fp = h->ot_ffn_pad, dt = h->ot_dtype, M = B * (L + 1);
    const float scale = set_attn_scale(d);
    auto slab_gemm = [&](const PackedGemm& c, int K) { GemmArgs g{}; use_gemm(g, c, K); g.slab = w.slab; g.slab_bytes = w.slab_bytes; return g; };
    if (head == 1) {
        TRY(ofx_launch_cir_prefix(h->tgt_img_emb, target_text, T.prefix, B, D, s));
        TRY(build_set(h, in, T.prefix, D, T.cu, T.L[0].Xin, B, L, s));
    } else {
        TRY(build_set(h, in, h->outfit_token, 0, T.cu, T.L[0].Xin, B, L, s));
    }
    const int* m_dev = T.cu + B;
    for (int l = 0; l < d.n_layers; ++l) {
        const OutfitLayer& Ly = h->ol[l];
        TapeLayer& t = T.L[l];
        const bool last = l + 1 == d.n_layers;
        LnArgs ln{t.Xin, nullptr, Ly.g1, Ly.be1, t.H1, M, D, D, OFX_OUT_OP, d.ln_eps}; ln.stats = t.st1;
        TRY(ofx_launch_layernorm_dev(ln, m_dev, dt, s));
        GemmArgs g1 = slab_gemm(Ly.in, D);
        g1.A = t.H1; g1.C = t.QKV; g1.m_dev = m_dev; g1.M = M; g1.N = 3 * D; g1.ldc = 3 * D; g1.out_kind = OFX_OUT_OP;      // q|k|v kept in the operand type
        TRY(ofx_launch_gemm(g1, dt, s));
        if (g_train_mfma_attn) {           // varlen MFMA attention on the operand-type q|k|v (probabilities rounded to the operand type, as autocast SDPA does)
            AttnArgs at{t.QKV, t.O, nullptr, B, L + 1, d.n_head, 3 * D, D, D, 2 * D, 0, 0, scale};
            at.cu_seqlens = T.cu; at.only_row0 = last ? 1 : 0; at.drop = make_drop(dropout_p, seed, 4 * l + 0);
            TRY(ofx_launch_attention_mfma(at, dt, s));
        } else {
            SetAttnArgs sa{t.QKV, t.O, T.cu, B, d.n_head, D, D, OFX_OUT_OP, L + 1, last ? 1 : 0, scale};
            sa.drop = make_drop(dropout_p, seed, 4 * l + 0); sa.qkv_op = 1;
            TRY(ofx_launch_set_attention(sa, dt, s));
        }
        // the rest of the layer: on the live rows, from the attention output and the layer input into the next layer's input
        int rows = M; const int* md = m_dev; const void* O = t.O; const float* Xin = t.Xin; float* Xout = last ? T.row0 : T.L[l + 1].Xin;
        if (last) {
            // Only the prefix row of every outfit feeds the heads (outfit_x.py:142,170): out-proj, LayerNorm-2 and the FFN of the last
            // layer run on those B rows (compacted: row b of the Xmid / st2 / H2 / Upre / A tape buffers; dropout rows = b).
            TRY(ofx_launch_gather_rows(t.O, T.cu, T.pO, B, D * 2, D * 2, s));
            TRY(ofx_launch_gather_rows(t.Xin, T.cu, T.pX, B, D * 4, D * 4, s));
            rows = B; md = nullptr; O = T.pO; Xin = T.pX;
        }
        GemmArgs g2 = slab_gemm(Ly.out, D);
        g2.A = O; g2.C = t.Xmid; g2.resid = Xin; g2.m_dev = md; g2.M = rows; g2.N = D; g2.ldc = D; g2.ldr = D; g2.out_kind = OFX_OUT_F32;
        g2.drop = make_drop(dropout_p, seed, 4 * l + 1);
        TRY(ofx_launch_gemm(g2, dt, s));
        LnArgs ln2{t.Xmid, nullptr, Ly.g2, Ly.be2, t.H2, rows, D, D, OFX_OUT_OP, d.ln_eps}; ln2.stats = t.st2;
        TRY(ofx_launch_layernorm_dev(ln2, md, dt, s));
        GemmArgs g3 = slab_gemm(Ly.l1, D);
        g3.A = t.H2; g3.C = t.A; g3.aux_out = t.Upre; g3.m_dev = md; g3.M = rows; g3.N = Fp; g3.ldc = Fp; g3.act = d.outfit_act; g3.out_kind = OFX_OUT_OP;
        g3.drop = make_drop(dropout_p, seed, 4 * l + 2);
        TRY(ofx_launch_gemm(g3, dt, s));
        GemmArgs g4 = slab_gemm(Ly.l2, Fp);
        g4.A = t.A; g4.C = Xout; g4.resid = t.Xmid; g4.m_dev = md; g4.M = rows; g4.N = D; g4.ldc = D; g4.ldr = D; g4.out_kind = OFX_OUT_F32;
        g4.drop = make_drop(dropout_p, seed, 4 * l + 3);
        TRY(ofx_launch_gemm(g4, dt, s));
    }
    if (head == 1) {                                                // cir_ffn = Linear(D, d_embed, bias=False): no dropout (outfit_x.py:61-63)
        TRY(ofx_launch_pack_rows(T.row0, T.row0b, B, B, D, D, D, 0, dt, s));
        GemmArgs g = slab_gemm(h->cir, D);
        g.A = T.row0b; g.C = logits; g.M = B; g.N = D; g.ldc = D; g.out_kind = OFX_OUT_F32;
        return ofx_launch_gemm(g, dt, s);
    }
    TRY(ofx_launch_drop_rows(T.row0, B, D, make_drop(dropout_p, seed, 4 * d.n_layers), s));     // the tape keeps the dropped-out rows
    return ofx_launch_cp_head(T.row0, h->cp_w, h->cp_b, logits, B, D, s);
}

// grads != NULL: one flat buffer in the library's padded layout (ofx_cp_train_grad_floats), overwritten.
// grad_ptrs != NULL: one destination per packed tensor in the PARAMETER's own shape (linear1 [F, D], linear2 [D, F], ...), NULL
// entries skipped; accumulate != 0 adds to what is there (p.grad of a torch parameter).
static int set_train_bwd_core(ofx_handle* h, void* tape_mem, size_t tape_bytes, const float* dlogits, int B, int L, float* grads,
                              size_t grad_floats, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream, int head,
                              float* const* grad_ptrs = nullptr, int accumulate = 0);
extern "C" int ofx_cp_train_bwd(ofx_handle* h, void* tape_mem, size_t tape_bytes, const float* dlogits, int B, int L, float* grads,
                                size_t grad_floats, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream) {
    return set_train_bwd_core(h, tape_mem, tape_bytes, dlogits, B, L, grads, grad_floats, ws, ws_bytes, dropout_p, seed, stream, 0);
}
extern "C" int ofx_cir_train_bwd(ofx_handle* h, void* tape_mem, size_t tape_bytes, const float* dy, int B, int L, float* grads,
                                 size_t grad_floats, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream) {
    return set_train_bwd_core(h, tape_mem, tape_bytes, dy, B, L, grads, grad_floats, ws, ws_bytes, dropout_p, seed, stream, 1);
}
extern "C" int ofx_cp_train_bwd_into(ofx_handle* h, void* tape_mem, size_t tape_bytes, const float* dlogits, int B, int L, float* const* grad_ptrs,
                                     int n_ptrs, int accumulate, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream) {
    OFX_REQUIRE(h && grad_ptrs && n_ptrs == 5 + 12 * h->d.n_layers, OFX_EINVAL, "cp_train_bwd_into: expected %d destinations", h ? 5 + 12 * h->d.n_layers : 0);
    return set_train_bwd_core(h, tape_mem, tape_bytes, dlogits, B, L, nullptr, 0, ws, ws_bytes, dropout_p, seed, stream, 0, grad_ptrs, accumulate);
}
extern "C" int ofx_cir_train_bwd_into(ofx_handle* h, void* tape_mem, size_t tape_bytes, const float* dy, int B, int L, float* const* grad_ptrs,
                                      int n_ptrs, int accumulate, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream) {
    OFX_REQUIRE(h && grad_ptrs && n_ptrs == 5 + 12 * h->d.n_layers, OFX_EINVAL, "cir_train_bwd_into: expected %d destinations", h ? 5 + 12 * h->d.n_layers : 0);
    return set_train_bwd_core(h, tape_mem, tape_bytes, dy, B, L, nullptr, 0, ws, ws_bytes, dropout_p, seed, stream, 1, grad_ptrs, accumulate);
}
extern "C" int ofx_train_arm_layer_events(ofx_handle* h, void* const* events, int n) {
    OFX_REQUIRE(h, OFX_EINVAL, "train_arm_layer_events: NULL handle");
    OFX_REQUIRE(n == 0 || (events && n == h->d.n_layers), OFX_EINVAL, "train_arm_layer_events: expected %d events (one per layer) or 0, got %d", h->d.n_layers, n);
    h->bwd_events.assign((hipEvent_t*)events, (hipEvent_t*)events + n);
    return OFX_OK;
}
static int set_train_bwd_core(ofx_handle* h, void* tape_mem, size_t tape_bytes, const float* dlogits, int B, int L, float* grads,
                              size_t grad_floats, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream, int head,
                              float* const* grad_ptrs, int accumulate) {
    // per-layer completion events (data-parallel overlap): consumed by this call whatever its outcome
    std::vector<hipEvent_t> layer_ev;
    if (h) layer_ev.swap(h->bwd_events);
    OFX_REQUIRE_TRAIN_SHAPE(h, "cp_train_bwd");
    OFX_REQUIRE(h && h->out_ready && h->ot_form == W_PLAIN, OFX_ESTATE, "cp_train_bwd: needs packed single-product weights");
    OFX_REQUIRE(tape_mem && dlogits && (grads || grad_ptrs) && ws && B > 0, OFX_EINVAL, "cp_train_bwd: bad argument");
    OFX_REQUIRE(h->d.outfit_act == OFX_ACT_MISH, OFX_ESTATE, "cp_train_bwd: only the Mish activation has a backward epilogue");
    const ofx_model_desc& d = h->d;
    hipStream_t s = (hipStream_t)stream;
    Bump tb(tape_mem, tape_bytes);
    Tape T;
    carve_tape(h, tb, B, L, &T);
    OFX_REQUIRE(tb.ok, OFX_EWORKSPACE, "cp_train_bwd: tape too small");
    Bump wb(ws, ws_bytes);
    BwdWs w;
    carve_bwd(h, wb, B, L, &w);
    OFX_REQUIRE(wb.ok, OFX_EWORKSPACE, "cp_train_bwd: workspace %zu < %zu bytes", ws_bytes, wb.off);
    std::vector<size_t> off; size_t total;
    grad_offsets(h, off, &total);
    OFX_REQUIRE(grad_ptrs || grad_floats >= total, OFX_EWORKSPACE, "cp_train_bwd: gradient buffer %zu < %zu floats", grad_floats, total);
    const int D = d.d_model, Fp = h->ot_ffn_pad, dt = h->ot_dtype, M = B * (L + 1), F = d.d_ffn;
    const int* m_dev = T.cu + B;
    const int acc = grad_ptrs ? accumulate : 0;
    // destination of packed tensor i; in the per-parameter form the FFN tensors have their real (unpadded) extents
    auto G = [&](int i) -> float* { return grad_ptrs ? grad_ptrs[i] : grads + off[i]; };
    const int Fv = grad_ptrs ? F : Fp;                 // valid rows of dW1 / entries of db1 / columns of dW2
    auto site = [&](int l, int k) { return make_drop(dropout_p, seed, 4 * l + k); };
    const DropArgs nodrop;
    // Both GEMMs of the backward run on (rows, md) = (M, m_dev), the pad-free live rows, or (B, nullptr), the compacted prefix rows of
    // the pruned last layer.
    // wgrad: dW[n_w, k_w] = dY[rows, n_w]^T X[rows, k_w], contraction over the rows -> out[:mv, :nv] (row pitch ldc): the per-parameter
    // form stores only the real FFN extent
    auto wgrad = [&](int rows, const int* md, const void* dY, int n_w, const void* X, int k_w, float* out, int ldc = 0, int mv = 0, int nv = 0) {
        return ofx_launch_gemm_tn(dY, n_w, X, k_w, out, ldc ? ldc : k_w, n_w, k_w, rows, md, w.slab, w.slab_bytes, dt, s, mv, nv, acc);
    };
    // dgrad: C[rows, n] = epilogue(dY[rows, k] Wt[n, k]^T), Wt the record's W^T operand copy: a plain weight, no bias
    auto dgrad = [&](int rows, const int* md, const void* dY, const PackedGemm& rec, void* C, int n, int k, int out_kind = OFX_OUT_F32, int act = OFX_ACT_NONE,
                     const float* resid = nullptr, const DropArgs& drop = DropArgs()) {
        PackedGemm wt; wt.w = rec.wt;
        GemmArgs g{}; use_gemm(g, wt, k); g.slab = w.slab; g.slab_bytes = w.slab_bytes;
        g.A = dY; g.C = C; g.M = rows; g.N = n; g.ldc = n; g.out_kind = out_kind; g.act = act; g.resid = resid; g.ldr = resid ? n : 0; g.m_dev = md; g.drop = drop;
        return ofx_launch_gemm(g, dt, s);
    };
    const auto attention_bwd = g_train_mfma_attn ? ofx_launch_set_attention_bwd_mfma : ofx_launch_set_attention_bwd;
    float* dX = w.dXa; float* dX2 = w.dXb_f;
    const int lastl = d.n_layers - 1;
    // ---- heads -> d row0 [B, D] (fp32, w.d_row0) and its operand copy times the last layer's dropout2 mask (w.gXb rows 0..B)
    if (head == 1) {
        // y = row0 Wc^T:  dWc = dy^T row0 (TN GEMM over the B rows), d row0 = dy Wc
        TRY(ofx_launch_pack_rows(dlogits, w.dyb, B, B, D, D, D, 0, dt, s));
        TRY(wgrad(B, nullptr, w.dyb, D, T.row0b, D, G(4)));
        TRY(dgrad(B, nullptr, w.dyb, h->cir, w.d_row0, D, D));
        TRY(ofx_launch_cp_head_bwd(nullptr, w.d_row0, nullptr, w.d_row0, w.gXb, nullptr, B, D, dt, nodrop, site(lastl, 3), s));
    } else {
        TRY(ofx_launch_cp_head_bwd(dlogits, h->cp_w, nullptr, w.d_row0, w.gXb, G(3), B, D, dt, site(d.n_layers, 0), site(lastl, 3), s, acc));
        TRY(ofx_launch_colsum(T.row0, 0, D, nullptr, dlogits, G(2), nullptr, nullptr, D, w.part, D, nullptr, B, dt, s, 0, acc));             // d cp_w = sum_b dlogit_b (row0_b . m_head)
    }
    TRY(ofx_launch_row_map(T.cu, w.rowmap, B, M, s));
    for (int l = lastl; l >= 0; --l) {
        const OutfitLayer& Ly = h->ol[l];
        const TapeLayer& t = T.L[l];
        const int g0 = 5 + 12 * l;                    // Win, bin, Wo, bo, W1, b1, W2, b2, g1, be1, g2, be2
        // The last layer's FFN, LayerNorm-2 and out-proj only saw the B prefix rows (compacted, static count): its upstream gradient is
        // the heads' d row0, and dXmid flows back into the full rows through the row map.  Below it, every row is live.
        const bool last = l == lastl;
        const int rows = last ? B : M;
        const int* md = last ? nullptr : m_dev;
        const void* O = last ? T.pO : t.O;
        const float* dXout = last ? w.d_row0 : dX;
        // ---- FFN branch: Xout = Xmid + mish(H2 W1^T + b1) W2^T + b2        (gXb = operand copy of dXout)
        if (last) TRY(ofx_launch_colsum(w.gXb, 1, D, nullptr, nullptr, G(g0 + 7), nullptr, nullptr, D, w.part, D, nullptr, B, dt, s, 0, acc));   // db2: no layer above supplies it
        TRY(wgrad(rows, md, w.gXb, D, t.A, Fp, G(g0 + 6), Fv, D, Fv));                                                                 // dW2 [D, Fp]
        TRY(dgrad(rows, md, w.gXb, Ly.l2, w.dU, Fp, D, OFX_OUT_OP, OFX_ACT_MISH_GRAD, t.Upre, site(l, 2)));                          // dU = (dXout W2) * mish'(Upre)
        TRY(ofx_launch_colsum(w.dU, 1, Fp, nullptr, nullptr, G(g0 + 5), nullptr, nullptr, Fp, w.part, Fp, md, rows, dt, s, Fv, acc));    // db1
        TRY(wgrad(rows, md, w.dU, Fp, t.H2, D, G(g0 + 4), D, Fv, D));                                                                  // dW1 [Fp, D]
        TRY(dgrad(rows, md, w.dU, Ly.l1, w.dH, D, Fp));                                                                             // dH2
        TRY(ofx_launch_ln_bwd(w.dH, t.Xmid, t.st2, Ly.g2, dXout, nullptr, dX2, w.gXb, G(g0 + 10), G(g0 + 11), G(g0 + 3), w.part, D, md, rows, dt, site(l, 1), s, acc));   // dXmid (+ dbo)
        // ---- attention branch: Xmid = Xin + O Wo^T + bo
        TRY(wgrad(rows, md, w.gXb, D, O, D, G(g0 + 2)));                                                                               // dWo [D, D]
        TRY(dgrad(rows, md, w.gXb, Ly.out, w.dO, D, D));                                                                           // dO
        TRY(attention_bwd(t.QKV, w.dO, w.gQb, T.cu, B, d.n_head, D, L + 1, set_attn_scale(d), dt, site(l, 0), last ? 1 : 0, s));                  // (last layer: only row 0 has a dO, all rows get dK, dV)
        TRY(ofx_launch_colsum(w.gQb, 1, 3 * D, nullptr, nullptr, G(g0 + 1), nullptr, nullptr, 3 * D, w.part, 3 * D, m_dev, M, dt, s, 0, acc));   // dbin
        TRY(wgrad(M, m_dev, w.gQb, 3 * D, t.H1, D, G(g0 + 0)));                                                                        // dWin [3D, D]
        TRY(dgrad(M, m_dev, w.gQb, Ly.in, w.dH, D, 3 * D));                                                                        // dH1
        // dXin = LayerNorm-1 backward + dXmid (last layer: at the prefix rows); its column sums are the bias gradient of the layer
        // below's linear2
        TRY(ofx_launch_ln_bwd(w.dH, t.Xin, t.st1, Ly.g1, dX2, last ? w.rowmap : nullptr, dX, w.gXb, G(g0 + 8), G(g0 + 9), l > 0 ? G(g0 - 12 + 7) : nullptr, w.part, D,
                              m_dev, M, dt, l > 0 ? site(l - 1, 3) : nodrop, s, acc));
        // all 12 gradient tensors of layer l are final: its linear2 bias gradient came from the LayerNorm-1 backward of layer l + 1, or,
        // for the last layer, from the head path above.  A data-parallel host may start reducing them now
        if (!layer_ev.empty()) OFX_HIP(hipEventRecord(layer_ev[l], s));
    }
    // CIR: the prefix is [target_item_image_emb | text]: d target_item_image_emb = sum_b dX0[cu[b]][:D/2]
    if (head == 1) return ofx_launch_colsum(dX, 0, D, T.cu, nullptr, G(1), nullptr, nullptr, D / 2, w.part, D / 2, nullptr, B, dt, s, 0, acc);
    // shared prefix token: d outfit_token = sum_b dX0[cu[b]]
    return ofx_launch_colsum(dX, 0, D, T.cu, nullptr, G(0), nullptr, nullptr, D, w.part, D, nullptr, B, dt, s, 0, acc);
}

// mask * 1/(1-p) of a dropout site as the kernels compute it (tests build a torch reference with the same masks)
extern "C" int ofx_dropout_mask(float dropout_p, unsigned seed, int site, int rows, int cols, float* out, ofx_stream stream) {
    OFX_REQUIRE(out && rows > 0 && cols > 0 && dropout_p >= 0.f && dropout_p < 1.f, OFX_EINVAL, "dropout_mask: bad argument");
    hipStream_t s = (hipStream_t)stream;
    TRY(ofx_launch_fill_f32(out, (size_t)rows * cols, 1.0f, s));
    return ofx_launch_drop_rows(out, rows, cols, make_drop(dropout_p, seed, (unsigned)site), s);
}

extern "C" int ofx_focal_loss(const float* logits, const float* labels, int B, float alpha, float gamma, float upstream, float* loss, float* dlogits,
                              ofx_stream stream) {
    OFX_REQUIRE(logits && labels && B > 0, OFX_EINVAL, "focal_loss: bad argument");
    return ofx_launch_focal_loss(logits, labels, B, alpha, gamma, upstream, loss, dlogits, (hipStream_t)stream);
}
extern "C" int ofx_focal_loss_ex(const float* logits, const float* labels, int B, float alpha, float gamma, float upstream, int reduction, float* loss,
                                 float* per_elem, float* dlogits, ofx_stream stream) {
    OFX_REQUIRE(logits && labels && B > 0 && reduction >= 0 && reduction <= 2, OFX_EINVAL, "focal_loss_ex: bad argument");
    OFX_REQUIRE(reduction != 0 || per_elem, OFX_EINVAL, "focal_loss_ex: reduction 'none' needs per_elem");
    return ofx_launch_focal_loss(logits, labels, B, alpha, gamma, upstream, loss, dlogits, (hipStream_t)stream, reduction, per_elem);
}

static bool rank_loss_shape_ok(int B, int K, int D) { return B >= 1 && K >= 0 && D >= 4 && D <= 4096 && D % 4 == 0; }
extern "C" size_t ofx_set_rank_loss_ws_bytes(int B, int K, int D) { return rank_loss_shape_ok(B, K, D) ? ofx_set_rank_loss_ws(B, K) : 0; }
extern "C" int ofx_set_rank_loss(const float* y, const float* y_hat, const float* neg, const uint8_t* neg_mask, int B, int K, int D, float margin,
                                 float upstream, float* loss, float* dy_hat, float* d_pos, float* d_neg, void* ws, size_t ws_bytes, ofx_stream stream) {
    OFX_REQUIRE(rank_loss_shape_ok(B, K, D), OFX_ESHAPE, "set_rank_loss: B = %d, K = %d, D = %d; needs B >= 1, K >= 0, D %% 4 == 0, 4 <= D <= 4096", B, K, D);
    OFX_REQUIRE(y && y_hat && loss && ws && (neg || K == 0), OFX_EINVAL, "set_rank_loss: NULL argument");
    OFX_REQUIRE((((uintptr_t)y | (uintptr_t)y_hat | (uintptr_t)neg | (uintptr_t)dy_hat | (uintptr_t)ws) & 15) == 0, OFX_EINVAL,
                "set_rank_loss: y, y_hat, neg, dy_hat and ws must be 16-byte aligned");
    OFX_REQUIRE(ws_bytes >= ofx_set_rank_loss_ws(B, K), OFX_EWORKSPACE, "set_rank_loss: workspace %zu < %zu bytes", ws_bytes, ofx_set_rank_loss_ws(B, K));
    return ofx_launch_set_rank_loss(y, y_hat, neg, neg_mask, B, K, D, margin, upstream, loss, dy_hat, d_pos, d_neg, ws, (hipStream_t)stream);
}

extern "C" int ofx_set_rank_loss_indexed(const float* table, int ld, long long n_table, const int* pos_index, const int* neg_index, const float* y_hat,
                                         int B, int K, int D, float margin, float upstream, float* loss, float* dy_hat, float* d_pos, float* d_neg,
                                         void* ws, size_t ws_bytes, ofx_stream stream) {
    OFX_REQUIRE(rank_loss_shape_ok(B, K, D), OFX_ESHAPE,
                "set_rank_loss_indexed: B = %d, K = %d, D = %d; needs B >= 1, K >= 0, D %% 4 == 0, 4 <= D <= 4096", B, K, D);
    OFX_REQUIRE(ld >= D && ld % 4 == 0 && n_table >= 1 && n_table <= INT_MAX, OFX_ESHAPE,
                "set_rank_loss_indexed: ld = %d, n_table = %lld; needs ld >= D = %d, ld %% 4 == 0, 1 <= n_table <= INT_MAX", ld, n_table, D);
    OFX_REQUIRE(table && pos_index && y_hat && loss && ws && (neg_index || K == 0), OFX_EINVAL, "set_rank_loss_indexed: NULL argument");
    OFX_REQUIRE((((uintptr_t)table | (uintptr_t)y_hat | (uintptr_t)dy_hat | (uintptr_t)ws) & 15) == 0 &&
                    (((uintptr_t)pos_index | (uintptr_t)neg_index) & 3) == 0,
                OFX_EINVAL, "set_rank_loss_indexed: table, y_hat, dy_hat and ws must be 16-byte aligned, the index arrays 4-byte aligned");
    OFX_REQUIRE(ws_bytes >= ofx_set_rank_loss_ws(B, K), OFX_EWORKSPACE, "set_rank_loss_indexed: workspace %zu < %zu bytes", ws_bytes,
                ofx_set_rank_loss_ws(B, K));
    return ofx_launch_set_rank_loss_indexed(table, ld, (int)n_table, pos_index, neg_index, y_hat, B, K, D, margin, upstream, loss, dy_hat, d_pos, d_neg, ws,
                                            (hipStream_t)stream);
}

extern "C" int ofx_cir_sample_batch(const int* outfit_cu, const int* outfit_rows, int n_outfits, int n_outfit_rows, const int* pos_cu, const int* pos_slots,
                                    int n_pos_slots, const int* pool_cu, const int* pool_rows, int n_pools, int n_pool_rows, const int* row_pool,
                                    const int* row_slot, int n_table, const int* outfit_ids, int B, unsigned seed, unsigned draw, int K, int max_len,
                                    int* item_index, int* cu_seqlens, int* target_item_index, int* neg_items_index, ofx_stream stream) {
    OFX_REQUIRE(B >= 1, OFX_EINVAL, "cir_sample_batch: B = %d; needs B >= 1", B);
    OFX_REQUIRE(K >= 0 && K <= 64 && max_len >= 1 && max_len <= 31, OFX_ESHAPE, "cir_sample_batch: K = %d, max_len = %d; needs 0 <= K <= 64, 1 <= max_len <= 31",
                K, max_len);
    OFX_REQUIRE(n_outfits >= 1 && n_table >= 1 && n_outfit_rows >= 0 && n_pos_slots >= 0 && n_pools >= 0 && n_pool_rows >= 0, OFX_ESHAPE,
                "cir_sample_batch: n_outfits = %d, n_table = %d (both >= 1), n_outfit_rows = %d, n_pos_slots = %d, n_pools = %d, n_pool_rows = %d (all >= 0)",
                n_outfits, n_table, n_outfit_rows, n_pos_slots, n_pools, n_pool_rows);
    OFX_REQUIRE((long long)B * std::max(K, max_len) <= INT_MAX, OFX_ESHAPE, "cir_sample_batch: B * max(K, max_len) = %lld exceeds INT_MAX",
                (long long)B * std::max(K, max_len));
    const void* ptrs[] = {outfit_cu, outfit_rows, pos_cu, pos_slots, pool_cu, pool_rows, row_pool, row_slot, outfit_ids, item_index, cu_seqlens, target_item_index};
    uintptr_t bits = (uintptr_t)neg_items_index;
    for (const void* p : ptrs) {
        OFX_REQUIRE(p, OFX_EINVAL, "cir_sample_batch: NULL argument");
        bits |= (uintptr_t)p;
    }
    OFX_REQUIRE(neg_items_index || K == 0, OFX_EINVAL, "cir_sample_batch: NULL neg_items_index with K = %d", K);
    OFX_REQUIRE((bits & 15) == 0, OFX_EINVAL, "cir_sample_batch: every array must be 16-byte aligned");
    CirSampleArgs a{outfit_cu, outfit_rows, pos_cu, pos_slots, pool_cu, pool_rows, row_pool, row_slot, outfit_ids,
                    n_outfits, n_outfit_rows, n_pos_slots, n_pools, n_pool_rows, n_table, B, K, max_len, seed, draw,
                    item_index, cu_seqlens, target_item_index, neg_items_index};
    return ofx_launch_cir_sample_batch(a, (hipStream_t)stream);
}

static bool adamw_shape_ok(long long n_arena) { return n_arena > 0 && n_arena % 64 == 0; }
extern "C" size_t ofx_adamw_step_ws_bytes(long long n_arena) { return adamw_shape_ok(n_arena) ? ofx_adamw_step_ws(n_arena) : 0; }
extern "C" int ofx_adamw_step(const ofx_opt_segment* segments, int n_segments, float* grad, float* exp_avg, float* exp_avg_sq, long long n_arena,
                              float* step, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm, double grad_scale,
                              float* grad_norm, int* skipped, void* ws, size_t ws_bytes, ofx_stream stream) {
    OFX_REQUIRE(segments && grad && exp_avg && exp_avg_sq && step && grad_norm && skipped && ws, OFX_EINVAL, "adamw_step: NULL argument");
    OFX_REQUIRE(n_segments >= 1 && n_segments <= 1024, OFX_ESHAPE, "adamw_step: n_segments = %d; needs 1 <= n_segments <= 1024", n_segments);
    OFX_REQUIRE(adamw_shape_ok(n_arena), OFX_ESHAPE, "adamw_step: n_arena = %lld; needs a positive multiple of 64", n_arena);
    OFX_REQUIRE((((uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)segments & 7) == 0, OFX_EINVAL,
                "adamw_step: grad, exp_avg, exp_avg_sq and ws must be 16-byte aligned, segments 8-byte aligned");
    OFX_REQUIRE(ws_bytes >= ofx_adamw_step_ws(n_arena), OFX_EWORKSPACE, "adamw_step: workspace %zu < %zu bytes", ws_bytes, ofx_adamw_step_ws(n_arena));
    return ofx_launch_adamw_step(segments, n_segments, grad, exp_avg, exp_avg_sq, n_arena, step, lr, beta1, beta2, eps, weight_decay, max_norm,
                                 grad_scale, grad_norm, skipped, ws, (hipStream_t)stream);
}
extern "C" int ofx_adamw_step_scaled(const ofx_opt_segment* segments, int n_segments, float* grad, float* exp_avg, float* exp_avg_sq, long long n_arena,
                                     float* step, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                                     double grad_scale, float* loss_scale, int* growth_tracker, double growth_factor, double backoff_factor,
                                     int growth_interval, float* grad_norm, int* skipped, void* ws, size_t ws_bytes, ofx_stream stream) {
    OFX_REQUIRE(segments && grad && exp_avg && exp_avg_sq && step && grad_norm && skipped && ws && loss_scale && growth_tracker, OFX_EINVAL,
                "adamw_step_scaled: NULL argument");
    OFX_REQUIRE(n_segments >= 1 && n_segments <= 1024, OFX_ESHAPE, "adamw_step_scaled: n_segments = %d; needs 1 <= n_segments <= 1024", n_segments);
    OFX_REQUIRE(adamw_shape_ok(n_arena), OFX_ESHAPE, "adamw_step_scaled: n_arena = %lld; needs a positive multiple of 64", n_arena);
    OFX_REQUIRE((((uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)segments & 7) == 0, OFX_EINVAL,
                "adamw_step_scaled: grad, exp_avg, exp_avg_sq and ws must be 16-byte aligned, segments 8-byte aligned");
    OFX_REQUIRE((((uintptr_t)loss_scale | (uintptr_t)growth_tracker) & 3) == 0, OFX_EINVAL,
                "adamw_step_scaled: loss_scale and growth_tracker must be 4-byte aligned");
    OFX_REQUIRE(growth_factor >= 1.0 && backoff_factor > 0.0 && backoff_factor <= 1.0 && growth_interval >= 1, OFX_EINVAL,      // NaNs fail too
                "adamw_step_scaled: growth_factor = %g, backoff_factor = %g, growth_interval = %d; needs growth >= 1, 0 < backoff <= 1, interval >= 1",
                growth_factor, backoff_factor, growth_interval);
    OFX_REQUIRE(ws_bytes >= ofx_adamw_step_ws(n_arena), OFX_EWORKSPACE, "adamw_step_scaled: workspace %zu < %zu bytes", ws_bytes, ofx_adamw_step_ws(n_arena));
    return ofx_launch_adamw_step_scaled(segments, n_segments, grad, exp_avg, exp_avg_sq, n_arena, step, lr, beta1, beta2, eps, weight_decay, max_norm,
                                        grad_scale, loss_scale, growth_tracker, growth_factor, backoff_factor, growth_interval, grad_norm, skipped,
                                        ws, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------- tuning
extern "C" int ofx_tune(int knob, int value) {
    ++g_config_generation;
    switch (knob) {
        case 2: case 5: case 11: case 15: case 16: case 18: return ofx_gemm_tune(knob, value);      // the GEMM launch knobs (GemmKnobs, gemm_plan.h)
        case 6: if (value != 2) { ofx_set_error("ofx_tune(6): %d is not 2 (the towers' LayerNorms are always folded)", value); return OFX_EINVAL; } return OFX_OK;
        case 7: g_train_mfma_attn = value; return OFX_OK;
        case 8: g_prune_q = value; return OFX_OK;
        case 9: g_fuse_qkv = value; return OFX_OK;
        case 10: g_set_fuse = value; return OFX_OK;
        case 17: g_topk_filter = value != 0; return OFX_OK;
        case 20: g_x3_vit_f32_attn = value != 0; return OFX_OK;
        case 21: g_text_shared_first = value != 0; return OFX_OK;
        case 22: g_fuse_qkv_w2f8 = value != 0; return OFX_OK;
        default: ofx_set_error("ofx_tune: unknown knob %d", knob); return OFX_EINVAL;
    }
}

// ------------------------------------------------------------------------------------- op level
// the arguments every op-level GEMM entry point shares; K = the depth of the W rows as stored
static GemmArgs op_gemm(const void* A, const void* W, void* C, const float* bias, const float* resid, int M, int N, int K, int lda, int ldc, int ldr,
                        int act, int out_kind) {
    GemmArgs g{}; g.A = A; g.W = W; g.C = C; g.bias = bias; g.resid = resid; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldc;
    g.ldr = ldr; g.act = act; g.out_kind = out_kind;
    return g;
}
extern "C" int ofx_gemm(const void* A, const void* W, void* C, const float* bias, const float* resid, int M, int N, int K,
                        int lda, int ldc, int ldr, int act, int out_kind, int op_dtype, ofx_stream stream) {
    return ofx_launch_gemm(op_gemm(A, W, C, bias, resid, M, N, K, lda, ldc, ldr, act, out_kind), op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_gemm_w2(const void* A, const void* W2, void* C, const float* bias, const float* resid, int M, int N, int K,
                           int lda, int ldc, int ldr, int act, int out_kind, int op_dtype, ofx_stream stream) {
    GemmArgs g = op_gemm(A, W2, C, bias, resid, M, N, 2 * K, lda, ldc, ldr, act, out_kind); g.a_wrap = K;
    return ofx_launch_gemm(g, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_gemm_x3(const void* A3, const void* W3, void* C, const float* bias, const float* resid, int M, int N, int K,
                           int lda, int ldc, int ldr, int act, int out_kind, int op_dtype, ofx_stream stream) {
    GemmArgs g = op_gemm(A3, W3, C, bias, resid, M, N, 3 * K, lda, ldc, ldr, act, out_kind); g.k_mult = 3;
    return ofx_launch_gemm(g, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_pack_lo8(const void* W2, void* W8, void* scale8, int N, int K, ofx_stream stream) {
    return ofx_launch_pack_lo8(W2, W8, scale8, N, K, (hipStream_t)stream);
}
extern "C" int ofx_gemm_w2f8(const void* A, const void* W2, const void* W8, const void* scale8, void* C, const float* bias, const float* resid, int M, int N, int K,
                             int lda, int ldc, int ldr, int act, int out_kind, ofx_stream stream) {
    GemmArgs g = op_gemm(A, W2, C, bias, resid, M, N, 2 * K, lda, ldc, ldr, act, out_kind); g.a_wrap = K; g.W8 = W8; g.w8_scale = scale8;
    return ofx_launch_gemm(g, OFX_F16, (hipStream_t)stream);
}
extern "C" int ofx_gemm_w2f8_fold(const void* A, const void* W2, const void* W8, const void* scale8, void* C, const float* bias, const float* row_stat, const float* col_sum,
                                  int M, int N, int K, int lda, int ldc, int act, ofx_stream stream) {
    OFX_REQUIRE(row_stat && col_sum, OFX_EINVAL, "gemm_w2f8_fold: row_stat and col_sum are required");
    GemmArgs g = op_gemm(A, W2, C, bias, nullptr, M, N, 2 * K, lda, ldc, 0, act, OFX_OUT_OP); g.a_wrap = K; g.W8 = W8; g.w8_scale = scale8;
    g.row_stat = row_stat; g.col_sum = col_sum; g.stat_ld = 1;
    return ofx_launch_gemm(g, OFX_F16, (hipStream_t)stream);
}
extern "C" size_t ofx_gemm_splitk_ws(int M, int N, int K) { return ofx_gemm_splitk_bytes(M, N, K); }
extern "C" int ofx_gemm_splitk(const void* A, const void* W, void* C, const float* bias, const float* resid, int M, int N, int K,
                               int lda, int ldc, int ldr, int act, int out_kind, int op_dtype, void* slab, size_t slab_bytes, ofx_stream stream) {
    GemmArgs g = op_gemm(A, W, C, bias, resid, M, N, K, lda, ldc, ldr, act, out_kind); g.slab = slab; g.slab_bytes = slab_bytes;
    return ofx_launch_gemm(g, op_dtype, (hipStream_t)stream);
}
extern "C" size_t ofx_gemm_tn_ws(int M, int N, int K) { return ofx_gemm_tn_slab_bytes(M, N, K); }
extern "C" int ofx_gemm_tn(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K, const int* k_dev,
                           void* slab, size_t slab_bytes, int op_dtype, ofx_stream stream) {
    return ofx_launch_gemm_tn(A, lda, B, ldb, C, ldc, M, N, K, k_dev, slab, slab_bytes, op_dtype, (hipStream_t)stream);
}
// the non-attention kernels of the training backward, one call each, dropout sites built as the step builds them
static bool op_dtype_ok(int op_dtype) { return op_dtype == OFX_BF16 || op_dtype == OFX_F16; }
static bool drop_p_ok(float p) { return p >= 0.f && p < 1.f; }
static bool aligned_to(size_t mask, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs) if ((uintptr_t)p & mask) return false;
    return true;
}
extern "C" int ofx_gemm_train(const void* A, const void* W, void* C, const float* bias, const float* resid, float* aux_out, int M, const int* m_dev,
                              int N, int K, int lda, int ldc, int ldr, int act, int out_kind, float dropout_p, unsigned seed, int site, int op_dtype,
                              void* slab, size_t slab_bytes, ofx_stream stream) {
    OFX_REQUIRE(A && W && C && drop_p_ok(dropout_p) && (act != OFX_ACT_MISH_GRAD || resid), OFX_EINVAL, "gemm_train: bad argument");
    OFX_REQUIRE(aligned_to(15, {bias, resid, aux_out, slab}) && aligned_to(3, {m_dev}), OFX_EINVAL,
                "gemm_train: bias, resid, aux_out and slab must be 16-byte aligned");
    GemmArgs g = op_gemm(A, W, C, bias, resid, M, N, K, lda, ldc, ldr, act, out_kind); g.slab = slab; g.slab_bytes = slab_bytes;
    g.aux_out = aux_out; g.m_dev = m_dev; g.drop = make_drop(dropout_p, seed, (unsigned)site);
    return ofx_launch_gemm(g, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_gemm_tn_into(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K, const int* k_dev,
                                int m_valid, int n_valid, int accumulate, void* slab, size_t slab_bytes, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(A && B && C && m_valid >= 0 && n_valid >= 0, OFX_EINVAL, "gemm_tn_into: bad argument");
    OFX_REQUIRE(aligned_to(15, {slab}) && aligned_to(3, {k_dev}), OFX_EINVAL, "gemm_tn_into: slab must be 16-byte aligned");
    return ofx_launch_gemm_tn(A, lda, B, ldb, C, ldc, M, N, K, k_dev, slab, slab_bytes, op_dtype, (hipStream_t)stream, m_valid, n_valid, accumulate ? 1 : 0);
}
extern "C" int ofx_transpose_cast(const float* src, void* dst, int R, int C, int ldd, void* row_dst, int ld_row, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(src && dst && op_dtype_ok(op_dtype), OFX_EINVAL, "transpose_cast: bad argument");
    OFX_REQUIRE(aligned_to(3, {src}) && aligned_to(1, {dst, row_dst}), OFX_EINVAL, "transpose_cast: misaligned pointer");
    OFX_REQUIRE(R > 0 && C > 0, OFX_ESHAPE, "transpose_cast: R=%d C=%d", R, C);
    return ofx_launch_transpose_cast(src, dst, R, C, ldd, op_dtype, (hipStream_t)stream, row_dst, ld_row);
}
static bool ln_bwd_d_ok(int D) { return D == 512 || D == 768 || D == 1024; }
extern "C" size_t ofx_layernorm_bwd_ws(int D) { return ln_bwd_d_ok(D) ? ofx_ln_bwd_part_floats(D) * sizeof(float) : 0; }
extern "C" int ofx_layernorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma, const float* add, const int* add_map,
                                 float* dx, void* dx_op, float* dgamma, float* dbeta, float* dcols, int M, const int* m_dev, int D, float dropout_p,
                                 unsigned seed, int site, int accumulate, int op_dtype, void* ws, size_t ws_bytes, ofx_stream stream) {
    OFX_REQUIRE(dy && x && stats && gamma && dx && dx_op && ws && (add || !add_map) && drop_p_ok(dropout_p) && op_dtype_ok(op_dtype), OFX_EINVAL,
                "layernorm_bwd: bad argument");
    OFX_REQUIRE(M > 0 && ln_bwd_d_ok(D), OFX_ESHAPE, "layernorm_bwd: M = %d, D = %d; needs M >= 1, D in {512, 768, 1024}", M, D);
    OFX_REQUIRE(aligned_to(15, {dy, x, gamma, add, dx, ws}) && aligned_to(7, {dx_op}) && aligned_to(3, {stats, add_map, dgamma, dbeta, dcols, m_dev}), OFX_EINVAL,
                "layernorm_bwd: dy, x, gamma, add, dx and ws must be 16-byte aligned, dx_op 8-byte aligned");
    OFX_REQUIRE(ws_bytes >= ofx_layernorm_bwd_ws(D), OFX_EWORKSPACE, "layernorm_bwd: workspace %zu < %zu bytes", ws_bytes, ofx_layernorm_bwd_ws(D));
    return ofx_launch_ln_bwd(dy, x, stats, gamma, add, add_map, dx, dx_op, dgamma, dbeta, dcols, (float*)ws, D, m_dev, M, op_dtype,
                             make_drop(dropout_p, seed, (unsigned)site), (hipStream_t)stream, accumulate ? 1 : 0);
}
static bool colsum_c_ok(int C) { return C > 0 && C % 4 == 0; }
extern "C" size_t ofx_colsum_ws(int C) { return colsum_c_ok(C) ? ofx_colsum_part_floats(C) * sizeof(float) : 0; }
extern "C" int ofx_colsum(const void* x, int x_kind, int ld, const int* gather, const float* row_scale, float* out0, float* out1, float* out2, int seg,
                          int C, int valid, int M, const int* m_dev, int accumulate, int op_dtype, void* ws, size_t ws_bytes, ofx_stream stream) {
    OFX_REQUIRE(x && ws && (out0 || out1 || out2) && (x_kind == 0 || (x_kind == 1 && op_dtype_ok(op_dtype))), OFX_EINVAL, "colsum: bad argument");
    OFX_REQUIRE(colsum_c_ok(C) && M > 0 && ld >= C && ld % 4 == 0 && seg > 0 && C <= 3 * (long long)seg && valid >= 0 && valid <= seg, OFX_ESHAPE,
                "colsum: C = %d, ld = %d, seg = %d, valid = %d, M = %d; needs C %% 4 == 0, ld >= C, ld %% 4 == 0, C <= 3 seg, valid <= seg, M >= 1", C, ld,
                seg, valid, M);
    OFX_REQUIRE(aligned_to(x_kind == 0 ? 15 : 7, {x}) && aligned_to(15, {ws}) && aligned_to(3, {gather, row_scale, out0, out1, out2, m_dev}), OFX_EINVAL,
                "colsum: x must be aligned to four of its elements, ws to 16 bytes");
    OFX_REQUIRE(ws_bytes >= ofx_colsum_ws(C), OFX_EWORKSPACE, "colsum: workspace %zu < %zu bytes", ws_bytes, ofx_colsum_ws(C));
    return ofx_launch_colsum(x, x_kind, ld, gather, row_scale, out0, out1, out2, seg, (float*)ws, C, m_dev, M, op_dtype, (hipStream_t)stream, valid,
                             accumulate ? 1 : 0);
}
extern "C" int ofx_head_bwd(const float* dlogits, const float* w, const int* cu, float* dX, void* dXb, float* db, int B, int D, float dropout_p,
                            unsigned seed, int head_site, int below_site, int accumulate, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(w && dX && dXb && (dlogits || !db) && drop_p_ok(dropout_p) && op_dtype_ok(op_dtype), OFX_EINVAL, "head_bwd: bad argument");
    OFX_REQUIRE(B > 0 && D > 0 && D % 4 == 0, OFX_ESHAPE, "head_bwd: B = %d, D = %d; needs B >= 1, D a positive multiple of 4", B, D);
    OFX_REQUIRE(aligned_to(15, {w, dX}) && aligned_to(7, {dXb}) && aligned_to(3, {dlogits, cu, db}), OFX_EINVAL,
                "head_bwd: w and dX must be 16-byte aligned, dXb 8-byte aligned");
    const DropArgs none;
    return ofx_launch_cp_head_bwd(dlogits, w, cu, dX, dXb, db, B, D, op_dtype, head_site < 0 ? none : make_drop(dropout_p, seed, (unsigned)head_site),
                                  below_site < 0 ? none : make_drop(dropout_p, seed, (unsigned)below_site), (hipStream_t)stream, accumulate ? 1 : 0);
}
// the towers' LayerNorm-fold chain, one call each: thin wrappers over the launchers the ViT and text layers use
static int fold_gemm_args(GemmArgs& g, const char* who, const void* A, const void* W, const void* W8, const void* scale8, int K, int w_form, int& op_dtype) {
    OFX_REQUIRE(w_form >= 0 && w_form <= 2 && op_dtype_ok(op_dtype) && (w_form != 2 || op_dtype == OFX_F16), OFX_EINVAL,
                "%s: w_form = %d (0 plain, 1 split, 2 split + fp8 lo copy, f16 only), op_dtype = %d", who, w_form, op_dtype);
    OFX_REQUIRE(A && W && (w_form != 2 || (W8 && scale8)), OFX_EINVAL, "%s: NULL operand", who);
    const WeightForm f = w_form ? W_SPLIT : W_PLAIN;
    g.A = A; g.W = W; g.K = w_kmul(f) * K;
    if (f == W_SPLIT) g.a_wrap = K;
    if (w_form == 2) { g.W8 = W8; g.w8_scale = scale8; }
    return OFX_OK;
}
extern "C" int ofx_gemm_fold_producer(const void* A, const void* W, const void* W8, const void* scale8, void* xb, void* xlo, float* stat_part,
                                      const float* bias, const float* resid, int M, int N, int K, int lda, int ldr, int act, int w_form, int op_dtype,
                                      ofx_stream stream) {
    GemmArgs g = op_gemm(nullptr, nullptr, xb, bias, resid, M, N, K, lda, N, ldr, act, OFX_OUT_OP);
    TRY(fold_gemm_args(g, "gemm_fold_producer", A, W, W8, scale8, K, w_form, op_dtype));
    OFX_REQUIRE(xb && xlo && stat_part, OFX_EINVAL, "gemm_fold_producer: xb, xlo and stat_part are all required");
    OFX_REQUIRE(aligned_to(15, {A, W, W8, xb, xlo, bias, resid}) && aligned_to(7, {stat_part}), OFX_EINVAL,
                "gemm_fold_producer: A, W, W8, xb, xlo, bias must be 16-byte aligned, stat_part 8-byte aligned");
    g.xb_out = xb; g.xlo = xlo; g.stat_part = stat_part;
    return ofx_launch_gemm(g, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_gemm_fold(const void* A, const void* W, void* C, const float* bias, const float* row_stat, int stat_ld, const float* col_sum,
                             int M, int N, int K, int lda, int ldc, int act, int w_form, int op_dtype, ofx_stream stream) {
    GemmArgs g = op_gemm(nullptr, nullptr, C, bias, nullptr, M, N, K, lda, ldc, 0, act, OFX_OUT_OP);
    OFX_REQUIRE(w_form != 2, OFX_EINVAL, "gemm_fold: w_form 2 is ofx_gemm_w2f8_fold");
    TRY(fold_gemm_args(g, "gemm_fold", A, W, nullptr, nullptr, K, w_form, op_dtype));
    OFX_REQUIRE(C && row_stat && col_sum, OFX_EINVAL, "gemm_fold: C, row_stat and col_sum are required");
    OFX_REQUIRE(aligned_to(15, {A, W, C, bias, col_sum}) && aligned_to(7, {row_stat}), OFX_EINVAL,
                "gemm_fold: A, W, C, bias and col_sum must be 16-byte aligned, row_stat 8-byte aligned");
    OFX_REQUIRE(stat_ld >= 1, OFX_ESHAPE, "gemm_fold: stat_ld = %d; needs >= 1", stat_ld);
    g.row_stat = row_stat; g.col_sum = col_sum; g.stat_ld = stat_ld;
    return ofx_launch_gemm(g, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_stats_finalize(const float* stat_part, int slots, int W, float eps, float* stat, int rows, ofx_stream stream) {
    OFX_REQUIRE(stat_part && stat && aligned_to(7, {stat_part, stat}), OFX_EINVAL, "stats_finalize: stat_part and stat are required, 8-byte aligned");
    OFX_REQUIRE(rows > 0 && slots > 0 && W > 0, OFX_ESHAPE, "stats_finalize: rows = %d, slots = %d, W = %d; all must be positive", rows, slots, W);
    return ofx_launch_stats_finalize(stat_part, slots, W, eps, stat, rows, (hipStream_t)stream);
}
extern "C" int ofx_row_stats_cast(const float* x, void* xb, void* xlo, float* stat, int rows, int W, float eps, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(x && xb && xlo && stat && op_dtype_ok(op_dtype), OFX_EINVAL, "row_stats_cast: bad argument");
    OFX_REQUIRE(aligned_to(15, {x}) && aligned_to(7, {xb, xlo, stat}), OFX_EINVAL, "row_stats_cast: x must be 16-byte aligned, xb, xlo and stat 8-byte aligned");
    OFX_REQUIRE(rows > 0 && W > 0 && W % 4 == 0, OFX_ESHAPE, "row_stats_cast: rows = %d, W = %d; needs rows >= 1, W a positive multiple of 4", rows, W);
    return ofx_launch_row_stats_cast(x, xb, xlo, stat, rows, W, eps, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_fold_pack(const float* w, const float* gamma, const float* beta, const float* bias, void* wf, float* col_sum, float* bias_f, int N, int K,
                             int split, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(w && gamma && beta && bias && wf && col_sum && bias_f && op_dtype_ok(op_dtype), OFX_EINVAL, "fold_pack: bad argument");
    OFX_REQUIRE(aligned_to(3, {w, gamma, beta, bias, col_sum, bias_f}) && aligned_to(1, {wf}), OFX_EINVAL, "fold_pack: misaligned pointer");
    OFX_REQUIRE(N > 0 && K > 0, OFX_ESHAPE, "fold_pack: N = %d, K = %d; both must be positive", N, K);
    return ofx_launch_fold_pack(w, gamma, beta, bias, wf, col_sum, bias_f, N, K, op_dtype, (hipStream_t)stream, split ? 1 : 0);
}
extern "C" int ofx_vit_embed_ln(const float* patch_out, const float* cls, const float* pos, const float* gamma, const float* beta, float* x, void* xb,
                                void* xlo, float* stat, int N, int S, int D, float eps, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(patch_out && cls && pos && gamma && beta && op_dtype_ok(op_dtype), OFX_EINVAL, "vit_embed_ln: bad argument");
    OFX_REQUIRE(x ? !xb && !xlo && !stat : xb && xlo && stat, OFX_EINVAL, "vit_embed_ln: writes either x or (xb, xlo, stat)");
    OFX_REQUIRE(aligned_to(15, {patch_out, cls, pos, gamma, beta, x}) && aligned_to(7, {xb, xlo, stat}), OFX_EINVAL,
                "vit_embed_ln: the fp32 arrays must be 16-byte aligned, xb, xlo and stat 8-byte aligned");
    OFX_REQUIRE(N > 0 && S > 0 && (long long)N * S <= INT_MAX, OFX_ESHAPE, "vit_embed_ln: N = %d, S = %d", N, S);
    return ofx_launch_vit_embed_ln(patch_out, cls, pos, gamma, beta, x, N, S, D, eps, (hipStream_t)stream, xb, stat, op_dtype, xlo);
}
extern "C" int ofx_gather_hilo(const void* hi, const void* lo, const int* idx, float* dst, int rows, int W, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(hi && lo && idx && dst && op_dtype_ok(op_dtype), OFX_EINVAL, "gather_hilo: bad argument");
    OFX_REQUIRE(aligned_to(7, {hi, lo}) && aligned_to(15, {dst}) && aligned_to(3, {idx}), OFX_EINVAL,
                "gather_hilo: hi and lo must be 8-byte aligned, dst 16-byte aligned");
    OFX_REQUIRE(rows > 0 && W > 0 && W % 4 == 0, OFX_ESHAPE, "gather_hilo: rows = %d, W = %d; needs rows >= 1, W a positive multiple of 4", rows, W);
    return ofx_launch_gather_hilo(hi, lo, idx, dst, rows, W, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_clip_preprocess_patches(const uint8_t* src, const long long* offsets, const int* heights, const int* widths, int N, int channels, int size,
                                           int patch, const float* mean, const float* stdv, void* patches, int op_dtype, void* ws, size_t ws_bytes,
                                           ofx_stream stream) {
    OFX_REQUIRE(src && offsets && heights && widths && mean && stdv && patches && ws && op_dtype_ok(op_dtype), OFX_EINVAL,
                "clip_preprocess_patches: bad argument (a NULL pointer or op_dtype = %d)", op_dtype);
    OFX_REQUIRE(patch > 0 && size > 0 && size % patch == 0, OFX_ESHAPE, "clip_preprocess_patches: size=%d patch=%d", size, patch);
    return ofx_preprocess_to(src, offsets, heights, widths, N, channels, size, mean, stdv, nullptr, patches, patch, op_dtype, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int ofx_patchify(const float* pixels, void* out, int N, int img, int patch, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(pixels && out && op_dtype_ok(op_dtype), OFX_EINVAL, "patchify: bad argument (a NULL pointer or op_dtype = %d)", op_dtype);
    OFX_REQUIRE(aligned_to(15, {pixels, out}), OFX_EINVAL, "patchify: pixels and out must be 16-byte aligned");
    OFX_REQUIRE(N > 0 && img > 0 && patch > 0, OFX_ESHAPE, "patchify: N = %d, img = %d, patch = %d; all must be positive", N, img, patch);
    return ofx_launch_patchify(pixels, out, N, img, patch, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_layernorm(const float* x, const int* row_idx, const float* gamma, const float* beta, void* y, int rows,
                             int D, int ldy, int out_kind, int op_dtype, float eps, ofx_stream stream) {
    LnArgs a{x, row_idx, gamma, beta, y, rows, D, ldy, out_kind, eps};
    return ofx_launch_layernorm(a, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_attention(const void* qkv, void* out, const int64_t* key_mask, int nseq, int seq_len, int n_head, int ld,
                             int ldo, int k_off, int v_off, int mask_ld, int causal, float scale, int op_dtype, ofx_stream stream) {
    AttnArgs a{qkv, out, key_mask, nseq, seq_len, n_head, ld, ldo, k_off, v_off, mask_ld, causal, scale};
    return ofx_launch_attention_mfma(a, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_attention_ex(const void* qkv, void* out, const int64_t* key_mask, int nseq, int seq_len, int n_head, int ld, int ldo, int k_off,
                                int v_off, int mask_ld, int causal, int only_row0, int split3_w, float scale, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(qkv && out && op_dtype_ok(op_dtype), OFX_EINVAL, "attention_ex: bad argument (a NULL pointer or op_dtype = %d)", op_dtype);
    OFX_REQUIRE(split3_w >= 0 && (!key_mask || mask_ld >= seq_len), OFX_ESHAPE, "attention_ex: split3_w=%d mask_ld=%d", split3_w, mask_ld);
    AttnArgs a{qkv, out, key_mask, nseq, seq_len, n_head, ld, ldo, k_off, v_off, mask_ld, causal ? 1 : 0, scale};
    a.only_row0 = only_row0 ? 1 : 0; a.split3_w = split3_w;
    return ofx_launch_attention_mfma(a, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_set_attention_slabs(const float* slabs, size_t plane_floats, int splits, const float* bias, void* out, const int* cu_seqlens, int nseq,
                                       int n_head, int D, int ldo, int out_kind, int max_len, int only_row0, float scale, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(slabs && out && cu_seqlens && nseq > 0 && n_head > 0 && splits >= 1 && op_dtype_ok(op_dtype) && aligned_to(15, {slabs, bias, out}) && plane_floats % 4 == 0,
                OFX_EINVAL, "set_attention_slabs: bad argument (a NULL or misaligned pointer, nseq = %d, splits = %d, op_dtype = %d)", nseq, splits, op_dtype);
    OFX_REQUIRE(out_kind >= 0 && out_kind <= 2, OFX_ESHAPE, "set_attention_slabs: out_kind=%d", out_kind);
    SetAttnArgs a{slabs, out, cu_seqlens, nseq, n_head, D, ldo, out_kind, max_len, only_row0 ? 1 : 0, scale};
    a.splits = splits; a.plane = plane_floats; a.bias = bias;
    return ofx_launch_set_attention(a, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_splitk_reduce_ln(const float* slab, size_t plane_floats, int splits, const float* bias, const float* resid, int ldr, float* x, int ldx,
                                    const float* gamma, const float* beta, void* y, int ldy, int out_kind, float eps, int rows, const int* m_dev, int D,
                                    int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(slab && x && gamma && beta && y && op_dtype_ok(op_dtype) && aligned_to(15, {slab, bias, resid, x, gamma, beta}) && aligned_to(out_kind == 0 ? 15 : 7, {y}) && aligned_to(3, {m_dev}) &&
                    plane_floats % 4 == 0,
                OFX_EINVAL, "splitk_reduce_ln: bad argument (a NULL or misaligned pointer or op_dtype = %d)", op_dtype);
    OFX_REQUIRE(out_kind >= 0 && out_kind <= 2 && (splits <= 1 || plane_floats >= (size_t)rows * D), OFX_ESHAPE, "splitk_reduce_ln: out_kind=%d, or slabs that overlap", out_kind);
    SplitKLnArgs a{slab, plane_floats, splits, bias, resid, ldr, x, ldx, gamma, beta, y, ldy, out_kind, eps, rows, D, m_dev};
    return ofx_launch_splitk_reduce_ln(a, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_fused_qkv_attention(const void* X, const void* Wqkv, const float* bias, const float* row_stat, const float* col_sum, void* out,
                                       int nseq, int seq_len, int width, int n_head, int ldx, int ldo, float scale, int op_dtype, ofx_stream stream) {
    return ofx_launch_fused_qkv_attn(X, Wqkv, bias, row_stat, col_sum, out, nseq, seq_len, width, n_head, ldx, ldo, scale, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_fused_qkv_attention_w2(const void* X, const void* Wqkv2, const float* bias, const float* row_stat, const float* col_sum, void* out,
                                          int nseq, int seq_len, int width, int n_head, int ldx, int ldo, float scale, int op_dtype, ofx_stream stream) {
    return ofx_launch_fused_qkv_attn(X, Wqkv2, bias, row_stat, col_sum, out, nseq, seq_len, width, n_head, ldx, ldo, scale, op_dtype, (hipStream_t)stream, FUSED_QKV_W2);
}
extern "C" int ofx_fused_qkv_attention_w2f8(const void* X, const void* Wqkv2, const void* W8, const void* scale8, const float* bias, const float* row_stat,
                                            const float* col_sum, void* out, int nseq, int seq_len, int width, int n_head, int ldx, int ldo, float scale, ofx_stream stream) {
    return ofx_launch_fused_qkv_attn(X, Wqkv2, bias, row_stat, col_sum, out, nseq, seq_len, width, n_head, ldx, ldo, scale, OFX_F16, (hipStream_t)stream, FUSED_QKV_W2F8, W8, scale8);
}
extern "C" int ofx_set_attention(const float* qkv, void* out, const int* cu_seqlens, int nseq, int n_head, int D, int ldo,
                                 int out_kind, int max_len, int only_row0, float scale, int op_dtype, ofx_stream stream) {
    SetAttnArgs a{qkv, out, cu_seqlens, nseq, n_head, D, ldo, out_kind, max_len, only_row0, scale};
    return ofx_launch_set_attention(a, op_dtype, (hipStream_t)stream);
}
// the training step's attention kernels (either setting of ofx_tune(7, v)), with the dropout site built as the step builds it
static bool train_attn_args_ok(const void* a, const void* b, const void* c, int nseq, float dropout_p) {
    return a && b && c && nseq > 0 && dropout_p >= 0.f && dropout_p < 1.f;
}
extern "C" int ofx_attention_varlen(const void* qkv, void* out, const int* cu_seqlens, int nseq, int max_len, int n_head, int ld, int ldo, int k_off,
                                    int v_off, int only_row0, float scale, float dropout_p, unsigned seed, int site, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(train_attn_args_ok(qkv, out, cu_seqlens, nseq, dropout_p), OFX_EINVAL, "attention_varlen: bad argument");
    // q | k | v rows as the training step lays them out; the MFMA attention reads heads of 64 columns and nothing else
    OFX_REQUIRE(n_head > 0 && k_off == n_head * 64 && v_off == 2 * k_off && ld >= 3 * k_off, OFX_ESHAPE,
                "attention_varlen: q | k | v rows of D = n_head * 64 columns (k_off=%d v_off=%d ld=%d n_head=%d); heads of 96 take ofx_set_attention", k_off, v_off, ld, n_head);
    AttnArgs a{qkv, out, nullptr, nseq, max_len, n_head, ld, ldo, k_off, v_off, 0, 0, scale};
    a.cu_seqlens = cu_seqlens; a.only_row0 = only_row0 ? 1 : 0; a.drop = make_drop(dropout_p, seed, (unsigned)site);
    return ofx_launch_attention_mfma(a, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_set_attention_op(const void* qkv, void* out, const int* cu_seqlens, int nseq, int n_head, int D, int ldo, int out_kind, int max_len,
                                    int only_row0, float scale, float dropout_p, unsigned seed, int site, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(train_attn_args_ok(qkv, out, cu_seqlens, nseq, dropout_p) && n_head > 0, OFX_EINVAL, "set_attention_op: bad argument");
    SetAttnArgs a{qkv, out, cu_seqlens, nseq, n_head, D, ldo, out_kind, max_len, only_row0 ? 1 : 0, scale};
    a.drop = make_drop(dropout_p, seed, (unsigned)site); a.qkv_op = 1;
    return ofx_launch_set_attention(a, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_set_attention_bwd(const void* qkv, const float* d_o, void* dqkv, const int* cu_seqlens, int nseq, int n_head, int D, int max_len,
                                     int only_row0, float scale, float dropout_p, unsigned seed, int site, int mfma, int op_dtype, ofx_stream stream) {
    OFX_REQUIRE(train_attn_args_ok(qkv, d_o, dqkv, nseq, dropout_p) && cu_seqlens && n_head > 0, OFX_EINVAL, "set_attention_bwd: bad argument");
    const auto launch = mfma ? ofx_launch_set_attention_bwd_mfma : ofx_launch_set_attention_bwd;
    return launch(qkv, d_o, dqkv, cu_seqlens, nseq, n_head, D, max_len, scale, op_dtype, make_drop(dropout_p, seed, (unsigned)site), only_row0 ? 1 : 0, (hipStream_t)stream);
}
extern "C" int ofx_attention_f32(const float* qkv, void* out, const int64_t* key_mask, int nseq, int seq_len, int n_head, int D, int ldo, int out_kind,
                                 int mask_ld, int causal, float scale, int op_dtype, ofx_stream stream) {
    SetAttnArgs a{qkv, out, nullptr, nseq, n_head, D, ldo, out_kind, seq_len, 0, scale};
    a.fixed_len = seq_len; a.causal = causal; a.key_mask = key_mask; a.mask_ld = mask_ld;
    return ofx_launch_set_attention(a, op_dtype, (hipStream_t)stream);
}
extern "C" int ofx_convert(const float* src, void* dst, int rows, int cols, int mode, int op_dtype, ofx_stream stream) {
    return ofx_launch_pack_rows(src, dst, rows, rows, cols, cols, cols, mode, op_dtype, (hipStream_t)stream);
}
