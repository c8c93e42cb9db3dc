// C-ABI entry points of libvar_hip.so (see include/var_hip.h).
#include <new>
#include <stdlib.h>
#include <string.h>

#include "var_common.h"

static char g_init_err[256] = "";

#define CHECK_CTX(ctx) do { if (!(ctx)) return VAR_ERR_ARG; } while (0)
#define SET_DEVICE(ctx) VAR_HIP_CHECK(ctx, hipSetDevice((ctx)->device))

extern "C" {

int var_param_count(void) { return VAR_N_PARAMS; }

const char* var_last_error(var_ctx* ctx) { return ctx ? ctx->err : g_init_err; }

static int default_streams();

int var_init(int device_id, var_ctx** out) {
    if (!out) return VAR_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || device_id < 0 || device_id >= n) {
        snprintf(g_init_err, sizeof(g_init_err), "var_init: device %d not available (%d HIP devices, %s)",
                 device_id, n, hipGetErrorString(e));
        return VAR_ERR_HIP;
    }
    var_ctx* c = new (std::nothrow) var_ctx();
    if (!c) return VAR_ERR_HIP;
    c->device = device_id;
    // Which parts of a step leave the caller's stream (bit 0: sound branch forward incl. MFCC, bit 1: sound
    // branch backward); var_set_streams changes the mask (0 = everything on the caller's stream, for per-kernel timing).
    c->streams = default_streams();
    c->pl = make_param_layout();
    c->kl = make_pack_layout();
    if (c->pl.total != VAR_N_PARAMS) {
        snprintf(g_init_err, sizeof(g_init_err), "var_init: layout mismatch %d", c->pl.total);
        delete c;
        return VAR_ERR_ARG;
    }
    e = hipSetDevice(device_id);
    if (e == hipSuccess) e = hipMalloc((void**)&c->default_w.data, sizeof(float) * (size_t)c->kl.total);
    c->default_w.owner = c;
    c->bound = &c->default_w;
    c->wpack = c->default_w.data;
    if (e == hipSuccess) e = hipMalloc((void**)&c->loss_buf, sizeof(float) * (64 + kPpoPartFloats + kOptMaxWG + kOptCarryFloats));
    if (e == hipSuccess) e = hipMemset(c->loss_buf, 0, sizeof(float) * (64 + kPpoPartFloats + kOptMaxWG + kOptCarryFloats));
    c->done_ctr = (unsigned*)(c->loss_buf + 32);
    c->jsig = (unsigned*)(c->loss_buf + 40);          // 16 words
    c->dist_ctr = (unsigned*)(c->loss_buf + 60);
    c->ppo_ctr = (unsigned*)(c->loss_buf + 61);
    c->ppo_part = c->loss_buf + 64;
    c->opt_part = c->ppo_part + kPpoPartFloats;
    c->opt_carry = c->opt_part + kOptMaxWG;
    if (e != hipSuccess) {
        snprintf(g_init_err, sizeof(g_init_err), "var_init: %s", hipGetErrorString(e));
        delete c;
        return VAR_ERR_HIP;
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = hipEventCreateWithFlags(&c->ev_fork[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        snprintf(g_init_err, sizeof(g_init_err), "var_init: %s", hipGetErrorString(e));
        delete c;
        return VAR_ERR_HIP;
    }
    if (mfcc_build_tables(c) != VAR_OK || pack_table_upload(c) != VAR_OK) {
        snprintf(g_init_err, sizeof(g_init_err), "var_init: %s", c->err);
        delete c;
        return VAR_ERR_HIP;
    }
    *out = c;
    return VAR_OK;
}

int var_destroy(var_ctx* c) {
    CHECK_CTX(c);
    (void)hipSetDevice(c->device);
    comm_free(c);
    mfcc_any_forget(c);
    ithor_free(c);
    armnet_free(c);
    ithor_policy_free(c);
    ithor_reward_free(c);
    for (auto& sl : c->ws_slot) if (sl.base) (void)hipFree(sl.base);
    for (int i = 0; i < c->n_retired; i++) (void)hipFree(c->retired[i]);
    free(c->retired);
    if (c->default_w.data) (void)hipFree(c->default_w.data);
    if (c->loss_buf) (void)hipFree(c->loss_buf);
    if (c->mfcc_tab) (void)hipFree(c->mfcc_tab);
    if (c->mfcc_psf_tab) (void)hipFree(c->mfcc_psf_tab);
    if (c->pack_segs_dev) (void)hipFree(c->pack_segs_dev);
    for (int i = 0; i < 2; i++) {
        if (c->ev_fork[i]) (void)hipEventDestroy(c->ev_fork[i]);
        if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
    }
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->prof_ev) {
        for (int i = 0; i < 2 * kProfMaxPairs; i++) (void)hipEventDestroy(c->prof_ev[i]);
        delete[] c->prof_ev;
    }
    delete c;
    return VAR_OK;
}

int retire_block(var_ctx* c, void* p) {
    if (c->n_retired == c->cap_retired) {
        const int cap = c->cap_retired ? 2 * c->cap_retired : 8;
        void** q = (void**)realloc(c->retired, sizeof(void*) * cap);
        if (!q) { VAR_SET_ERR(c, "var_plan: out of host memory"); return VAR_ERR_HIP; }
        c->retired = q; c->cap_retired = cap;
    }
    c->retired[c->n_retired++] = p;
    return VAR_OK;
}

int var_plan_generation(var_ctx* c) { return c ? c->plan_gen : VAR_ERR_ARG; }
int var_saved_generation(var_ctx* c) { return c ? (c->saved_B > 0 ? c->saved_gen : 0) : VAR_ERR_ARG; }

int var_weights_create(var_ctx* c, var_weights** out) {
    CHECK_CTX(c);
    if (!out) return VAR_ERR_ARG;
    *out = nullptr;
    SET_DEVICE(c);
    var_weights* w = new (std::nothrow) var_weights();
    if (!w) return VAR_ERR_HIP;
    w->owner = c;
    hipError_t e = hipMalloc((void**)&w->data, sizeof(float) * (size_t)c->kl.total);
    if (e != hipSuccess) { VAR_SET_ERR(c, "var_weights_create: %s", hipGetErrorString(e)); delete w; return VAR_ERR_HIP; }
    *out = w;
    return VAR_OK;
}

int var_weights_destroy(var_ctx* c, var_weights* w) {
    CHECK_CTX(c);
    if (!w || w->owner != c || w == &c->default_w) { VAR_SET_ERR(c, "var_weights_destroy: not a handle of this context"); return VAR_ERR_ARG; }
    SET_DEVICE(c);
    if (c->bound == w) { c->bound = &c->default_w; c->wpack = c->default_w.data; }
    // like a superseded workspace, the image may still be referenced by captured graphs: retire it
    int rc = retire_block(c, w->data);
    delete w;
    return rc;
}

int var_weights_bind(var_ctx* c, var_weights* w) {
    CHECK_CTX(c);
    if (!w) w = &c->default_w;
    if (w->owner != c) { VAR_SET_ERR(c, "var_weights_bind: handle belongs to another context"); return VAR_ERR_ARG; }
    c->bound = w;
    c->wpack = w->data;
    return VAR_OK;
}

// every entry that reads the packed image checks that it was packed from the arena it is given
static int check_weights(var_ctx* c, const float* params, const char* who) {
    if (c->bound->params != params) {
        VAR_SET_ERR(c, "%s: the bound weight image was %s -- var_weights_bind + var_pack_weights first", who,
                    c->bound->params ? "packed from another parameter arena" : "never packed");
        return VAR_ERR_STATE;
    }
    return VAR_OK;
}

// Carve the workspace block `base` (or, with base == nullptr, only size it) for (B, img_hw) and point the context at it.
static size_t plan_layout(var_ctx* c, char* base, int max_batch, int img_hw) {
    const size_t B = (size_t)max_batch;
    int hs[6];
    hs[0] = img_hw;
    for (int i = 0; i < 5; i++) hs[i + 1] = conv_out(hs[i]);
    size_t off = 0;
    auto carve = [&](size_t nfloats) { size_t o = off; off += (nfloats * 4 + 255) & ~(size_t)255; return o; };
    size_t o_act[6], o_gact[6], o_sact[5], o_gsact[5];
    for (int l = 1; l <= 5; l++) {
        size_t n = B * kImgCh[l] * hs[l] * hs[l];
        // 84 x 84: act1 lives band by band in the forward head's LDS tile layout (img_head2.hip / img_tail2.hip):
        // [image][7 bands][32 channels][300 floats]; its gradient never exists in HBM (gact[1] is var_debug_buffer's scratch)
        if (l == 1 && img_hw == 84) n = B * kAct1TiledFloats;
        o_act[l] = carve(n);
        o_gact[l] = carve(n);
    }
    for (int l = 1; l <= 4; l++) {
        const size_t n = 2 * B * 32 * kSndT[l];
        o_sact[l] = carve(n);
        o_gsact[l] = carve(n);
    }
    const size_t o_hid_i = carve(B * kHid), o_hid_s = carve(2 * B * kHid);
    const size_t o_emb = carve(9 * B), o_emb_raw = carve(9 * B), o_gemb = carve(24 * B), o_hpart = carve(48 * B);
    const size_t o_ghid = carve(6 * B * kHid);
    const size_t n_img_slab = img_slab_floats(), n_snd_slab = snd_slab_floats();
    const size_t o_slab = carve(n_img_slab + n_snd_slab);
    const size_t o_mfcc = carve(2 * B * VAR_MFCC_FRAMES * VAR_MFCC_COEFFS);
    if (!base) return off;
    c->ws = base;
    c->ws_bytes = off;
    auto P = [&](size_t o) { return (float*)(c->ws + o); };
    for (int l = 1; l <= 5; l++) { c->act[l] = P(o_act[l]); c->gact[l] = P(o_gact[l]); }
    for (int l = 1; l <= 4; l++) { c->sact[l] = P(o_sact[l]); c->gsact[l] = P(o_gsact[l]); }
    c->hid_i = P(o_hid_i); c->hid_s = P(o_hid_s);
    c->head_part = P(o_hpart);
    c->emb = P(o_emb); c->emb_raw = P(o_emb_raw); c->gemb = P(o_gemb); c->ghid = P(o_ghid);
    c->slabs = P(o_slab);
    c->mfcc_buf = P(o_mfcc);
    c->slab_floats = n_img_slab + n_snd_slab;
    c->snd_slab_off = n_img_slab;
    c->maxB = max_batch;
    c->H = img_hw;
    for (int i = 0; i < 6; i++) c->hs[i] = hs[i];
    c->saved_B = 0;
    return off;
}

int var_plan(var_ctx* c, int max_batch, int img_hw) {
    CHECK_CTX(c);
    if (max_batch <= 0 || (img_hw != 84 && img_hw != 96)) {
        VAR_SET_ERR(c, "var_plan: batch %d / image size %d unsupported (size must be 84 or 96)", max_batch, img_hw);
        return VAR_ERR_ARG;
    }
    SET_DEVICE(c);
    if (c->ws && c->maxB >= max_batch && c->H == img_hw) return VAR_OK;
    // One workspace per image size, each only ever growing: two models of different image size alternating on one context
    // switch between their two blocks instead of allocating a fresh one per switch (round 2 replaced the block on every
    // change of size: hundreds of MB each time, none released before var_destroy).  A block that must GROW is retired, not
    // freed: HIP graphs captured against it (VARTrainer.capture_*, IntrinsicReward.capture) keep replaying on their own,
    // still valid, buffers.  Freed in var_destroy.
    var_ctx::WsSlot& slot = c->ws_slot[img_hw == 84 ? 0 : 1];
    if (!slot.base || slot.maxB < max_batch) {
        if (slot.base) { int rc = retire_block(c, slot.base); if (rc != VAR_OK) return rc; slot.base = nullptr; }
        if (c->ws && c->H == img_hw) c->ws = nullptr;          // (the active block was this slot's: just retired)
        const int Bn = slot.maxB > max_batch ? slot.maxB : max_batch;
        const size_t bytes = plan_layout(c, nullptr, Bn, img_hw);
        char* blk = nullptr;
        VAR_HIP_CHECK(c, hipMalloc((void**)&blk, bytes));
        VAR_HIP_CHECK(c, hipMemset(blk, 0, bytes));
        slot.base = blk; slot.maxB = Bn;
    }
    c->plan_gen++;                                              // the workspace pointers change: saved forwards are gone
    plan_layout(c, slot.base, slot.maxB, img_hw);
    return VAR_OK;
}

int var_pack_weights(var_ctx* c, void* stream, const float* params) {
    CHECK_CTX(c);
    if (!params) { VAR_SET_ERR(c, "var_pack_weights: null params"); return VAR_ERR_ARG; }
    SET_DEVICE(c);
    c->bound->params = params;
    return launch_pack_weights(c, (hipStream_t)stream, params);
}

static int check_plan(var_ctx* c, int B, int H, const char* who) {
    if (!c->ws) { VAR_SET_ERR(c, "%s: var_plan() has not been called", who); return VAR_ERR_PLAN; }
    if (B <= 0) { VAR_SET_ERR(c, "%s: batch %d", who, B); return VAR_ERR_ARG; }
    if (B > c->maxB || H != c->H) {
        VAR_SET_ERR(c, "%s: batch %d / size %d exceeds the plan (%d / %d)", who, B, H, c->maxB, c->H);
        return VAR_ERR_PLAN;
    }
    return VAR_OK;
}

// Fork the sound branch onto the side stream (it runs beside the image branch: the MFCC front-end
// is VALU work, the image convolutions are matrix-core work) and join it back before the heads.

struct AudioIn {            // optional in-step front-end: pcm != NULL => MFCC is computed here
    const int16_t* pcm = nullptr; const int* lens = nullptr; const int* clip_index = nullptr; int pcm_stride = 0;
};

static int fork_side(var_ctx* c, hipStream_t s, int i) {
    if (!(c->streams & (1 << i))) return VAR_OK;
    VAR_HIP_CHECK(c, hipEventRecord(c->ev_fork[i], s));
    VAR_HIP_CHECK(c, hipStreamWaitEvent(c->side, c->ev_fork[i], 0));
    return VAR_OK;
}
static int join_side(var_ctx* c, hipStream_t s, int i) {
    if (!(c->streams & (1 << i))) return VAR_OK;
    VAR_HIP_CHECK(c, hipEventRecord(c->ev_join[i], c->side));
    VAR_HIP_CHECK(c, hipStreamWaitEvent(s, c->ev_join[i], 0));
    return VAR_OK;
}

// up to five (dst, src, n) segments copied by ONE launch: the encoder outputs of var_arm_encoder_fwd (five
// hipMemcpyAsync calls cost more host time than the B = 8 forward's kernels)
struct CopySegs { float* dst[5]; const float* src[5]; int n[5]; int count; };
__global__ void __launch_bounds__(256) copy_out_kernel(CopySegs S) {
    for (int k = 0; k < S.count; ++k)
        for (int e = blockIdx.x * 256 + threadIdx.x; e < S.n[k]; e += gridDim.x * 256) S.dst[k][e] = S.src[k][e];
}

// gemb = [g0 | g1 | g2], n floats each; a null source contributes zeros
__global__ void __launch_bounds__(256) gemb_in_kernel(const float* __restrict__ g0, const float* __restrict__ g1, const float* __restrict__ g2,
                                                      float* __restrict__ gemb, int n) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    gemb[e] = g0 ? g0[e] : 0.f;
    gemb[n + e] = g1 ? g1[e] : 0.f;
    gemb[2 * n + e] = g2 ? g2[e] : 0.f;
}

__global__ void __launch_bounds__(256) row_dot_kernel(const float* __restrict__ a, const float* __restrict__ b, int rows, int dim,
                                                      float* __restrict__ out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float s = 0.f;
    for (int k = 0; k < dim; ++k) s += a[(size_t)r * dim + k] * b[(size_t)r * dim + k];
    out[r] = s;
}

// calcReward with RLRewardSoundSound on: row_dot_kernel's sum against the goal embedding for the image rows and for the current
// sound's rows, ONE fp32 add of the two (numpy's grouping: two float32 row sums, then their sum); c = NULL leaves row_dot_kernel's bits
__global__ void __launch_bounds__(256) reward_dots_kernel(const float* __restrict__ a, const float* __restrict__ g, const float* __restrict__ c,
                                                          int rows, int dim, float* __restrict__ out, float* __restrict__ out_img,
                                                          float* __restrict__ out_snd) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float s = 0.f, t = 0.f;
    for (int k = 0; k < dim; ++k) s += a[(size_t)r * dim + k] * g[(size_t)r * dim + k];
    if (c)
        for (int k = 0; k < dim; ++k) t += c[(size_t)r * dim + k] * g[(size_t)r * dim + k];
    out[r] = c ? s + t : s;
    if (out_img) out_img[r] = s;
    if (out_snd) out_snd[r] = t;
}

// reward_dots_kernel with the sound embeddings served from a device clip table (rows x dim) by per-row ids.  Goal id gid >= 0:
// table[gid], which also becomes the row's goal_feat; gid == -1 (or no goal ids): goal_feat[r], the row's cached embedding.  With
// current ids cur_feat[r] = table[cid] and out = s + t in reward_dots_kernel's grouping; without them out = s.  An id outside its
// range (goal < -1 or >= table_rows, current < 0 or >= table_rows) leaves NaN in every output of the row and goal_feat[r] as it
// was.  Loads are unconditional from clamped rows; the value is selected afterwards.
__global__ void __launch_bounds__(256) reward_dots_ids_kernel(const float* __restrict__ a, const float* __restrict__ table, int table_rows,
                                                              const int* __restrict__ goal_ids, const int* __restrict__ cur_ids,
                                                              float* goal_feat, float* __restrict__ cur_feat, int rows, int dim,
                                                              float* __restrict__ out, float* __restrict__ out_img,
                                                              float* __restrict__ out_snd) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int gid = goal_ids ? goal_ids[r] : -1, cid = cur_ids ? cur_ids[r] : 0;
    const bool bad = gid < -1 || gid >= table_rows || cid < 0 || cid >= table_rows;
    const bool fresh = gid >= 0 && !bad;
    const float* tg = table + (size_t)(gid >= 0 && gid < table_rows ? gid : 0) * dim;
    const float* tc = table + (size_t)(cid >= 0 && cid < table_rows ? cid : 0) * dim;
    float* gr = goal_feat + (size_t)r * dim;
    const float qnan = __int_as_float(0x7fc00000);
    float s = 0.f, t = 0.f;
    for (int k = 0; k < dim; ++k) {
        const float fresh_v = tg[k], kept_v = gr[k];
        const float g = fresh ? fresh_v : kept_v;
        s += a[(size_t)r * dim + k] * g;
        if (fresh) gr[k] = g;
    }
    if (cur_ids)
        for (int k = 0; k < dim; ++k) {
            const float cv = tc[k];
            t += cv * gr[k];                                   // (this thread's own stores above, or the cached row)
            cur_feat[(size_t)r * dim + k] = bad ? qnan : cv;
        }
    out[r] = bad ? qnan : (cur_ids ? s + t : s);
    if (out_img) out_img[r] = bad ? qnan : s;
    if (out_snd) out_snd[r] = bad ? qnan : t;
}

// inference-only forwards (save_for_bwd = 2) of at most kHead1MaxB images take the round-2 conv 1 + 2 head, at 84 x 84 and at most
// kSmallMidB images also the small conv 3-5 kernels (img_conv_fwd.hip)
static constexpr int kHead1MaxB = 64;
static constexpr int kSmallMidB = 16;

// Which kernels one encoder forward launches and on which streams -- every rule in this one place.  pos / neg: the sound inputs
// as the forward sees them (the in-step MFCC's output included); finish: the embeddings are to be finished (normalised) by the
// forward; join_requested / capturing: the caller asked for the device-side hand-over and `s` is being captured; dot_armed:
// var_set_reward_dot armed this forward.
static FwdPlan plan_encoder_fwd(int H, int B, int save_for_bwd, bool image, bool pos, bool neg, bool finish, bool join_requested,
                                bool capturing, int streams, bool dot_armed, bool front_in_place = false) {
    FwdPlan p;
    const bool fwd_only = save_for_bwd == 2;
    const bool snd = pos || neg;
    // The role-specialised head (img_head2.hip) walks an image's seven bands inside ONE workgroup -- the right shape for a full
    // batch, the wrong one for the RL stage's 8 images, where the per-image latency is the kernel time: an inference-only forward
    // of a small batch takes the round-2 head, which spreads an image's tiles over workgroups; its NCHW act1 is never read by a
    // backward.  At 84 x 84 img_head2 leaves act1 band-tiled for img_tail2.hip, at 96 x 96 as NCHW (img_tail2.hip gathers its
    // bands from the rows).
    const bool head2 = !(fwd_only && B <= kHead1MaxB);
    // The one-launch image forward (conv 1-5 + head, img_fwd_all_kernel: one image per workgroup in both halves) takes 71 us
    // against 41.6 + 36.3 for the two launches -- alone.  Beside the sound branch it LOSES (0.3045 vs 0.3017 ms per step,
    // alternating runs): the step is bound by CU time, not by the image chain's latency, and the sound kernels get onto the CUs at
    // the image kernels' boundaries -- one boundary fewer pushes the sound forward behind the whole image forward.  So: image-only
    // forwards (the frozen encoder at full batch, the projection of a dataset) take the fused launch, a forward with a sound
    // branch the two launches.
    if (head2 && H == 84 && B <= kHead2G && !snd) p.img = ImgPath::All;
    else if (fwd_only && B <= kSmallMidB && H == 84) p.img = ImgPath::Head1Small;
    else p.img = head2 ? ImgPath::Head2Mid3 : ImgPath::Head1Mid3;
    p.act1_tiled = head2 && H == 84;
    p.head_in_conv = p.img != ImgPath::Head1Small;
    p.conv_finish = p.head_in_conv && finish;
    // small batches (the RL stage's 8 envs) stay on the caller's stream: every kernel is a few us there and a fork / join pair
    // costs more than the overlap gives
    p.fork_ok = (streams & 1) && B > 32;
    // The in-place front-end (served clips are not copied: a few us of lookups) runs on the caller's stream IN FRONT of the fork:
    // on the side stream it ended before the image chain's first kernel had got through its queue hand-over, the sound forward
    // took half of the CUs first and img_head2's persistent workgroups doubled up on the rest (measured: img_head2 36.8 -> 51.7 us,
    // img_mid3 47.6 -> 59.4, the step 0.264 -> 0.288 ms).  In front of the fork the image chain follows it on the same queue and
    // it is the sound branch that pays the hand-over, behind img_head2's placement.
    p.mfcc_main = !p.fork_ok || front_in_place;
    // The device-side hand-over only under stream capture: in a replayed graph both branches sit in the device's queues before
    // either starts, so a wait can only be as long as the other branch's kernels; launched eagerly, a host thread that is
    // descheduled between the two branches' launches would turn into a time-out and a step with stale numbers -- and eagerly the
    // edges' cost drowns in launch overhead.
    p.dev_join = join_requested && capturing && p.fork_ok && (streams & 2) && !(streams & 64) && image && pos && neg;
    // The reward's dot rides in the image-head launch where that launch finishes the embeddings itself (one row block: the small
    // path), and is one row_dot_kernel after the embeddings otherwise
    if (dot_armed && image && finish) p.dot = p.img == ImgPath::Head1Small ? RewardDot::InHead : RewardDot::RowDot;
    return p;
}

// join_requested: the caller (the fused training step) goes straight on into encoder_bwd, whose first kernel on `s` is the only
// consumer of the side stream's results: no join here when the plan takes the device-side hand-over -- that kernel waits for the
// sound heads on the device (heads.hip)
static int encoder_fwd(var_ctx* c, hipStream_t s, const float* params, const void* image, int is_u8,
                       long bstride, const int* image_index, const float* pos, const float* neg,
                       const AudioIn* audio, int B, int save_for_bwd, bool finish, bool join_requested, bool dot_armed) {
    int rc;
    if (audio && audio->pcm) {
        pos = c->mfcc_buf;
        neg = c->mfcc_buf + (size_t)B * VAR_MFCC_FRAMES * VAR_MFCC_COEFFS;
    }
    const bool snd = pos || neg;
    // Where the sound CNN reads each clip slot (clip_src.h).  When the front-end runs HERE, into the library's own buffer, under a
    // clip cache bound for this pool, served and empty slots are read in place -- from the cache row, from nowhere -- and the
    // front-end neither copies nor zeroes them: the buffer has no reader but the sound kernels of this forward and its backwards.
    // (Bit 7 of the stream mask keeps the copy; features handed to outside readers -- var_mfcc, var_mfcc_ex -- are always copied.)
    ClipSrc src = {pos, neg, B, nullptr, nullptr, nullptr, nullptr, 0, VAR_MFCC_FRAMES};
    const bool in_place = audio && audio->pcm && !(c->streams & 128) &&
                          mfcc_cache_matches(c, audio->pcm, audio->pcm_stride, VAR_MFCC_FRAMES);
    if (in_place) {
        src.lens = audio->lens; src.clip_index = audio->clip_index;
        src.cache_lens = c->mfcc_cache.lens; src.cache_feats = c->mfcc_cache.feats; src.cache_rows = c->mfcc_cache.rows;
    }
    // (decided before the first launch: the image forward's last kernel raises the flag the sound rows wait for)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (join_requested && hipStreamIsCapturing(s, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    const FwdPlan p = plan_encoder_fwd(c->H, B, save_for_bwd, image, pos, neg, finish, join_requested,
                                       cap == hipStreamCaptureStatusActive, c->streams, dot_armed, in_place);
    c->fwd_plan = p;
    hipStream_t ss = p.fork_ok ? c->side : s;
    // Launch ORDER matters under graph replay: the chain that is enqueued first after a fork keeps the hardware
    // queue of its predecessor, the other branch pays a cross-queue hand-over (5-10 us).  So the caller's stream
    // (MFCC -> image CNN -> image head) is enqueued first and the sound branch, which has slack, afterwards.
    bool forked = false;
    if (snd && audio && audio->pcm) {
        if (!p.mfcc_main) { if ((rc = fork_side(c, s, 0)) != VAR_OK) return rc; forked = true; }
        if ((rc = launch_mfcc(c, p.mfcc_main ? s : ss, audio->pcm, audio->lens, audio->clip_index, 2 * B, audio->pcm_stride,
                              VAR_MFCC_FRAMES, c->mfcc_buf, in_place)) != VAR_OK) return rc;
    }
    if (snd && p.fork_ok && !forked && (rc = fork_side(c, s, 0)) != VAR_OK) return rc;     // the side stream starts after the caller's prior work
    if (image) {
        if ((rc = launch_img_fwd(c, s, p, params, image, is_u8, bstride, image_index, B)) != VAR_OK) return rc;
        if ((rc = launch_heads_fwd(c, s, s, p, params, B, true, false, false, finish)) != VAR_OK) return rc;
        if (p.dot == RewardDot::RowDot) {
            hipLaunchKernelGGL(row_dot_kernel, dim3((B + 255) / 256), dim3(256), 0, s, (const float*)c->emb, c->dot_with, B, kEmb, c->dot_out);
            VAR_HIP_CHECK(c, hipGetLastError());
        }
    }
    if (snd) {
        if ((rc = launch_snd_fwd(c, ss, params, src, B)) != VAR_OK) return rc;
        if ((rc = launch_heads_fwd(c, ss, ss, p, params, B, false, pos != nullptr, neg != nullptr, finish)) != VAR_OK) return rc;
        if (p.fork_ok && !p.dev_join && (rc = join_side(c, s, 0)) != VAR_OK) return rc;
    }
    c->saved_B = B;
    c->saved_gen = ++c->fwd_gen;
    c->saved_image = image;
    c->saved_u8 = is_u8;
    c->saved_bstride = bstride;
    c->saved_index = image_index;
    c->saved_pos = pos;
    c->saved_neg = neg;
    c->saved_src = src;
    return VAR_OK;
}

int var_arm_encoder_fwd(var_ctx* c, void* stream, const float* params, const void* image, int image_is_u8,
                        long image_bstride, const float* mfcc_pos, const float* mfcc_neg, int B, int H,
                        float* image_feat, float* pos_feat, float* neg_feat, float* image_raw, float* pos_raw,
                        int save_for_bwd) {
    CHECK_CTX(c);
    if (!params) { VAR_SET_ERR(c, "var_arm_encoder_fwd: null params"); return VAR_ERR_ARG; }
    if (image && image_bstride < 3L * H * H) { VAR_SET_ERR(c, "var_arm_encoder_fwd: image stride %ld < 3*H*H", image_bstride); return VAR_ERR_ARG; }
    int rc = check_plan(c, B, H, "var_arm_encoder_fwd");
    if (rc != VAR_OK) return rc;
    if ((rc = check_weights(c, params, "var_arm_encoder_fwd")) != VAR_OK) return rc;
    SET_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    // the normalised embeddings go to the caller's buffers from the heads' finish kernels themselves
    c->out_img = image ? image_feat : nullptr; c->out_pos = mfcc_pos ? pos_feat : nullptr; c->out_neg = mfcc_neg ? neg_feat : nullptr;
    rc = encoder_fwd(c, s, params, image, image_is_u8, image_bstride, nullptr, mfcc_pos, mfcc_neg, nullptr, B, save_for_bwd, true,
                     false, c->dot_out != nullptr);
    c->out_img = c->out_pos = c->out_neg = nullptr;
    c->dot_with = nullptr; c->dot_out = nullptr;      // (var_set_reward_dot arms one forward)
    if (rc != VAR_OK) return rc;
    if (save_for_bwd != 1) c->saved_B = 0;
    CopySegs S{};
    auto seg = [&](float* dst, const float* src, int n) { S.dst[S.count] = dst; S.src[S.count] = src; S.n[S.count] = n; S.count++; };
    if (image && image_raw) seg(image_raw, c->act[5], kImgFeat * B);
    if (mfcc_pos && pos_raw) seg(pos_raw, c->sact[4], kSndFeat * B);
    if (S.count) {
        const int grid = (kImgFeat * B + 255) / 256;
        hipLaunchKernelGGL(copy_out_kernel, dim3(grid < 1024 ? grid : 1024), dim3(256), 0, s, S);
        VAR_HIP_CHECK(c, hipGetLastError());
    }
    return VAR_OK;
}

int var_row_dot(var_ctx* c, void* stream, const float* a, const float* b, int rows, int dim, float* out) {
    CHECK_CTX(c);
    if (!a || !b || !out || rows < 1 || dim < 1 || dim > 64) { VAR_SET_ERR(c, "var_row_dot: bad argument (rows %d, dim %d)", rows, dim); return VAR_ERR_ARG; }
    SET_DEVICE(c);
    hipLaunchKernelGGL(row_dot_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, b, rows, dim, out);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}

int var_reward_dots(var_ctx* c, void* stream, const float* image_feat, const float* goal_feat, const float* cur_feat, int rows, int dim,
                    float* out, float* out_img, float* out_snd) {
    CHECK_CTX(c);
    if (!image_feat || !goal_feat || !out || rows < 1 || dim < 1 || dim > 64) {
        VAR_SET_ERR(c, "var_reward_dots: bad argument (rows %d, dim %d)", rows, dim);
        return VAR_ERR_ARG;
    }
    SET_DEVICE(c);
    hipLaunchKernelGGL(reward_dots_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, image_feat, goal_feat, cur_feat, rows,
                       dim, out, out_img, out_snd);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}

int var_reward_dots_ids(var_ctx* c, void* stream, const float* image_feat, const float* table, int table_rows, const int* goal_ids,
                        const int* cur_ids, float* goal_feat, float* cur_feat, int rows, int dim, float* out, float* out_img,
                        float* out_snd) {
    CHECK_CTX(c);
    if (!image_feat || !table || table_rows < 1 || !goal_feat || (cur_ids && !cur_feat) || !out || rows < 1 || dim < 1 || dim > 64) {
        VAR_SET_ERR(c, "var_reward_dots_ids: bad argument (rows %d, dim %d, table_rows %d)", rows, dim, table_rows);
        return VAR_ERR_ARG;
    }
    SET_DEVICE(c);
    hipLaunchKernelGGL(reward_dots_ids_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, image_feat, table, table_rows,
                       goal_ids, cur_ids, goal_feat, cur_feat, rows, dim, out, out_img, out_snd);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}

int var_set_reward_dot(var_ctx* c, const float* goal_feat, float* reward_out) {
    CHECK_CTX(c);
    if ((goal_feat == nullptr) != (reward_out == nullptr)) { VAR_SET_ERR(c, "var_set_reward_dot: both pointers or neither"); return VAR_ERR_ARG; }
    c->dot_with = goal_feat;
    c->dot_out = reward_out;
    return VAR_OK;
}

// fused: the head rows finish the embeddings and form the triplet gradient themselves (heads.hip); the loss value
// is computed on the side branch
static int encoder_bwd(var_ctx* c, hipStream_t s, const float* params, float* grads, bool fused = false,
                       float margin = 0.f, float inv_count = 0.f, float* loss_out = nullptr) {
    const int B = c->saved_B;
    int rc;
    if (!c->saved_image || !c->saved_pos || !c->saved_neg) {
        // a branch that did not run contributes zero gradient
        if ((rc = var_zero_async(c, s, grads, sizeof(float) * VAR_N_PARAMS)) != VAR_OK) return rc;
    }
    const int snd_lo = c->saved_pos ? 0 : B, snd_hi = c->saved_neg ? 2 * B : B;
    // streams: s = image head + the image backward chain, side = sound head + sound CNN backward + loss value
    hipStream_t ss = (c->streams & 2) ? c->side : s;
    // (same ordering rule as in the forward: the caller's chain first, then the side branch)
    // (dev_join: the side stream has not been joined since the forward's fork and needs no edge from `s` either: its rows kernel
    // waits for the image partials on the device)
    const bool dev_join = c->fwd_plan.dev_join;
    if (!dev_join && (rc = fork_side(c, s, 1)) != VAR_OK) return rc;
    if (c->saved_image) {
        if ((rc = launch_heads_bwd(c, s, s, params, grads, B, true, 0, 0, dev_join, fused, margin, inv_count, fused ? loss_out : nullptr)) != VAR_OK) return rc;
        if ((rc = launch_img_bwd(c, s, params, grads, B)) != VAR_OK) return rc;
    }
    if ((rc = launch_heads_bwd(c, ss, ss, params, grads, B, false, snd_lo, snd_hi, dev_join, fused, margin, inv_count)) != VAR_OK) return rc;
    // (fused: the loss value is summed by the image head's backward from the terms its rows kernel leaves -- heads.hip)
    if ((rc = launch_snd_bwd(c, ss, params, grads, B)) != VAR_OK) return rc;
    return join_side(c, s, 1);
}

int var_arm_encoder_bwd(var_ctx* c, void* stream, const float* params, const float* g_image_feat,
                        const float* g_pos_feat, const float* g_neg_feat, float* grads) {
    CHECK_CTX(c);
    if (!params || !grads) { VAR_SET_ERR(c, "var_arm_encoder_bwd: null params/grads"); return VAR_ERR_ARG; }
    if (c->saved_B <= 0) { VAR_SET_ERR(c, "var_arm_encoder_bwd: no forward saved (save_for_bwd=1 required)"); return VAR_ERR_STATE; }
    { int rc = check_weights(c, params, "var_arm_encoder_bwd"); if (rc != VAR_OK) return rc; }
    SET_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    const int B = c->saved_B;
    // the three embedding gradients -> gemb in ONE launch (a branch without a gradient: zeros): three copy launches were 17 us
    // of a 354-us in-batch step
    hipLaunchKernelGGL(gemb_in_kernel, dim3((3 * B + 255) / 256), dim3(256), 0, s, g_image_feat, g_pos_feat, g_neg_feat, c->gemb, 3 * B);
    VAR_HIP_CHECK(c, hipGetLastError());
    return encoder_bwd(c, s, params, grads);
}

int var_triplet_fwd_bwd(var_ctx* c, void* stream, const float* a, const float* p, const float* n, int B,
                        float margin, float inv_count, float* loss_out, float* ga, float* gp, float* gn) {
    CHECK_CTX(c);
    if (!a || !p || !n || !loss_out || B <= 0) { VAR_SET_ERR(c, "var_triplet_fwd_bwd: bad argument"); return VAR_ERR_ARG; }
    SET_DEVICE(c);
    return launch_triplet(c, (hipStream_t)stream, a, p, n, B, margin, inv_count, loss_out, ga, gp, gn);
}

static int loss_grad_impl(var_ctx* c, hipStream_t s, const float* params, const void* image, int image_is_u8,
                          long image_bstride, const int* image_index, const float* mfcc_pos, const float* mfcc_neg,
                          const AudioIn* audio, int B, int H, float margin, float inv_count, float* grads,
                          float* loss_out, float* feats_out, const char* who) {
    if (image_bstride < 3L * H * H) { VAR_SET_ERR(c, "%s: image stride %ld < 3*H*H", who, image_bstride); return VAR_ERR_ARG; }
    int rc = check_plan(c, B, H, who);
    if (rc != VAR_OK) return rc;
    if ((rc = check_weights(c, params, who)) != VAR_OK) return rc;
    SET_DEVICE(c);
    // The training step proper (all three branches, no embedding output requested) takes the fused path: no finish
    // and no triplet kernel on the caller's chain.  (With feats_out the separate finish / triplet kernels run:
    // tests/test_gpu_round2.py::test_config2_batch256_full_batch_parity covers both.)
    const bool fused = !feats_out && image && (mfcc_pos || (audio && audio->pcm)) && (mfcc_neg || (audio && audio->pcm));
    if ((rc = encoder_fwd(c, s, params, image, image_is_u8, image_bstride, image_index, mfcc_pos, mfcc_neg, audio, B, 1,
                          !fused, fused, false)) != VAR_OK) return rc;
    if (fused) {
        rc = encoder_bwd(c, s, params, grads, true, margin, inv_count, loss_out);
        c->fwd_plan.dev_join = false;            // (the hand-over is this backward's: a later var_arm_encoder_bwd takes the edges)
        return rc;
    }
    if ((rc = launch_triplet(c, s, c->emb, c->emb + 3 * B, c->emb + 6 * B, B, margin, inv_count, loss_out,
                             c->gemb, c->gemb + 3 * B, c->gemb + 6 * B)) != VAR_OK) return rc;
    if (feats_out)
        if ((rc = var_copy_async(c, s, feats_out, c->emb, sizeof(float) * 9 * (size_t)B)) != VAR_OK) return rc;
    return encoder_bwd(c, s, params, grads);
}

int var_arm_loss_grad(var_ctx* c, void* stream, const float* params, const void* image, int image_is_u8,
                      long image_bstride, const float* mfcc_pos, const float* mfcc_neg, int B, int H,
                      float margin, float inv_count, float* grads, float* loss_out, float* feats_out) {
    CHECK_CTX(c);
    if (!params || !image || !mfcc_pos || !mfcc_neg || !grads || !loss_out) {
        VAR_SET_ERR(c, "var_arm_loss_grad: null argument");
        return VAR_ERR_ARG;
    }
    return loss_grad_impl(c, (hipStream_t)stream, params, image, image_is_u8, image_bstride, nullptr, mfcc_pos,
                          mfcc_neg, nullptr, B, H, margin, inv_count, grads, loss_out, feats_out, "var_arm_loss_grad");
}

int var_arm_loss_grad_gather(var_ctx* c, void* stream, const float* params, const void* image, int image_is_u8,
                             long image_bstride, const int* image_index, const float* mfcc_pos, const float* mfcc_neg,
                             int B, int H, float margin, float inv_count, float* grads, float* loss_out,
                             float* feats_out) {
    CHECK_CTX(c);
    if (!params || !image || !mfcc_pos || !mfcc_neg || !grads || !loss_out) {
        VAR_SET_ERR(c, "var_arm_loss_grad_gather: null argument");
        return VAR_ERR_ARG;
    }
    return loss_grad_impl(c, (hipStream_t)stream, params, image, image_is_u8, image_bstride, image_index, mfcc_pos,
                          mfcc_neg, nullptr, B, H, margin, inv_count, grads, loss_out, feats_out,
                          "var_arm_loss_grad_gather");
}

int var_arm_loss_grad_pcm(var_ctx* c, void* stream, const float* params, const void* image, int image_is_u8,
                          long image_bstride, const int* image_index, const int16_t* pcm, int pcm_stride,
                          const int* clip_index, const int* lens, int B, int H, float margin, float inv_count,
                          float* grads, float* loss_out, float* feats_out) {
    CHECK_CTX(c);
    if (!params || !image || !pcm || !lens || !grads || !loss_out || pcm_stride <= 0) {
        VAR_SET_ERR(c, "var_arm_loss_grad_pcm: null argument");
        return VAR_ERR_ARG;
    }
    AudioIn a;
    a.pcm = pcm; a.lens = lens; a.clip_index = clip_index; a.pcm_stride = pcm_stride;
    return loss_grad_impl(c, (hipStream_t)stream, params, image, image_is_u8, image_bstride, image_index, nullptr,
                          nullptr, &a, B, H, margin, inv_count, grads, loss_out, feats_out, "var_arm_loss_grad_pcm");
}

int var_adam_step(var_ctx* c, void* stream, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                  long n, float lr, float beta1, float beta2, float eps, float weight_decay, int step) {
    CHECK_CTX(c);
    if (!params || !grads || !exp_avg || !exp_avg_sq || n <= 0 || step < 1) {
        VAR_SET_ERR(c, "var_adam_step: bad argument");
        return VAR_ERR_ARG;
    }
    SET_DEVICE(c);
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_adam(c, s, params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step);
    if (rc != VAR_OK) return rc;
    if (n == VAR_N_PARAMS && c->bound->params == params) return launch_pack_weights(c, s, params);
    return VAR_OK;
}

// the device-counter step behind both entries; `who` names the entry in the error text
static int adam_step_dev_impl(var_ctx* c, void* stream, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                              long n, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                              int* step_dev, const int* index_table, int row_ints, int n_rows, int* cursor_dev,
                              int* index_row, int ahead_from, const char* who) {
    CHECK_CTX(c);
    if (!params || !grads || !exp_avg || !exp_avg_sq || !lr_dev || !step_dev || n <= 0) {
        VAR_SET_ERR(c, "%s: bad argument", who);
        return VAR_ERR_ARG;
    }
    if (index_table && (!cursor_dev || !index_row || row_ints <= 0 || n_rows <= 0)) {
        VAR_SET_ERR(c, "%s: index table without cursor / row buffer / sizes", who);
        return VAR_ERR_ARG;
    }
    SET_DEVICE(c);
    return launch_adam_dev(c, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n, lr_dev, beta1, beta2, eps,
                           weight_decay, step_dev, n == VAR_N_PARAMS && c->bound->params == params, index_table, row_ints, n_rows, cursor_dev, index_row,
                           ahead_from);
}

int var_adam_step_dev(var_ctx* c, void* stream, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                      long n, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                      int* step_dev) {
    return adam_step_dev_impl(c, stream, params, grads, exp_avg, exp_avg_sq, n, lr_dev, beta1, beta2, eps, weight_decay,
                              step_dev, nullptr, 0, 0, nullptr, nullptr, 0, "var_adam_step_dev");
}

int var_adam_step_graph(var_ctx* c, void* stream, float* params, const float* grads, float* exp_avg,
                        float* exp_avg_sq, long n, const float* lr_dev, float beta1, float beta2, float eps,
                        float weight_decay, int* step_dev, const int* index_table, int row_ints, int n_rows,
                        int* cursor_dev, int* index_row, int ahead_from) {
    return adam_step_dev_impl(c, stream, params, grads, exp_avg, exp_avg_sq, n, lr_dev, beta1, beta2, eps, weight_decay,
                              step_dev, index_table, row_ints, n_rows, cursor_dev, index_row, ahead_from, "var_adam_step_graph");
}

int var_mfcc(var_ctx* c, void* stream, const int16_t* pcm, const int* lens, const int* clip_index, int nclips,
             int pcm_stride, int out_frames, float* out) {
    CHECK_CTX(c);
    if (!pcm || !lens || !out || nclips <= 0 || pcm_stride <= 0 || out_frames <= 0) {
        VAR_SET_ERR(c, "var_mfcc: bad argument");
        return VAR_ERR_ARG;
    }
    SET_DEVICE(c);
    return launch_mfcc(c, (hipStream_t)stream, pcm, lens, clip_index, nclips, pcm_stride, out_frames, out);
}

// measurement hook (tools/mfcc_time.py): the in-place form of the cached front-end on its own -- the launch the training step
// makes under a binding; served and empty slots of `out` are left as they are
int var_debug_mfcc_in_place(var_ctx* c, void* stream, const int16_t* pcm, const int* lens, const int* clip_index, int nclips,
                            int pcm_stride, float* out) {
    CHECK_CTX(c);
    if (!pcm || !lens || !out || nclips <= 0 || pcm_stride <= 0) { VAR_SET_ERR(c, "var_debug_mfcc_in_place: bad argument"); return VAR_ERR_ARG; }
    if (!mfcc_cache_matches(c, pcm, pcm_stride, VAR_MFCC_FRAMES)) { VAR_SET_ERR(c, "var_debug_mfcc_in_place: no cache bound for this pool"); return VAR_ERR_STATE; }
    SET_DEVICE(c);
    return launch_mfcc(c, (hipStream_t)stream, pcm, lens, clip_index, nclips, pcm_stride, VAR_MFCC_FRAMES, out, true);
}

int var_mfcc_cache_bind(var_ctx* c, const int16_t* pcm, int rows, int pcm_stride, int out_frames, const int* cache_lens,
                        const float* cache_feats) {
    CHECK_CTX(c);
    if (!pcm || !cache_lens || !cache_feats || rows <= 0 || pcm_stride <= 0 || out_frames <= 0 ||
        (long)rows * out_frames >= (1L << 31)) {
        VAR_SET_ERR(c, "var_mfcc_cache_bind: bad argument");
        return VAR_ERR_ARG;
    }
    c->mfcc_cache = {pcm, rows, pcm_stride, out_frames, cache_lens, cache_feats};
    return VAR_OK;
}

int var_mfcc_cache_unbind(var_ctx* c) {
    CHECK_CTX(c);
    c->mfcc_cache = {nullptr, 0, 0, 0, nullptr, nullptr};
    return VAR_OK;
}

int var_mfcc_ex(var_ctx* c, void* stream, const int16_t* pcm, const int* lens, const int* clip_index, int nclips,
                int pcm_stride, int out_frames, int n_fft, int win_length, int hop_length, float* out) {
    CHECK_CTX(c);
    if (!pcm || !lens || !out || nclips <= 0 || pcm_stride <= 0 || out_frames <= 0) {
        VAR_SET_ERR(c, "var_mfcc_ex: bad argument");
        return VAR_ERR_ARG;
    }
    SET_DEVICE(c);
    if (n_fft == 512 && win_length == 400 && hop_length == 160)
        return launch_mfcc(c, (hipStream_t)stream, pcm, lens, clip_index, nclips, pcm_stride, out_frames, out);
    return launch_mfcc_any(c, (hipStream_t)stream, pcm, lens, clip_index, nclips, pcm_stride, out_frames, n_fft, win_length,
                           hop_length, out);
}

// what each profiled launch computes (both image sizes; bench.py maps (tag, image size) to the kernel's name)
static const char* kTagNames[TAG_COUNT] = {
    "(unused)", "img conv1+conv2 forward", "img conv3+4+5 forward + image head", "(unused)",
    "(unused)", "(unused)", "(unused)", "img conv3+4+5 weight gradients",
    "(unused)", "(unused)", "(unused)",
    "img conv2 data gradient + conv2, conv1 weight gradients",
    "img conv5-4-3 data gradient chain", "(unused)", "(unused)", "img weight-gradient slab fold",
    "snd_fwd_kernel", "snd_dgrad_kernel", "snd_wgrad_kernel", "snd_reduce_kernel", "heads_fwd_kernel",
    "heads_bwd_rows_kernel", "heads_bwd_gemm_kernel", "triplet_kernel", "adam_kernel", "pack_weights_kernel",
    "mfcc_kernel", "ithor conv 11x5 s2 forward", "ithor conv 11x5 s2 data gradient", "ithor conv 11x5 s2 weight gradient"};

int var_profile_tag_count(void) { return TAG_COUNT; }
const char* var_profile_tag_name(int tag) { return (tag >= 0 && tag < TAG_COUNT) ? kTagNames[tag] : ""; }

/* Record HIP events (on the launch stream) around every launch of kernel family `tag`
 * from now on (-1 = off).  Not for use under graph capture. */
static int default_streams() { return kDefaultStreams; }

int var_set_streams(var_ctx* c, int mask) {
    if (!c) return -1;
    const int old = c->streams;
    // bit 6: keep the graph edge between the forward's two streams; bit 7: served clips are copied into the feature buffer
    c->streams = mask < 0 ? default_streams() : (mask & (3 | 64 | 128));
    return old;
}

int var_join_status(var_ctx* c, unsigned* timeouts) {
    CHECK_CTX(c);
    if (!timeouts) { VAR_SET_ERR(c, "var_join_status: null argument"); return VAR_ERR_ARG; }
    SET_DEVICE(c);
    unsigned w[8];
    VAR_HIP_CHECK(c, hipMemcpy(w, c->jsig, sizeof(w), hipMemcpyDeviceToHost));
    *timeouts = w[3] + w[7];
    return VAR_OK;
}

int var_profile_select(var_ctx* c, int tag) {
    CHECK_CTX(c);
    SET_DEVICE(c);
    if (tag >= TAG_COUNT) { VAR_SET_ERR(c, "var_profile_select: bad tag %d", tag); return VAR_ERR_ARG; }
    if (tag >= 0 && !c->prof_ev) {
        c->prof_ev = new hipEvent_t[2 * kProfMaxPairs];
        for (int i = 0; i < 2 * kProfMaxPairs; i++) VAR_HIP_CHECK(c, hipEventCreate(&c->prof_ev[i]));
    }
    c->prof_tag = tag;
    c->prof_n = 0;
    return VAR_OK;
}

/* Sum of the event-pair durations recorded since var_profile_select, and their count. Synchronises. */
int var_profile_read(var_ctx* c, float* total_ms, int* count) {
    CHECK_CTX(c);
    if (!total_ms || !count) return VAR_ERR_ARG;
    SET_DEVICE(c);
    float tot = 0.f;
    for (int i = 0; i < c->prof_n; i++) {
        float ms = 0.f;
        VAR_HIP_CHECK(c, hipEventSynchronize(c->prof_ev[2 * i + 1]));
        VAR_HIP_CHECK(c, hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
        tot += ms;
    }
    *total_ms = tot;
    *count = c->prof_n;
    return VAR_OK;
}

/* Testing hook: address and length (floats) of a workspace buffer, by name
 * ("act1".."act5", "gact1".."gact5", "sact1".."sact4", "gsact1".."gsact4", "emb", "gemb", "wpack", the heads' rows
 * "emb_raw", "head_part", "graw", "ghid";
 * iTHOR workspace: "ithor_s1".."ithor_s3", "ithor_gs1".."ithor_gs3": sound conv outputs / their gradients, sized for
 * the planned batch; the acting forwards' workspaces: "arm_..." (armnet.hip), "ipol_..." (ithor_policy.hip), the reward plan's: "irew_..."
 * (ithor_reward.hip), names in include/var_hip.h). */
int var_debug_buffer(var_ctx* c, const char* name, void** ptr, long* nfloats) {
    CHECK_CTX(c);
    if (!name || !ptr || !nfloats) return VAR_ERR_ARG;
    const size_t B = c->maxB;
    *ptr = nullptr; *nfloats = 0;
    if (!strcmp(name, "wpack")) { *ptr = c->wpack; *nfloats = c->kl.total; return VAR_OK; }
    if (!strncmp(name, "ithor_", 6)) return ithor_debug_buffer(c, name + 6, ptr, nfloats);
    if (!strncmp(name, "arm_", 4)) return armnet_debug_buffer(c, name + 4, ptr, nfloats);
    if (!strncmp(name, "ipol_", 5)) return ithor_policy_debug_buffer(c, name + 5, ptr, nfloats);
    if (!strncmp(name, "irew_", 5)) return ithor_reward_debug_buffer(c, name + 5, ptr, nfloats);
    if (!c->ws) { VAR_SET_ERR(c, "var_debug_buffer: no plan"); return VAR_ERR_PLAN; }
    for (int l = 1; l <= 5; l++) {
        char a[16], g[16];
        snprintf(a, sizeof a, "act%d", l); snprintf(g, sizeof g, "gact%d", l);
        const long n = (long)(B * kImgCh[l] * c->hs[l] * c->hs[l]);
        if (!strcmp(name, a)) {
            *ptr = c->act[l]; *nfloats = n;
            if (l == 1 && c->fwd_plan.act1_tiled) {          // the tiled form -> NCHW, into the (otherwise unused) gact[1] block
                int rc = launch_act1_untile(c, nullptr, (int)B);
                if (rc != VAR_OK) return rc;
                VAR_HIP_CHECK(c, hipStreamSynchronize(nullptr));
                *ptr = c->gact[1];
            }
            return VAR_OK;
        }
        if (!strcmp(name, g)) { *ptr = c->gact[l]; *nfloats = n; return VAR_OK; }
    }
    for (int l = 1; l <= 4; l++) {
        char a[16], g[16];
        snprintf(a, sizeof a, "sact%d", l); snprintf(g, sizeof g, "gsact%d", l);
        const long n = (long)(2 * B * 32 * kSndT[l]);
        if (!strcmp(name, a)) { *ptr = c->sact[l]; *nfloats = n; return VAR_OK; }
        if (!strcmp(name, g)) { *ptr = c->gsact[l]; *nfloats = n; return VAR_OK; }
    }
    if (!strcmp(name, "hid_i")) { *ptr = c->hid_i; *nfloats = (long)B * kHid; return VAR_OK; }
    if (!strcmp(name, "hid_s")) { *ptr = c->hid_s; *nfloats = 2 * (long)B * kHid; return VAR_OK; }
    if (!strcmp(name, "emb")) { *ptr = c->emb; *nfloats = 9 * (long)B; return VAR_OK; }
    if (!strcmp(name, "mfcc")) { *ptr = c->mfcc_buf; *nfloats = 2 * (long)B * VAR_MFCC_FRAMES * VAR_MFCC_COEFFS; return VAR_OK; }
    if (!strcmp(name, "slabs")) { *ptr = c->slabs; *nfloats = (long)c->slab_floats; return VAR_OK; }
    if (!strcmp(name, "gemb")) { *ptr = c->gemb; *nfloats = 9 * (long)B; return VAR_OK; }
    // the heads' rows, all (3 maxB) stacks [image | positive | negative] filled with B-based offsets (heads.hip)
    if (!strcmp(name, "emb_raw")) { *ptr = c->emb_raw; *nfloats = 9 * (long)B; return VAR_OK; }
    if (!strcmp(name, "head_part")) { *ptr = c->head_part; *nfloats = 48 * (long)B; return VAR_OK; }
    if (!strcmp(name, "graw")) { *ptr = c->gemb + 9 * B; *nfloats = 12 * (long)B; return VAR_OK; }
    if (!strcmp(name, "ghid")) { *ptr = c->ghid; *nfloats = 3 * (long)B * kHid; return VAR_OK; }
    VAR_SET_ERR(c, "var_debug_buffer: unknown buffer '%s'", name);
    return VAR_ERR_ARG;
}

}  // extern "C"
