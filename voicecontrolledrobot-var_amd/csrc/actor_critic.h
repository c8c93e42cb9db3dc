// What the two actor-critic forwards share (armnet.hip: armNet_VAR, ithor_policy.hip: ai2thorNet_VAR): the elementwise
// kernels, the gather-GEMM launch helpers, the workspace both plans lay out, the argument check of the forwards, status /
// free, and the per-layer path (B > 8) from the GRU step to the head.  Include after gg.h, c3f.h and chain.h; every translation
// unit gets its own copy (anonymous namespace).  The layouts, the Kuka band configurations and the chain schedules stay per
// model.  What ithor_reward.hip needs as well (it has no MLP trunk and no chain) sits in image_stack.h.
#pragma once
#include "image_stack.h"

namespace {

// Drop the state in *slot (a struct with a device block `ws`).  A re-plan retires the block, never frees it: a captured
// graph may still replay on it (retire_block keeps it until var_destroy).
template <class S>
int ws_drop(var_ctx* c, void** slot, bool retire) {
    S* st = (S*)*slot;
    if (!st) return VAR_OK;
    if (st->ws && retire) RUN(retire_block(c, st->ws));
    else if (st->ws) (void)hipFree(st->ws);
    delete st;
    *slot = nullptr;
    return VAR_OK;
}

static __global__ void ac_pool_kernel(const float* __restrict__ x, float* __restrict__ y, long n, int H, int HP) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int px = (int)(i % HP), py = (int)((i / HP) % HP);
    const long plane = i / ((long)HP * HP);
    const float* q = x + plane * H * H + (long)(2 * py) * H + 2 * px;
    y[i] = fmaxf(fmaxf(q[0], q[1]), fmaxf(q[H], q[H + 1]));
}
// out = a + b (fusion sums), or out[b][:] = [u[b][:nu] | v[b][:nv]] (the Kuka motor input), or h * mask per row
static __global__ void ac_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}
static __global__ void ac_cat_kernel(const float* __restrict__ u, int nu, const float* __restrict__ v, int nv, float* __restrict__ out, int B) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * (nu + nv)) return;
    const int b = i / (nu + nv), j = i - b * (nu + nv);
    out[i] = j < nu ? u[b * nu + j] : v[b * nv + j - nu];
}
static __global__ void ac_mask_kernel(const float* __restrict__ h, const float* __restrict__ mask, float* __restrict__ out, int B, int H) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * H) out[i] = h[i] * mask[i / H];
}
// torch.nn.GRU cell (gate order r, z, n); gi / gh include their biases
static __global__ void ac_gru_cell_kernel(const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ h,
                                          float* __restrict__ out, float* __restrict__ out2, int B, int H) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, j = i - b * H;
    const float* a = gi + (long)b * 3 * H;
    const float* g = gh + (long)b * 3 * H;
    const float r = 1.f / (1.f + expf(-(a[j] + g[j])));
    const float z = 1.f / (1.f + expf(-(a[H + j] + g[H + j])));
    const float n = tanhf(a[2 * H + j] + r * g[2 * H + j]);
    const float v = (1.f - z) * n + z * h[i];
    out[i] = v;
    if (out2) out2[i] = v;
}

struct Lin { int w, b, in, out; };
inline dim3 g1(long n) { return dim3((unsigned)((n + 255) / 256)); }
constexpr long kSlab = 8L << 20;   // floats of split-K scratch

// ---- the gather-GEMM path (gg.h), layer by layer; slab: kSlab floats of split-K scratch; BF: gg.h's bf16 operand rounding
template <class G, bool U8, bool BF = false>
int conv(var_ctx* c, hipStream_t s, float* slab, const ConvDims& d, const void* x, const float* w, const float* bias, float* y) {
    ConvFwdP<G, U8, false> p{};
    p.M = d.B * d.HO * d.WO; p.N = d.COUT; p.K = d.CIN * G::KHW;
    const long out = (long)p.M * p.N;
    p.nsplit = gg_small_split(((p.M + GG_MT - 1) / GG_MT) * ((p.N + 63) / 64), p.K, out, kSlab);
    p.d = d; p.x = x; p.w = w; p.bias = bias; p.y = y; p.slab = slab; p.sstride = out;
    RUN((gg_launch<ConvFwdP<G, U8, false>, GG_KC, BF>(c, s, p)));
    if (p.nsplit > 1) {
        hipLaunchKernelGGL(gg_finish_kernel, g1(out), dim3(256), 0, s, y, slab, out, p.nsplit, out, bias, d.COUT, d.HO * d.WO, 1);
        AC_CHECK(c);
    }
    return VAR_OK;
}
int linear(var_ctx* c, hipStream_t s, float* slab, const float* P, const Lin& l, const float* X, float* Y, int rows, int relu) {
    const long out = (long)rows * l.out;
    const int ns = gg_small_split(((l.out + GG_MT - 1) / GG_MT) * ((rows + 63) / 64), l.in, out, kSlab);
    if (ns > 1) {
        DenseP<true, true, 2> p{};
        p.M = l.out; p.N = rows; p.K = l.in; p.nsplit = ns;
        p.A = P + l.w; p.sam = l.in; p.sak = 1; p.Bm = X; p.sbk = 1; p.sbn = l.in; p.C = slab; p.scm = 1; p.scn = l.out; p.sC = out;
        RUN(gg_launch(c, s, p));
        hipLaunchKernelGGL(gg_finish_kernel, g1(out), dim3(256), 0, s, Y, slab, out, ns, out, P + l.b, l.out, 1, relu);
        AC_CHECK(c);
        return VAR_OK;
    }
    DenseP<true, true, 0> p{};
    p.M = l.out; p.N = rows; p.K = l.in; p.nsplit = 1;
    p.A = P + l.w; p.sam = l.in; p.sak = 1; p.Bm = X; p.sbk = 1; p.sbn = l.in; p.C = Y; p.scm = 1; p.scn = l.out;
    p.bias = P + l.b; p.relu = relu;
    return gg_launch(c, s, p);
}
int add(var_ctx* c, hipStream_t s, const float* a, const float* b, float* out, int n) {
    hipLaunchKernelGGL(ac_add_kernel, g1(n), dim3(256), 0, s, a, b, out, n);
    AC_CHECK(c);
    return VAR_OK;
}
// 2 x 2 max pool of B maps of ch channels, side hin
int pool(var_ctx* c, hipStream_t s, const float* x, float* y, int B, int ch, int hin) {
    const long n = (long)B * ch * (hin / 2) * (hin / 2);
    hipLaunchKernelGGL(ac_pool_kernel, g1(n), dim3(256), 0, s, x, y, n, hin, hin / 2);
    AC_CHECK(c);
    return VAR_OK;
}

// ---- the workspace: one device block per plan, cut into 64-float-aligned pieces
struct Take {      // without a base it only adds up
    float* base = nullptr;
    long total = 0;
    float* operator()(long n) { const long o = total; total += (n + 63) & ~63L; return base ? base + o : nullptr; }
};
// the parameter offsets both layouts name alike: what the path from the GRU step to the value reads
struct Trunk {
    int g_wih, g_whh, g_bih, g_bhh;
    Lin im2, snd[3], fus[2], all[2], actor[2], critic[2], clin;
};
struct Workspace {
    int maxB = 0;
    float* ws = nullptr;
    float *t0 = nullptr, *t1 = nullptr, *t2 = nullptr, *t3 = nullptr;   // (B,512) scratch rows
    float *flat_img = nullptr, *motor = nullptr, *sound = nullptr, *fusion = nullptr, *h0 = nullptr, *gi = nullptr, *gh = nullptr;
    float* slab = nullptr;
    float* chain = nullptr;        // the small-batch MLP chain's handed-over vectors (chain.h), chain_floats of them
    long chain_floats = 0;
    unsigned* sync = nullptr;      // chain.h: [1] finished workgroups, [2] epoch of the last launch that timed out, [3] epoch of the next
                                   // launch, [4] sticky: some launch timed out since the last clear
    c3f::f32x4* wpk = nullptr;     // the band convolutions' filters in MFMA A-fragment order (c3f.h), re-packed per forward
    c3f::PackDesc pack{};
    // host-side record of the last chain launch's handed-over vectors, by their schedule's names (var_debug_buffer)
    struct ChainVec { const char* name; float* ptr; int width; };
    ChainVec cvec[kChainBufs];
    int ncvec = 0;

    // the pieces both models have, after a model's own feature maps: hidden size rh, nchain floats of chain area
    void take_shared(Take& t, int rh, long nchain) {
        const long B = maxB;
        chain_floats = nchain;
        t0 = t(B * 512); t1 = t(B * 512); t2 = t(B * 512); t3 = t(B * 512);
        flat_img = t(B * 256); motor = t(B * 256); sound = t(B * 256); fusion = t(B * 256); h0 = t(B * rh);
        gi = t(B * 3 * rh); gh = t(B * 3 * rh); slab = t(kSlab);
        chain = t(chain_floats); sync = (unsigned*)t(64);
        wpk = (c3f::f32x4*)t(4L * pack.first[pack.n_layers]);
    }
};
// lay(Take&) cuts the block: run once for the size, once on the allocation; then the chain area carries no tag of any launch
template <class F>
int ws_alloc(var_ctx* c, Workspace* st, F lay) {
    Take size;
    lay(size);
    VAR_HIP_CHECK(c, hipMalloc((void**)&st->ws, (size_t)size.total * sizeof(float)));
    Take cut{st->ws};
    lay(cut);
    VAR_HIP_CHECK(c, hipMemset(st->chain, 0, (size_t)st->chain_floats * sizeof(float)));
    const unsigned init[4] = {0u, 0u, 0u, 1u};                  // [3]: the first launch's epoch
    VAR_HIP_CHECK(c, hipMemset(st->sync, 0, 64 * sizeof(float)));
    VAR_HIP_CHECK(c, hipMemcpy(st->sync, init, sizeof(init), hipMemcpyHostToDevice));
    return VAR_OK;
}

// var_debug_buffer: the pieces both workspaces have, lengths those of the PLAN's batch.  A chain vector (by the name its
// schedule gives it, once a chain launch has run on this plan) is its raw area of (value, tag) pairs, [kChainRows][width] x 2
// words.  1 = found.
inline int ws_debug_buffer(const Workspace* st, int rh, const char* name, void** ptr, long* nfloats) {
    const long B = st->maxB;
    const struct { const char* name; float* p; long n; } fixed[] = {
        {"t0", st->t0, B * 512}, {"t1", st->t1, B * 512}, {"t2", st->t2, B * 512}, {"t3", st->t3, B * 512},
        {"flat_img", st->flat_img, B * 256}, {"motor", st->motor, B * 256}, {"sound", st->sound, B * 256}, {"fusion", st->fusion, B * 256},
        {"h0", st->h0, B * rh}, {"gi", st->gi, B * 3 * rh}, {"gh", st->gh, B * 3 * rh}, {"sync", (float*)st->sync, 64},
        {"chain", st->chain, st->chain_floats}};
    for (auto& f : fixed)
        if (!strcmp(name, f.name)) { *ptr = f.p; *nfloats = f.n; return 1; }
    for (int i = 0; i < st->ncvec; ++i)
        if (!strcmp(name, st->cvec[i].name)) { *ptr = st->cvec[i].ptr; *nfloats = 2L * kChainRows * st->cvec[i].width; return 1; }
    return 0;
}
#define CHAIN_VEC(id, width) {id, width, #id}

// ---- the entry points' common parts; fn: the C function's name for the message, model: "var_armnet" / "var_ithor_policy"
// all_set: no pointer the model requires is NULL.  The image is (B, >= 3, 96, 96) with image_bstride elements between images.
inline int check_forward_args(var_ctx* c, const char* fn, bool all_set, int B, long image_bstride, const float* rnn_hxs,
                              const float* rnn_hxs_out, int rh) {
    if (!all_set || B < 1) { VAR_SET_ERR(c, "%s: NULL argument or B < 1", fn); return VAR_ERR_ARG; }
    if (image_bstride < 3L * 96 * 96) { VAR_SET_ERR(c, "%s: image stride %ld < 3*96*96", fn, image_bstride); return VAR_ERR_ARG; }
    // the small-batch chain reads rnn_hxs from every workgroup of its GRU stage while one of them writes rnn_hxs_out
    const char *a0 = (const char*)rnn_hxs, *b0 = (const char*)rnn_hxs_out;
    const size_t n = (size_t)B * rh * sizeof(float);
    if (a0 < b0 + n && b0 < a0 + n) {
        VAR_SET_ERR(c, "%s: rnn_hxs_out overlaps rnn_hxs (an in-place state update is not supported)", fn);
        return VAR_ERR_ARG;
    }
    return VAR_OK;
}
inline int chain_status(var_ctx* c, const Workspace* st, unsigned* word, const char* model) {
    if (!c) return VAR_ERR_ARG;
    if (!st || !word) { VAR_SET_ERR(c, "%s_status: %s_plan first", model, model); return VAR_ERR_PLAN; }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    return chain_status_word(c, st->sync, word);
}
inline int chain_clear(var_ctx* c, const Workspace* st, const char* model) {
    if (!c) return VAR_ERR_ARG;
    if (!st) { VAR_SET_ERR(c, "%s_clear_status: %s_plan first", model, model); return VAR_ERR_PLAN; }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    return chain_clear_status(c, st->sync);
}

// ---- B > 8 rows, one launch per layer, from the GRU step on.  x: imgMotorMlp's output (B, rin); st->flat_img: image_flatten;
// hnew: the scratch row (B, rh) of the new hidden state; head_out may be NULL (get_value)
int layer_tail(var_ctx* c, hipStream_t s, Workspace* st, const float* P, const Trunk& L, const Lin& head, int rin, int rh, const float* x,
               float* hnew, const float* goal, const float* hxs, const float* masks, int B, float* value, float* actor_features,
               float* head_out, float* hxs_out) {
    float* slab = st->slab;
    // one GRU step from hxs * masks (models/ppo/model.py:118-121)
    hipLaunchKernelGGL(ac_mask_kernel, g1((long)B * rh), dim3(256), 0, s, hxs, masks, st->h0, B, rh);
    AC_CHECK(c);
    const Lin ih{L.g_wih, L.g_bih, rin, 3 * rh}, hh{L.g_whh, L.g_bhh, rh, 3 * rh};
    RUN(linear(c, s, slab, P, ih, x, st->gi, B, 0));
    RUN(linear(c, s, slab, P, hh, st->h0, st->gh, B, 0));
    hipLaunchKernelGGL(ac_gru_cell_kernel, g1((long)B * rh), dim3(256), 0, s, st->gi, st->gh, st->h0, hnew, hxs_out, B, rh);
    AC_CHECK(c);
    RUN(linear(c, s, slab, P, L.im2, hnew, st->t0, B, 1));                         // imageMotorRnn (B,256)
    // sound, fusion
    RUN(linear(c, s, slab, P, L.snd[0], goal, st->t1, B, 1));
    RUN(linear(c, s, slab, P, L.snd[1], st->t1, st->t2, B, 1));
    RUN(linear(c, s, slab, P, L.snd[2], st->t2, st->sound, B, 1));
    RUN(add(c, s, st->sound, st->flat_img, st->t1, B * 256));
    RUN(linear(c, s, slab, P, L.fus[0], st->t1, st->t2, B, 1));
    RUN(linear(c, s, slab, P, L.fus[1], st->t2, st->fusion, B, 1));
    RUN(add(c, s, st->fusion, st->t0, st->t1, B * 256));
    RUN(linear(c, s, slab, P, L.all[0], st->t1, st->t2, B, 1));
    RUN(linear(c, s, slab, P, L.all[1], st->t2, st->t3, B, 1));                    // x (B,128)
    RUN(linear(c, s, slab, P, L.critic[0], st->t3, st->t0, B, 1));
    RUN(linear(c, s, slab, P, L.critic[1], st->t0, st->t1, B, 1));
    RUN(linear(c, s, slab, P, L.clin, st->t1, value, B, 0));
    RUN(linear(c, s, slab, P, L.actor[0], st->t3, st->t0, B, 1));
    RUN(linear(c, s, slab, P, L.actor[1], st->t0, actor_features, B, 1));
    if (head_out) RUN(linear(c, s, slab, P, head, actor_features, head_out, B, 0));
    return VAR_OK;
}

}  // namespace
