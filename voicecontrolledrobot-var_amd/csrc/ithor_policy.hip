// iTHOR RL actor-critic forward on gfx950: models/RL/ai2thor_RL_model.py:7-121 `ai2thorNet_VAR` (96x96 image stack: 6
// convolutions / 4 max pools -> 1152, the occupancy branch: 2 convolutions 9 -> 5 -> 3 + 2 Linear layers, the motor / image /
// sound MLPs, one GRU(128 -> 1024) step through NNBase._forward_gru's acting path, models/ppo/model.py:116-121, fusion and the
// actor / critic trunks) followed by Categorical's logit layer (models/ppo/distributions.py), i.e. everything of Policy.act
// up to the sampling.  Inference only.  The same three regimes as armnet.hip: up to 64 images the image stack runs on the
// LDS-band kernels of c3f.h (filters re-packed per call inside conv 1's launch), up to 8 rows the 22 Linear layers + GRU
// step run as one persistent launch (chain.h), larger batches take the gather-GEMM of gg.h layer by layer with the
// parameters in place in their state_dict() layouts.  var_ithor_policy_forward_ex's flags bit 0 runs the imgCNN convolutions on
// operands rounded to bf16 as armnet.hip's does (conv 2..5 on c3f_bf16.h's band kernel); the occupancy convolutions stay fp32.
// What this forward shares with armnet.hip -- the elementwise kernels, the
// launch helpers, the workspace, the band configurations of the image stack (also ithor_reward.hip's), the per-layer path from
// the GRU step on -- lives in actor_critic.h.
#include <string.h>

#include <type_traits>

#include "gg.h"

namespace {
PH_DECL();
}
#include "c3f.h"
#include "chain.h"
#include "actor_critic.h"

namespace {
constexpr int kCh[7] = {3, 32, 32, 64, 64, 128, 128};       // imgCNN channels, conv l: kCh[l - 1] -> kCh[l]
constexpr int kSide[7] = {96, 96, 96, 48, 24, 12, 3};       // output side of conv l (before its pool)
constexpr int kRepr = 3, kRin = 128, kRh = 1024, kAct = 128, kFlat = 1152, kOcc = 288, kMaxActions = 16;

struct PolLayout : Trunk {
    int cw[6], cb[6];          // imgCNN.{0,2,5,8,11,14}
    int ow[2], ob[2];          // occupancyCNNMLP.{0,2}
    Lin occ[2];                // occupancyCNNMLP.{5,7}
    Lin motor[2], cnn[2], im[2], logit;
    int total;
};

PolLayout make_layout(int n_actions) {
    PolLayout L{};
    int o = 0;
    L.g_wih = o; o += 3 * kRh * kRin; L.g_whh = o; o += 3 * kRh * kRh; L.g_bih = o; o += 3 * kRh; L.g_bhh = o; o += 3 * kRh;
    for (int i = 0; i < 6; i++) { L.cw[i] = o; o += kCh[i + 1] * kCh[i] * 9; L.cb[i] = o; o += kCh[i + 1]; }
    L.ow[0] = o; o += 64 * 9; L.ob[0] = o; o += 64;
    L.ow[1] = o; o += 32 * 64 * 9; L.ob[1] = o; o += 32;
    auto lin = [&](int in, int out) { Lin l{o, o + in * out, in, out}; o += in * out + out; return l; };
    L.occ[0] = lin(kOcc, 128); L.occ[1] = lin(128, 256);
    L.motor[0] = lin(kRepr, 64); L.motor[1] = lin(64, 256);
    L.cnn[0] = lin(kFlat, 512); L.cnn[1] = lin(512, 256);
    L.im[0] = lin(256, 64); L.im[1] = lin(64, kRin);
    L.im2 = lin(kRh, 256);
    L.snd[0] = lin(kRepr, 128); L.snd[1] = lin(128, 256); L.snd[2] = lin(256, 256);
    L.fus[0] = lin(256, 512); L.fus[1] = lin(512, 256);
    L.all[0] = lin(256, 256); L.all[1] = lin(256, 128);
    L.actor[0] = lin(128, 128); L.actor[1] = lin(128, kAct);
    L.critic[0] = lin(128, 128); L.critic[1] = lin(128, 128);
    L.clin = lin(128, 1);
    L.logit = lin(kAct, n_actions);
    L.total = o;
    return L;
}

constexpr long kChainFloats = (long)kChainRows * 32768;

struct pol_state : Workspace {
    int n_actions = 0;
    PolLayout L;
    float *a[7] = {nullptr}, *p[5] = {nullptr};        // conv outputs 1..6 (a[2..5]: the gather-GEMM path only), pooled maps 1..4
    float* occf = nullptr;                             // (B, 288): the occupancy convolutions' flattened output
    float *occ = nullptr, *h1 = nullptr;               // the occupancy branch (B, 256), the new hidden state (B, 1024)
};

// occupancyCNNMLP's two convolutions (1 -> 64, 3x3 s2 p1, 9 -> 5; 64 -> 32, 3x3 s2 p1, 5 -> 3; ReLU each): 0.2 MFLOP per env,
// the (B, 288) flattened maps feed the first occupancy Linear layer.  A workgroup = (env, kOccCo output channels of the second
// convolution): it recomputes the first one (14 K FMAs), stages its share of the second filter in LDS and splits each output's
// 576 products over kOccKs threads (one thread per output streaming them from memory took 100 us, from LDS 32 us).
constexpr int kOccT = 256, kOccCo = 2, kOccKs = 8;
template <bool U8>
__global__ void __launch_bounds__(kOccT) ip_occ_kernel(const void* __restrict__ occ, const float* __restrict__ P, int w0, int b0, int w1,
                                                      int b1, float* __restrict__ out) {
    __shared__ float x[81];
    __shared__ float h[64 * 25];
    __shared__ float wl[kOccCo * 64 * 9];
    const int b = blockIdx.x / (32 / kOccCo), co0 = (blockIdx.x % (32 / kOccCo)) * kOccCo, tid = threadIdx.x;
    if (tid < 81) x[tid] = U8 ? (float)((const uint8_t*)occ)[(long)b * 81 + tid] / 255.f : ((const float*)occ)[(long)b * 81 + tid];
    for (int e = tid; e < kOccCo * 64 * 9; e += kOccT) wl[e] = P[w1 + (long)co0 * 64 * 9 + e];
    __syncthreads();
    for (int e = tid; e < 64 * 25; e += kOccT) {
        const int co = e / 25, py = (e % 25) / 5, px = e % 5;
        float s = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = 2 * py - 1 + ky, ix = 2 * px - 1 + kx;
                if (iy >= 0 && iy < 9 && ix >= 0 && ix < 9) s = fmaf(P[w0 + co * 9 + ky * 3 + kx], x[iy * 9 + ix], s);
            }
        s += P[b0 + co];
        h[e] = s > 0.f ? s : 0.f;
    }
    __syncthreads();
    // second convolution: kOccCo * 9 outputs x kOccKs slices of 64 / kOccKs input channels, the partial sums folded in slice order
    constexpr int NO = kOccCo * 9, CS = 64 / kOccKs;
    __shared__ float red[kOccKs * NO];
    if (tid < NO * kOccKs) {
        const int o = tid % NO, sl = tid / NO, col = o / 9, py = (o % 9) / 3, px = o % 3;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CS; ++c) {
            const int ci = sl * CS + c;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int iy = 2 * py - 1 + ky, ix = 2 * px - 1 + kx;
                    if (iy >= 0 && iy < 5 && ix >= 0 && ix < 5) s = fmaf(wl[(col * 64 + ci) * 9 + ky * 3 + kx], h[ci * 25 + iy * 5 + ix], s);
                }
        }
        red[sl * NO + o] = s;
    }
    __syncthreads();
    if (tid < NO) {
        float s = red[tid];
#pragma unroll
        for (int sl = 1; sl < kOccKs; ++sl) s += red[sl * NO + tid];
        s += P[b1 + co0 + tid / 9];
        out[(long)b * kOcc + co0 * 9 + tid] = s > 0.f ? s : 0.f;
    }
}

// Everything after the convolutions for B <= 8 rows as ONE persistent launch (chain.h).  Stages (jobs of one stage run side
// by side; W_hh . (h * mask) depends on kernel inputs only and streams its 12.6 MB in the first stage):
//   1 cnnMlp.0 (1152 -> 512), motorMlp.0 (3 -> 64), soundMlp.0 (3 -> 128), occupancy Linear 0 (288 -> 128), W_hh (1024 -> 3072)
//   2 cnnMlp.2 -> image_flatten, motorMlp.2 -> motor, soundMlp.2, occupancy Linear 1 -> occupancy
//   3 imgMotorMlp.0 (image_flatten + motor + occupancy), soundMlp.4 -> sound
//   4 imgMotorMlp.2, fusionMlp.0 (sound + image_flatten)      5 W_ih (128 -> 3072), fusionMlp.2 -> fusion
//   6 GRU cell -> imgMotorMlp2      7 mlp_all.0 (fusion + imageMotorRnn)      8 mlp_all.2
//   9 critic.0, actor.0      10 critic.2, actor.2 -> actor features      11 critic_linear -> value, Categorical linear -> logits
int chain_forward(var_ctx* c, hipStream_t s, pol_state* st, const float* P, const float* image_feat, const float* goal,
                  const float* hxs, const float* masks, int B, float* value, float* actor_features, float* logits, float* hxs_out) {
    const PolLayout& L = st->L;
    ChainDesc D{};
    D.P = P; D.B = B; D.H = kRh; D.sync = st->sync;
    enum { A6, OCCF, IMGF, GOAL, HXS, MASK, HOUT, VALUE, AFEAT, LOGITS, CNN0, FLAT, M0, MOTOR, S0, S1, SOUND, O0, OCC, GH, IM0, X, F0,
           FUSION, GI, IMR, ALL0, ALL1, C0, C1, A0, AFT, NBUF };
    static_assert(NBUF <= kChainBufs, "buffer table");
    float* sc = st->chain;
    auto scratch = [&](int width) { float* p = sc; sc += kChainRows * width * 2; return p; };     // (value, tag) pairs
    D.buf[A6] = st->a[6]; D.buf[OCCF] = st->occf; D.buf[IMGF] = (float*)image_feat; D.buf[GOAL] = (float*)goal;
    D.buf[HXS] = (float*)hxs; D.buf[MASK] = (float*)masks; D.buf[HOUT] = hxs_out; D.buf[VALUE] = value; D.buf[AFEAT] = actor_features;
    D.buf[LOGITS] = logits ? logits : scratch(kMaxActions);
    const struct { int id, width; const char* name; } widths[] = {
        CHAIN_VEC(CNN0, 512), CHAIN_VEC(FLAT, 256), CHAIN_VEC(M0, 64), CHAIN_VEC(MOTOR, 256), CHAIN_VEC(S0, 128), CHAIN_VEC(S1, 256),
        CHAIN_VEC(SOUND, 256), CHAIN_VEC(O0, 128), CHAIN_VEC(OCC, 256), CHAIN_VEC(GH, 3 * kRh), CHAIN_VEC(IM0, 64), CHAIN_VEC(X, kRin),
        CHAIN_VEC(F0, 512), CHAIN_VEC(FUSION, 256), CHAIN_VEC(GI, 3 * kRh), CHAIN_VEC(IMR, 256), CHAIN_VEC(ALL0, 256), CHAIN_VEC(ALL1, 128),
        CHAIN_VEC(C0, 128), CHAIN_VEC(C1, 128), CHAIN_VEC(A0, 128), CHAIN_VEC(AFT, kAct)};
    st->ncvec = 0;
    for (auto& wd : widths) {                                                                   // handed over inside the launch
        D.buf[wd.id] = scratch(wd.width); D.tagged |= 1ull << wd.id;
        st->cvec[st->ncvec++] = {wd.name, D.buf[wd.id], wd.width};
    }
    D.b_hxs = HXS; D.b_mask = MASK; D.b_hout = HOUT;
    ChainBuilder cb(D);
    auto job = [&](const Lin& l, int kind, int in0, int in1, int out, int relu, int out2 = -1, int in2 = -1) {
        cb.job(l.w, l.b, l.in, l.out, kind, in0, in1, 0, out, relu, out2, in2);
    };
    const Lin ih{L.g_wih, L.g_bih, kRin, 3 * kRh}, hh{L.g_whh, L.g_bhh, kRh, 3 * kRh};
    cb.stage(); job(L.cnn[0], IN_PLAIN, A6, -1, CNN0, 1); job(L.motor[0], IN_PLAIN, IMGF, -1, M0, 1); job(L.snd[0], IN_PLAIN, GOAL, -1, S0, 1);
                job(L.occ[0], IN_PLAIN, OCCF, -1, O0, 1); job(hh, IN_MASK, HXS, MASK, GH, 0);
    cb.split();
    cb.stage(); job(L.cnn[1], IN_PLAIN, CNN0, -1, FLAT, 1); job(L.motor[1], IN_PLAIN, M0, -1, MOTOR, 1); job(L.snd[1], IN_PLAIN, S0, -1, S1, 1);
                job(L.occ[1], IN_PLAIN, O0, -1, OCC, 1);
    cb.split();
    cb.stage(); job(L.im[0], IN_SUM, FLAT, MOTOR, IM0, 1, -1, OCC); job(L.snd[2], IN_PLAIN, S1, -1, SOUND, 1);
    cb.split();
    cb.stage(); job(L.im[1], IN_PLAIN, IM0, -1, X, 1); job(L.fus[0], IN_SUM, SOUND, FLAT, F0, 1);
    cb.split();
    cb.stage(); job(ih, IN_PLAIN, X, -1, GI, 0); job(L.fus[1], IN_PLAIN, F0, -1, FUSION, 1);
    cb.split();
    cb.stage(); job(L.im2, IN_GRU, GI, GH, IMR, 1);                                  // the GRU cell is its input transform
    cb.split();
    cb.stage(); job(L.all[0], IN_SUM, FUSION, IMR, ALL0, 1);
    cb.split();
    cb.stage(); job(L.all[1], IN_PLAIN, ALL0, -1, ALL1, 1);
    cb.split();
    cb.stage(); job(L.critic[0], IN_PLAIN, ALL1, -1, C0, 1); job(L.actor[0], IN_PLAIN, ALL1, -1, A0, 1);
    cb.split();
    cb.stage(); job(L.critic[1], IN_PLAIN, C0, -1, C1, 1); job(L.actor[1], IN_PLAIN, A0, -1, AFT, 1, AFEAT);
    cb.split();
    cb.stage(); job(L.clin, IN_PLAIN, C1, -1, VALUE, 0); job(L.logit, IN_PLAIN, AFT, -1, LOGITS, 0);
    cb.split();
    D.nstages = cb.ns;
    if (cb.overflow() || sc - st->chain > kChainFloats) {
        VAR_SET_ERR(c, "ithor policy chain: table overflow");
        return VAR_ERR_ARG;
    }
    return chain_launch(c, s, D, cb.lds_max, kChainG);
}

}  // namespace

void ithor_policy_free(var_ctx* c) { (void)ws_drop<pol_state>(c, &c->ipol, false); }

// var_debug_buffer's "ipol_" names: conv outputs a1..a6 (a2..a5: the gather-GEMM path only), pooled maps p1..p4, the occupancy
// branch (occf: its convolutions' (B, 288); occ and h1: the per-layer path's (B, 256) and new hidden state), then what both
// workspaces have (ws_debug_buffer; the per-layer path's "occ" (B, 256) is not the chain's "OCC" pair vector)
int ithor_policy_debug_buffer(var_ctx* c, const char* name, void** ptr, long* nfloats) {
    pol_state* st = (pol_state*)c->ipol;
    if (!st) { VAR_SET_ERR(c, "var_debug_buffer: no var_ithor_policy_plan"); return VAR_ERR_PLAN; }
    const long B = st->maxB;
    const int pside[5] = {0, 48, 24, 12, 6}, pch[5] = {0, 32, 64, 64, 128};
    if ((name[0] == 'a' || name[0] == 'p') && name[1] >= '1' && name[1] <= '6' && !name[2]) {
        const int l = name[1] - '0';
        if (name[0] == 'a') { *ptr = st->a[l]; *nfloats = B * kCh[l] * kSide[l] * kSide[l]; return VAR_OK; }
        if (l <= 4) { *ptr = st->p[l]; *nfloats = B * pch[l] * pside[l] * pside[l]; return VAR_OK; }
    }
    if (!strcmp(name, "occf")) { *ptr = st->occf; *nfloats = B * kOcc; return VAR_OK; }
    if (!strcmp(name, "occ")) { *ptr = st->occ; *nfloats = B * 256; return VAR_OK; }
    if (!strcmp(name, "h1")) { *ptr = st->h1; *nfloats = B * kRh; return VAR_OK; }
    if (ws_debug_buffer(st, kRh, name, ptr, nfloats)) return VAR_OK;
    VAR_SET_ERR(c, "var_debug_buffer: unknown iTHOR policy buffer '%s'", name);
    return VAR_ERR_ARG;
}

extern "C" {

int var_ithor_policy_param_count(int n_actions) {
    if (n_actions < 1 || n_actions > kMaxActions) return VAR_ERR_ARG;
    return make_layout(n_actions).total;
}

int var_ithor_policy_plan(var_ctx* c, int max_batch) {
    if (!c) return VAR_ERR_ARG;
    if (max_batch < 1 || max_batch > 4096) { VAR_SET_ERR(c, "var_ithor_policy_plan: batch %d outside 1..4096", max_batch); return VAR_ERR_ARG; }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    if (c->ipol && ((pol_state*)c->ipol)->maxB >= max_batch) return VAR_OK;
    RUN(ws_drop<pol_state>(c, &c->ipol, true));
    pol_state* st = new pol_state();
    c->ipol = st;
    st->maxB = max_batch;
    st->pack = make_pack_desc(kCh + 1, make_layout(1).cw + 1, 5);      // conv 2..6 (they sit before the action-sized layer)
    return ws_alloc(c, st, [st](Take& t) {
        const long B = st->maxB;
        for (int l = 1; l <= 6; ++l) st->a[l] = t(B * kCh[l] * kSide[l] * kSide[l]);
        st->p[1] = t(B * 32 * 48 * 48); st->p[2] = t(B * 64 * 24 * 24); st->p[3] = t(B * 64 * 12 * 12); st->p[4] = t(B * 128 * 6 * 6);
        st->occf = t(B * kOcc); st->occ = t(B * 256); st->h1 = t(B * kRh);
        st->take_shared(t, kRh, kChainFloats);
    });
}

int var_ithor_policy_forward_ex(var_ctx* c, void* stream, const float* params, int n_actions, const void* image, int image_is_u8,
                                long image_bstride, const void* occupancy, int occupancy_is_u8, const float* image_feat,
                                const float* goal_sound_feat, const float* rnn_hxs, const float* masks, int B, float* value,
                                float* actor_features, float* logits, float* rnn_hxs_out, int flags) {
    if (!c) return VAR_ERR_ARG;
    RUN(check_flags(c, "var_ithor_policy_forward_ex", flags));
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    pol_state* st = (pol_state*)c->ipol;
    if (!st || B > st->maxB) { VAR_SET_ERR(c, "var_ithor_policy_forward: var_ithor_policy_plan(%d) first", B); return VAR_ERR_PLAN; }
    RUN(check_forward_args(c, "var_ithor_policy_forward", params && image && occupancy && image_feat && goal_sound_feat && rnn_hxs && masks &&
                           value && actor_features && rnn_hxs_out, B, image_bstride, rnn_hxs, rnn_hxs_out, kRh));
    if (n_actions < 1 || n_actions > kMaxActions) {
        VAR_SET_ERR(c, "var_ithor_policy_forward: n_actions %d outside 1..%d", n_actions, kMaxActions);
        return VAR_ERR_ARG;
    }
    if (st->n_actions != n_actions) { st->L = make_layout(n_actions); st->n_actions = n_actions; }
    hipStream_t s = (hipStream_t)stream;
    const PolLayout& L = st->L;
    const float* P = params;
    float* slab = st->slab;
    // occupancyCNNMLP's convolutions (any batch)
    if (occupancy_is_u8) hipLaunchKernelGGL(ip_occ_kernel<true>, dim3(B * (32 / kOccCo)), dim3(kOccT), 0, s, occupancy, P, L.ow[0], L.ob[0], L.ow[1], L.ob[1], st->occf);
    else hipLaunchKernelGGL(ip_occ_kernel<false>, dim3(B * (32 / kOccCo)), dim3(kOccT), 0, s, occupancy, P, L.ow[0], L.ob[0], L.ow[1], L.ob[1], st->occf);
    AC_CHECK(c);
    // imgCNN; BF (flags bit 0): every convolution multiplies operands rounded to bf16 where it stages them, everything stored stays
    // fp32 (the occupancy convolutions above stay fp32)
    auto img_cnn = [&](auto bf16) -> int {
        constexpr bool BF = decltype(bf16)::value;
        if (B <= kBandMaxB) {      // conv 1 and the filter pack of conv 2..6 in one launch (c3f.h)
            const c3f::PackDesc& d = st->pack;
            RUN(conv1(c, s, image, image_is_u8, image_bstride, P, L.cw[0], L.cb[0], st->a[1], B, st->wpk, d, BF, kIthorBands));
            RUN((band<IthorC2, IthorB2, BF>(c, s, st->a[1], st->wpk + d.wp_off[0], P + L.cb[1], st->p[1], B)));
            RUN((band<IthorC3, IthorB3, BF>(c, s, st->p[1], st->wpk + d.wp_off[1], P + L.cb[2], st->p[2], B)));
            RUN((band<IthorC4, IthorB4, BF>(c, s, st->p[2], st->wpk + d.wp_off[2], P + L.cb[3], st->p[3], B)));
            RUN((band<IthorC5, IthorB5, BF>(c, s, st->p[3], st->wpk + d.wp_off[3], P + L.cb[4], st->p[4], B)));
            RUN((c3f::launch_small<IthorC6, BF>(c, s, st->p[4], st->wpk + d.wp_off[4], P + L.cb[5], st->a[6], B)));
            return VAR_OK;
        }
        using S1 = Geo<3, 3, 1, 1, 1, 1>;
        using S2P1 = Geo<3, 3, 2, 2, 1, 1>;
        auto dims = [&](int l, int hin, int stride) { return conv_dims(B, kCh[l - 1], hin, hin, kCh[l], 3, 3, stride, stride, 1, 1); };
        ConvDims d1 = dims(1, 96, 1);
        d1.xb = image_bstride;
        if (image_is_u8) RUN((conv<S1, true, BF>(c, s, slab, d1, image, P + L.cw[0], P + L.cb[0], st->a[1])));
        else RUN((conv<S1, false, BF>(c, s, slab, d1, image, P + L.cw[0], P + L.cb[0], st->a[1])));
        RUN((conv<S1, false, BF>(c, s, slab, dims(2, 96, 1), st->a[1], P + L.cw[1], P + L.cb[1], st->a[2])));
        RUN(pool(c, s, st->a[2], st->p[1], B, 32, 96));
        RUN((conv<S1, false, BF>(c, s, slab, dims(3, 48, 1), st->p[1], P + L.cw[2], P + L.cb[2], st->a[3])));
        RUN(pool(c, s, st->a[3], st->p[2], B, 64, 48));
        RUN((conv<S1, false, BF>(c, s, slab, dims(4, 24, 1), st->p[2], P + L.cw[3], P + L.cb[3], st->a[4])));
        RUN(pool(c, s, st->a[4], st->p[3], B, 64, 24));
        RUN((conv<S1, false, BF>(c, s, slab, dims(5, 12, 1), st->p[3], P + L.cw[4], P + L.cb[4], st->a[5])));
        RUN(pool(c, s, st->a[5], st->p[4], B, 128, 12));
        RUN((conv<S2P1, false, BF>(c, s, slab, dims(6, 6, 2), st->p[4], P + L.cw[5], P + L.cb[5], st->a[6])));
        return VAR_OK;
    };
    RUN((flags & kFlagBf16) ? img_cnn(std::true_type{}) : img_cnn(std::false_type{}));
    if (B <= kChainRows)      // the RL stage's batch: everything after the convolutions in one persistent launch
        return chain_forward(c, s, st, P, image_feat, goal_sound_feat, rnn_hxs, masks, B, value, actor_features, logits, rnn_hxs_out);
    // B > 8 rows: one launch per Linear layer (+ the sums, the mask and the GRU cell)
    // image_flatten = cnnMlp(flatten), motor = motorMlp(image_feat), occupancy = the occupancy Linear layers
    RUN(linear(c, s, slab, P, L.cnn[0], st->a[6], st->t0, B, 1));
    RUN(linear(c, s, slab, P, L.cnn[1], st->t0, st->flat_img, B, 1));
    RUN(linear(c, s, slab, P, L.motor[0], image_feat, st->t0, B, 1));
    RUN(linear(c, s, slab, P, L.motor[1], st->t0, st->motor, B, 1));
    RUN(linear(c, s, slab, P, L.occ[0], st->occf, st->t0, B, 1));
    RUN(linear(c, s, slab, P, L.occ[1], st->t0, st->occ, B, 1));
    // imageMotor = imgMotorMlp(image_flatten + motor + occupancy)
    RUN(add(c, s, st->flat_img, st->motor, st->t0, B * 256));
    RUN(add(c, s, st->t0, st->occ, st->t1, B * 256));
    RUN(linear(c, s, slab, P, L.im[0], st->t1, st->t0, B, 1));
    RUN(linear(c, s, slab, P, L.im[1], st->t0, st->t2, B, 1));                       // (B,128)
    return layer_tail(c, s, st, P, L, L.logit, kRin, kRh, st->t2, st->h1, goal_sound_feat, rnn_hxs, masks, B, value, actor_features, logits,
                      rnn_hxs_out);
}

int var_ithor_policy_forward(var_ctx* c, void* stream, const float* params, int n_actions, const void* image, int image_is_u8,
                             long image_bstride, const void* occupancy, int occupancy_is_u8, const float* image_feat,
                             const float* goal_sound_feat, const float* rnn_hxs, const float* masks, int B, float* value,
                             float* actor_features, float* logits, float* rnn_hxs_out) {
    return var_ithor_policy_forward_ex(c, stream, params, n_actions, image, image_is_u8, image_bstride, occupancy, occupancy_is_u8, image_feat,
                                       goal_sound_feat, rnn_hxs, masks, B, value, actor_features, logits, rnn_hxs_out, 0);
}

int var_ithor_policy_status(var_ctx* c, unsigned* word) { return chain_status(c, c ? (pol_state*)c->ipol : nullptr, word, "var_ithor_policy"); }

int var_ithor_policy_clear_status(var_ctx* c) { return chain_clear(c, c ? (pol_state*)c->ipol : nullptr, "var_ithor_policy"); }

}  // extern "C"
