// RL actor-critic forward on gfx950 (BASELINE config 5 second half):
// models/RL/arm_RL_model.py:7-134 `armNet_VAR` (96x96 branch: 8 convolutions / 3 max pools -> 1152, the motor /
// image / sound MLPs, one GRU(128 -> 512) step through NNBase._forward_gru's acting path, models/ppo/model.py:116-121,
// fusion and the actor / critic trunks) followed by DiagGaussian's mean layer (models/ppo/distributions.py:65-84), i.e.
// everything of Policy.act up to the sampling.  Inference only (the PPO update stays in PyTorch).  Up to 64 images the
// convolutions run on the LDS-band kernels of c3f.h (filters re-packed per call inside conv 1's launch) and, up to 8 rows, the
// 22 Linear layers + GRU step on the one-launch chain below; larger batches take the gather-GEMM of gg.h layer by layer with
// the parameters in place in their state_dict() layouts.  var_armnet_forward_ex's flags bit 0 runs every convolution on operands
// rounded to bf16 (conv 2..6 on c3f_bf16.h's band kernel, conv 1 / 7 / 8 rounding where they stage, the gather-GEMM with BF = true);
// everything behind the convolutions is the same code in both precisions.  What this forward shares with ithor_policy.hip -- the elementwise
// kernels, the launch helpers, the workspace, the per-layer path from the GRU step on -- lives in actor_critic.h.
#include <string.h>

#include <type_traits>

#include "gg.h"

namespace {
PH_DECL();
}
#include "c3f.h"
#ifdef VAR_PHASES
extern "C" int var_debug_phases_armchain(unsigned long long* out) {
    unsigned long long z[32] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(z)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
#include "chain.h"
#include "actor_critic.h"

namespace {
constexpr int kCh[9] = {3, 32, 32, 64, 64, 128, 128, 256, 128};
constexpr int kRepr = 3, kRobot = 2, kRin = 128, kRh = 512, kAct = 128, kActions = 2, kFlat = 1152;
constexpr long kChainFloats = (long)kChainRows * 16384;

struct ArmLayout : Trunk {
    int cw[8], cb[8];
    Lin motor[3], cnn[2], im[2], mean;
    int logstd;
    int total;
};

ArmLayout make_layout() {
    ArmLayout L{};
    int o = 0;
    L.g_wih = o; o += 3 * kRh * kRin; L.g_whh = o; o += 3 * kRh * kRh; L.g_bih = o; o += 3 * kRh; L.g_bhh = o; o += 3 * kRh;
    for (int i = 0; i < 8; i++) { L.cw[i] = o; o += kCh[i + 1] * kCh[i] * 9; L.cb[i] = o; o += kCh[i + 1]; }
    auto lin = [&](int in, int out) { Lin l{o, o + in * out, in, out}; o += in * out + out; return l; };
    L.motor[0] = lin(kRepr + kRobot, 256); L.motor[1] = lin(256, 512); L.motor[2] = lin(512, 256);
    L.cnn[0] = lin(kFlat, 512); L.cnn[1] = lin(512, 256);
    L.im[0] = lin(256, 256); L.im[1] = lin(256, kRin);
    L.im2 = lin(kRh, 256);
    L.snd[0] = lin(kRepr, 128); L.snd[1] = lin(128, 256); L.snd[2] = lin(256, 256);
    L.fus[0] = lin(256, 512); L.fus[1] = lin(512, 256);
    L.all[0] = lin(256, 256); L.all[1] = lin(256, 128);
    L.actor[0] = lin(128, 128); L.actor[1] = lin(128, kAct);
    L.critic[0] = lin(128, 128); L.critic[1] = lin(128, 128);
    L.clin = lin(128, 1);
    L.mean = lin(kAct, kActions);
    L.logstd = o; o += kActions;
    L.total = o;
    return L;
}

struct arm_state : Workspace {
    ArmLayout L;
    float *a[9] = {nullptr}, *p[4] = {nullptr};      // conv outputs 1..8, pooled maps 1..3
    bool drop_one = false;         // tests: the next chain launch runs one workgroup short (var_debug_armnet_drop_workgroup)
};

// conv 2..6 of the 96x96 stack as band kernels (c3f.h): bands / channel groups chosen for ~192-256 workgroups at 8 images
using ArmC2 = c3f::Cfg<32, 32, 96, 4, 2, 1, true>;
using ArmC3 = c3f::Cfg<32, 64, 48, 6, 1, 1, false>;
using ArmC4 = c3f::Cfg<64, 64, 48, 6, 1, 1, true>;
using ArmC5 = c3f::Cfg<64, 128, 24, 8, 1, 1, false>;
using ArmC6 = c3f::Cfg<128, 128, 24, 4, 2, 2, true>;
// the same bands on c3f_bf16.h's kernel (flags bit 0); kArmBands: the band layers among the pack's layers (bit i = conv i + 2)
using ArmB2 = c3f::CfgB<32, 32, 96, 4, 2, 1, true>;
using ArmB3 = c3f::CfgB<32, 64, 48, 6, 1, 1, false>;
using ArmB4 = c3f::CfgB<64, 64, 48, 6, 1, 1, true>;
using ArmB5 = c3f::CfgB<64, 128, 24, 8, 1, 1, false>;
using ArmB6 = c3f::CfgB<128, 128, 24, 4, 2, 2, true>;
constexpr unsigned kArmBands = 0x1F;
using ArmC7 = c3f::SmallCfg<128, 256, 12, 2, 5>;
using ArmC8 = c3f::SmallCfg<256, 128, 5, 1, 3>;

int chain_forward(var_ctx* c, hipStream_t s, arm_state* st, const float* P, const float* image_feat, const float* robot_pose,
                  const float* goal, const float* hxs, const float* masks, int B, float* value, float* actor_features, float* action_mean,
                  float* hxs_out) {
    const ArmLayout& L = st->L;
    ChainDesc D{};
    D.P = P; D.B = B; D.H = kRh; D.sync = st->sync;
    enum { A8, IMGF, POSE, GOAL, HXS, MASK, HOUT, VALUE, AFEAT, MEAN, CNN0, FLAT, M0, M1, MOTOR, S0, S1, SOUND, GH, IM0, X, F0, FUSION, GI, IMR,
           ALL0, ALL1, C0, C1, A0, AFT, NBUF };
    static_assert(NBUF <= kChainBufs, "buffer table");
    float* sc = st->chain;
    auto scratch = [&](int width) { float* p = sc; sc += kChainRows * width * 2; return p; };     // (value, tag) pairs
    D.buf[A8] = st->a[8]; D.buf[IMGF] = (float*)image_feat; D.buf[POSE] = (float*)robot_pose; D.buf[GOAL] = (float*)goal;
    D.buf[HXS] = (float*)hxs; D.buf[MASK] = (float*)masks; D.buf[HOUT] = hxs_out; D.buf[VALUE] = value; D.buf[AFEAT] = actor_features;
    D.buf[MEAN] = action_mean ? action_mean : scratch(kActions);
    const struct { int id, width; const char* name; } widths[] = {
        CHAIN_VEC(CNN0, 512), CHAIN_VEC(FLAT, 256), CHAIN_VEC(M0, 256), CHAIN_VEC(M1, 512), CHAIN_VEC(MOTOR, 256), CHAIN_VEC(S0, 128),
        CHAIN_VEC(S1, 256), CHAIN_VEC(SOUND, 256), CHAIN_VEC(GH, 3 * kRh), CHAIN_VEC(IM0, 256), CHAIN_VEC(X, kRin), CHAIN_VEC(F0, 512),
        CHAIN_VEC(FUSION, 256), CHAIN_VEC(GI, 3 * kRh), CHAIN_VEC(IMR, 256), CHAIN_VEC(ALL0, 256), CHAIN_VEC(ALL1, 128), CHAIN_VEC(C0, 128),
        CHAIN_VEC(C1, 128), CHAIN_VEC(A0, 128), CHAIN_VEC(AFT, kAct)};
    st->ncvec = 0;
    for (auto& wd : widths) {                                                                   // handed over inside the launch
        D.buf[wd.id] = scratch(wd.width); D.tagged |= 1ull << wd.id;
        st->cvec[st->ncvec++] = {wd.name, D.buf[wd.id], wd.width};
    }
    D.b_hxs = HXS; D.b_mask = MASK; D.b_hout = HOUT;
    ChainBuilder cb(D);
    auto stage = [&]() { cb.stage(); };
    auto job = [&](const Lin& l, int kind, int in0, int in1, int cat0, int out, int relu, int out2 = -1) {
        cb.job(l.w, l.b, l.in, l.out, kind, in0, in1, cat0, out, relu, out2);
    };
    auto split = [&]() { cb.split(); };
    const Lin ih{L.g_wih, L.g_bih, kRin, 3 * kRh}, hh{L.g_whh, L.g_bhh, kRh, 3 * kRh};
    stage(); job(L.cnn[0], IN_PLAIN, A8, -1, 0, CNN0, 1); job(L.motor[0], IN_CAT, IMGF, POSE, kRepr, M0, 1);
             job(L.snd[0], IN_PLAIN, GOAL, -1, 0, S0, 1); job(hh, IN_MASK, HXS, MASK, 0, GH, 0);
    split();
    stage(); job(L.cnn[1], IN_PLAIN, CNN0, -1, 0, FLAT, 1); job(L.motor[1], IN_PLAIN, M0, -1, 0, M1, 1); job(L.snd[1], IN_PLAIN, S0, -1, 0, S1, 1);
    split();
    stage(); job(L.motor[2], IN_PLAIN, M1, -1, 0, MOTOR, 1); job(L.snd[2], IN_PLAIN, S1, -1, 0, SOUND, 1);
    split();
    stage(); job(L.im[0], IN_SUM, FLAT, MOTOR, 0, IM0, 1); job(L.fus[0], IN_SUM, SOUND, FLAT, 0, F0, 1);
    split();
    stage(); job(L.im[1], IN_PLAIN, IM0, -1, 0, X, 1); job(L.fus[1], IN_PLAIN, F0, -1, 0, FUSION, 1);
    split();
    stage(); job(ih, IN_PLAIN, X, -1, 0, GI, 0);
    split();
    stage(); job(L.im2, IN_GRU, GI, GH, 0, IMR, 1);                                   // the GRU cell is its input transform
    split();
    stage(); job(L.all[0], IN_SUM, FUSION, IMR, 0, ALL0, 1);
    split();
    stage(); job(L.all[1], IN_PLAIN, ALL0, -1, 0, ALL1, 1);
    split();
    stage(); job(L.critic[0], IN_PLAIN, ALL1, -1, 0, C0, 1); job(L.actor[0], IN_PLAIN, ALL1, -1, 0, A0, 1);
    split();
    stage(); job(L.critic[1], IN_PLAIN, C0, -1, 0, C1, 1); job(L.actor[1], IN_PLAIN, A0, -1, 0, AFT, 1, AFEAT);
    split();
    stage(); job(L.clin, IN_PLAIN, C1, -1, 0, VALUE, 0); job(L.mean, IN_PLAIN, AFT, -1, 0, MEAN, 0);
    split();
    D.nstages = cb.ns;
    if (cb.overflow() || sc - st->chain > kChainFloats) {
        VAR_SET_ERR(c, "armnet chain: table overflow");
        return VAR_ERR_ARG;
    }
    const int grid = kChainG - (st->drop_one ? 1 : 0);          // (one short: its outputs never arrive, every consumer's wait expires)
    st->drop_one = false;
    RUN(chain_launch(c, s, D, cb.lds_max, grid));
    return VAR_OK;
}
}  // namespace

void armnet_free(var_ctx* c) { (void)ws_drop<arm_state>(c, &c->arm, false); }

// var_debug_buffer's "arm_" names: conv outputs a1..a8 (a2 / a4 / a6: the gather-GEMM path only), pooled maps p1..p3, then
// what both workspaces have (ws_debug_buffer)
int armnet_debug_buffer(var_ctx* c, const char* name, void** ptr, long* nfloats) {
    arm_state* st = (arm_state*)c->arm;
    if (!st) { VAR_SET_ERR(c, "var_debug_buffer: no var_armnet_plan"); return VAR_ERR_PLAN; }
    const long B = st->maxB;
    const int side[9] = {96, 96, 96, 48, 48, 24, 24, 5, 3}, pside[4] = {0, 48, 24, 12}, pch[4] = {0, 32, 64, 128};
    if ((name[0] == 'a' || name[0] == 'p') && name[1] >= '1' && name[1] <= '8' && !name[2]) {
        const int l = name[1] - '0';
        if (name[0] == 'a') { *ptr = st->a[l]; *nfloats = B * kCh[l] * side[l] * side[l]; return VAR_OK; }
        if (l <= 3) { *ptr = st->p[l]; *nfloats = B * pch[l] * pside[l] * pside[l]; return VAR_OK; }
    }
    if (ws_debug_buffer(st, kRh, name, ptr, nfloats)) return VAR_OK;
    VAR_SET_ERR(c, "var_debug_buffer: unknown armnet buffer '%s'", name);
    return VAR_ERR_ARG;
}

extern "C" {

int var_armnet_param_count(void) { return make_layout().total; }

int var_armnet_plan(var_ctx* c, int max_batch) {
    if (!c) return VAR_ERR_ARG;
    if (max_batch < 1 || max_batch > 4096) { VAR_SET_ERR(c, "var_armnet_plan: batch %d outside 1..4096", max_batch); return VAR_ERR_ARG; }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    if (c->arm && ((arm_state*)c->arm)->maxB >= max_batch) return VAR_OK;
    RUN(ws_drop<arm_state>(c, &c->arm, true));
    c->plan_gen++;      // (var_ithor_policy_plan has no such line)
    arm_state* st = new arm_state();
    c->arm = st;
    st->L = make_layout();
    st->maxB = max_batch;
    st->pack = make_pack_desc(kCh + 1, st->L.cw + 1, 7);          // conv 2..8
    return ws_alloc(c, st, [st](Take& t) {
        const long B = st->maxB;
        const int side[9] = {96, 96, 96, 48, 48, 24, 24, 5, 3};      // output side of conv l
        for (int l = 1; l <= 8; ++l) st->a[l] = t(B * kCh[l] * side[l] * side[l]);
        st->p[1] = t(B * 32 * 48 * 48); st->p[2] = t(B * 64 * 24 * 24); st->p[3] = t(B * 128 * 12 * 12);
        st->take_shared(t, kRh, kChainFloats);
    });
}

int var_armnet_forward_ex(var_ctx* c, void* stream, const float* params, const void* image, int image_is_u8, long image_bstride,
                          const float* image_feat, const float* robot_pose, const float* goal_sound_feat,
                          const float* rnn_hxs, const float* masks, int B,
                          float* value, float* actor_features, float* action_mean, float* rnn_hxs_out, int flags) {
    if (!c) return VAR_ERR_ARG;
    RUN(check_flags(c, "var_armnet_forward_ex", flags));
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    arm_state* st = (arm_state*)c->arm;
    if (!st || B > st->maxB) { VAR_SET_ERR(c, "var_armnet_forward: var_armnet_plan(%d) first", B); return VAR_ERR_PLAN; }
    RUN(check_forward_args(c, "var_armnet_forward", params && image && image_feat && robot_pose && goal_sound_feat && rnn_hxs && masks &&
                           value && actor_features && rnn_hxs_out, B, image_bstride, rnn_hxs, rnn_hxs_out, kRh));
    hipStream_t s = (hipStream_t)stream;
    const ArmLayout& L = st->L;
    const float* P = params;
    float* slab = st->slab;
    // imgCNN; BF (flags bit 0): every convolution multiplies operands rounded to bf16 where it stages them, everything stored stays fp32
    auto img_cnn = [&](auto bf16) -> int {
        constexpr bool BF = decltype(bf16)::value;
        if (B <= kBandMaxB) {      // conv 1 and the filter pack of conv 2..8 in one launch (c3f.h)
            const c3f::PackDesc& d = st->pack;
            RUN(conv1(c, s, image, image_is_u8, image_bstride, P, L.cw[0], L.cb[0], st->a[1], B, st->wpk, d, BF, kArmBands));
            RUN((band<ArmC2, ArmB2, BF>(c, s, st->a[1], st->wpk + d.wp_off[0], P + L.cb[1], st->p[1], B)));
            RUN((band<ArmC3, ArmB3, BF>(c, s, st->p[1], st->wpk + d.wp_off[1], P + L.cb[2], st->a[3], B)));
            RUN((band<ArmC4, ArmB4, BF>(c, s, st->a[3], st->wpk + d.wp_off[2], P + L.cb[3], st->p[2], B)));
            RUN((band<ArmC5, ArmB5, BF>(c, s, st->p[2], st->wpk + d.wp_off[3], P + L.cb[4], st->a[5], B)));
            RUN((band<ArmC6, ArmB6, BF>(c, s, st->a[5], st->wpk + d.wp_off[4], P + L.cb[5], st->p[3], B)));
            RUN((c3f::launch_small<ArmC7, BF>(c, s, st->p[3], st->wpk + d.wp_off[5], P + L.cb[6], st->a[7], B)));
            RUN((c3f::launch_small<ArmC8, BF>(c, s, st->a[7], st->wpk + d.wp_off[6], P + L.cb[7], st->a[8], B)));
            return VAR_OK;
        }
        using S1 = Geo<3, 3, 1, 1, 1, 1>;
        using S2P0 = Geo<3, 3, 2, 2, 0, 0>;
        using S1P0 = Geo<3, 3, 1, 1, 0, 0>;
        auto dims = [&](int l, int hin, int stride, int pad) {
            return conv_dims(B, kCh[l - 1], hin, hin, kCh[l], 3, 3, stride, stride, pad, pad);
        };
        ConvDims d1 = dims(1, 96, 1, 1);
        d1.xb = image_bstride;
        if (image_is_u8) RUN((conv<S1, true, BF>(c, s, slab, d1, image, P + L.cw[0], P + L.cb[0], st->a[1])));
        else RUN((conv<S1, false, BF>(c, s, slab, d1, image, P + L.cw[0], P + L.cb[0], st->a[1])));
        RUN((conv<S1, false, BF>(c, s, slab, dims(2, 96, 1, 1), st->a[1], P + L.cw[1], P + L.cb[1], st->a[2])));
        RUN(pool(c, s, st->a[2], st->p[1], B, 32, 96));
        RUN((conv<S1, false, BF>(c, s, slab, dims(3, 48, 1, 1), st->p[1], P + L.cw[2], P + L.cb[2], st->a[3])));
        RUN((conv<S1, false, BF>(c, s, slab, dims(4, 48, 1, 1), st->a[3], P + L.cw[3], P + L.cb[3], st->a[4])));
        RUN(pool(c, s, st->a[4], st->p[2], B, 64, 48));
        RUN((conv<S1, false, BF>(c, s, slab, dims(5, 24, 1, 1), st->p[2], P + L.cw[4], P + L.cb[4], st->a[5])));
        RUN((conv<S1, false, BF>(c, s, slab, dims(6, 24, 1, 1), st->a[5], P + L.cw[5], P + L.cb[5], st->a[6])));
        RUN(pool(c, s, st->a[6], st->p[3], B, 128, 24));
        RUN((conv<S2P0, false, BF>(c, s, slab, dims(7, 12, 2, 0), st->p[3], P + L.cw[6], P + L.cb[6], st->a[7])));
        RUN((conv<S1P0, false, BF>(c, s, slab, dims(8, 5, 1, 0), st->a[7], P + L.cw[7], P + L.cb[7], st->a[8])));
        return VAR_OK;
    };
    RUN((flags & kFlagBf16) ? img_cnn(std::true_type{}) : img_cnn(std::false_type{}));
    if (B <= kChainRows)      // the RL stage's batch: everything after the convolutions in one persistent launch
        return chain_forward(c, s, st, P, image_feat, robot_pose, goal_sound_feat, rnn_hxs, masks, B, value, actor_features, action_mean,
                             rnn_hxs_out);
    // image_flatten = cnnMlp(flatten)
    RUN(linear(c, s, slab, P, L.cnn[0], st->a[8], st->t0, B, 1));
    RUN(linear(c, s, slab, P, L.cnn[1], st->t0, st->flat_img, B, 1));
    // motor = motorMlp(cat(image_feat, robot_pose))
    hipLaunchKernelGGL(ac_cat_kernel, g1(B * 5), dim3(256), 0, s, image_feat, kRepr, robot_pose, kRobot, st->t0, B);
    AC_CHECK(c);
    RUN(linear(c, s, slab, P, L.motor[0], st->t0, st->t1, B, 1));
    RUN(linear(c, s, slab, P, L.motor[1], st->t1, st->t2, B, 1));
    RUN(linear(c, s, slab, P, L.motor[2], st->t2, st->motor, B, 1));
    // imageMotor = imgMotorMlp(image_flatten + motor)
    RUN(add(c, s, st->flat_img, st->motor, st->t0, B * 256));
    RUN(linear(c, s, slab, P, L.im[0], st->t0, st->t1, B, 1));
    RUN(linear(c, s, slab, P, L.im[1], st->t1, st->t2, B, 1));                       // (B,128)
    return layer_tail(c, s, st, P, L, L.mean, kRin, kRh, st->t2, st->t3, goal_sound_feat, rnn_hxs, masks, B, value, actor_features,
                      action_mean, rnn_hxs_out);
}

int var_armnet_forward(var_ctx* c, void* stream, const float* params, const void* image, int image_is_u8, long image_bstride,
                       const float* image_feat, const float* robot_pose, const float* goal_sound_feat,
                       const float* rnn_hxs, const float* masks, int B,
                       float* value, float* actor_features, float* action_mean, float* rnn_hxs_out) {
    return var_armnet_forward_ex(c, stream, params, image, image_is_u8, image_bstride, image_feat, robot_pose, goal_sound_feat, rnn_hxs, masks,
                                 B, value, actor_features, action_mean, rnn_hxs_out, 0);
}

int var_armnet_status(var_ctx* c, unsigned* word) { return chain_status(c, c ? (arm_state*)c->arm : nullptr, word, "var_armnet"); }

int var_armnet_clear_status(var_ctx* c) { return chain_clear(c, c ? (arm_state*)c->arm : nullptr, "var_armnet"); }

int var_debug_armnet_drop_workgroup(var_ctx* c) {
    if (!c) return VAR_ERR_ARG;
    arm_state* st = (arm_state*)c->arm;
    if (!st) { VAR_SET_ERR(c, "var_debug_armnet_drop_workgroup: var_armnet_plan first"); return VAR_ERR_PLAN; }
    st->drop_one = true;
    return VAR_OK;
}

}  // extern "C"
