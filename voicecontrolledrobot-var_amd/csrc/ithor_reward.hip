// The frozen iTHOR encoder's reward step at RL batch sizes on gfx950: what the vectorised-env wrapper asks of the pretext model on
// every environment step (Envs/vec_env/vec_pretext_normalize.py:82-101 getEmbeddings / calcReward, processAI2Thor :125-146;
// models/pretext/pretext_base.py:10-41 with the goal embedding cached for the whole batch; ai2thor_pretext_model.py:14-58).
// Inference only, fp32 only, 96 x 96 images, at most kBandMaxB images.
//   image-only step (every environment step): conv 1 | four band convolutions with the pool fused | the stride-2 conv 6 (c3f.h,
//       the shapes of the iTHOR policy's image stack) | ONE tail launch: Linear(1152,128)+ReLU, Linear(128,3), F.normalize, the
//       row dot with the cached goal embedding -- 7 launches;
//   goal step (once per episode): the same, and between conv 6 and the tail the sound branch of ithor.hip's fp32 forward: three
//       convolutions and the input projection on the gather-GEMM (gg.h), the bidirectional GRU, the three-layer head.  Up to
//       kFusedClips clips a GRU time step is ONE launch (recurrent product of both directions on f32 MFMA + b_hh + gates + h');
//       above that the split-K product + gate kernel pair of ithor.hip's schedule.
//   sound-sound step (config.RLRewardSoundSound, var_ithor_reward_step_ex with current clips: EVERY environment step): the
//       current clips take the goal clips' sound branch -- with them in one pass of 2B clips while 2B <= kFusedClips (8 envs fill
//       the fused GRU step's 16 columns: still one launch per time step), in a pass of their own otherwise -- and the tail's last
//       workgroup also normalises their embedding and forms <image, goal> + <current, goal>.
//   id step (var_ithor_reward_step_ids): the sounds' embeddings are rows of a device clip table that var_ithor_reward_embed
//       filled once per checkpoint (passes of up to kFusedClips clips through the sound branch + one normalising launch each);
//       the step is the image stack and ONE tail whose finishing thread gathers by per-row ids read on the device -- 7 launches
//       on every kind of step, the goal cached per env.
// The encoder is frozen: var_ithor_reward_pack copies the parameter arena into the plan's own memory and lays conv 2..6 out in
// MFMA A-fragment order ONCE; every step reads that snapshot, so parameters loaded later change nothing until the next pack.
// The plan owns every buffer it touches (nothing of var_ithor_plan / var_ithor_policy_plan / var_plan is borrowed), and no
// kernel here waits for another workgroup.  The band configurations of the image stack, the filter-pack descriptor and the
// conv 1 launch are the iTHOR policy's: image_stack.h.
#include <string.h>

#include "gg.h"

namespace {
PH_DECL();
}
#include "c3f.h"
#include "image_stack.h"

namespace {
constexpr int kCh[7] = {3, 32, 32, 64, 64, 128, 128};
constexpr int kT = 600, kF = 40;                       // sound_dim (1,600,40)
constexpr int kSeq = 73, kGin = 448, kGh = 512, kG3 = 1536;
constexpr int kIRaw = 1152, kSRaw = 1024, kHidI = 128;
constexpr int kFusedClips = 16;                        // one MFMA column block of rw_gru_step_kernel
constexpr int kRecSplit = 4;                           // K splits of the two-launch recurrent product (ithor.hip: rec_split at <= 64 clips)

// state_dict() order of IthorVARPretextNet, restated from ithor.hip's make_ithor_layout (that file is the training path and stays
// as it is); var_ithor_reward_plan refuses to plan unless the total equals var_ithor_param_count()
struct RewLayout {
    int iw[6], ib[6];
    int w_ih[2], w_hh[2], b_ih[2], b_hh[2];
    int sw[3], sb[3];
    int ih_w0, ih_b0, ih_w1, ih_b1;
    int sh_w0, sh_b0, sh_w1, sh_b1, sh_w2, sh_b2;
    int total;
};
constexpr int kSK[3] = {121, 64 * 55, 64 * 21};
RewLayout make_layout() {
    RewLayout L{};
    int o = 0;
    for (int i = 0; i < 6; i++) { L.iw[i] = o; o += kCh[i + 1] * kCh[i] * 9; L.ib[i] = o; o += kCh[i + 1]; }
    for (int d = 0; d < 2; d++) {
        L.w_ih[d] = o; o += kG3 * kGin; L.w_hh[d] = o; o += kG3 * kGh;
        L.b_ih[d] = o; o += kG3;        L.b_hh[d] = o; o += kG3;
    }
    for (int i = 0; i < 3; i++) { L.sw[i] = o; o += 64 * kSK[i]; L.sb[i] = o; o += 64; }
    L.ih_w0 = o; o += kHidI * kIRaw; L.ih_b0 = o; o += kHidI; L.ih_w1 = o; o += 3 * kHidI; L.ih_b1 = o; o += 3;
    L.sh_w0 = o; o += 128 * kSRaw; L.sh_b0 = o; o += 128; L.sh_w1 = o; o += 64 * 128; L.sh_b1 = o; o += 64;
    L.sh_w2 = o; o += 3 * 64;      L.sh_b2 = o; o += 3;
    L.total = o;
    return L;
}

using GS1 = Geo<11, 11, 2, 2, 5, 5>;
using GS2 = Geo<11, 5, 2, 2, 5, 5>;
using GS3 = Geo<7, 3, 2, 2, 1, 1>;

struct rew_state {
    RewLayout L;
    int maxB = 0;
    int flags = 0;                           // VAR_IREW_* of the plan
    bool packed = false;
    const float* packed_from = nullptr;      // the arena of the last pack: a step with another one is refused
    float* ws = nullptr;
    float* frozen = nullptr;                 // the snapshot of the parameter arena every step reads
    c3f::f32x4* wpk = nullptr;               // conv 2..6 of the snapshot in MFMA A-fragment order
    c3f::PackDesc pack{};
    float *a1 = nullptr, *p[5] = {nullptr}, *a6 = nullptr, *hid = nullptr;
    unsigned* ctr = nullptr;                 // arrivals of the tail's workgroups (rewinds itself)
    float *s[4] = {nullptr}, *GI = nullptr, *GH = nullptr, *Hb = nullptr, *hs1 = nullptr, *hs2 = nullptr, *graw = nullptr;
    float* craw = nullptr;                   // VAR_IREW_SOUND_SOUND: the current clips' head output of a pass of their own
};
inline rew_state* rew(var_ctx* c) { return (rew_state*)c->irew; }

// ---- the filter pack of conv 2..6 (c3f::pack_item), once per var_ithor_reward_pack
__global__ void __launch_bounds__(256) rw_pack_kernel(const float* __restrict__ params, c3f::f32x4* __restrict__ wp, c3f::PackDesc d) {
    c3f::pack_item(params, wp, d, (int)blockIdx.x * 256 + threadIdx.x);
}

// ---- the tail: image head, F.normalize, the row dot -------------------------------------------------------------------
// The 590 KB of Linear(1152,128) are what it moves.  Workgroup j owns hidden unit j: its weight row (4.6 KB) sits in the
// registers of every wave (lanes stride K in 16-byte pieces), wave w takes the images w, w + 4, ..., four of them in flight;
// a wave reduces its sums with a butterfly (fixed order), lane 0 applies bias + ReLU and hands the unit over as an agent-scope
// store.  The LAST workgroup to arrive (counter pattern of heads.hip's small-batch finish: no wait anywhere) finishes the rows:
// Linear(128,3) as four 32-unit partials per row folded in a fixed order, x / max(|x|, 1e-12) (l2norm_fwd_kernel's form), the
// goal embedding from its raw head output when this is a goal step, and sum_d image_feat * goal_feat (row_dot_kernel's order).
// SS (RLRewardSoundSound, a step with current clips): the same thread also normalises the row's current-sound embedding from
// cur_raw and forms calcReward's sum in reward_dots_kernel's grouping -- reward = <image, goal> + <current, goal>, two fp32 row
// sums and one add; the two dots go out where asked for.  SS = false is the kernel as it always was.
// IDS (var_ithor_reward_step_ids): the sound embeddings are rows of a device clip table, picked by per-row ids the finishing
// thread reads itself -- nothing of a sound pass is waited for.  Goal id g >= 0: table[g], also written to goal_feat[row]; g == -1
// (or no goal ids at all): goal_feat[row], the row's cached embedding.  With current ids cur_feat[row] = table[c] and the reward
// is SS's sum; without them it is SS = false's.  A row with an id outside its range (goal < -1 or >= table_rows; current < 0 or
// >= table_rows) gets NaN in image_feat, cur_feat and the rewards and keeps its goal_feat.  Every load is unconditional from a
// clamped address, the value is selected afterwards.  IDS = false discards all of it: the two kernels above stay as they were.
constexpr int kTailWG = kHidI;
template <bool SS, bool IDS = false>
__global__ void __launch_bounds__(256) rw_tail_kernel(const float* __restrict__ a6, const float* __restrict__ w0, const float* __restrict__ b0,
                                                     const float* __restrict__ w1, const float* __restrict__ b1, int B, float* hid,
                                                     unsigned* ctr, const float* __restrict__ goal_raw, float* goal_feat,
                                                     float* __restrict__ image_feat, float* __restrict__ reward,
                                                     const float* __restrict__ cur_raw, float* __restrict__ cur_feat,
                                                     float* __restrict__ reward_img, float* __restrict__ reward_snd,
                                                     const float* __restrict__ table = nullptr, int table_rows = 0,
                                                     const int* __restrict__ goal_ids = nullptr, const int* __restrict__ cur_ids = nullptr) {
    constexpr int N4 = kIRaw / 4, PER = (N4 + 63) / 64;       // 288 16-byte pieces of a row, 5 per lane (the last one half a wave)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = blockIdx.x;
    float4 w[PER];
    {
        const float4* wr = (const float4*)(w0 + (size_t)j * kIRaw);
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int e = lane + 64 * u;
            w[u] = wr[e < N4 ? e : N4 - 1];
            if (e >= N4) w[u] = float4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const float bias = b0[j];
    for (int g = 0; g < B; g += 16) {
        float4 x[4][PER];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int b = g + 4 * q + wave;
            b = b < B ? b : B - 1;
            const float4* xr = (const float4*)(a6 + (size_t)b * kIRaw);
#pragma unroll
            for (int u = 0; u < PER; ++u) { const int e = lane + 64 * u; x[q][u] = xr[e < N4 ? e : N4 - 1]; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                acc += x[q][u].x * w[u].x; acc += x[q][u].y * w[u].y; acc += x[q][u].z * w[u].z; acc += x[q][u].w * w[u].w;
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
            const int b = g + 4 * q + wave;
            if (lane == 0 && b < B) { const float v = acc + bias; join_store(hid + (size_t)b * kHidI + j, v > 0.f ? v : 0.f); }
        }
    }
    __shared__ int last_s;
    __syncthreads();                                           // (every join_store of this workgroup is acknowledged)
    if (tid == 0) {
        last_s = atomicAdd(ctr, 1u) == gridDim.x - 1;
        if (last_s) atomicExch(ctr, 0u);
    }
    __syncthreads();
    if (!last_s) return;
    const int row = tid >> 2, q = tid & 3;                     // 64 rows x 4 partials of 32 hidden units
    const int rc = row < B ? row : B - 1;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
        const float h = join_load(hid + (size_t)rc * kHidI + 32 * q + k);
        s0 += h * w1[32 * q + k]; s1 += h * w1[kHidI + 32 * q + k]; s2 += h * w1[2 * kHidI + 32 * q + k];
    }
    // lanes 4 row .. 4 row + 3 of a wave: ((p0 + p1) + (p2 + p3))
    s0 += __shfl_xor(s0, 1); s1 += __shfl_xor(s1, 1); s2 += __shfl_xor(s2, 1);
    s0 += __shfl_xor(s0, 2); s1 += __shfl_xor(s1, 2); s2 += __shfl_xor(s2, 2);
    if (q != 0 || row >= B) return;
    const float a = s0 + b1[0], b = s1 + b1[1], c = s2 + b1[2];
    const float nrm = fmaxf(sqrtf(a * a + b * b + c * c), 1e-12f);
    const float y0 = a / nrm, y1 = b / nrm, y2 = c / nrm;
    if constexpr (IDS) {
        const int gid = goal_ids ? goal_ids[row] : -1, cid = cur_ids ? cur_ids[row] : 0;
        const bool bad = gid < -1 || gid >= table_rows || cid < 0 || cid >= table_rows;
        const bool fresh = gid >= 0 && !bad;                   // a new goal: the table's row, and it becomes the cached one
        const float* tg = table + 3 * (gid >= 0 && gid < table_rows ? gid : 0);
        const float* tc = table + 3 * (cid >= 0 && cid < table_rows ? cid : 0);
        const float n0 = tg[0], n1 = tg[1], n2 = tg[2], k0 = goal_feat[3 * row], k1 = goal_feat[3 * row + 1], k2 = goal_feat[3 * row + 2];
        const float c0 = tc[0], c1 = tc[1], c2 = tc[2];
        const float g0 = fresh ? n0 : k0, g1 = fresh ? n1 : k1, g2 = fresh ? n2 : k2;
        const float qnan = __int_as_float(0x7fc00000);
        if (fresh) { goal_feat[3 * row] = g0; goal_feat[3 * row + 1] = g1; goal_feat[3 * row + 2] = g2; }
        image_feat[3 * row] = bad ? qnan : y0; image_feat[3 * row + 1] = bad ? qnan : y1; image_feat[3 * row + 2] = bad ? qnan : y2;
        float sd = 0.f;
        sd += y0 * g0; sd += y1 * g1; sd += y2 * g2;
        if (!cur_ids) { reward[row] = bad ? qnan : sd; return; }
        cur_feat[3 * row] = bad ? qnan : c0; cur_feat[3 * row + 1] = bad ? qnan : c1; cur_feat[3 * row + 2] = bad ? qnan : c2;
        float ss = 0.f;
        ss += c0 * g0; ss += c1 * g1; ss += c2 * g2;
        reward[row] = bad ? qnan : sd + ss;
        if (reward_img) reward_img[row] = bad ? qnan : sd;
        if (reward_snd) reward_snd[row] = bad ? qnan : ss;
        return;
    }
    float g0, g1, g2;
    if (goal_raw) {
        const float u = goal_raw[3 * row], v = goal_raw[3 * row + 1], t = goal_raw[3 * row + 2];
        const float gn = fmaxf(sqrtf(u * u + v * v + t * t), 1e-12f);
        g0 = u / gn; g1 = v / gn; g2 = t / gn;
        goal_feat[3 * row] = g0; goal_feat[3 * row + 1] = g1; goal_feat[3 * row + 2] = g2;
    } else {
        g0 = goal_feat[3 * row]; g1 = goal_feat[3 * row + 1]; g2 = goal_feat[3 * row + 2];
    }
    image_feat[3 * row] = y0; image_feat[3 * row + 1] = y1; image_feat[3 * row + 2] = y2;
    float sd = 0.f;
    sd += y0 * g0; sd += y1 * g1; sd += y2 * g2;
    if constexpr (!SS) {
        reward[row] = sd;
    } else {
        const float u = cur_raw[3 * row], v = cur_raw[3 * row + 1], t = cur_raw[3 * row + 2];
        const float cn = fmaxf(sqrtf(u * u + v * v + t * t), 1e-12f);
        const float c0 = u / cn, c1 = v / cn, c2 = t / cn;
        cur_feat[3 * row] = c0; cur_feat[3 * row + 1] = c1; cur_feat[3 * row + 2] = c2;
        float ss = 0.f;
        ss += c0 * g0; ss += c1 * g1; ss += c2 * g2;
        reward[row] = sd + ss;
        if (reward_img) reward_img[row] = sd;
        if (reward_snd) reward_snd[row] = ss;
    }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// ---- one fp32 GRU time step, both directions, at most 16 clips, ONE launch (torch.nn.GRU gate order r, z, n) --------------
//   gh = W_hh h + b_hh;  r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h' = (1 - z) * n + z * h
// (the sigmoid / tanh forms and the grouping gi + (gh + b) of ithor.hip's gru_gate_fwd_kernel: the two forms differ by the
// product's summation order only).  GI (dir, clip*73 + t, 1536) holds x W_ih^T + b_ih; the states live as (clip, [forward 512 |
// reverse 512]) rows, so the last step leaves cat(h_n[0], h_n[1]) as the sound head reads it.
// A workgroup owns 4 hidden units of one direction = 12 rows of W_hh (24 KB): 2 x 128 workgroups.  One v_mfma_f32_16x16x4_f32
// tile: row 4 u + g = gate g of unit u (g = 3 is padding), column = clip; the four waves split K = 512 in quarters -- 8 16-byte
// loads of its weight row and 8 of its clip's state per lane, 32 matrix instructions -- and their tiles are folded through LDS in
// wave order.  D[row 4 (lane >> 4) + r][column lane & 15]: a lane ends up with r, z, n of ONE (unit, clip) -- the gate
// arithmetic needs no further exchange.  Plain kernel boundaries order the steps.
constexpr int kGruWG = 2 * (kGh / 4);
__global__ void __launch_bounds__(256) rw_gru_step_kernel(const float* __restrict__ w_hh, const float* __restrict__ b_hh, long dirP,
                                                         const float* __restrict__ GI, long dirGI, const float* __restrict__ hprev,
                                                         float* __restrict__ hnext, int nclips, int step, int first) {
    __shared__ float red[4][3][64];
    const int tid = threadIdx.x, lane = tid & 63, kq = tid >> 6, l15 = lane & 15, lk = lane >> 4;
    const int dir = blockIdx.x / (kGh / 4), j0 = (blockIdx.x - dir * (kGh / 4)) * 4;
    const int t = dir ? kSeq - 1 - step : step;
    // wave 0 finishes: its (unit lk, clip l15) operands of the gate arithmetic leave before the product
    const int j = j0 + lk, clip = l15 < nclips ? l15 : nclips - 1;
    float gi[3] = {0.f, 0.f, 0.f}, bh[3] = {0.f, 0.f, 0.f}, hp = 0.f;
    if (kq == 0) {
        const float* gp = GI + dir * dirGI + ((long)clip * kSeq + t) * kG3 + j;
        const float* bp = b_hh + dir * dirP + j;
#pragma unroll
        for (int g = 0; g < 3; ++g) { gi[g] = gp[g * kGh]; bh[g] = bp[g * kGh]; }
        if (!first) hp = hprev[(long)clip * kSRaw + dir * kGh + j];
    }
    c3f::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (!first) {                                              // (the initial state is zero: nothing to multiply)
        const int gate = (l15 & 3) < 3 ? (l15 & 3) : 2;        // the padding rows repeat gate n; their results are dropped
        const float4* wr = (const float4*)(w_hh + dir * dirP + ((long)gate * kGh + j0 + (l15 >> 2)) * kGh + kq * 128 + 4 * lk);
        const float4* hr = (const float4*)(hprev + (long)clip * kSRaw + dir * kGh + kq * 128 + 4 * lk);
        float4 a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { a[u] = wr[4 * u]; b[u] = hr[4 * u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {                          // k = 128 kq + 16 u + 4 lk + e on both operands
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, b[u].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, b[u].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, b[u].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, b[u].w, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) red[kq][g][lane] = acc[g];
    __syncthreads();
    if (kq != 0 || l15 >= nclips) return;
    float gh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) gh[g] = (red[0][g][lane] + red[1][g][lane]) + (red[2][g][lane] + red[3][g][lane]);
    const float r = sigmoidf_(gi[0] + (gh[0] + bh[0]));
    const float z = sigmoidf_(gi[1] + (gh[1] + bh[1]));
    const float ghn = gh[2] + bh[2];
    const float n = tanhf(gi[2] + r * ghn);
    hnext[(long)clip * kSRaw + dir * kGh + j] = (1.f - z) * n + z * hp;
}

// ---- more than 16 clips: the gate half of ithor.hip's two-launch step (gru_gate_fwd_kernel without the saved gates) over the
// (clip, [forward | reverse]) state rows; GH holds h W_hh^T without the bias as `nsplit` split-K slabs, added in order
__global__ void rw_gru_gate_kernel(const float* __restrict__ GI, const float* __restrict__ GH, int nsplit, const float* __restrict__ hprev,
                                   float* __restrict__ hnext, const float* __restrict__ b_hh, long dirP, int nclips, int step, long dirGI,
                                   int first) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nclips * kGh) return;
    const int dir = blockIdx.y;
    const int clip = i / kGh, j = i - clip * kGh;
    const int t = dir ? kSeq - 1 - step : step;
    const float* gi = GI + dir * dirGI + ((long)clip * kSeq + t) * kG3;
    const float* gh = GH + (long)dir * nclips * kG3 + (long)clip * kG3;
    const float* bh = b_hh + dir * dirP;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    for (int sp = 0; sp < (first ? 0 : nsplit); ++sp) {
        const float* q = gh + (long)sp * 2 * nclips * kG3;
        g0 += q[j]; g1 += q[kGh + j]; g2 += q[2 * kGh + j];
    }
    const float r = sigmoidf_(gi[j] + (g0 + bh[j]));
    const float z = sigmoidf_(gi[kGh + j] + (g1 + bh[kGh + j]));
    const float ghn = g2 + bh[2 * kGh + j];
    const float n = tanhf(gi[2 * kGh + j] + r * ghn);
    const float hp = first ? 0.f : hprev[(long)clip * kSRaw + dir * kGh + j];
    hnext[(long)clip * kSRaw + dir * kGh + j] = (1.f - z) * n + z * hp;
}

// var_ithor_reward_embed: F.normalize of a pass's head outputs, the tail's expression (x / max(|x|, 1e-12)), a thread per clip
__global__ void __launch_bounds__(64) rw_embed_finish_kernel(const float* __restrict__ raw, float* __restrict__ out, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float u = raw[3 * i], v = raw[3 * i + 1], t = raw[3 * i + 2];
    const float gn = fmaxf(sqrtf(u * u + v * v + t * t), 1e-12f);
    out[3 * i] = u / gn; out[3 * i + 1] = v / gn; out[3 * i + 2] = t / gn;
}

// the fp32 gather-GEMM, whatever var_ithor_set_bf16 says
template <class G, bool SEQ>
int snd_conv(var_ctx* c, hipStream_t s, const ConvDims& d, const float* x, const float* w, const float* bias, float* y) {
    ConvFwdP<G, false, SEQ> p{};
    p.M = d.B * d.HO * d.WO; p.N = d.COUT; p.K = d.CIN * G::KHW; p.nsplit = 1;
    p.d = d; p.x = x; p.w = w; p.bias = bias; p.y = y;
    return gg_launch<ConvFwdP<G, false, SEQ>, GG_KC, false>(c, s, p);
}
// Y (rows, O) = X (rows, K) W^T + b, optional ReLU
int linear(var_ctx* c, hipStream_t s, const float* X, const float* W, const float* b, float* Y, int rows, int K, int O, int relu) {
    DenseP<true, true, 0> p{};
    p.M = O; p.N = rows; p.K = K; p.nsplit = 1;
    p.A = W; p.sam = K; p.sak = 1; p.Bm = X; p.sbk = 1; p.sbn = K; p.C = Y; p.scm = 1; p.scn = O; p.bias = b; p.relu = relu;
    return gg_launch<DenseP<true, true, 0>, GG_KC, false>(c, s, p);
}

// the sound branch of ithor.hip's fp32 forward for a set of n clips -> out (B,3), the head's output before F.normalize.  With
// `more` (a second set of n clips, 2n <= kFusedClips) both sets go through in ONE pass of B = 2n clips, `more` behind `clips` in
// every buffer: conv 1 runs per set (each set is its caller's own array), every later layer once.  No kernel below mixes clips
// (the gather-GEMMs run unsplit, a clip is one MFMA column of the fused GRU step), so a clip's rows have the bits of a pass
// without the other set.
int goal_branch(var_ctx* c, hipStream_t s, rew_state* st, const float* clips, const float* more, int n, float* out) {
    const RewLayout& L = st->L;
    const float* P = st->frozen;
    const int B = more ? 2 * n : n;
    RUN((snd_conv<GS1, false>(c, s, conv_dims(n, 1, kT, kF, 64, 11, 11, 2, 2, 5, 5), clips, P + L.sw[0], P + L.sb[0], st->s[1])));
    if (more)
        RUN((snd_conv<GS1, false>(c, s, conv_dims(n, 1, kT, kF, 64, 11, 11, 2, 2, 5, 5), more, P + L.sw[0], P + L.sb[0],
                                  st->s[1] + (long)n * 64 * 300 * 20)));
    RUN((snd_conv<GS2, false>(c, s, conv_dims(B, 64, 300, 20, 64, 11, 5, 2, 2, 5, 5), st->s[1], P + L.sw[1], P + L.sb[1], st->s[2])));
    RUN((snd_conv<GS3, true>(c, s, conv_dims(B, 64, 150, 13, 64, 7, 3, 2, 2, 1, 1), st->s[2], P + L.sw[2], P + L.sb[2], st->s[3])));
    const int rows = B * kSeq;
    const long dirP = L.w_ih[1] - L.w_ih[0], dirGI = (long)rows * kG3;
    {
        DenseP<true, true, 0> p{};
        p.M = kG3; p.N = rows; p.K = kGin; p.nsplit = 1;
        p.A = P + L.w_ih[0]; p.sam = kGin; p.sak = 1; p.zA = dirP;
        p.Bm = st->s[3]; p.sbk = 1; p.sbn = kGin; p.zB = 0;
        p.C = st->GI; p.scm = 1; p.scn = kG3; p.zC = dirGI; p.bias = P + L.b_ih[0]; p.zbias = dirP;
        RUN((gg_launch<DenseP<true, true, 0>, GG_KC, false>(c, s, p, 2)));
    }
    // the states ping-pong between two (clip, 1024) slots; step 73 writes slot 1
    const long slot = (long)st->maxB * kSRaw;
    for (int step = 0; step < kSeq; ++step) {
        const float* hprev = st->Hb + (step & 1) * slot;
        float* hnext = st->Hb + ((step + 1) & 1) * slot;
        if (B <= kFusedClips) {
            hipLaunchKernelGGL(rw_gru_step_kernel, dim3(kGruWG), dim3(256), 0, s, P + L.w_hh[0], P + L.b_hh[0], dirP, st->GI, dirGI, hprev,
                               hnext, B, step, step == 0 ? 1 : 0);
            AC_CHECK(c);
            continue;
        }
        if (step > 0) {      // (h_0 = 0: no product)
            DenseP<true, true, 2> p{};
            p.M = kG3; p.N = B; p.K = kGh; p.nsplit = kRecSplit;
            p.A = P + L.w_hh[0]; p.sam = kGh; p.sak = 1; p.zA = dirP;
            p.Bm = hprev; p.sbk = 1; p.sbn = kSRaw; p.zB = kGh;
            p.C = st->GH; p.scm = 1; p.scn = kG3; p.zC = (long)B * kG3; p.sC = 2L * B * kG3;
            RUN((gg_launch<DenseP<true, true, 2>, GG_KC, false>(c, s, p, 2)));
        }
        hipLaunchKernelGGL(rw_gru_gate_kernel, dim3((B * kGh + 255) / 256, 2), dim3(256), 0, s, st->GI, st->GH, kRecSplit, hprev, hnext,
                           P + L.b_hh[0], dirP, B, step, dirGI, step == 0 ? 1 : 0);
        AC_CHECK(c);
    }
    const float* sraw = st->Hb + (kSeq & 1) * slot;
    RUN(linear(c, s, sraw, P + L.sh_w0, P + L.sh_b0, st->hs1, B, kSRaw, 128, 1));
    RUN(linear(c, s, st->hs1, P + L.sh_w1, P + L.sh_b1, st->hs2, B, 128, 64, 1));
    RUN(linear(c, s, st->hs2, P + L.sh_w2, P + L.sh_b2, out, B, 64, 3, 0));
    return VAR_OK;
}

// the image stack of every step, six launches: image -> a6 (B, 1152), what the tail reads
int image_convs(var_ctx* c, hipStream_t s, rew_state* st, const void* image, int image_is_u8, long image_bstride, int B) {
    const RewLayout& L = st->L;
    const float* P = st->frozen;
    const c3f::PackDesc& d = st->pack;
    // conv 1: c1f_pack_kernel's convolution workgroups alone (the filters were packed once)
    RUN(conv1(c, s, image, image_is_u8, image_bstride, P, L.iw[0], L.ib[0], st->a1, B, nullptr, c3f::PackDesc{}));
    RUN(c3f::launch<IthorC2>(c, s, st->a1, st->wpk + d.wp_off[0], P + L.ib[1], st->p[1], B));
    RUN(c3f::launch<IthorC3>(c, s, st->p[1], st->wpk + d.wp_off[1], P + L.ib[2], st->p[2], B));
    RUN(c3f::launch<IthorC4>(c, s, st->p[2], st->wpk + d.wp_off[2], P + L.ib[3], st->p[3], B));
    RUN(c3f::launch<IthorC5>(c, s, st->p[3], st->wpk + d.wp_off[3], P + L.ib[4], st->p[4], B));
    RUN(c3f::launch_small<IthorC6>(c, s, st->p[4], st->wpk + d.wp_off[4], P + L.ib[5], st->a6, B));
    return VAR_OK;
}
}  // namespace

void ithor_reward_free(var_ctx* c) {
    rew_state* st = rew(c);
    if (!st) return;
    if (st->ws) (void)hipFree(st->ws);
    delete st;
    c->irew = nullptr;
}

// var_debug_buffer's "irew_" names, lengths those of the PLAN's batch (a step of B rows fills the first B rows of each, except
// gi (dir stride B * 73 * 1536) and gh (slab stride 2 * B * 1536, dir stride B * 1536), which follow B; the two hb slots are
// maxB * 1024 apart): a1, p1..p4, a6 (maxB, 1152), hid (maxB, 128), s1, s2, s3 (clip, 73, 448), gi, gh, hb, hs1, hs2, graw,
// craw (a plan with VAR_IREW_SOUND_SOUND; empty otherwise), frozen (the parameter snapshot)
int ithor_reward_debug_buffer(var_ctx* c, const char* name, void** ptr, long* nfloats) {
    rew_state* st = rew(c);
    if (!st) { VAR_SET_ERR(c, "var_debug_buffer: no var_ithor_reward_plan"); return VAR_ERR_PLAN; }
    const long B = st->maxB;
    const struct { const char* name; float* p; long n; } tab[] = {
        {"a1", st->a1, B * 32 * 96 * 96}, {"p1", st->p[1], B * 32 * 48 * 48}, {"p2", st->p[2], B * 64 * 24 * 24},
        {"p3", st->p[3], B * 64 * 12 * 12}, {"p4", st->p[4], B * 128 * 6 * 6}, {"a6", st->a6, B * kIRaw}, {"hid", st->hid, B * kHidI},
        {"s1", st->s[1], B * 64 * 300 * 20}, {"s2", st->s[2], B * 64 * 150 * 13}, {"s3", st->s[3], B * kSeq * kGin},
        {"gi", st->GI, 2 * B * kSeq * kG3}, {"gh", st->GH, (long)kRecSplit * 2 * B * kG3}, {"hb", st->Hb, 2 * B * kSRaw},
        {"hs1", st->hs1, B * 128}, {"hs2", st->hs2, B * 64}, {"graw", st->graw, B * 3}, {"craw", st->craw, st->craw ? B * 3 : 0},
        {"frozen", st->frozen, st->L.total},
    };
    for (const auto& e : tab)
        if (!strcmp(name, e.name)) { *ptr = e.p; *nfloats = e.n; return VAR_OK; }
    VAR_SET_ERR(c, "var_debug_buffer: unknown iTHOR reward buffer '%s'", name);
    return VAR_ERR_ARG;
}

extern "C" {

int var_ithor_reward_plan(var_ctx* c, int max_batch, int img_hw) { return var_ithor_reward_plan_ex(c, max_batch, img_hw, 0); }

int var_ithor_reward_plan_ex(var_ctx* c, int max_batch, int img_hw, int flags) {
    if (!c) return VAR_ERR_ARG;
    if (flags & ~VAR_IREW_SOUND_SOUND) { VAR_SET_ERR(c, "var_ithor_reward_plan_ex: unknown flags 0x%x", flags); return VAR_ERR_ARG; }
    if (img_hw != 96) {
        VAR_SET_ERR(c, "var_ithor_reward_plan: image side %d, the band kernels take 96 (use var_ithor_encoder_fwd otherwise)", img_hw);
        return VAR_ERR_ARG;
    }
    if (max_batch < 1 || max_batch > kBandMaxB) {
        VAR_SET_ERR(c, "var_ithor_reward_plan: batch %d outside 1..%d (use var_ithor_encoder_fwd beyond)", max_batch, kBandMaxB);
        return VAR_ERR_ARG;
    }
    const RewLayout L = make_layout();
    if (L.total != var_ithor_param_count()) {      // the layout above restates ithor.hip's: both must describe the same arena
        VAR_SET_ERR(c, "var_ithor_reward_plan: layout of %d floats, var_ithor_param_count() is %d", L.total, var_ithor_param_count());
        return VAR_ERR_STATE;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    rew_state* st = rew(c);
    // sound-sound: the goal and the current clips of up to kFusedClips / 2 envs share one pass of the sound branch, so the plan is
    // made for that many rows (throughout: the image buffers of 16 rows are under 30 MB, and every irew_ length stays one batch)
    if (flags & VAR_IREW_SOUND_SOUND) {
        const int both = 2 * max_batch < kFusedClips ? 2 * max_batch : kFusedClips;
        max_batch = max_batch > both ? max_batch : both;
    }
    if (st && st->maxB >= max_batch && (st->flags & flags) == flags) return VAR_OK;
    if (st) {      // retire (do not free) the superseded block: a captured reward graph may still replay on it
        if (st->ws) { int rc = retire_block(c, st->ws); if (rc != VAR_OK) return rc; }
        max_batch = max_batch > st->maxB ? max_batch : st->maxB;      // (only grows, whatever made it grow)
        flags |= st->flags;
        delete st;
        c->irew = nullptr;
    }
    st = new rew_state();
    c->irew = st;
    st->L = L;
    st->maxB = max_batch;
    st->flags = flags;
    st->pack = make_pack_desc(kCh + 1, st->L.iw + 1, 5);          // conv 2..6
    const long B = max_batch;
    long total = 0;
    auto take = [&](long n) { long o = total; total += (n + 63) & ~63L; return o; };
    const long ofz = take(st->L.total), owpk = take(4L * st->pack.first[5]);
    const long oa1 = take(B * 32 * 96 * 96);
    const long op1 = take(B * 32 * 48 * 48), op2 = take(B * 64 * 24 * 24), op3 = take(B * 64 * 12 * 12), op4 = take(B * 128 * 6 * 6);
    const long oa6 = take(B * kIRaw), ohid = take(B * kHidI), octr = take(64);
    const long os1 = take(B * 64 * 300 * 20), os2 = take(B * 64 * 150 * 13), os3 = take(B * kSeq * kGin);
    const long oGI = take(2 * B * kSeq * kG3), oGH = take((long)kRecSplit * 2 * B * kG3), oHb = take(2 * B * kSRaw);
    const long ohs1 = take(B * 128), ohs2 = take(B * 64), ograw = take(B * 3);
    const long ocraw = (flags & VAR_IREW_SOUND_SOUND) ? take(B * 3) : -1;
    VAR_HIP_CHECK(c, hipMalloc((void**)&st->ws, (size_t)total * sizeof(float)));
    float* w = st->ws;
    st->frozen = w + ofz; st->wpk = (c3f::f32x4*)(w + owpk);
    st->a1 = w + oa1; st->p[1] = w + op1; st->p[2] = w + op2; st->p[3] = w + op3; st->p[4] = w + op4;
    st->a6 = w + oa6; st->hid = w + ohid; st->ctr = (unsigned*)(w + octr);
    st->s[1] = w + os1; st->s[2] = w + os2; st->s[3] = w + os3;
    st->GI = w + oGI; st->GH = w + oGH; st->Hb = w + oHb; st->hs1 = w + ohs1; st->hs2 = w + ohs2; st->graw = w + ograw;
    st->craw = ocraw >= 0 ? w + ocraw : nullptr;
    VAR_HIP_CHECK(c, hipMemset(st->ctr, 0, 64 * sizeof(float)));
    VAR_HIP_CHECK(c, hipDeviceSynchronize());
    return VAR_OK;
}

int var_ithor_reward_pack(var_ctx* c, void* stream, const float* params) {
    if (!c) return VAR_ERR_ARG;
    rew_state* st = rew(c);
    if (!st) { VAR_SET_ERR(c, "var_ithor_reward_pack: var_ithor_reward_plan first"); return VAR_ERR_PLAN; }
    if (!params) { VAR_SET_ERR(c, "var_ithor_reward_pack: params is NULL"); return VAR_ERR_ARG; }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    RUN(var_copy_async(c, s, st->frozen, params, sizeof(float) * (size_t)st->L.total));
    hipLaunchKernelGGL(rw_pack_kernel, dim3((st->pack.first[5] + 255) / 256), dim3(256), 0, s, (const float*)st->frozen, st->wpk, st->pack);
    AC_CHECK(c);
    st->packed = true;
    st->packed_from = params;
    return VAR_OK;
}

int var_ithor_reward_step(var_ctx* c, void* stream, const float* params, const void* image, int image_is_u8, long image_bstride,
                          const float* goal_mfcc, int B, float* image_feat, float* goal_feat, float* reward) {
    return var_ithor_reward_step_ex(c, stream, params, image, image_is_u8, image_bstride, goal_mfcc, nullptr, B, image_feat, goal_feat,
                                    nullptr, reward, nullptr, nullptr);
}

int var_ithor_reward_step_ex(var_ctx* c, void* stream, const float* params, const void* image, int image_is_u8, long image_bstride,
                             const float* goal_mfcc, const float* cur_mfcc, int B, float* image_feat, float* goal_feat, float* cur_feat,
                             float* reward, float* reward_img, float* reward_snd) {
    if (!c) return VAR_ERR_ARG;
    rew_state* st = rew(c);
    if (!st || B > st->maxB) { VAR_SET_ERR(c, "var_ithor_reward_step: var_ithor_reward_plan(%d, 96) first", B); return VAR_ERR_PLAN; }
    if (!params || !image || !image_feat || !goal_feat || !reward || B < 1 || (cur_mfcc && !cur_feat)) {
        VAR_SET_ERR(c, "var_ithor_reward_step: NULL argument or B < 1");
        return VAR_ERR_ARG;
    }
    // goal and current clips share one pass where both fit the fused GRU step's column block
    const bool merged = goal_mfcc && cur_mfcc && 2 * B <= kFusedClips;
    if (cur_mfcc && (!(st->flags & VAR_IREW_SOUND_SOUND) || (merged && 2 * B > st->maxB))) {
        VAR_SET_ERR(c, "var_ithor_reward_step_ex: var_ithor_reward_plan_ex(%d, 96, VAR_IREW_SOUND_SOUND) first", B);
        return VAR_ERR_PLAN;
    }
    if (image_bstride < 3L * 96 * 96) {
        VAR_SET_ERR(c, "var_ithor_reward_step: image stride %ld < 3*96*96", image_bstride);
        return VAR_ERR_ARG;
    }
    if (!st->packed) { VAR_SET_ERR(c, "var_ithor_reward_step: var_ithor_reward_pack first"); return VAR_ERR_STATE; }
    if (params != st->packed_from) {
        VAR_SET_ERR(c, "var_ithor_reward_step: params is not the arena of the last var_ithor_reward_pack (pack again)");
        return VAR_ERR_STATE;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const RewLayout& L = st->L;
    const float* P = st->frozen;
    RUN(image_convs(c, s, st, image, image_is_u8, image_bstride, B));
    const float* craw = nullptr;
    if (merged) {
        RUN(goal_branch(c, s, st, goal_mfcc, cur_mfcc, B, st->graw));
        craw = st->graw + 3 * B;
    } else {
        if (goal_mfcc) RUN(goal_branch(c, s, st, goal_mfcc, nullptr, B, st->graw));
        if (cur_mfcc) { RUN(goal_branch(c, s, st, cur_mfcc, nullptr, B, st->craw)); craw = st->craw; }
    }
    const float* graw = goal_mfcc ? (const float*)st->graw : (const float*)nullptr;
    if (cur_mfcc)
        hipLaunchKernelGGL(rw_tail_kernel<true>, dim3(kTailWG), dim3(256), 0, s, (const float*)st->a6, P + L.ih_w0, P + L.ih_b0, P + L.ih_w1,
                           P + L.ih_b1, B, st->hid, st->ctr, graw, goal_feat, image_feat, reward, craw, cur_feat, reward_img, reward_snd);
    else
        hipLaunchKernelGGL(rw_tail_kernel<false>, dim3(kTailWG), dim3(256), 0, s, (const float*)st->a6, P + L.ih_w0, P + L.ih_b0, P + L.ih_w1,
                           P + L.ih_b1, B, st->hid, st->ctr, graw, goal_feat, image_feat, reward, (const float*)nullptr, (float*)nullptr,
                           (float*)nullptr, (float*)nullptr);
    AC_CHECK(c);
    return VAR_OK;
}

int var_ithor_reward_embed(var_ctx* c, void* stream, const float* params, const float* mfcc, int n, float* out) {
    if (!c) return VAR_ERR_ARG;
    rew_state* st = rew(c);
    if (!st) { VAR_SET_ERR(c, "var_ithor_reward_embed: var_ithor_reward_plan first"); return VAR_ERR_PLAN; }
    if (!params || !mfcc || !out || n < 1) { VAR_SET_ERR(c, "var_ithor_reward_embed: NULL argument or n < 1"); return VAR_ERR_ARG; }
    if (!st->packed) { VAR_SET_ERR(c, "var_ithor_reward_embed: var_ithor_reward_pack first"); return VAR_ERR_STATE; }
    if (params != st->packed_from) {
        VAR_SET_ERR(c, "var_ithor_reward_embed: params is not the arena of the last var_ithor_reward_pack (pack again)");
        return VAR_ERR_STATE;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // passes over the plan's own sound buffers, each on the fused GRU route: a clip never mixes with the others of its pass
    const int pass = st->maxB < kFusedClips ? st->maxB : kFusedClips;
    for (int at = 0; at < n; at += pass) {
        const int m = n - at < pass ? n - at : pass;
        RUN(goal_branch(c, s, st, mfcc + (size_t)at * kT * kF, nullptr, m, st->graw));
        hipLaunchKernelGGL(rw_embed_finish_kernel, dim3(1), dim3(64), 0, s, (const float*)st->graw, out + (size_t)3 * at, m);
        AC_CHECK(c);
    }
    return VAR_OK;
}

int var_ithor_reward_step_ids(var_ctx* c, void* stream, const float* params, const void* image, int image_is_u8, long image_bstride,
                              const float* table, int table_rows, const int* goal_ids, const int* cur_ids, int B, float* image_feat,
                              float* goal_feat, float* cur_feat, float* reward, float* reward_img, float* reward_snd) {
    if (!c) return VAR_ERR_ARG;
    rew_state* st = rew(c);
    if (!st || B > st->maxB) { VAR_SET_ERR(c, "var_ithor_reward_step_ids: var_ithor_reward_plan(%d, 96) first", B); return VAR_ERR_PLAN; }
    if (!params || !image || !image_feat || !goal_feat || !reward || B < 1 || (cur_ids && !cur_feat)) {
        VAR_SET_ERR(c, "var_ithor_reward_step_ids: NULL argument or B < 1");
        return VAR_ERR_ARG;
    }
    if (!table || table_rows < 1) {
        VAR_SET_ERR(c, "var_ithor_reward_step_ids: no clip table (table_rows %d)", table_rows);
        return VAR_ERR_ARG;
    }
    if (image_bstride < 3L * 96 * 96) {
        VAR_SET_ERR(c, "var_ithor_reward_step_ids: image stride %ld < 3*96*96", image_bstride);
        return VAR_ERR_ARG;
    }
    if (!st->packed) { VAR_SET_ERR(c, "var_ithor_reward_step_ids: var_ithor_reward_pack first"); return VAR_ERR_STATE; }
    if (params != st->packed_from) {
        VAR_SET_ERR(c, "var_ithor_reward_step_ids: params is not the arena of the last var_ithor_reward_pack (pack again)");
        return VAR_ERR_STATE;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const RewLayout& L = st->L;
    const float* P = st->frozen;
    RUN(image_convs(c, s, st, image, image_is_u8, image_bstride, B));
    hipLaunchKernelGGL((rw_tail_kernel<false, true>), dim3(kTailWG), dim3(256), 0, s, (const float*)st->a6, P + L.ih_w0, P + L.ih_b0,
                       P + L.ih_w1, P + L.ih_b1, B, st->hid, st->ctr, (const float*)nullptr, goal_feat, image_feat, reward,
                       (const float*)nullptr, cur_feat, reward_img, reward_snd, table, table_rows, goal_ids, cur_ids);
    AC_CHECK(c);
    return VAR_OK;
}

}  // extern "C"
