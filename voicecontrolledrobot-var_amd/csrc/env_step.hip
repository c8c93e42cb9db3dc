// The env wrapper's step between "the simulator returned" and "the next act may run" (Envs/vec_env/vec_pretext_normalize.py:47-61,
// 96-101; RL.py:171-185), two launches that a captured graph replays with frozen arguments:
//   var_reward_norm_step  calcReward's sum, the discounted-return normalisation with its running variance, the clip, masks and
//                         bad_masks, the episode bookkeeping of RL.py:171-176 and the rollout slot -- one workgroup, float64
//   var_rollout_move_at   var_rollout_move whose destinations are selected by a slot word on the device (RolloutStorage.insert)
// float64 throughout, each operation rounded once (-ffp-contract=off): the state follows the reference's numpy bit for bit.
#include "var_common.h"
#include "rollout_move.h"

namespace {

constexpr int kMaxEnvs = 128;                                   // numpy's pairwise recursion starts beyond 128 elements

// np.add.reduce over a contiguous float64 vector of n <= 128 elements (numpy's pairwise sum below its block size): left to
// right under 8 elements; else eight running sums over blocks of eight, folded ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
// remaining elements one by one.  SQ: sum (a - mean) * (a - mean) instead (numpy's _var).
template <bool SQ>
__device__ __forceinline__ double numpy_sum(const double* a, int n, double mean) {
    auto at = [&](int i) { const double v = a[i]; if (!SQ) return v; const double d = v - mean; return d * d; };
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += at(i);
        return res;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = at(k);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += at(i + k);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += at(i);
    return res;
}

__global__ void __launch_bounds__(kMaxEnvs) reward_norm_kernel(const float* __restrict__ dot, const double* __restrict__ env_reward,
                                                               const unsigned char* __restrict__ done,
                                                               const unsigned char* __restrict__ bad, int N, double gamma,
                                                               double cliprew, double epsilon, int normalise, int num_steps,
                                                               double* __restrict__ ret, double* __restrict__ rms,
                                                               double* __restrict__ episode, int* __restrict__ slot,
                                                               float* __restrict__ reward, float* __restrict__ masks,
                                                               float* __restrict__ bad_masks, double* __restrict__ orig_reward) {
    __shared__ double ret_s[kMaxEnvs];
    __shared__ double var_s;
    const int i = threadIdx.x;
    double rews = 0.0, r = 0.0;
    if (i < N) {
        rews = (dot ? (double)dot[i] : 0.0) + env_reward[i];    // calcReward (:96-101; the sound-sound term is off)
        r = ret[i] * gamma + rews;                              // :55
        ret_s[i] = r;
    }
    __syncthreads();
    if (i == 0) {
        if (normalise) {                                        // :57, running_mean_std.py:14-35
            const double cnt = (double)N;
            const double bmean = numpy_sum<false>(ret_s, N, 0.0) / cnt;
            const double bvar = numpy_sum<true>(ret_s, N, bmean) / cnt;
            const double mean = rms[0], var = rms[1], count = rms[2];
            const double delta = bmean - mean;
            const double total = count + cnt;
            const double m2 = (var * count + bvar * cnt) + (((delta * delta) * count) * cnt) / total;
            const double nvar = m2 / total;
            rms[0] = mean + (delta * cnt) / total;
            rms[1] = nvar;
            rms[2] = total;
            var_s = nvar;
        }
        const int s = slot[0];
        slot[1] = s;
        slot[0] = (s + 1) % num_steps;
    }
    __syncthreads();
    if (i >= N) return;
    double out = rews;
    if (normalise) {                                            // :58
        out = rews / sqrt(var_s + epsilon);
        out = out < -cliprew ? -cliprew : (out > cliprew ? cliprew : out);     // (np.clip: a NaN stays a NaN)
    }
    const bool d = done[i] != 0;
    orig_reward[i] = rews;                                      // :53
    reward[i] = (float)out;
    masks[i] = d ? 0.f : 1.f;                                   // RL.py:179-183
    bad_masks[i] = (bad && bad[i]) ? 0.f : 1.f;
    ret[i] = d ? 0.0 : r;                                       // :59
    const double run = episode[i] + rews;                       // RL.py:171-176
    if (d) { episode[N + i] = run; episode[2 * N + i] = episode[2 * N + i] + 1.0; }
    episode[i] = d ? 0.0 : run;
}

// ---- var_rollout_move_at ----------------------------------------------------------------------------------------------------
struct SlotTable { long stride[VAR_MOVE_MAX_SEGS]; int add[VAR_MOVE_MAX_SEGS], n_slots[VAR_MOVE_MAX_SEGS]; };

__global__ void __launch_bounds__(var_move::kThreads) rollout_move_at_kernel(var_move::MoveTable tab, SlotTable st,
                                                                            const int* __restrict__ slot, int n_env) {
    const unsigned b = blockIdx.x;
    const int si = var_move::move_segment_of(tab, b);
    long off = 0;
    if (st.stride[si] != 0) {
        const long s = (long)slot[0] + st.add[si];
        if (s < 0 || s >= st.n_slots[si]) return;               // a slot outside the store: the segment is left unwritten
        off = s * st.stride[si];
    }
    var_move::move_piece(tab.s[si], b, nullptr, n_env, n_env, off);
}

}  // namespace

extern "C" int var_reward_norm_step(var_ctx* c, void* stream, const float* dot, const double* env_reward, const unsigned char* done,
                                    const unsigned char* bad, int N, double gamma, double cliprew, double epsilon, int normalise,
                                    int num_steps, double* ret, double* rms, double* episode, int* slot, float* reward, float* masks,
                                    float* bad_masks, double* orig_reward) {
    if (!c) return VAR_ERR_ARG;
    if (N < 1 || N > kMaxEnvs || num_steps < 1) {
        VAR_SET_ERR(c, "var_reward_norm_step: N %d (1..%d), num_steps %d (>= 1)", N, kMaxEnvs, num_steps);
        return VAR_ERR_ARG;
    }
    if (!env_reward || !done || !ret || !rms || !episode || !slot || !reward || !masks || !bad_masks || !orig_reward) {
        VAR_SET_ERR(c, "var_reward_norm_step: a NULL pointer (only dot and bad may be NULL)");
        return VAR_ERR_ARG;
    }
    const size_t n8 = sizeof(double) * (size_t)N, n4 = sizeof(float) * (size_t)N;
    const void* outs[] = {ret, rms, episode, slot, reward, masks, bad_masks, orig_reward};
    const size_t outn[] = {n8, 3 * sizeof(double), 3 * n8, 2 * sizeof(int), n4, n4, n4, n8};
    const void* ins[] = {dot, env_reward, done, bad};
    const size_t inn[] = {n4, n8, (size_t)N, (size_t)N};
    for (int i = 0; i < 8; ++i) {
        for (int j = 0; j < 4; ++j) {
            if (ins[j] && var_move::overlap(outs[i], outn[i], ins[j], inn[j])) {
                VAR_SET_ERR(c, "var_reward_norm_step: output or state %d overlaps input %d", i, j);
                return VAR_ERR_ARG;
            }
        }
        for (int j = i + 1; j < 8; ++j) {
            if (var_move::overlap(outs[i], outn[i], outs[j], outn[j])) {
                VAR_SET_ERR(c, "var_reward_norm_step: outputs / state %d and %d overlap", i, j);
                return VAR_ERR_ARG;
            }
        }
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(reward_norm_kernel, dim3(1), dim3(kMaxEnvs), 0, (hipStream_t)stream, dot, env_reward, done, bad, N, gamma,
                       cliprew, epsilon, normalise, num_steps, ret, rms, episode, slot, reward, masks, bad_masks, orig_reward);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}

extern "C" int var_rollout_move_at(var_ctx* c, void* stream, const var_move_at_seg* segs, int n_seg, const int* slot, int n_env) {
    if (!c) return VAR_ERR_ARG;
    if (!segs || n_seg < 1 || n_seg > VAR_MOVE_MAX_SEGS) {
        VAR_SET_ERR(c, "var_rollout_move_at: %d segments (1..%d, table not NULL)", n_seg, VAR_MOVE_MAX_SEGS);
        return VAR_ERR_ARG;
    }
    if (!slot || n_env < 1) { VAR_SET_ERR(c, "var_rollout_move_at: slot NULL or n_env %d < 1", n_env); return VAR_ERR_ARG; }
    var_move::MoveTable tab{};
    SlotTable st{};
    tab.n = n_seg;
    size_t sext[VAR_MOVE_MAX_SEGS], dext[VAR_MOVE_MAX_SEGS];
    unsigned long long blocks = 0;
    for (int i = 0; i < n_seg; ++i) {
        const var_move_at_seg& u = segs[i];
        if (u.dst_slot_stride < 0 || u.n_slots < 1 || (u.dst_slot_stride == 0 && u.n_slots != 1)) {
            VAR_SET_ERR(c, "var_rollout_move_at: segment %d: dst_slot_stride %ld < 0, n_slots %d < 1, or more than one slot "
                           "at stride 0", i, u.dst_slot_stride, u.n_slots);
            return VAR_ERR_ARG;
        }
        const int rc = var_move::move_plan_seg(c, "var_rollout_move_at", i, u.seg, n_env, n_env, (unsigned long long)u.dst_slot_stride,
                                               tab.s[i], blocks, sext[i], dext[i]);
        if (rc != VAR_OK) return rc;
        if (u.dst_slot_stride != 0 && (size_t)u.dst_slot_stride < dext[i]) {
            VAR_SET_ERR(c, "var_rollout_move_at: segment %d: slots of the destination overlap each other", i);
            return VAR_ERR_ARG;
        }
        dext[i] += (size_t)(u.n_slots - 1) * (size_t)u.dst_slot_stride;      // every slot the device word may select
        st.stride[i] = u.dst_slot_stride; st.add[i] = u.slot_add; st.n_slots[i] = u.n_slots;
    }
    for (int i = 0; i < n_seg; ++i) {
        if (var_move::overlap(segs[i].seg.dst, dext[i], slot, sizeof(int))) {
            VAR_SET_ERR(c, "var_rollout_move_at: the destination range of segment %d holds the slot word", i);
            return VAR_ERR_ARG;
        }
        for (int j = 0; j < n_seg; ++j) {
            if (var_move::overlap(segs[i].seg.dst, dext[i], segs[j].seg.src, sext[j]) ||
                (i < j && var_move::overlap(segs[i].seg.dst, dext[i], segs[j].seg.dst, dext[j]))) {
                VAR_SET_ERR(c, "var_rollout_move_at: the destination range of segment %d overlaps a range of segment %d", i, j);
                return VAR_ERR_ARG;
            }
        }
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(rollout_move_at_kernel, dim3((unsigned)blocks), dim3(var_move::kThreads), 0, (hipStream_t)stream, tab, st, slot,
                       n_env);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}
