// What surrounds the networks in one PPO rollout (models/ppo/storage.py, models/ppo/algo/ppo.py:38-87), three launches:
//   var_rollout_move     one strided row copy behind RolloutStorage.insert / after_update and one recurrent_generator minibatch
//   var_rollout_returns  compute_returns (all four modes) and the normalised advantages, one workgroup
//   var_ppo_head         the clipped-surrogate / value / entropy loss of one minibatch with its gradients
// Latency work: each replaces tens to hundreds of torch launches on (N,1) / (T*N,1) tensors.  fp32, no product is contracted
// into an fma (-ffp-contract=off): the recurrences below round where the reference's torch expressions round.
#include "var_common.h"
#include "rollout_move.h"
#include "ppo_row.h"

namespace {

constexpr int kThreads = var_move::kThreads;

using var_ppo::block_sum;                                      // (ppo_row.h: the fixed-order workgroup sum)

// ---- var_rollout_move -----------------------------------------------------------------------------------------------------
// The piece copy, the segment table and its host-side planning live in rollout_move.h (var_rollout_move_at shares them).
using var_move::MoveTable;
using var_move::overlap;                                       // (var_rollout_returns)

__global__ void __launch_bounds__(kThreads) rollout_move_kernel(MoveTable tab, const int* __restrict__ ind, int n_env, int n_src_env) {
    const unsigned b = blockIdx.x;
    var_move::move_piece(tab.s[var_move::move_segment_of(tab, b)], b, ind, n_env, n_src_env, 0);
}

// ---- var_rollout_returns --------------------------------------------------------------------------------------------------
// Thread `env` walks its column backwards, eight steps' loads ahead of the eight dependent updates; then, behind a barrier, all
// threads take the T * N advantages flat: mean, squared deviations, the normalised values.  MODE: 0 GAE, 1 plain returns;
// PROPER: use_proper_time_limits.
constexpr int kAhead = 8;
template <int GAE, int PROPER>
__device__ __forceinline__ void returns_columns(const float* __restrict__ r, float* v, const float* __restrict__ m,
                                                const float* __restrict__ bm, const float* __restrict__ next_value, float* ret,
                                                int T, int N, float g, float gl) {
    for (int env = threadIdx.x; env < N; env += kThreads) {
        const float nv = next_value[env];
        if (GAE) v[(long)T * N + env] = nv; else ret[(long)T * N + env] = nv;
        float a = 0.f, v1 = nv, ret1 = nv;                      // gae | value_preds[t + 1] | returns[t + 1]
        for (int t0 = T - 1; t0 >= 0; t0 -= kAhead) {
            float rr[kAhead], vv[kAhead], mm[kAhead], bb[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) {
                const int t = t0 - k >= 0 ? t0 - k : 0;
                const long i = (long)t * N + env;
                rr[k] = r[i]; mm[k] = m[i + N];
                vv[k] = (GAE || PROPER) ? v[i] : 0.f;
                bb[k] = PROPER ? bm[i + N] : 1.f;
            }
#pragma unroll
            for (int k = 0; k < kAhead; ++k) {
                const int t = t0 - k;
                if (t >= 0) {
                    const long i = (long)t * N + env;
                    if (GAE) {
                        const float d = (rr[k] + (g * v1) * mm[k]) - vv[k];
                        a = d + (gl * mm[k]) * a;
                        if (PROPER) a = a * bb[k];
                        ret[i] = a + vv[k];
                        v1 = vv[k];
                    } else {
                        if (PROPER) ret1 = ((ret1 * g) * mm[k] + rr[k]) * bb[k] + (1.f - bb[k]) * vv[k];
                        else ret1 = (ret1 * g) * mm[k] + rr[k];
                        ret[i] = ret1;
                    }
                }
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads) rollout_returns_kernel(const float* __restrict__ r, float* v, const float* __restrict__ m,
                                                                  const float* __restrict__ bm, const float* __restrict__ next_value,
                                                                  float* ret, float* __restrict__ adv, int T, int N, int mode, float g,
                                                                  float gl) {
    __shared__ float sm4[4];
    if (mode == 0) returns_columns<1, 0>(r, v, m, bm, next_value, ret, T, N, g, gl);
    else if (mode == 1) returns_columns<1, 1>(r, v, m, bm, next_value, ret, T, N, g, gl);
    else if (mode == 2) returns_columns<0, 0>(r, v, m, bm, next_value, ret, T, N, g, gl);
    else returns_columns<0, 1>(r, v, m, bm, next_value, ret, T, N, g, gl);
    if (!adv) return;
    __syncthreads();                                           // the columns' stores: visible to the whole workgroup
    const long TN = (long)T * N;
    float s = 0.f;
    for (long i = threadIdx.x; i < TN; i += kThreads) s += ret[i] - v[i];
    const float mean = block_sum(s, sm4) / (float)TN;
    float q = 0.f;
    for (long i = threadIdx.x; i < TN; i += kThreads) { const float d = (ret[i] - v[i]) - mean; q += d * d; }
    const float sd = sqrtf(block_sum(q, sm4) / (float)(TN - 1));
    for (long i = threadIdx.x; i < TN; i += kThreads) adv[i] = ((ret[i] - v[i]) - mean) / (sd + 1e-5f);
}

// ---- var_ppo_head ---------------------------------------------------------------------------------------------------------
// One thread per row, rows grid-strided over at most kPpoMaxWG workgroups.  A row writes its own gradients (1 / M is known);
// the sums -- value loss, action loss, entropy, d total / d logstd -- go workgroup by workgroup into the context's partials
// (agent-scope stores), and the LAST workgroup to take a ticket folds them (policy_dist_kernel's counter: no wait anywhere).
// The row math, the fold and the last step live in ppo_row.h (var_ppo_head_linear shares them).

template <int KIND>
__global__ void __launch_bounds__(kThreads) ppo_head_kernel(const float* __restrict__ head, const float* __restrict__ logstd,
                                                           const float* __restrict__ value, const void* __restrict__ action,
                                                           const float* __restrict__ old_logp, const float* __restrict__ adv,
                                                           const float* __restrict__ returns, const float* __restrict__ value_preds,
                                                           int n, long M, float clip, float vcoef, float ecoef, int clipped,
                                                           float* __restrict__ out, float* __restrict__ g_head,
                                                           float* __restrict__ g_value, float* __restrict__ g_logstd,
                                                           float* __restrict__ logp_out, float* part, unsigned* ticket) {
    __shared__ float sm4[4];
    __shared__ int last_s;
    const int tid = threadIdx.x;
    const float invM = 1.f / (float)M;
    var_ppo::RowSums s;
    for (long row = (long)blockIdx.x * kThreads + tid; row < M; row += (long)gridDim.x * kThreads) {
        var_ppo::ppo_row<KIND>(head + row * n, g_head + row * n, row, logstd, value, action, old_logp, adv, returns, value_preds, n,
                               invM, clip, vcoef, ecoef, clipped, g_value, logp_out, s);
    }
    float tot[kPpoSums];
    var_ppo::ppo_block_sums<KIND>(s, sm4, tot);
    if (gridDim.x > 1) {
        if (tid < kPpoSums - 1) {
            float mine = tot[0];
#pragma unroll
            for (int q = 1; q < kPpoSums - 1; ++q) mine = tid == q ? tot[q] : mine;
            join_store(part + tid * kPpoMaxWG + blockIdx.x, mine);
        }
        __syncthreads();                                       // (the partials of this workgroup are acknowledged)
        if (tid == 0) {
            last_s = atomicAdd(ticket, 1u) == gridDim.x - 1;
            if (last_s) atomicExch(ticket, 0u);
        }
        __syncthreads();
        if (!last_s) return;
        var_ppo::ppo_fold_sums<KIND>(part, kPpoMaxWG, 1, (int)gridDim.x, sm4, tot);
    }
    if (tid != 0) return;
    var_ppo::ppo_finish<KIND>(tot, logstd, n, invM, vcoef, ecoef, out, g_logstd);
}

}  // namespace

extern "C" int var_rollout_move(var_ctx* c, void* stream, const var_move_seg* segs, int n_seg, const int* ind, int n_env,
                                int n_src_env) {
    if (!c) return VAR_ERR_ARG;
    MoveTable tab{};
    size_t dext[VAR_MOVE_MAX_SEGS];
    unsigned long long blocks = 0;
    const int rc = var_move::move_plan_gather(c, "var_rollout_move", segs, n_seg, ind != nullptr, n_env, n_src_env, tab, blocks, dext);
    if (rc != VAR_OK) return rc;
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(rollout_move_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, tab, ind, n_env, n_src_env);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}

extern "C" int var_rollout_returns(var_ctx* c, void* stream, const float* rewards, float* value_preds, const float* masks,
                                   const float* bad_masks, const float* next_value, int T, int N, int use_gae, double gamma,
                                   double gae_lambda, int use_proper_time_limits, float* returns, float* advantages) {
    if (!c) return VAR_ERR_ARG;
    if (T < 1 || N < 1) { VAR_SET_ERR(c, "var_rollout_returns: T %d, N %d (>= 1)", T, N); return VAR_ERR_ARG; }
    if (!rewards || !value_preds || !masks || !next_value || !returns || (use_proper_time_limits && !bad_masks)) {
        VAR_SET_ERR(c, "var_rollout_returns: rewards, value_preds, masks, next_value, returns%s must not be NULL",
                    use_proper_time_limits ? ", bad_masks" : "");
        return VAR_ERR_ARG;
    }
    if (advantages && (long)T * N < 2) {
        VAR_SET_ERR(c, "var_rollout_returns: advantages of T * N = 1 value have no standard deviation");
        return VAR_ERR_ARG;
    }
    const size_t tn = sizeof(float) * (size_t)T * N, tn1 = tn + sizeof(float) * (size_t)N;
    if (overlap(returns, tn1, value_preds, tn1) || overlap(returns, tn1, rewards, tn) || overlap(returns, tn1, masks, tn1) ||
        overlap(returns, tn1, next_value, sizeof(float) * N) || (bad_masks && overlap(returns, tn1, bad_masks, tn1)) ||
        (advantages && (overlap(advantages, tn, returns, tn1) || overlap(advantages, tn, value_preds, tn1) ||
                        overlap(advantages, tn, rewards, tn) || overlap(advantages, tn, masks, tn1) ||
                        overlap(advantages, tn, next_value, sizeof(float) * N) || (bad_masks && overlap(advantages, tn, bad_masks, tn1)))) ||
        (use_gae && (overlap(value_preds, tn1, rewards, tn) || overlap(value_preds, tn1, masks, tn1) ||
                     overlap(value_preds, tn1, next_value, sizeof(float) * N) || (bad_masks && overlap(value_preds, tn1, bad_masks, tn1))))) {
        VAR_SET_ERR(c, "var_rollout_returns: an output overlaps an input or the other output");
        return VAR_ERR_ARG;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    const int mode = (use_gae ? 0 : 2) + (use_proper_time_limits ? 1 : 0);
    hipLaunchKernelGGL(rollout_returns_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, rewards, value_preds, masks, bad_masks,
                       next_value, returns, advantages, T, N, mode, (float)gamma, (float)(gamma * gae_lambda));
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}

extern "C" int var_ppo_head(var_ctx* c, void* stream, int kind, const float* head, const float* logstd, const float* value,
                            const void* action, const float* old_logp, const float* adv, const float* returns,
                            const float* value_preds, int n, long M, float clip, float value_coef, float entropy_coef,
                            int use_clipped_value_loss, float* out, float* g_head, float* g_value, float* g_logstd, float* logp) {
    if (!c) return VAR_ERR_ARG;
    const int rc = var_ppo::ppo_check_args(c, "var_ppo_head", kind, n, M, clip, value, action, old_logp, adv, returns, value_preds,
                                           use_clipped_value_loss, logstd, g_logstd, out, g_value);
    if (rc != VAR_OK) return rc;
    if (!head || !g_head) { VAR_SET_ERR(c, "var_ppo_head: head and g_head must not be NULL"); return VAR_ERR_ARG; }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    long wg = (M + kThreads - 1) / kThreads;
    if (wg > kPpoMaxWG) wg = kPpoMaxWG;
    auto kern = kind == 0 ? ppo_head_kernel<0> : ppo_head_kernel<1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)wg), dim3(kThreads), 0, (hipStream_t)stream, head, logstd, value, action, old_logp, adv,
                       returns, value_preds, n, M, clip, value_coef, entropy_coef, use_clipped_value_loss, out, g_head, g_value, g_logstd,
                       logp, c->ppo_part, c->ppo_ctr);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}
