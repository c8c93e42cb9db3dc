// What surrounds the networks in one PPO rollout (models/ppo/storage.py, models/ppo/algo/ppo.py:38-87), three launches:
//   var_rollout_move     one strided row copy behind RolloutStorage.insert / after_update and one recurrent_generator minibatch
//   var_rollout_returns  compute_returns (all four modes) and the normalised advantages, one workgroup
//   var_ppo_head         the clipped-surrogate / value / entropy loss of one minibatch with its gradients
// Latency work: each replaces tens to hundreds of torch launches on (N,1) / (T*N,1) tensors.  fp32, no product is contracted
// into an fma (-ffp-contract=off): the recurrences below round where the reference's torch expressions round.
#include "var_common.h"
#include "rollout_move.h"

namespace {

constexpr int kThreads = var_move::kThreads;

// Sum over the workgroup in a fixed order: butterfly inside each wave, then the four wave sums in index order.  Every thread
// returns the same value; two calls may follow each other (the barrier at the top protects the previous call's reads).
__device__ __forceinline__ float block_sum(float v, float* sm4) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sm4[0] + sm4[1]) + sm4[2]) + sm4[3];
}

// ---- var_rollout_move -----------------------------------------------------------------------------------------------------
// The piece copy, the segment table and its host-side planning live in rollout_move.h (var_rollout_move_at shares them).
using var_move::MoveTable;
using var_move::overlap;

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
constexpr int kMaxGauss = 4, kMaxCat = 16;
constexpr float kHalfLog2Pi = 0.9189385332046727f;

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
    float s_v = 0.f, s_a = 0.f, s_e = 0.f, s_ls[kMaxGauss] = {0.f, 0.f, 0.f, 0.f};
    for (long row = (long)blockIdx.x * kThreads + tid; row < M; row += (long)gridDim.x * kThreads) {
        // value loss (ppo.py:73-82)
        const float v = value[row], rt = returns[row];
        float gv;
        if (clipped) {
            const float vp = value_preds[row], dv = v - vp;
            const float vpc = vp + fminf(fmaxf(dv, -clip), clip);
            const float e1 = v - rt, e2 = vpc - rt, l1 = e1 * e1, l2 = e2 * e2;
            s_v += fmaxf(l1, l2);
            const float w1 = l1 > l2 ? 1.f : (l1 == l2 ? 0.5f : 0.f), w2 = 1.f - w1;
            const float gate = (dv >= -clip && dv <= clip) ? 1.f : 0.f;
            gv = w1 * (2.f * e1) + (w2 * gate) * (2.f * e2);
        } else {
            const float e1 = rt - v;
            s_v += e1 * e1;
            gv = -2.f * e1;
        }
        g_value[row] = (0.5f * vcoef * invM) * gv;
        const float ol = old_logp[row], ad = adv[row];
        if (KIND == 0) {
            float lp = 0.f, diff[kMaxGauss], var[kMaxGauss];
#pragma unroll
            for (int d = 0; d < kMaxGauss; ++d) {
                diff[d] = 0.f; var[d] = 1.f;
                if (d < n) {
                    const float ls = logstd[d], sd = expf(ls);
                    diff[d] = ((const float*)action)[row * n + d] - head[row * n + d];
                    var[d] = sd * sd;
                    lp += -(diff[d] * diff[d]) / (2.f * var[d]) - ls - kHalfLog2Pi;
                }
            }
            if (logp_out) logp_out[row] = lp;
            const float ratio = expf(lp - ol);
            const float s1 = ratio * ad, s2 = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip) * ad;
            s_a += fminf(s1, s2);
            const float glp = s1 <= s2 ? -(ad * ratio) * invM : 0.f;      // d action_loss / d logp
#pragma unroll
            for (int d = 0; d < kMaxGauss; ++d) {
                if (d < n) {
                    g_head[row * n + d] = glp * (diff[d] / var[d]);
                    s_ls[d] += glp * ((diff[d] * diff[d]) / var[d] - 1.f);
                }
            }
        } else {
            float l[kMaxCat];
            float mx = head[row * n];
#pragma unroll
            for (int k = 0; k < kMaxCat; ++k) { l[k] = k < n ? head[row * n + k] : 0.f; if (k > 0 && k < n) mx = fmaxf(mx, l[k]); }
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < kMaxCat; ++k) sum += k < n ? expf(l[k] - mx) : 0.f;
            const float lse = logf(sum);
            const long long a = ((const long long*)action)[row];
            float la = __builtin_nanf(""), H = 0.f, pk[kMaxCat];   // an action outside [0, n) gives NaN, never a wild read
#pragma unroll
            for (int k = 0; k < kMaxCat; ++k) {
                l[k] = (l[k] - mx) - lse;                          // log p_k
                pk[k] = k < n ? expf(l[k]) : 0.f;
                H -= k < n ? pk[k] * l[k] : 0.f;
                la = (long long)k == a && k < n ? l[k] : la;
            }
            if (logp_out) logp_out[row] = la;
            const float ratio = expf(la - ol);
            const float s1 = ratio * ad, s2 = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip) * ad;
            s_a += fminf(s1, s2);
            s_e += H;
            const float glp = s1 <= s2 ? -(ad * ratio) * invM : 0.f;
            const float ge = ecoef * invM;                         // total has -ecoef * mean(H): dH / dl_k = -p_k (log p_k + H)
#pragma unroll
            for (int k = 0; k < kMaxCat; ++k) {
                if (k < n) g_head[row * n + k] = glp * (((long long)k == a ? 1.f : 0.f) - pk[k]) + ge * (pk[k] * (l[k] + H));
            }
        }
    }
    float tot[kPpoSums];
    tot[0] = block_sum(s_v, sm4); tot[1] = block_sum(s_a, sm4); tot[2] = block_sum(s_e, sm4);
#pragma unroll
    for (int d = 0; d < kMaxGauss; ++d) tot[3 + d] = KIND == 0 ? block_sum(s_ls[d], sm4) : 0.f;
    tot[7] = 0.f;
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
#pragma unroll
        for (int q = 0; q < kPpoSums - 1; ++q) {
            const bool live = (KIND == 0 ? q != 2 : q < 3) && tid < (int)gridDim.x;
            tot[q] = block_sum(live ? join_load(part + q * kPpoMaxWG + tid) : 0.f, sm4);
        }
    }
    if (tid != 0) return;
    const float vl = 0.5f * (tot[0] * invM), al = -(tot[1] * invM);
    float ent;
    if (KIND == 0) {
        float e = 0.f;
#pragma unroll
        for (int d = 0; d < kMaxGauss; ++d) {
            if (d < n) {
                e += (0.5f + kHalfLog2Pi) + logstd[d];
                g_logstd[d] = tot[3 + d] - ecoef / (float)n;
            }
        }
        ent = e / (float)n;
    } else {
        ent = tot[2] * invM;
    }
    out[0] = vl; out[1] = al; out[2] = ent;
    out[3] = (vl * vcoef + al) - ent * ecoef;
}

}  // namespace

extern "C" int var_rollout_move(var_ctx* c, void* stream, const var_move_seg* segs, int n_seg, const int* ind, int n_env,
                                int n_src_env) {
    if (!c) return VAR_ERR_ARG;
    if (!segs || n_seg < 1 || n_seg > VAR_MOVE_MAX_SEGS) {
        VAR_SET_ERR(c, "var_rollout_move: %d segments (1..%d, table not NULL)", n_seg, VAR_MOVE_MAX_SEGS);
        return VAR_ERR_ARG;
    }
    if (n_env < 1 || n_src_env < 1 || (!ind && n_env > n_src_env)) {
        VAR_SET_ERR(c, "var_rollout_move: n_env %d, n_src_env %d (>= 1; without an index list n_env <= n_src_env)", n_env, n_src_env);
        return VAR_ERR_ARG;
    }
    MoveTable tab{};
    tab.n = n_seg;
    size_t sext[VAR_MOVE_MAX_SEGS], dext[VAR_MOVE_MAX_SEGS];
    unsigned long long blocks = 0;
    for (int i = 0; i < n_seg; ++i) {
        const int rc = var_move::move_plan_seg(c, "var_rollout_move", i, segs[i], n_env, n_src_env, 0, tab.s[i], blocks, sext[i], dext[i]);
        if (rc != VAR_OK) return rc;
    }
    for (int i = 0; i < n_seg; ++i) {
        for (int j = 0; j < n_seg; ++j) {
            if (overlap(segs[i].dst, dext[i], segs[j].src, sext[j]) || (i < j && overlap(segs[i].dst, dext[i], segs[j].dst, dext[j]))) {
                VAR_SET_ERR(c, "var_rollout_move: the destination range of segment %d overlaps a range of segment %d", i, j);
                return VAR_ERR_ARG;
            }
        }
    }
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
    if (kind != 0 && kind != 1) { VAR_SET_ERR(c, "var_ppo_head: kind %d (0 DiagGaussian, 1 Categorical)", kind); return VAR_ERR_ARG; }
    if (M < 1) { VAR_SET_ERR(c, "var_ppo_head: M %ld < 1", M); return VAR_ERR_ARG; }
    const int nmax = kind == 0 ? kMaxGauss : kMaxCat;
    if (n < 1 || n > nmax) { VAR_SET_ERR(c, "var_ppo_head: n %d outside 1..%d", n, nmax); return VAR_ERR_ARG; }
    if (!head || !value || !action || !old_logp || !adv || !returns || !out || !g_head || !g_value ||
        (use_clipped_value_loss && !value_preds) || (kind == 0 && (!logstd || !g_logstd))) {
        VAR_SET_ERR(c, "var_ppo_head: a NULL pointer (only value_preds without the clipped value loss, and logstd / g_logstd "
                       "of a Categorical head, may be NULL)");
        return VAR_ERR_ARG;
    }
    if (!(clip >= 0.f)) { VAR_SET_ERR(c, "var_ppo_head: clip %g < 0", (double)clip); return VAR_ERR_ARG; }
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
