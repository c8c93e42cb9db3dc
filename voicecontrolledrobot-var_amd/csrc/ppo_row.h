// The PPO loss of one minibatch row (models/ppo/algo/ppo.py:66-87) with its gradients, and the last step from the folded sums to
// out[4] / g_logstd: ONE definition for var_ppo_head (rollout.hip: the head comes from memory) and var_ppo_head_linear
// (ppo_step.hip: the head comes from the Linear in front of it).  The kinks are documented in include/var_hip.h.  fp32, no
// product is contracted into an fma (-ffp-contract=off).
#pragma once
#include "var_common.h"

namespace var_ppo {

constexpr int kThreads = 256;
constexpr int kMaxGauss = 4, kMaxCat = 16;
constexpr float kHalfLog2Pi = 0.9189385332046727f;

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

// What one thread adds up over its rows: value loss, action loss, entropy, d total / d logstd.
struct RowSums { float v = 0.f, a = 0.f, e = 0.f, ls[kMaxGauss] = {0.f, 0.f, 0.f, 0.f}; };

// Row `row`: reads its n head values at head_row, writes its n gradients to g_head_row (either may be global or LDS) and
// g_value[row] (1 / M is known), adds its terms to `s`.
template <int KIND>
__device__ __forceinline__ void ppo_row(const float* head_row, float* g_head_row, long row, const float* __restrict__ logstd,
                                        const float* __restrict__ value, const void* __restrict__ action,
                                        const float* __restrict__ old_logp, const float* __restrict__ adv,
                                        const float* __restrict__ returns, const float* __restrict__ value_preds, int n, float invM,
                                        float clip, float vcoef, float ecoef, int clipped, float* __restrict__ g_value,
                                        float* __restrict__ logp_out, RowSums& s) {
    // value loss (ppo.py:73-82)
    const float v = value[row], rt = returns[row];
    float gv;
    if (clipped) {
        const float vp = value_preds[row], dv = v - vp;
        const float vpc = vp + fminf(fmaxf(dv, -clip), clip);
        const float e1 = v - rt, e2 = vpc - rt, l1 = e1 * e1, l2 = e2 * e2;
        s.v += fmaxf(l1, l2);
        const float w1 = l1 > l2 ? 1.f : (l1 == l2 ? 0.5f : 0.f), w2 = 1.f - w1;
        const float gate = (dv >= -clip && dv <= clip) ? 1.f : 0.f;
        gv = w1 * (2.f * e1) + (w2 * gate) * (2.f * e2);
    } else {
        const float e1 = rt - v;
        s.v += e1 * e1;
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
                diff[d] = ((const float*)action)[row * n + d] - head_row[d];
                var[d] = sd * sd;
                lp += -(diff[d] * diff[d]) / (2.f * var[d]) - ls - kHalfLog2Pi;
            }
        }
        if (logp_out) logp_out[row] = lp;
        const float ratio = expf(lp - ol);
        const float s1 = ratio * ad, s2 = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip) * ad;
        s.a += fminf(s1, s2);
        const float glp = s1 <= s2 ? -(ad * ratio) * invM : 0.f;      // d action_loss / d logp
#pragma unroll
        for (int d = 0; d < kMaxGauss; ++d) {
            if (d < n) {
                g_head_row[d] = glp * (diff[d] / var[d]);
                s.ls[d] += glp * ((diff[d] * diff[d]) / var[d] - 1.f);
            }
        }
    } else {
        float l[kMaxCat];
        float mx = head_row[0];
#pragma unroll
        for (int k = 0; k < kMaxCat; ++k) { l[k] = k < n ? head_row[k] : 0.f; if (k > 0 && k < n) mx = fmaxf(mx, l[k]); }
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
        s.a += fminf(s1, s2);
        s.e += H;
        const float glp = s1 <= s2 ? -(ad * ratio) * invM : 0.f;
        const float ge = ecoef * invM;                         // total has -ecoef * mean(H): dH / dl_k = -p_k (log p_k + H)
#pragma unroll
        for (int k = 0; k < kMaxCat; ++k) {
            if (k < n) g_head_row[k] = glp * (((long long)k == a ? 1.f : 0.f) - pk[k]) + ge * (pk[k] * (l[k] + H));
        }
    }
}

// The workgroup's sums of its threads' RowSums, tot[kPpoSums] in the order of the partials: v, a, e, ls[0..3], 0.
template <int KIND>
__device__ __forceinline__ void ppo_block_sums(const RowSums& s, float* sm4, float* tot) {
    tot[0] = block_sum(s.v, sm4); tot[1] = block_sum(s.a, sm4); tot[2] = block_sum(s.e, sm4);
#pragma unroll
    for (int d = 0; d < kMaxGauss; ++d) tot[3 + d] = KIND == 0 ? block_sum(s.ls[d], sm4) : 0.f;
    tot[7] = 0.f;
}

// The fold of n_wg workgroups' partials (part[q * stride_q + w * stride_w]), workgroup w's taken by thread w, into tot[].
template <int KIND>
__device__ __forceinline__ void ppo_fold_sums(const float* part, long stride_q, long stride_w, int n_wg, float* sm4, float* tot) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < kPpoSums - 1; ++q) {
        const bool live = (KIND == 0 ? q != 2 : q < 3) && tid < n_wg;
        tot[q] = block_sum(live ? join_load(part + q * stride_q + tid * stride_w) : 0.f, sm4);
    }
}

// One thread: the folded sums -> out[4] = {value_loss, action_loss, dist_entropy, total} and g_logstd.
template <int KIND>
__device__ __forceinline__ void ppo_finish(const float* tot, const float* __restrict__ logstd, int n, float invM, float vcoef,
                                           float ecoef, float* __restrict__ out, float* __restrict__ g_logstd) {
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

// What both entries refuse of the loss's arguments (`who` names the entry); VAR_OK or VAR_ERR_ARG with the message set.
inline int ppo_check_args(var_ctx* c, const char* who, int kind, int n, long M, float clip, const void* value, const void* action,
                          const void* old_logp, const void* adv, const void* returns, const void* value_preds, int clipped,
                          const void* logstd, const void* g_logstd, const void* out, const void* g_value) {
    if (kind != 0 && kind != 1) { VAR_SET_ERR(c, "%s: kind %d (0 DiagGaussian, 1 Categorical)", who, kind); return VAR_ERR_ARG; }
    if (M < 1) { VAR_SET_ERR(c, "%s: M %ld < 1", who, M); return VAR_ERR_ARG; }
    const int nmax = kind == 0 ? kMaxGauss : kMaxCat;
    if (n < 1 || n > nmax) { VAR_SET_ERR(c, "%s: n %d outside 1..%d", who, n, nmax); return VAR_ERR_ARG; }
    if (!value || !action || !old_logp || !adv || !returns || !out || !g_value || (clipped && !value_preds) ||
        (kind == 0 && (!logstd || !g_logstd))) {
        VAR_SET_ERR(c, "%s: a NULL pointer (only value_preds without the clipped value loss, and logstd / g_logstd "
                       "of a Categorical head, may be NULL)", who);
        return VAR_ERR_ARG;
    }
    if (!(clip >= 0.f)) { VAR_SET_ERR(c, "%s: clip %g < 0", who, (double)clip); return VAR_ERR_ARG; }
    return VAR_OK;
}

}  // namespace var_ppo
