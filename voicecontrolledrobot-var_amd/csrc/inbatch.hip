// In-batch-negatives contrastive head (BASELINE.json north_star / configs[2]; an EXTENSION -- the reference trains
// with the explicit-negative triplet loss only): every anchor image embedding a_i is scored
// against ALL candidate sound embeddings c_j of the global batch (the positives and the explicit negatives of every
// sample, all-gathered over the ranks) with a softmax over negative pairwise distances
//     d_ij = || a_i - c_j + 1e-6 ||_2   (torch's pairwise_distance convention, as in TripletMarginLoss)
//     L = inv_count * sum_i [ logsumexp_j(-d_ij / tau) + d_{i,t(i)} / tau ],   t(i) = column of sample i's positive.
// One wavefront per anchor row: lanes stride over the candidates, online max/sum per lane, wave-shuffle combine
// (no LDS, no atomics); a second kernel, one wavefront per candidate, forms the candidate gradients from the saved
// row log-sum-exps (so each rank's partial candidate gradient is bitwise reproducible; under data parallelism the
// partials are summed with one small all-reduce and each rank keeps the slice of its own clips).
#include <math.h>

#include "var_common.h"

namespace {
constexpr float kPdEps = 1e-6f;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float dist3(const float* a, const float* c, float& ux, float& uy, float& uz) {
    ux = a[0] - c[0] + kPdEps; uy = a[1] - c[1] + kPdEps; uz = a[2] - c[2] + kPdEps;
    return sqrtf(ux * ux + uy * uy + uz * uz);
}

// Class-aware forms (var_inbatch_loss_fwd_bwd_ex; they extend the head above, which ignores labels: with taskNum + 1
// classes a fifth of an anchor's "negatives" carry the anchor's own class).  y_i = anchor_cls[i], z_j = cand_cls[j]:
//   VAR_INBATCH_OTHER_CLASS     the softmax runs over N_i = { j : z_j != y_i } + { t(i) }; the other candidates of the anchor's
//                               class are skipped by both kernels (no term in the sum, no gradient);
//   VAR_INBATCH_MULTI_POSITIVE  L_i = logsumexp_j l_ij - (1/|P_i|) sum_{p in P_i} l_ip,  P_i = { j : z_j = y_i } + { t(i) }.
// The mode is a template parameter: mode 0 is the code this file always had, and a mode whose masks select nothing runs the
// same operations in the same order (bit-equal results).  A masked candidate is SKIPPED, never given l = -inf: a lane whose
// running max is still -inf would otherwise evaluate exp(-inf - (-inf)).
enum { kAll = VAR_INBATCH_ALL, kOtherClass = VAR_INBATCH_OTHER_CLASS, kMultiPositive = VAR_INBATCH_MULTI_POSITIVE };

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float row_loss(float L, float dpos, float inv_tau, float inv_count) {
    return (L + dpos * inv_tau) * inv_count;
}

// rows: lse_i (mode 1: over N_i), row loss, gradient wrt the anchor; mode 2 also leaves 1 / |P_i|
template <int MODE>
__global__ void __launch_bounds__(256) inbatch_rows_kernel(const float* __restrict__ a, const float* __restrict__ cand,
                                                          const int* __restrict__ target, const int* __restrict__ acls,
                                                          const int* __restrict__ ccls, int B, int M, float inv_tau,
                                                          float inv_count, float* __restrict__ lse, float* __restrict__ rowloss,
                                                          float* __restrict__ invp, float* __restrict__ ga) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= B) return;
    const float* ai = a + 3 * i;
    const int t = target[i];
    const int y = MODE == kAll ? 0 : acls[i];
    float mx = -INFINITY, sm = 0.f, dpos = 0.f;
    int npos = 0;
    for (int j = lane; j < M; j += 64) {
        if (MODE == kOtherClass && ccls[j] == y && j != t) continue;
        float ux, uy, uz;
        const float d = dist3(ai, cand + 3 * j, ux, uy, uz);
        const float l = -d * inv_tau;
        const float nm = fmaxf(mx, l);
        sm = sm * expf(mx - nm) + expf(l - nm);
        mx = nm;
        if (MODE == kMultiPositive && (ccls[j] == y || j == t)) { dpos += d; ++npos; }
    }
    const float gmx = wave_max(mx);
    const float gs = wave_sum(sm * expf(mx - gmx));          // lanes without a candidate hold sm = 0, mx = -inf -> 0
    const float L = gmx + logf(gs);
    float ip = 1.f;
    if (MODE == kMultiPositive) {
        ip = 1.f / (float)wave_sum_int(npos);                 // t(i) is in P_i: at least 1
        dpos = wave_sum(dpos) * ip;
    }
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int j = lane; j < M; j += 64) {
        if (MODE == kOtherClass && ccls[j] == y && j != t) continue;
        float ux, uy, uz;
        const float d = dist3(ai, cand + 3 * j, ux, uy, uz);
        float pos = j == t ? 1.f : 0.f;
        if (MODE == kMultiPositive) pos = (ccls[j] == y || j == t) ? ip : 0.f;
        const float s = expf(-d * inv_tau - L) - pos;
        const float w = -s * inv_tau * inv_count / fmaxf(d, 1e-12f);      // dL/dd_ij / d_ij
        gx += w * ux; gy += w * uy; gz += w * uz;
    }
    gx = wave_sum(gx); gy = wave_sum(gy); gz = wave_sum(gz);
    if (lane == 0) {
        if (MODE != kMultiPositive) {
            float ux, uy, uz;
            dpos = dist3(ai, cand + 3 * t, ux, uy, uz);
        }
        lse[i] = L;
        rowloss[i] = row_loss(L, dpos, inv_tau, inv_count);
        if (MODE == kMultiPositive) invp[i] = ip;
        ga[3 * i] = gx; ga[3 * i + 1] = gy; ga[3 * i + 2] = gz;
    }
}

// columns: gradient wrt candidate j from the B local rows (partial under data parallelism)
// (the block after the last column block adds the row losses up in a fixed order: the sum only needs the rows kernel, and a
//  launch of its own cost 6 us on the step's critical path)
__device__ __forceinline__ void inbatch_loss_sum(const float* __restrict__ rowloss, int B, float* __restrict__ out) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) acc += rowloss[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

template <int MODE>
__global__ void __launch_bounds__(256) inbatch_cols_kernel(const float* __restrict__ a, const float* __restrict__ cand,
                                                          const int* __restrict__ target, const int* __restrict__ acls,
                                                          const int* __restrict__ ccls, const float* __restrict__ lse,
                                                          const float* __restrict__ invp, int B, int M, float inv_tau,
                                                          float inv_count, float* __restrict__ gc,
                                                          const float* __restrict__ rowloss, float* __restrict__ loss_out) {
    if ((int)blockIdx.x == (M + 3) / 4) { inbatch_loss_sum(rowloss, B, loss_out); return; }
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= M) return;
    const float* cj = cand + 3 * j;
    const int z = MODE == kAll ? 0 : ccls[j];
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int i = lane; i < B; i += 64) {
        const bool hit = target[i] == j;
        if (MODE == kOtherClass && acls[i] == z && !hit) continue;
        float ux, uy, uz;
        const float d = dist3(a + 3 * i, cj, ux, uy, uz);
        float pos = hit ? 1.f : 0.f;
        if (MODE == kMultiPositive) pos = (acls[i] == z || hit) ? invp[i] : 0.f;
        const float s = expf(-d * inv_tau - lse[i]) - pos;
        const float w = -s * inv_tau * inv_count / fmaxf(d, 1e-12f);
        gx -= w * ux; gy -= w * uy; gz -= w * uz;
    }
    gx = wave_sum(gx); gy = wave_sum(gy); gz = wave_sum(gz);
    if (lane == 0) { gc[3 * j] = gx; gc[3 * j + 1] = gy; gc[3 * j + 2] = gz; }
}

template <int MODE>
int inbatch_launch(var_ctx* c, hipStream_t s, const float* anchor, const float* cand, const int* target, const int* acls,
                   const int* ccls, int B, int M, float tau, float inv_count, float* scratch, float* loss_out, float* g_anchor,
                   float* g_cand) {
    float* lse = scratch;            // B
    float* rowloss = scratch + B;    // B
    float* invp = MODE == kMultiPositive ? scratch + 2 * B : nullptr;      // B, mode 2 only
    hipLaunchKernelGGL(inbatch_rows_kernel<MODE>, dim3((B + 3) / 4), dim3(256), 0, s, anchor, cand, target, acls, ccls, B, M,
                       1.f / tau, inv_count, lse, rowloss, invp, g_anchor);
    VAR_HIP_CHECK(c, hipGetLastError());
    hipLaunchKernelGGL(inbatch_cols_kernel<MODE>, dim3((M + 3) / 4 + 1), dim3(256), 0, s, anchor, cand, target, acls, ccls, lse,
                       (const float*)invp, B, M, 1.f / tau, inv_count, g_cand, rowloss, loss_out);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}

}  // namespace

extern "C" int var_inbatch_loss_fwd_bwd(var_ctx* c, void* stream, const float* anchor, const float* cand, const int* target,
                                        int B, int M, float tau, float inv_count, float* scratch, float* loss_out,
                                        float* g_anchor, float* g_cand) {
    if (!c) return VAR_ERR_ARG;
    if (!anchor || !cand || !target || !scratch || !loss_out || !g_anchor || !g_cand || B < 1 || M < 1 || !(tau > 0.f)) {
        VAR_SET_ERR(c, "var_inbatch_loss_fwd_bwd: bad argument");
        return VAR_ERR_ARG;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    return inbatch_launch<kAll>(c, (hipStream_t)stream, anchor, cand, target, nullptr, nullptr, B, M, tau, inv_count, scratch,
                                loss_out, g_anchor, g_cand);
}

extern "C" int var_inbatch_loss_fwd_bwd_ex(var_ctx* c, void* stream, const float* anchor, const float* cand, const int* target,
                                           const int* anchor_cls, const int* cand_cls, int B, int M, float tau, float inv_count,
                                           int mode, float* scratch, float* loss_out, float* g_anchor, float* g_cand) {
    if (!c) return VAR_ERR_ARG;
    if (!anchor || !cand || !target || !scratch || !loss_out || !g_anchor || !g_cand || B < 1 || M < 1 || !(tau > 0.f)) {
        VAR_SET_ERR(c, "var_inbatch_loss_fwd_bwd_ex: bad argument");
        return VAR_ERR_ARG;
    }
    if (mode < kAll || mode > kMultiPositive) {
        VAR_SET_ERR(c, "var_inbatch_loss_fwd_bwd_ex: mode is VAR_INBATCH_ALL, _OTHER_CLASS or _MULTI_POSITIVE");
        return VAR_ERR_ARG;
    }
    if (mode != kAll && (!anchor_cls || !cand_cls)) {
        VAR_SET_ERR(c, "var_inbatch_loss_fwd_bwd_ex: the class-aware modes need anchor_cls and cand_cls");
        return VAR_ERR_ARG;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (mode == kOtherClass)
        return inbatch_launch<kOtherClass>(c, s, anchor, cand, target, anchor_cls, cand_cls, B, M, tau, inv_count, scratch,
                                           loss_out, g_anchor, g_cand);
    if (mode == kMultiPositive)
        return inbatch_launch<kMultiPositive>(c, s, anchor, cand, target, anchor_cls, cand_cls, B, M, tau, inv_count, scratch,
                                              loss_out, g_anchor, g_cand);
    return inbatch_launch<kAll>(c, s, anchor, cand, target, nullptr, nullptr, B, M, tau, inv_count, scratch, loss_out, g_anchor,
                                g_cand);
}
