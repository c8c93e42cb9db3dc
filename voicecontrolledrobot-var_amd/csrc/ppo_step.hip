// What a captured PPO minibatch step needs beside the networks (include/var_hip.h):
//   var_ppo_head_linear      the distribution head's Linear (dist.fc_mean / dist.linear, 128 -> n) fused with var_ppo_head's loss:
//                            head, the losses and every gradient from the actor features, two launches (rows, then the fold)
//   var_rollout_move_cursor  var_rollout_move whose index list starts at a device word: one launch serves every minibatch
// fp32, no product is contracted into an fma (-ffp-contract=off), no floating-point atomics, nothing waits for another workgroup.
#include "var_common.h"
#include "rollout_move.h"
#include "ppo_row.h"

namespace {

constexpr int kThreads = var_ppo::kThreads;
constexpr int kF = 128, kF4 = kF / 4;        // actor features per row, as floats and as 16-byte pieces
constexpr int kRowsWG = kThreads;            // rows a workgroup takes per round: one per thread in the loss, as var_ppo_head
constexpr int kMaxWG = kPpoMaxWG;            // rows are grid-strided over at most this many workgroups
constexpr int kSub = 32, kLanes = 8;         // the Linear: 32 rows at a time, a row's 32 pieces over 8 lanes
constexpr int kTail = 32;                    // a workgroup's partials: [g_W n * 128][g_b 16][the loss sums 8][8 unused]

__host__ __device__ inline long part_stride(int n) { return (long)n * kF + kTail; }
inline long workgroups_of(long M) { const long wg = (M + kRowsWG - 1) / kRowsWG; return wg > kMaxWG ? kMaxWG : wg; }

// ---- var_ppo_head_linear: the rows -----------------------------------------------------------------------------------------
// Per round of 256 rows: (1) the Linear, a row's dot products split over 8 lanes (each four 16-byte pieces of the row, read
// straight from memory; W from LDS), the 8 partial sums joined by a butterfly; (2) the loss, one thread per row on the head in
// LDS (ppo_row.h: var_ppo_head's own code, the same row -> thread -> workgroup layout, hence the same sums); (3) g_features with
// the mapping of (1), and the round's share of g_W / g_b: thread (rs, j4) keeps piece j4 of g_W's n rows for the rows rs, rs + 8,
// ... in registers over all rounds.  At the end the eight row slices are added through LDS in index order and the workgroup
// leaves its partials in the caller's workspace; head_linear_fold_kernel adds the workgroups up.
template <int KIND>
__global__ void __launch_bounds__(kThreads) head_linear_kernel(const float* __restrict__ features, const float* __restrict__ W,
                                                              const float* __restrict__ b, const float* __restrict__ logstd,
                                                              const float* __restrict__ value, const void* __restrict__ action,
                                                              const float* __restrict__ old_logp, const float* __restrict__ adv,
                                                              const float* __restrict__ returns, const float* __restrict__ value_preds,
                                                              int n, long M, float clip, float vcoef, float ecoef, int clipped,
                                                              float* __restrict__ head, float* __restrict__ g_features,
                                                              float* __restrict__ g_value, float* __restrict__ part) {
    constexpr int NMAX = KIND == 0 ? var_ppo::kMaxGauss : var_ppo::kMaxCat;
    constexpr int HS = NMAX + 1;             // odd row stride: the loss's row-per-thread reads fall on distinct banks
    __shared__ float4 W_s[NMAX * kF4];
    __shared__ float4 gw_s[NMAX * kF4];
    __shared__ float b_s[NMAX], gb_s[NMAX];
    __shared__ float head_s[kRowsWG * HS], gh_s[kRowsWG * HS];
    __shared__ float sm4[4];
    const int tid = threadIdx.x;
    const float4* __restrict__ feat4 = (const float4*)features;
    for (int i = tid; i < n * kF; i += kThreads) ((float*)W_s)[i] = W[i];    // (word loads: W lies in a parameter arena, at any word)
    if (tid < n) b_s[tid] = b[tid];
    __syncthreads();

    const float invM = 1.f / (float)M;
    const int p = tid & (kLanes - 1), rl = tid / kLanes;         // the Linear: lane of the row, row of the 32
    const int j4 = tid & (kF4 - 1), rs = tid / kF4;              // g_W: piece of the row, row slice
    var_ppo::RowSums sums;
    float4 acc[NMAX];
    float gb[NMAX];
#pragma unroll
    for (int k = 0; k < NMAX; ++k) { acc[k] = make_float4(0.f, 0.f, 0.f, 0.f); gb[k] = 0.f; }

    for (long base = (long)blockIdx.x * kRowsWG; base < M; base += (long)gridDim.x * kRowsWG) {
        const long left = M - base;
        const int rows = left < kRowsWG ? (int)left : kRowsWG;
        // (1) head = features . W^T + b
        for (int s = 0; s < kRowsWG / kSub && s * kSub < rows; ++s) {
            const int r = s * kSub + rl;
            const long row = base + (r < rows ? r : rows - 1);   // (lanes past the end redo the last row: the butterfly stays whole)
            float4 x[kF4 / kLanes];
#pragma unroll
            for (int i = 0; i < kF4 / kLanes; ++i) x[i] = feat4[row * kF4 + p + kLanes * i];
#pragma unroll
            for (int k = 0; k < NMAX; ++k) {
                if (k < n) {
                    float a = 0.f;
#pragma unroll
                    for (int i = 0; i < kF4 / kLanes; ++i) {
                        const float4 w = W_s[k * kF4 + p + kLanes * i];
                        a += x[i].x * w.x; a += x[i].y * w.y; a += x[i].z * w.z; a += x[i].w * w.w;
                    }
                    a += __shfl_xor(a, 1); a += __shfl_xor(a, 2); a += __shfl_xor(a, 4);
                    if (p == (k & (kLanes - 1)) && r < rows) head_s[r * HS + k] = a + b_s[k];
                }
            }
        }
        __syncthreads();
        // (2) the loss of row base + tid; the head leaves as whole rows
        for (int i = tid; i < rows * n; i += kThreads) head[base * n + i] = head_s[(i / n) * HS + i % n];
        if (tid < rows) {
            var_ppo::ppo_row<KIND>(head_s + tid * HS, gh_s + tid * HS, base + tid, logstd, value, action, old_logp, adv, returns,
                                   value_preds, n, invM, clip, vcoef, ecoef, clipped, g_value, nullptr, sums);
        }
        __syncthreads();
        // (3) g_features = g_head . W
        for (int s = 0; s < kRowsWG / kSub && s * kSub < rows; ++s) {
            const int r = s * kSub + rl;
            if (r < rows) {
#pragma unroll
                for (int i = 0; i < kF4 / kLanes; ++i) {
                    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int k = 0; k < NMAX; ++k) {
                        if (k < n) {
                            const float gh = gh_s[r * HS + k];
                            const float4 w = W_s[k * kF4 + p + kLanes * i];
                            g.x += gh * w.x; g.y += gh * w.y; g.z += gh * w.z; g.w += gh * w.w;
                        }
                    }
                    ((float4*)g_features)[(base + r) * kF4 + p + kLanes * i] = g;
                }
            }
        }
        // g_W += g_head^T . features, g_b += sum of g_head, the rows rs, rs + 8, ... of this round
        for (int r = rs; r < rows; r += kThreads / kF4) {
            const float4 x = feat4[(base + r) * kF4 + j4];
#pragma unroll
            for (int k = 0; k < NMAX; ++k) {
                if (k < n) {
                    const float gh = gh_s[r * HS + k];
                    acc[k].x += gh * x.x; acc[k].y += gh * x.y; acc[k].z += gh * x.z; acc[k].w += gh * x.w;
                    gb[k] += gh;
                }
            }
        }
        __syncthreads();                                         // (head_s / gh_s are free for the next round)
    }

    float tot[kPpoSums];
    var_ppo::ppo_block_sums<KIND>(sums, sm4, tot);
    float* mine = part + (long)blockIdx.x * part_stride(n);
    if (tid < kPpoSums - 1) {
        float t = tot[0];
#pragma unroll
        for (int q = 1; q < kPpoSums - 1; ++q) t = tid == q ? tot[q] : t;
        mine[n * kF + 16 + tid] = t;
    }
    for (int slice = 0; slice < kThreads / kF4; ++slice) {       // the eight row slices, added in index order
        if (rs == slice) {
#pragma unroll
            for (int k = 0; k < NMAX; ++k) {
                if (k < n) {
                    float4 g = acc[k];
                    float s = gb[k];
                    if (slice > 0) {
                        const float4 o = gw_s[k * kF4 + j4];
                        g.x = o.x + g.x; g.y = o.y + g.y; g.z = o.z + g.z; g.w = o.w + g.w;
                        s = gb_s[k] + s;
                    }
                    gw_s[k * kF4 + j4] = g;
                    if (j4 == 0) gb_s[k] = s;
                }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < n * kF4; i += kThreads) ((float4*)mine)[i] = gw_s[i];
    if (tid < n) mine[n * kF + tid] = gb_s[tid];
}

// ---- var_ppo_head_linear: the fold -----------------------------------------------------------------------------------------
// g_W and g_b: one thread per element adds the workgroups' partials in index order.  Workgroup 0 also folds the loss sums as
// var_ppo_head's last workgroup does, writes out[4] / g_logstd and, given a cursor, the statistics row and both cursor words.
template <int KIND>
__global__ void __launch_bounds__(kThreads) head_linear_fold_kernel(const float* __restrict__ part, int n_wg, int n, long M,
                                                                   const float* __restrict__ logstd, float vcoef, float ecoef,
                                                                   float* __restrict__ out, float* __restrict__ g_W,
                                                                   float* __restrict__ g_b, float* __restrict__ g_logstd,
                                                                   float* __restrict__ stats, int n_stats_rows, int* __restrict__ cursor,
                                                                   int n_env) {
    __shared__ float sm4[4];
    const int tid = threadIdx.x;
    const long S = part_stride(n);
    const int e = blockIdx.x * kThreads + tid;
    if (e < n * kF) {
        float a = part[e];
        for (int w = 1; w < n_wg; ++w) a += part[w * S + e];
        g_W[e] = a;
    }
    if (blockIdx.x != 0) return;
    if (tid < n) {
        float a = part[n * kF + tid];
        for (int w = 1; w < n_wg; ++w) a += part[w * S + n * kF + tid];
        g_b[tid] = a;
    }
    const float* sums = part + n * kF + 16;
    float tot[kPpoSums];
    if (n_wg > 1) {
        var_ppo::ppo_fold_sums<KIND>(sums, 1, S, n_wg, sm4, tot);
    } else {
#pragma unroll
        for (int q = 0; q < kPpoSums - 1; ++q) tot[q] = sums[q];
    }
    if (tid != 0) return;
    float res[4];
    var_ppo::ppo_finish<KIND>(tot, logstd, n, 1.f / (float)M, vcoef, ecoef, res, g_logstd);
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = res[q];
    if (cursor) {
        const int row = cursor[1];
        if (row >= 0 && row < n_stats_rows) { stats[3 * row] = res[0]; stats[3 * row + 1] = res[1]; stats[3 * row + 2] = res[2]; }
        cursor[0] += n_env;
        cursor[1] = row + 1;
    }
}

// ---- var_rollout_move_cursor -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(var_move::kThreads) rollout_move_cursor_kernel(var_move::MoveTable tab, const int* __restrict__ ind_base,
                                                                                int n_ind, const int* __restrict__ cursor, int n_env,
                                                                                int n_src_env) {
    const long first = cursor[0];
    if (first < 0 || first + n_env > n_ind) return;             // a list that would leave ind_base[0 .. n_ind): nothing is written
    const unsigned blk = blockIdx.x;
    var_move::move_piece(tab.s[var_move::move_segment_of(tab, blk)], blk, ind_base + first, n_env, n_src_env, 0);
}

inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" long var_ppo_head_linear_workspace_bytes(int kind, int n, long M) {
    if ((kind != 0 && kind != 1) || M < 1 || n < 1 || n > (kind == 0 ? var_ppo::kMaxGauss : var_ppo::kMaxCat)) return VAR_ERR_ARG;
    return workgroups_of(M) * part_stride(n) * (long)sizeof(float);
}

extern "C" int var_ppo_head_linear(var_ctx* c, void* stream, int kind, const float* features, const float* W, const float* b,
                                   const float* logstd, const float* value, const void* action, const float* old_logp,
                                   const float* adv, const float* returns, const float* value_preds, int n, long M, float clip,
                                   float value_coef, float entropy_coef, int use_clipped_value_loss, float* head, float* out,
                                   float* g_features, float* g_W, float* g_b, float* g_value, float* g_logstd, void* workspace,
                                   long workspace_bytes, float* stats, int n_stats_rows, int* cursor, int n_env) {
    if (!c) return VAR_ERR_ARG;
    const char* who = "var_ppo_head_linear";
    const int rc = var_ppo::ppo_check_args(c, who, kind, n, M, clip, value, action, old_logp, adv, returns, value_preds,
                                           use_clipped_value_loss, logstd, g_logstd, out, g_value);
    if (rc != VAR_OK) return rc;
    if (!features || !W || !b || !head || !g_features || !g_W || !g_b || !workspace) {
        VAR_SET_ERR(c, "%s: features, W, b, head, g_features, g_W, g_b and the workspace must not be NULL", who);
        return VAR_ERR_ARG;
    }
    const long need = var_ppo_head_linear_workspace_bytes(kind, n, M);
    if (workspace_bytes < need) {
        VAR_SET_ERR(c, "%s: workspace of %ld bytes, %ld needed (var_ppo_head_linear_workspace_bytes)", who, workspace_bytes, need);
        return VAR_ERR_ARG;
    }
    if (misaligned(workspace) || misaligned(features) || misaligned(g_features)) {
        VAR_SET_ERR(c, "%s: features, g_features and the workspace must be 16-byte aligned", who);
        return VAR_ERR_ARG;
    }
    if ((stats == nullptr) != (cursor == nullptr) || (cursor && (n_stats_rows < 1 || n_env < 0))) {
        VAR_SET_ERR(c, "%s: stats and cursor go together, with n_stats_rows >= 1 and n_env >= 0 (%d, %d)", who, n_stats_rows, n_env);
        return VAR_ERR_ARG;
    }
    const size_t f4 = sizeof(float), m = (size_t)M;
    const void* outs[] = {head, out, g_features, g_W, g_b, g_value, kind == 0 ? g_logstd : nullptr, workspace, stats, cursor};
    const size_t outn[] = {f4 * m * n, 4 * f4, f4 * m * kF, f4 * n * kF, f4 * n, f4 * m, f4 * n, (size_t)need,
                           3 * f4 * (size_t)(cursor ? n_stats_rows : 0), 2 * sizeof(int)};
    const void* ins[] = {features, W, b, kind == 0 ? logstd : nullptr, value, action, old_logp, adv, returns,
                         use_clipped_value_loss ? value_preds : nullptr};
    const size_t inn[] = {f4 * m * kF, f4 * n * kF, f4 * n, f4 * n, f4 * m, kind == 0 ? f4 * m * n : sizeof(long long) * m, f4 * m, f4 * m,
                          f4 * m, f4 * m};
    constexpr int n_out = sizeof(outs) / sizeof(outs[0]), n_in = sizeof(ins) / sizeof(ins[0]);
    for (int i = 0; i < n_out; ++i) {
        if (!outs[i]) continue;
        for (int j = 0; j < n_in; ++j) {
            if (ins[j] && var_move::overlap(outs[i], outn[i], ins[j], inn[j])) {
                VAR_SET_ERR(c, "%s: output %d overlaps input %d", who, i, j);
                return VAR_ERR_ARG;
            }
        }
        for (int j = i + 1; j < n_out; ++j) {
            if (outs[j] && var_move::overlap(outs[i], outn[i], outs[j], outn[j])) {
                VAR_SET_ERR(c, "%s: outputs %d and %d overlap", who, i, j);
                return VAR_ERR_ARG;
            }
        }
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    const int wg = (int)workgroups_of(M);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    auto rows = kind == 0 ? head_linear_kernel<0> : head_linear_kernel<1>;
    hipLaunchKernelGGL(rows, dim3((unsigned)wg), dim3(kThreads), 0, s, features, W, b, logstd, value, action, old_logp, adv, returns,
                       value_preds, n, M, clip, value_coef, entropy_coef, use_clipped_value_loss, head, g_features, g_value, part);
    VAR_HIP_CHECK(c, hipGetLastError());
    auto fold = kind == 0 ? head_linear_fold_kernel<0> : head_linear_fold_kernel<1>;
    hipLaunchKernelGGL(fold, dim3((unsigned)((n * kF + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (const float*)part, wg, n, M,
                       logstd, value_coef, entropy_coef, out, g_W, g_b, g_logstd, stats, n_stats_rows, cursor, n_env);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}

extern "C" int var_rollout_move_cursor(var_ctx* c, void* stream, const var_move_seg* segs, int n_seg, const int* ind_base, int n_ind,
                                       const int* cursor, int n_env, int n_src_env) {
    if (!c) return VAR_ERR_ARG;
    const char* who = "var_rollout_move_cursor";
    if (!ind_base || !cursor || n_ind < 1) {
        VAR_SET_ERR(c, "%s: ind_base or cursor NULL, or n_ind %d < 1", who, n_ind);
        return VAR_ERR_ARG;
    }
    var_move::MoveTable tab{};
    size_t dext[VAR_MOVE_MAX_SEGS];
    unsigned long long blocks = 0;
    const int rc = var_move::move_plan_gather(c, who, segs, n_seg, true, n_env, n_src_env, tab, blocks, dext);
    if (rc != VAR_OK) return rc;
    if (n_env > n_ind) { VAR_SET_ERR(c, "%s: n_env %d > n_ind %d: no cursor value fits", who, n_env, n_ind); return VAR_ERR_ARG; }
    for (int i = 0; i < n_seg; ++i) {
        if (var_move::overlap(segs[i].dst, dext[i], cursor, sizeof(int)) ||
            var_move::overlap(segs[i].dst, dext[i], ind_base, sizeof(int) * (size_t)n_ind)) {
            VAR_SET_ERR(c, "%s: the destination range of segment %d holds the cursor or the index list", who, i);
            return VAR_ERR_ARG;
        }
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(rollout_move_cursor_kernel, dim3((unsigned)blocks), dim3(var_move::kThreads), 0, (hipStream_t)stream, tab,
                       ind_base, n_ind, cursor, n_env, n_src_env);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}
