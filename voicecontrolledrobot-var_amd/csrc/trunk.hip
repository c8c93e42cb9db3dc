// The PPO update's MLP trunk, forward and backward: everything between imgCNN's flattened output and the distribution head of
// armNet_VAR (kind 0, models/RL/arm_RL_model.py:102-134) and ai2thorNet_VAR (kind 1, models/RL/ai2thor_RL_model.py:85-115), the
// 20 | 21 Linear + ReLU layers of actor_critic.py's _build_trunk (plus occupancyCNNMLP's two), three residual sums and the masked
// GRU of gru_seq.hip in the middle (include/var_hip.h has the definition).
//   var_trunk_fwd   11 stage launches + the GRU's 1 + T.  Layers of one dependency depth share a launch: a job table passed by
//                   value in the kernel arguments (rollout.hip's pattern) maps a workgroup to (layer, tile).
//   var_trunk_bwd   11 stage launches + var_gru_seq_bwd's.  One launch does, for every layer of its stage, dX = G W,
//                   dW = G^T X_in and db = the column sums of G, where G = (sum of the incoming dY arrays) * [Y > 0] is formed
//                   on load from the saved activation and never stored.
// An operand may be the sum of up to three arrays, added on load as (a0 + a1) + a2: the residual sums cost no launch and no
// buffer, and the dX of a summed input is simply read by each of its producers as one of their incoming arrays.
// Every product is v_mfma_f32_16x16x4_f32: a workgroup owns one 16 R x 16 R output tile (R = 2 where that still gives 256
// workgroups, else 1: a function of the shape alone), its four waves take the reduction's chunks of 16 in turn (chunk u goes
// to wave u & 3) and their tiles are folded through LDS as (w0 + w1) + (w2 + w3).  An accumulator sees its k in the same order
// whatever R.  Kernel boundaries order the stages: no grid barrier, no spin-wait, no atomics; equal inputs give equal bits.
#include "gg.h"

namespace {

constexpr int kMaxJobs = 14;
constexpr int kMaxLayers = 21;
constexpr int kMaxRows = 16384;        // T * N: every operand offset stays far below 2^31 elements
constexpr int kStages = 11;

// element (r, k) = (a[0][o] + a[1][o]) + a[2][o] with o = r * rs + k * ks, zero where gate[o] <= 0 (autograd's ReLU gradient)
struct Op {
    const float* a[3];
    const float* gate;
    int rs, ks;
    int vec;             // ks == 1 and every row 16-byte aligned: four k in one load
};
// kind 0: c[i * ldc + j] = act(bias[j] + sum_k p(i, k) q(j, k)), I x J outputs, tj tiles of 16 rt along j
// kind 1: c[j] = sum_{m < I} p(m, j) carried in float64, J columns (p.rs = the row stride, p.ks = 1)
struct Job {
    Op p, q;
    float* c;
    float* c2;           // a second copy of the result (same layout), or NULL
    const float* bias;
    int I, J, K, ldc, relu, kind, tj, rt;
};
struct Jobs {
    int n;
    int first[kMaxJobs + 1];     // first[j] = the first workgroup of job j
    Job j[kMaxJobs];
};

__device__ __forceinline__ float op_at(const Op& o, long off) {
    float v = o.a[0][off];
    if (o.a[1]) v += o.a[1][off];
    if (o.a[2]) v += o.a[2][off];
    if (o.gate) v = o.gate[off] > 0.f ? v : 0.f;
    return v;
}

// k0 .. k0 + 3 of row r (k0 a multiple of 4); k >= K reads as zero
__device__ __forceinline__ float4 op_ld4(const Op& o, int r, int k0, int K) {
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (o.vec) {
        if (k0 < K) {                                          // K is a multiple of 4 here: all four or none
            const long off = (long)r * o.rs + k0;
            v = *(const float4*)(o.a[0] + off);
            if (o.a[1]) { const float4 t = *(const float4*)(o.a[1] + off); v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
            if (o.a[2]) { const float4 t = *(const float4*)(o.a[2] + off); v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w; }
            if (o.gate) {
                const float4 g = *(const float4*)(o.gate + off);
                v.x = g.x > 0.f ? v.x : 0.f; v.y = g.y > 0.f ? v.y : 0.f; v.z = g.z > 0.f ? v.z : 0.f; v.w = g.w > 0.f ? v.w : 0.f;
            }
        }
    } else {
        float t[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool ok = k0 + e < K;
            const float x = op_at(o, (long)r * o.rs + (long)(ok ? k0 + e : 0) * o.ks);
            t[e] = ok ? x : 0.f;
        }
        v.x = t[0]; v.y = t[1]; v.z = t[2]; v.w = t[3];
    }
    return v;
}

// One 16 R x 16 R tile.  Lane (l15 = lane & 15, lk = lane >> 4) supplies row l15 of each operand at k = 16 u + 4 lk + e to the
// e-th of a chunk's four matrix instructions; D[row 4 lk + r][column l15] comes back in acc[r].
template <int R>
__device__ __forceinline__ void product_tile(const Job& jb, int tile, float* __restrict__ red) {
    const int tid = threadIdx.x, lane = tid & 63, kq = tid >> 6, l15 = lane & 15, lk = lane >> 4;
    const int ti = tile / jb.tj, tj = tile - ti * jb.tj;
    const int i0 = ti * 16 * R, j0 = tj * 16 * R;
    const int I = jb.I, J = jb.J, K = jb.K;
    int ri[R], rj[R];
#pragma unroll
    for (int a = 0; a < R; ++a) {
        ri[a] = min(i0 + 16 * a + l15, I - 1);                 // rows past the edge repeat the last one; their results are dropped
        rj[a] = min(j0 + 16 * a + l15, J - 1);
    }
    f32x4 acc[R][R];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nch = (K + 15) >> 4;
    for (int u = kq; u < nch; u += 4) {
        const int k0 = 16 * u + 4 * lk;
        float4 pa[R], qb[R];
#pragma unroll
        for (int a = 0; a < R; ++a) { pa[a] = op_ld4(jb.p, ri[a], k0, K); qb[a] = op_ld4(jb.q, rj[a], k0, K); }
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int b = 0; b < R; ++b) {
                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[a].x, qb[b].x, acc[a][b], 0, 0, 0);
                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[a].y, qb[b].y, acc[a][b], 0, 0, 0);
                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[a].z, qb[b].z, acc[a][b], 0, 0, 0);
                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[a].w, qb[b].w, acc[a][b], 0, 0, 0);
            }
    }
    constexpr int S = R * R * 4;                               // red[wave][S][64]
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(kq * S + (a * R + b) * 4 + r) * 64 + lane] = acc[a][b][r];
    __syncthreads();
#pragma unroll
    for (int s = kq; s < S; s += 4) {                          // slice s = (a R + b) 4 + r of the tile, one element per lane
        const int o = s * 64 + lane;
        float v = (red[o] + red[S * 64 + o]) + (red[2 * S * 64 + o] + red[3 * S * 64 + o]);
        const int ab = s >> 2, r = s & 3, a = ab / R, b = ab - a * R;
        const int i = i0 + 16 * a + 4 * lk + r, j = j0 + 16 * b + l15;
        if (i < I && j < J) {
            if (jb.bias) v += jb.bias[j];
            if (jb.relu) v = v > 0.f ? v : 0.f;
            jb.c[(long)i * jb.ldc + j] = v;
            if (jb.c2) jb.c2[(long)i * jb.ldc + j] = v;
        }
    }
}

// 16 columns per workgroup, 256 rows a pass (sixteen loads per thread in flight; rows past the end count as zero).  The sum is
// carried in float64 and rounded to fp32 once, at the end: thread (c, rl) adds rows base + rl + 16 i in order of i, thread c < 16
// adds the sixteen partial sums of its column in order of rl through LDS, and the passes are added in order.  A bias gradient is
// a sum that may cancel (critic_linear's is ONE number, the sum of d_value): an fp32 chain in row order missed the tests' bound,
// four times torch's fp32 distance from float64, from 481 rows up, and an fp32 tree still did at 1000 (DESIGN.md has the figures).
__device__ __forceinline__ void column_sums(const Job& jb, int tile, float* __restrict__ red_f) {
    double* red = (double*)red_f;                              // 256 doubles of the buffer
    const int tid = threadIdx.x, c = tid & 15, rl = tid >> 4;
    const int j0 = tile * 16, col = min(j0 + c, jb.J - 1), rows = jb.I;
    double v = 0.0;
    for (int base = 0; base < rows; base += 256) {
        float t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int m = base + rl + 16 * i;
            t[i] = m < rows ? op_at(jb.p, (long)m * jb.p.rs + col) : 0.f;
        }
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += (double)t[i];
        red[rl * 16 + c] = s;
        __syncthreads();
        if (tid < 16) {
#pragma unroll 1                                              // (unrolled, the sixteen doubles cost the kernel half its occupancy)
            for (int m = 0; m < 16; ++m) v += red[m * 16 + tid];
        }
        __syncthreads();
    }
    if (tid < 16 && j0 + tid < jb.J) jb.c[j0 + tid] = (float)v;
}

template <bool BWD>
__global__ void __launch_bounds__(256) trunk_stage_kernel(const Jobs jobs) {
    __shared__ __attribute__((aligned(16))) float red[4 * 16 * 64];
    int j = 0;
    while (j + 1 < jobs.n && (int)blockIdx.x >= jobs.first[j + 1]) ++j;
    const Job& jb = jobs.j[j];
    const int tile = (int)blockIdx.x - jobs.first[j];
    if (BWD && jb.kind == 1) column_sums(jb, tile, red);
    else if (jb.rt == 2) product_tile<2>(jb, tile, red);
    else product_tile<1>(jb, tile, red);
}

// ---- the two networks as tables ---------------------------------------------------------------------------------------------
enum { T_FEAT = -1, T_MOTOR = -2, T_SOUND = -3, T_OCC = -4, T_GRU = -5 };   // a layer's sources: these, or a layer's output

struct Layer {
    int in, out, nsrc, src[3], stage, relu;
};
struct Model {
    int kind, H, nl, motor_in, x_layer, rnn_layer, value_layer, actor_layer;
    Layer L[kMaxLayers];
};

// the layers in state_dict order (occupancyCNNMLP.5 / .7 first for kind 1, then motorMlp, cnnMlp, imgMotorMlp, imgMotorMlp2,
// soundMlp, fusionMlp, mlp_all, actor, critic, critic_linear); stage = the forward launch a layer runs in
inline Model make_model(int kind) {
    Model m{};
    m.kind = kind;
    m.H = kind ? 1024 : 512;
    m.motor_in = kind ? 3 : 5;
    auto add = [&](int in, int out, int stage, int s0, int s1 = 0, int s2 = 0, int nsrc = 1, int relu = 1) {
        Layer& l = m.L[m.nl];
        l.in = in; l.out = out; l.stage = stage; l.nsrc = nsrc; l.src[0] = s0; l.src[1] = s1; l.src[2] = s2; l.relu = relu;
        return m.nl++;
    };
    int occ = 0, motor;
    if (kind) {
        occ = add(288, 128, 1, T_OCC);
        occ = add(128, 256, 2, occ);
        motor = add(3, 64, 1, T_MOTOR);
        motor = add(64, 256, 2, motor);
    } else {
        motor = add(5, 256, 1, T_MOTOR);
        motor = add(256, 512, 2, motor);
        motor = add(512, 256, 3, motor);
    }
    int flat = add(1152, 512, 1, T_FEAT);
    flat = add(512, 256, 2, flat);
    const int hid = kind ? 64 : 256;
    int x = kind ? add(256, hid, 4, flat, motor, occ, 3) : add(256, hid, 4, flat, motor, 0, 2);
    x = add(hid, 128, 5, x);
    m.x_layer = x;
    const int rnn = add(m.H, 256, 6, T_GRU);
    m.rnn_layer = rnn;
    int sound = add(3, 128, 1, T_SOUND);
    sound = add(128, 256, 2, sound);
    sound = add(256, 256, 3, sound);
    int fusion = add(256, 512, 4, sound, flat, 0, 2);
    fusion = add(512, 256, 5, fusion);
    int y = add(256, 256, 7, fusion, rnn, 0, 2);
    y = add(256, 128, 8, y);
    int actor = add(128, 128, 9, y);
    m.actor_layer = add(128, 128, 10, actor);
    int critic = add(128, 128, 9, y);
    critic = add(128, 128, 10, critic);
    m.value_layer = add(128, 1, 11, critic, 0, 0, 1, 0);
    return m;
}

inline const Model& model_of(int kind) {
    static const Model m0 = make_model(0), m1 = make_model(1);
    return kind ? m1 : m0;
}

inline long align64(long floats) { return (floats + 63) & ~63L; }

inline long param_floats(const Model& m, int i) {
    const long H = m.H;
    if (i == 0) return 3 * H * 128;
    if (i == 1) return 3 * H * H;
    if (i < 4) return 3 * H;
    const Layer& l = m.L[(i - 4) >> 1];
    return (i & 1) ? l.out : (long)l.out * l.in;
}
inline long grad_offset(const Model& m, int i) {               // i == n_params: the buffer's length
    long o = 0;
    for (int k = 0; k < i; ++k) o += align64(param_floats(m, k));
    return o;
}

// saved: every layer's activation, then the GRU's output g (M, H), then var_gru_seq_fwd's own 5 M H
inline long saved_offset(const Model& m, long M, int i) {      // i == nl: g, nl + 1: the GRU's, nl + 2: the length
    long o = 0;
    for (int k = 0; k < i && k < m.nl; ++k) o += align64(M * m.L[k].out);
    if (i > m.nl) o += align64(M * m.H);
    if (i > m.nl + 1) o += align64(5 * M * m.H);
    return o;
}

// backward workspace, in floats after the GRU's: one dX per layer (M, in), the GRU's d_x (M, 128), zeros for an absent d_value /
// d_actor_features
struct BwdLayout {
    long dx[kMaxLayers], gru_dx, zeros, total;
};
inline BwdLayout bwd_layout(const Model& m, long M) {
    BwdLayout b{};
    long o = 0;
    for (int l = 0; l < m.nl; ++l) { b.dx[l] = o; o += align64(M * m.L[l].in); }
    b.gru_dx = o; o += align64(M * 128);
    b.zeros = o; o += align64(M * 128);
    b.total = o;
    return b;
}

inline long gru_ws_bytes(const Model& m, int T, int N) { return (var_gru_seq_workspace_bytes(T, N, 128, m.H) + 255) & ~255L; }

inline const char* shape_error(int kind, int T, int N) {
    if (kind != 0 && kind != 1) return "kind must be 0 (arm_VAR) or 1 (ai2thor_VAR)";
    if (N < 1 || N > 64) return "N outside 1..64";
    if (T < 1) return "T < 1";
    if ((long)T * N > kMaxRows) return "T * N above 16384 rows";
    return nullptr;
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *p = (const char*)a, *q = (const char*)b;
    return a && b && p < q + nb && q < p + na;
}
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline Op make_op(const float* a0, const float* a1, const float* a2, const float* gate, int rs, int ks, int K) {
    Op o{};
    o.a[0] = a0; o.a[1] = a1; o.a[2] = a2; o.gate = gate; o.rs = rs; o.ks = ks;
    o.vec = ks == 1 && !(rs & 3) && !(K & 3) && al16(a0) && al16(a1) && al16(a2) && al16(gate);
    return o;
}

inline void push(Jobs& js, int& blocks, const Job& j) {
    js.first[js.n] = blocks;
    js.j[js.n++] = j;
    blocks += j.kind == 1 ? (j.J + 15) / 16 : ((j.I + 16 * j.rt - 1) / (16 * j.rt)) * j.tj;
    js.first[js.n] = blocks;
}
inline Job product_job(const Op& p, const Op& q, float* c, const float* bias, int I, int J, int K, int ldc, int relu) {
    Job j{};
    j.p = p; j.q = q; j.c = c; j.bias = bias; j.I = I; j.J = J; j.K = K; j.ldc = ldc; j.relu = relu; j.kind = 0;
    j.rt = ((I + 31) / 32) * ((J + 31) / 32) >= 256 ? 2 : 1;    // the shape alone picks the tile
    j.tj = (J + 16 * j.rt - 1) / (16 * j.rt);
    return j;
}

struct Ptrs {
    const float* ext[5];                                       // by -(id) - 1: feat, motor_in, sound_in, occ, g
    const float* act[kMaxLayers];
};
inline const float* tensor(const Ptrs& p, int id) { return id < 0 ? p.ext[-id - 1] : p.act[id]; }

inline Op input_op(const Model& m, const Ptrs& p, const Layer& l, int rs, int ks, int K) {
    const float* a[3] = {nullptr, nullptr, nullptr};
    for (int s = 0; s < l.nsrc; ++s) a[s] = tensor(p, l.src[s]);
    return make_op(a[0], a[1], a[2], nullptr, rs, ks, K);
}

}  // namespace

extern "C" int var_trunk_n_layers(int kind) { return kind == 0 || kind == 1 ? model_of(kind).nl : VAR_ERR_ARG; }
extern "C" int var_trunk_n_params(int kind) { return kind == 0 || kind == 1 ? 4 + 2 * model_of(kind).nl : VAR_ERR_ARG; }
extern "C" long var_trunk_param_floats(int kind, int i) {
    if ((kind != 0 && kind != 1) || i < 0 || i >= var_trunk_n_params(kind)) return VAR_ERR_ARG;
    return param_floats(model_of(kind), i);
}
extern "C" long var_trunk_grad_offset(int kind, int i) {
    if ((kind != 0 && kind != 1) || i < 0 || i > var_trunk_n_params(kind)) return VAR_ERR_ARG;
    return grad_offset(model_of(kind), i);
}
extern "C" long var_trunk_saved_offset(int kind, int T, int N, int i) {
    if (shape_error(kind, T, N) || i < 0 || i > model_of(kind).nl + 2) return VAR_ERR_ARG;
    return saved_offset(model_of(kind), (long)T * N, i);
}
extern "C" long var_trunk_saved_floats(int kind, int T, int N) {
    if (shape_error(kind, T, N)) return VAR_ERR_ARG;
    const Model& m = model_of(kind);
    return saved_offset(m, (long)T * N, m.nl + 2);
}
extern "C" long var_trunk_workspace_bytes(int kind, int T, int N) {
    if (shape_error(kind, T, N)) return VAR_ERR_ARG;
    const Model& m = model_of(kind);
    const long M = (long)T * N, g = gru_ws_bytes(m, T, N);
    const long fwd = g + 4 * saved_offset(m, M, m.nl + 2), bwd = g + 4 * bwd_layout(m, M).total;
    return fwd > bwd ? fwd : bwd;
}

extern "C" int var_trunk_fwd(var_ctx* c, void* stream, int kind, const float* const* params, const float* feat, const float* occ,
                             const float* motor_in, const float* sound_in, const float* hxs, const float* masks, int T, int N,
                             float* value, float* actor_features, float* h_T, float* saved, void* workspace, long workspace_bytes) {
    if (!c) return VAR_ERR_ARG;
    if (const char* why = shape_error(kind, T, N)) {
        VAR_SET_ERR(c, "var_trunk_fwd: %s (kind %d, T %d, N %d)", why, kind, T, N);
        return VAR_ERR_ARG;
    }
    const Model& m = model_of(kind);
    const int np = 4 + 2 * m.nl;
    if (!params || !feat || !motor_in || !sound_in || !hxs || !masks || !value || !actor_features || !h_T || !workspace) {
        VAR_SET_ERR(c, "var_trunk_fwd: a NULL pointer (only `saved`, and `occ` for kind 0, may be NULL)");
        return VAR_ERR_ARG;
    }
    if (kind == 1 && !occ) {
        VAR_SET_ERR(c, "var_trunk_fwd: kind 1 (ai2thor_VAR) needs occ (M, 288)");
        return VAR_ERR_ARG;
    }
    for (int i = 0; i < np; ++i)
        if (!params[i]) {
            VAR_SET_ERR(c, "var_trunk_fwd: params[%d] is NULL (%d device pointers in var_trunk_param_floats' order)", i, np);
            return VAR_ERR_ARG;
        }
    const long M = (long)T * N, need = var_trunk_workspace_bytes(kind, T, N);
    if (workspace_bytes < need) {
        VAR_SET_ERR(c, "var_trunk_fwd: workspace of %ld bytes, %ld needed (var_trunk_workspace_bytes)", workspace_bytes, need);
        return VAR_ERR_ARG;
    }
    if (!al16(workspace) || !al16(saved) || !al16(hxs)) {
        VAR_SET_ERR(c, "var_trunk_fwd: hxs, saved and the workspace must be 16-byte aligned");
        return VAR_ERR_ARG;
    }
    const size_t sb = 4 * (size_t)saved_offset(m, M, m.nl + 2), hb = 4 * (size_t)N * m.H;
    {
        const void* in[6] = {feat, occ, motor_in, sound_in, hxs, masks};
        const size_t inb[6] = {4 * (size_t)M * 1152, 4 * (size_t)M * 288, 4 * (size_t)M * m.motor_in, 4 * (size_t)M * 3, hb, 4 * (size_t)M};
        const void* out[5] = {value, actor_features, h_T, saved, workspace};
        const size_t outb[5] = {4 * (size_t)M, 4 * (size_t)M * 128, hb, sb, (size_t)need};
        for (int o = 0; o < 5; ++o) {
            for (int i = 0; i < 6; ++i)
                if (overlap(out[o], outb[o], in[i], inb[i])) {
                    VAR_SET_ERR(c, "var_trunk_fwd: an output (value, actor_features, h_T, saved, workspace: #%d) overlaps an input (#%d)", o, i);
                    return VAR_ERR_ARG;
                }
            for (int p = o + 1; p < 5; ++p)
                if (overlap(out[o], outb[o], out[p], outb[p])) {
                    VAR_SET_ERR(c, "var_trunk_fwd: outputs #%d and #%d overlap", o, p);
                    return VAR_ERR_ARG;
                }
        }
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const long gws = gru_ws_bytes(m, T, N);
    float* sv = saved ? saved : (float*)((char*)workspace + gws);            // nobody differentiates: the activations live in the workspace
    Ptrs p{};
    p.ext[0] = feat; p.ext[1] = motor_in; p.ext[2] = sound_in; p.ext[3] = occ;
    float* g = sv + saved_offset(m, M, m.nl);
    p.ext[4] = g;
    float* act[kMaxLayers];
    for (int l = 0; l < m.nl; ++l) p.act[l] = act[l] = sv + saved_offset(m, M, l);
    for (int stage = 1; stage <= kStages; ++stage) {
        Jobs js{};
        int blocks = 0;
        for (int l = 0; l < m.nl; ++l) {
            const Layer& L = m.L[l];
            if (L.stage != stage) continue;
            const Op w = make_op(params[4 + 2 * l], nullptr, nullptr, nullptr, L.in, 1, L.in);
            Job j = product_job(input_op(m, p, L, L.in, 1, L.in), w, act[l], params[5 + 2 * l], (int)M, L.out, L.in, L.out, L.relu);
            j.c2 = l == m.value_layer ? value : (l == m.actor_layer ? actor_features : nullptr);   // the two outputs, next to their saved copies
            push(js, blocks, j);
        }
        hipLaunchKernelGGL(trunk_stage_kernel<false>, dim3(blocks), dim3(256), 0, s, js);
        VAR_HIP_CHECK(c, hipGetLastError());
        if (stage == 5) {                                                    // x is complete: the recurrent sequence
            const int rc = var_gru_seq_fwd(c, stream, p.act[m.x_layer], hxs, masks, params[0], params[1], params[2], params[3], T, N, 128,
                                           m.H, g, h_T, saved ? sv + saved_offset(m, M, m.nl + 1) : nullptr, workspace, gws);
            if (rc != VAR_OK) return rc;
        }
    }
    return VAR_OK;
}

extern "C" int var_trunk_bwd(var_ctx* c, void* stream, int kind, const float* const* params, const float* feat, const float* occ,
                             const float* motor_in, const float* sound_in, const float* masks, int T, int N, const float* saved,
                             const float* d_value, const float* d_actor_features, const float* d_hT, float* d_feat, float* d_occ,
                             float* d_hxs, float* d_params, void* workspace, long workspace_bytes) {
    if (!c) return VAR_ERR_ARG;
    if (const char* why = shape_error(kind, T, N)) {
        VAR_SET_ERR(c, "var_trunk_bwd: %s (kind %d, T %d, N %d)", why, kind, T, N);
        return VAR_ERR_ARG;
    }
    const Model& m = model_of(kind);
    const int np = 4 + 2 * m.nl;
    if (!params || !feat || !motor_in || !sound_in || !masks || !saved || !d_feat || !d_hxs || !d_params || !workspace) {
        VAR_SET_ERR(c, "var_trunk_bwd: a NULL pointer (only d_value, d_actor_features, d_hT, and occ / d_occ for kind 0, may be NULL)");
        return VAR_ERR_ARG;
    }
    if (kind == 1 && (!occ || !d_occ)) {
        VAR_SET_ERR(c, "var_trunk_bwd: kind 1 (ai2thor_VAR) needs occ and d_occ (M, 288)");
        return VAR_ERR_ARG;
    }
    for (int i = 0; i < np; ++i)
        if (!params[i]) {
            VAR_SET_ERR(c, "var_trunk_bwd: params[%d] is NULL (%d device pointers in var_trunk_param_floats' order)", i, np);
            return VAR_ERR_ARG;
        }
    const long M = (long)T * N, need = var_trunk_workspace_bytes(kind, T, N);
    if (workspace_bytes < need) {
        VAR_SET_ERR(c, "var_trunk_bwd: workspace of %ld bytes, %ld needed (var_trunk_workspace_bytes)", workspace_bytes, need);
        return VAR_ERR_ARG;
    }
    if (!al16(workspace) || !al16(saved)) {
        VAR_SET_ERR(c, "var_trunk_bwd: saved and the workspace must be 16-byte aligned");
        return VAR_ERR_ARG;
    }
    const size_t sb = 4 * (size_t)saved_offset(m, M, m.nl + 2), hb = 4 * (size_t)N * m.H;
    {
        const void* in[9] = {feat, occ, motor_in, sound_in, masks, saved, d_value, d_actor_features, d_hT};
        const size_t inb[9] = {4 * (size_t)M * 1152, 4 * (size_t)M * 288, 4 * (size_t)M * m.motor_in, 4 * (size_t)M * 3, 4 * (size_t)M, sb,
                               4 * (size_t)M, 4 * (size_t)M * 128, hb};
        const void* out[5] = {d_feat, d_occ, d_hxs, d_params, workspace};
        const size_t outb[5] = {4 * (size_t)M * 1152, 4 * (size_t)M * 288, hb, 4 * (size_t)grad_offset(m, np), (size_t)need};
        for (int o = 0; o < 5; ++o) {
            for (int i = 0; i < 9; ++i)
                if (overlap(out[o], outb[o], in[i], inb[i])) {
                    VAR_SET_ERR(c, "var_trunk_bwd: an output (d_feat, d_occ, d_hxs, d_params, workspace: #%d) overlaps an input (#%d)", o, i);
                    return VAR_ERR_ARG;
                }
            for (int p = o + 1; p < 5; ++p)
                if (overlap(out[o], outb[o], out[p], outb[p])) {
                    VAR_SET_ERR(c, "var_trunk_bwd: outputs #%d and #%d overlap", o, p);
                    return VAR_ERR_ARG;
                }
        }
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const long gws = gru_ws_bytes(m, T, N);
    float* ws = (float*)((char*)workspace + gws);
    const BwdLayout bl = bwd_layout(m, M);
    Ptrs p{};
    p.ext[0] = feat; p.ext[1] = motor_in; p.ext[2] = sound_in; p.ext[3] = occ;
    p.ext[4] = saved + saved_offset(m, M, m.nl);
    for (int l = 0; l < m.nl; ++l) p.act[l] = saved + saved_offset(m, M, l);
    if (!d_value || !d_actor_features) {
        const int rc = var_zero_async(c, s, ws + bl.zeros, 4 * (size_t)M * 128);
        if (rc != VAR_OK) return rc;
    }
    // where each layer's dX goes (NULL: its input carries no gradient)
    float* dx[kMaxLayers];
    for (int l = 0; l < m.nl; ++l) {
        const Layer& L = m.L[l];
        dx[l] = ws + bl.dx[l];
        if (L.nsrc == 1 && L.src[0] == T_FEAT) dx[l] = d_feat;
        if (L.nsrc == 1 && L.src[0] == T_OCC) dx[l] = d_occ;
        if (L.nsrc == 1 && (L.src[0] == T_MOTOR || L.src[0] == T_SOUND)) dx[l] = nullptr;
    }
    float* gru_dx = ws + bl.gru_dx;
    for (int stage = kStages; stage >= 1; --stage) {
        if (stage == 5) {                                                    // d_g is complete: back through the recurrent sequence
            float* dp = d_params;
            const int rc = var_gru_seq_bwd(c, stream, p.act[m.x_layer], masks, params[0], params[1], saved + saved_offset(m, M, m.nl + 1),
                                           dx[m.rnn_layer], d_hT, T, N, 128, m.H, gru_dx, d_hxs, dp + grad_offset(m, 0), dp + grad_offset(m, 1),
                                           dp + grad_offset(m, 2), dp + grad_offset(m, 3), workspace, gws);
            if (rc != VAR_OK) return rc;
        }
        Jobs js{};
        int blocks = 0;
        for (int l = 0; l < m.nl; ++l) {
            const Layer& L = m.L[l];
            if (L.stage != stage) continue;
            // the incoming dY arrays: the dX of every layer that reads this one's output, or what the caller (the GRU) hands in
            const float* in[3] = {nullptr, nullptr, nullptr};
            int n_in = 0;
            if (l == m.value_layer) in[n_in++] = d_value ? d_value : ws + bl.zeros;
            if (l == m.actor_layer) in[n_in++] = d_actor_features ? d_actor_features : ws + bl.zeros;
            if (l == m.x_layer) in[n_in++] = gru_dx;
            for (int k = 0; k < m.nl; ++k)
                for (int q = 0; q < m.L[k].nsrc; ++q)
                    if (m.L[k].src[q] == l && n_in < 3) in[n_in++] = dx[k];
            const float* gate = L.relu ? p.act[l] : nullptr;
            const float* W = params[4 + 2 * l];
            if (dx[l])   // dX (M, in) = G (M, out) W (out, in)
                push(js, blocks, product_job(make_op(in[0], in[1], in[2], gate, L.out, 1, L.out), make_op(W, nullptr, nullptr, nullptr, 1, L.in, L.out),
                                             dx[l], nullptr, (int)M, L.in, L.out, L.in, 0));
            // dW (out, in) = G^T X_in, K = M
            push(js, blocks, product_job(make_op(in[0], in[1], in[2], gate, 1, L.out, (int)M), input_op(m, p, L, 1, L.in, (int)M),
                                         d_params + grad_offset(m, 4 + 2 * l), nullptr, L.out, L.in, (int)M, L.in, 0));
            Job cs{};   // db (out) = the column sums of G
            cs.p = make_op(in[0], in[1], in[2], gate, L.out, 1, 1);
            cs.c = d_params + grad_offset(m, 5 + 2 * l); cs.I = (int)M; cs.J = L.out; cs.kind = 1; cs.rt = 1; cs.tj = 1;
            push(js, blocks, cs);
        }
        hipLaunchKernelGGL(trunk_stage_kernel<true>, dim3(blocks), dim3(256), 0, s, js);
        VAR_HIP_CHECK(c, hipGetLastError());
    }
    return VAR_OK;
}
