// The recurrent sequence of one PPO minibatch, forward and backward (models/ppo/model.py:116-171, NNBase._forward_gru): a
// one-layer, one-direction torch.nn.GRU (gate order r, z, n) whose state is multiplied by the step's mask before every step,
//   h' = h_{t-1} * m_t;  gi = W_ih x_t + b_ih;  gh = W_hh h' + b_hh
//   r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h_t = (1 - z) * n + z * h'
// For 0/1 masks that is the reference's segmented form (it multiplies the whole state by masks[t] at every step where some row
// is 0; at the other steps every mask is 1.0 and the product is the identity) without its host read of the zero steps.  Other
// mask values are multiplied in as they are, which the reference does not do.  fp32; the sigmoid / tanh forms and the grouping
// gi + (gh + b) of ithor.hip's gru_gate_fwd_kernel; no product is contracted into an fma.
//   var_gru_seq_fwd   input projection over all T*N rows (one DenseP product) + ONE launch per time step
//   var_gru_seq_bwd   W_hh transposed once into the workspace + ONE launch per time step, walking t downwards, + one for what
//                     flows past m_0 into hxs + the batched products d_x, d_w_ih, d_w_hh (split-K slabs added in fixed order)
//                     and the two bias column sums.  No atomics anywhere: equal inputs give equal bits.
// Plain kernel boundaries order the steps: no kernel waits for another workgroup, nothing can time out.
#include "gg.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// B k-steps of 16 of one wave's share of a product: the 2 B 16-byte loads leave first, then the 4 B matrix instructions in k
// order (whatever B, an accumulator sees its k in the same order: the batch size changes the latency, not the bits).
// k = 16 (u + i) + 4 (lane >> 4) + e on both operands; the second operand is scaled by m (the step's mask, or 1).
template <int B>
__device__ __forceinline__ void mac16(const float4* __restrict__ wr, const float4* __restrict__ hr, int u, float m, f32x4& acc) {
    float4 a[B], b[B];
#pragma unroll
    for (int i = 0; i < B; ++i) { a[i] = wr[4 * (u + i)]; b[i] = hr[4 * (u + i)]; }
#pragma unroll
    for (int i = 0; i < B; ++i) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b[i].x * m, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b[i].y * m, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b[i].z * m, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b[i].w * m, acc, 0, 0, 0);
    }
}
__device__ __forceinline__ void mac_all(const float4* __restrict__ wr, const float4* __restrict__ hr, int nu, float m, f32x4& acc) {
    int u = 0;
    for (; u + 8 <= nu; u += 8) mac16<8>(wr, hr, u, m, acc);
    if (u + 4 <= nu) { mac16<4>(wr, hr, u, m, acc); u += 4; }
    for (; u < nu; ++u) mac16<1>(wr, hr, u, m, acc);
}

// ---- forward step -------------------------------------------------------------------------------------------------------
// ithor_reward.hip's rw_gru_step_kernel at a run-time H and one direction.  Workgroup (bx, by) owns hidden units 4 bx .. 4 bx + 3
// (12 rows of W_hh) and environments 16 by .. 16 by + 15.  One v_mfma_f32_16x16x4_f32 tile: row 4 u + g = gate g of unit u (g = 3
// is padding), column = environment; the four waves split K = H in quarters and their tiles are folded through LDS in wave
// order.  D[row 4 (lane >> 4) + r][column lane & 15]: a lane of wave 0 ends up with r, z, n of ONE (unit, environment).
// The mask goes into the state operand on its way to the matrix core.  A step reads (hprev, mask, its GI rows) and writes its
// own rows only: its result does not depend on T.
__global__ void __launch_bounds__(256) gru_seq_step_fwd_kernel(const float* __restrict__ w_hh, const float* __restrict__ b_hh,
                                                              const float* __restrict__ gi_t, const float* __restrict__ hprev,
                                                              const float* __restrict__ mask, float* __restrict__ out_t,
                                                              float* __restrict__ h_last, float* __restrict__ sv_t, long sv_stride,
                                                              int N, int H) {
    __shared__ float red[4][3][64];
    const int tid = threadIdx.x, lane = tid & 63, kq = tid >> 6, l15 = lane & 15, lk = lane >> 4;
    const int j0 = blockIdx.x * 4;
    const int env = blockIdx.y * 16 + l15, e = env < N ? env : N - 1;
    const float m = mask[e];
    const int j = j0 + lk;
    float gi[3] = {0.f, 0.f, 0.f}, bh[3] = {0.f, 0.f, 0.f}, hp = 0.f;
    if (kq == 0) {                                             // wave 0 finishes: its gate operands leave before the product
        const float* gp = gi_t + (long)e * 3 * H + j;
        const float* bp = b_hh + j;
#pragma unroll
        for (int g = 0; g < 3; ++g) { gi[g] = gp[(long)g * H]; bh[g] = bp[(long)g * H]; }
        hp = hprev[(long)e * H + j] * m;
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    {
        const int kw = H >> 2;                                 // this wave's quarter of K, a multiple of 16
        const int gate = (l15 & 3) < 3 ? (l15 & 3) : 2;        // the padding rows repeat gate n; their results are dropped
        const float4* wr = (const float4*)(w_hh + ((long)gate * H + j0 + (l15 >> 2)) * H + kq * kw + 4 * lk);
        const float4* hr = (const float4*)(hprev + (long)e * H + kq * kw + 4 * lk);
        mac_all(wr, hr, kw >> 4, m, acc);                      // k = kw kq + 16 u + 4 lk + e on both operands
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) red[kq][g][lane] = acc[g];
    __syncthreads();
    if (kq != 0 || env >= N) return;
    float gh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) gh[g] = (red[0][g][lane] + red[1][g][lane]) + (red[2][g][lane] + red[3][g][lane]);
    const float r = sigmoidf_(gi[0] + (gh[0] + bh[0]));
    const float z = sigmoidf_(gi[1] + (gh[1] + bh[1]));
    const float ghn = gh[2] + bh[2];
    const float n = tanhf(gi[2] + r * ghn);
    const float h = (1.f - z) * n + z * hp;
    const long o = (long)env * H + j;
    out_t[o] = h;
    if (h_last) h_last[o] = h;
    if (sv_t) { sv_t[o] = r; sv_t[sv_stride + o] = z; sv_t[2 * sv_stride + o] = n; sv_t[3 * sv_stride + o] = ghn; sv_t[4 * sv_stride + o] = hp; }
}

// ---- backward step ------------------------------------------------------------------------------------------------------
// Workgroup (bx, by) owns hidden units 16 bx .. 16 bx + 15 and environments 16 by .. 16 by + 15.  It first completes
//   dh_t[n,k] = d_out_t[n,k] + m_{t+1}[n] * (dh_{t+1}[n,k] * z_{t+1}[n,k] + sum_j dgh_{t+1}[n,j] * W_hh[j,k])
// from what the previous launch wrote: one 16x16x4 tile, row = unit, column = environment, K = 3H split over the four waves
// (W_hh^T (H, 3H) and the dgh rows are both contiguous along j), folded through LDS in wave order.  Then thread (unit tid & 15,
// environment tid >> 4) forms step t's gate gradients (ithor.hip's gru_gate_bwd_kernel) and writes dgi_t, dgh_t and
// dhz[n,k] = dh_t * z_t, the direct path the next launch reads back for the same (n,k) -- it is read and written by one thread.
// mode 0: the last step (nothing behind it: the carry is d_hT or zero), 1: a step with a successor, 2: no step, only the carry
// past m_0, written to d_hxs.
__global__ void __launch_bounds__(256) gru_seq_step_bwd_kernel(const float* __restrict__ wt, const float* __restrict__ dgh_next,
                                                              const float* __restrict__ m_next, const float* __restrict__ d_hT,
                                                              float* __restrict__ dhz, const float* __restrict__ d_out_t,
                                                              const float* __restrict__ sv_t, long sv_stride, float* __restrict__ dgi_t,
                                                              float* __restrict__ dgh_t, float* __restrict__ d_hxs, int N, int H,
                                                              int mode) {
    __shared__ float red[4][4][64];
    const int tid = threadIdx.x, lane = tid & 63, kq = tid >> 6, l15 = lane & 15, lk = lane >> 4;
    const int k0 = blockIdx.x * 16, e0 = blockIdx.y * 16;
    const int ul = tid & 15, cl = tid >> 4;
    const int env = e0 + cl, k = k0 + ul;
    const bool live = env < N;
    const long o = (long)(live ? env : N - 1) * H + k;
    float r = 0.f, z = 0.f, n = 0.f, ghn = 0.f, hp = 0.f, dout = 0.f;
    if (mode != 2) {                                           // the gate operands leave before the product
        r = sv_t[o]; z = sv_t[sv_stride + o]; n = sv_t[2 * sv_stride + o]; ghn = sv_t[3 * sv_stride + o]; hp = sv_t[4 * sv_stride + o];
        dout = d_out_t[o];
    }
    float carry = 0.f;
    if (mode == 0) {
        if (d_hT) carry = d_hT[o];
    } else {
        const float direct = dhz[o], mn = m_next[live ? env : N - 1];
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int kw = (3 * H) >> 2;                           // this wave's quarter of K = 3H, a multiple of 16
        const int ec = e0 + l15 < N ? e0 + l15 : N - 1;
        const float4* wr = (const float4*)(wt + (long)(k0 + l15) * 3 * H + kq * kw + 4 * lk);
        const float4* gr = (const float4*)(dgh_next + (long)ec * 3 * H + kq * kw + 4 * lk);
        mac_all(wr, gr, kw >> 4, 1.f, acc);
#pragma unroll
        for (int q = 0; q < 4; ++q) red[kq][q][lane] = acc[q];
        __syncthreads();
        const int src = 16 * (ul >> 2) + cl, q = ul & 3;       // D[row 4 (lane >> 4) + q][column lane & 15]
        const float prod = (red[0][q][src] + red[1][q][src]) + (red[2][q][src] + red[3][q][src]);
        carry = mn * (direct + prod);
    }
    if (!live) return;
    if (mode == 2) { d_hxs[o] = carry; return; }
    const float dh = dout + carry;
    const float dn_pre = dh * (1.f - z) * (1.f - n * n);
    const float dz_pre = dh * (hp - n) * z * (1.f - z);
    const float dr_pre = dn_pre * ghn * r * (1.f - r);
    const long g = (long)env * 3 * H + k;
    dgi_t[g] = dr_pre; dgi_t[g + H] = dz_pre; dgi_t[g + 2 * H] = dn_pre;
    dgh_t[g] = dr_pre; dgh_t[g + H] = dz_pre; dgh_t[g + 2 * H] = dn_pre * r;
    dhz[o] = dh * z;
}

// wt (H, 3H) = w_hh (3H, H) transposed, 32 x 32 tiles through LDS (both sides multiples of 32)
__global__ void __launch_bounds__(256) gru_seq_transpose_kernel(const float* __restrict__ w, float* __restrict__ wt, int rows, int cols) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) tile[ty + 8 * i][tx] = w[(long)(r0 + ty + 8 * i) * cols + c0 + tx];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) wt[(long)(c0 + ty + 8 * i) * rows + r0 + tx] = tile[tx][ty + 8 * i];
}

// db_ih[j] = sum_rows dgi[row][j], db_hh[j] = sum_rows dgh[row][j] (blockIdx.y picks the pair): one thread per column, the
// rows in index order, eight loads in flight
__global__ void __launch_bounds__(256) gru_seq_bias_kernel(const float* __restrict__ dgi, const float* __restrict__ dgh,
                                                          float* __restrict__ db_ih, float* __restrict__ db_hh, long rows, int cols) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= cols) return;
    const float* g = blockIdx.y ? dgh : dgi;
    float v = 0.f;
    long row = 0;
    for (; row + 8 <= rows; row += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = g[(row + u) * cols + j];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; row < rows; ++row) v += g[row * cols + j];
    (blockIdx.y ? db_hh : db_ih)[j] = v;
}

constexpr long kMaxElems = 1L << 30;      // gg.h addresses its operands with 32-bit byte offsets: T*N*3H floats stay below 4 GB

inline long align256(long bytes) { return (bytes + 255) & ~255L; }

// K splits of one batched product (tiles of 128 x 64 | 32, as gg_launch picks them): a function of the shape alone
inline int split_of(int M, int Ncols, int K) {
    const int tiles = ((M + GG_MT - 1) / GG_MT) * (Ncols <= 32 ? 1 : (Ncols + 63) / 64);
    return gg_small_split(tiles, K, (long)M * Ncols, 1L << 40);
}
inline long slab_floats_of(int M, int Ncols, int K) {
    const int ns = split_of(M, Ncols, K);
    return ns > 1 ? (long)ns * M * Ncols : 0;
}

struct Sizes {
    long rows, gi, wt, dg, dhz, slabs, fwd_bytes, bwd_bytes;
};
inline Sizes sizes_of(int T, int N, int I, int H) {
    Sizes s{};
    s.rows = (long)T * N;
    s.gi = align256(4 * s.rows * 3 * H);
    s.wt = align256(4L * 3 * H * H);
    s.dg = align256(4 * s.rows * 3 * H);
    s.dhz = align256(4L * N * H);
    long sl = slab_floats_of(I, (int)s.rows, 3 * H);            // d_x
    const long a = slab_floats_of(I, 3 * H, (int)s.rows);       // d_w_ih
    const long b = slab_floats_of(H, 3 * H, (int)s.rows);       // d_w_hh
    sl = sl > a ? sl : a;
    sl = sl > b ? sl : b;
    s.slabs = align256(4 * sl);
    s.fwd_bytes = s.gi;
    s.bwd_bytes = s.wt + 2 * s.dg + s.dhz + s.slabs;
    return s;
}

// NULL when the shape is fine, else what is wrong with it
inline const char* shape_error(int T, int N, int I, int H) {
    if (H < 64 || H > 1024 || (H & 63)) return "H must be a multiple of 64, 64..1024";
    if (I < 1 || I > 1024) return "I outside 1..1024";
    if (N < 1 || N > 64) return "N outside 1..64";
    if (T < 1) return "T < 1";
    if ((long)T * N * 3 * H > kMaxElems) return "T * N * 3H above 2^30 elements";
    return nullptr;
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *p = (const char*)a, *q = (const char*)b;
    return p < q + nb && q < p + na;
}
inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

// C (M x Ncols, C[m*scm + n*scn]) = sum_k A(m,k) B(k,n): straight, or as split-K slabs in `slabs` added in slab order
template <bool AKF, bool BKF>
int product(var_ctx* c, hipStream_t s, int M, int Ncols, int K, const float* A, long sam, long sak, const float* B, long sbk, long sbn,
            float* C, float* slabs) {
    const int ns = split_of(M, Ncols, K);
    if (ns <= 1) {
        DenseP<AKF, BKF, 0> p{};
        p.M = M; p.N = Ncols; p.K = K; p.nsplit = 1;
        p.A = A; p.sam = sam; p.sak = sak; p.Bm = B; p.sbk = sbk; p.sbn = sbn; p.C = C; p.scm = 1; p.scn = M;
        return gg_launch<DenseP<AKF, BKF, 0>, GG_KC, false>(c, s, p);
    }
    DenseP<AKF, BKF, 2> p{};
    p.M = M; p.N = Ncols; p.K = K; p.nsplit = ns;
    p.A = A; p.sam = sam; p.sak = sak; p.Bm = B; p.sbk = sbk; p.sbn = sbn; p.C = slabs; p.scm = 1; p.scn = M; p.sC = (long)M * Ncols;
    const int rc = gg_launch<DenseP<AKF, BKF, 2>, GG_KC, false>(c, s, p);
    if (rc != VAR_OK) return rc;
    const long n = (long)M * Ncols;
    hipLaunchKernelGGL(gg_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, C, slabs, n, ns, n, (const float*)nullptr, 1, 1, 0);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}

}  // namespace

extern "C" long var_gru_seq_workspace_bytes(int T, int N, int I, int H) {
    if (shape_error(T, N, I, H)) return VAR_ERR_ARG;
    const Sizes s = sizes_of(T, N, I, H);
    return s.fwd_bytes > s.bwd_bytes ? s.fwd_bytes : s.bwd_bytes;
}

extern "C" int var_gru_seq_fwd(var_ctx* c, void* stream, const float* x, const float* hxs, const float* masks, const float* w_ih,
                               const float* w_hh, const float* b_ih, const float* b_hh, int T, int N, int I, int H, float* out,
                               float* h_T, float* saved, void* workspace, long workspace_bytes) {
    if (!c) return VAR_ERR_ARG;
    if (const char* why = shape_error(T, N, I, H)) {
        VAR_SET_ERR(c, "var_gru_seq_fwd: %s (T %d, N %d, I %d, H %d)", why, T, N, I, H);
        return VAR_ERR_ARG;
    }
    if (!x || !hxs || !masks || !w_ih || !w_hh || !b_ih || !b_hh || !out || !h_T || !workspace) {
        VAR_SET_ERR(c, "var_gru_seq_fwd: a NULL pointer (only `saved` may be NULL: a forward nobody differentiates)");
        return VAR_ERR_ARG;
    }
    const Sizes z = sizes_of(T, N, I, H);
    if (workspace_bytes < z.fwd_bytes) {
        VAR_SET_ERR(c, "var_gru_seq_fwd: workspace of %ld bytes, %ld needed (var_gru_seq_workspace_bytes)", workspace_bytes, z.fwd_bytes);
        return VAR_ERR_ARG;
    }
    if (misaligned(hxs) || misaligned(w_hh) || misaligned(out) || misaligned(workspace)) {
        VAR_SET_ERR(c, "var_gru_seq_fwd: hxs, w_hh, out and the workspace must be 16-byte aligned");
        return VAR_ERR_ARG;
    }
    const size_t ob = 4 * (size_t)z.rows * H, hb = 4 * (size_t)N * H;
    if (overlap(out, ob, x, 4 * (size_t)z.rows * I) || overlap(out, ob, hxs, hb) || overlap(h_T, hb, hxs, hb) || overlap(h_T, hb, out, ob) ||
        overlap(workspace, (size_t)z.fwd_bytes, out, ob) || overlap(workspace, (size_t)z.fwd_bytes, hxs, hb) ||
        (saved && (overlap(saved, 5 * ob, out, ob) || overlap(saved, 5 * ob, hxs, hb)))) {
        VAR_SET_ERR(c, "var_gru_seq_fwd: out overlaps x or hxs, or h_T / saved / the workspace overlap out or hxs");
        return VAR_ERR_ARG;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    float* GI = (float*)workspace;
    {   // GI (T*N, 3H) = X W_ih^T + b_ih
        DenseP<true, true, 0> p{};
        p.M = 3 * H; p.N = (int)z.rows; p.K = I; p.nsplit = 1;
        p.A = w_ih; p.sam = I; p.sak = 1; p.Bm = x; p.sbk = 1; p.sbn = I; p.C = GI; p.scm = 1; p.scn = 3 * H; p.bias = b_ih;
        const int rc = gg_launch<DenseP<true, true, 0>, GG_KC, false>(c, s, p);
        if (rc != VAR_OK) return rc;
    }
    const long svs = z.rows * H;
    const dim3 grid(H / 4, (N + 15) / 16);
    for (int t = 0; t < T; ++t) {
        const float* hprev = t ? out + (long)(t - 1) * N * H : hxs;
        hipLaunchKernelGGL(gru_seq_step_fwd_kernel, grid, dim3(256), 0, s, w_hh, b_hh, GI + (long)t * N * 3 * H, hprev, masks + (long)t * N,
                           out + (long)t * N * H, t == T - 1 ? h_T : (float*)nullptr, saved ? saved + (long)t * N * H : (float*)nullptr, svs,
                           N, H);
        VAR_HIP_CHECK(c, hipGetLastError());
    }
    return VAR_OK;
}

extern "C" int var_gru_seq_bwd(var_ctx* c, void* stream, const float* x, const float* masks, const float* w_ih, const float* w_hh,
                               const float* saved, const float* d_out, const float* d_hT, int T, int N, int I, int H, float* d_x,
                               float* d_hxs, float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh, void* workspace,
                               long workspace_bytes) {
    if (!c) return VAR_ERR_ARG;
    if (const char* why = shape_error(T, N, I, H)) {
        VAR_SET_ERR(c, "var_gru_seq_bwd: %s (T %d, N %d, I %d, H %d)", why, T, N, I, H);
        return VAR_ERR_ARG;
    }
    if (!x || !masks || !w_ih || !w_hh || !saved || !d_out || !d_x || !d_hxs || !d_w_ih || !d_w_hh || !d_b_ih || !d_b_hh || !workspace) {
        VAR_SET_ERR(c, "var_gru_seq_bwd: a NULL pointer (only d_hT may be NULL: no gradient reaches h_T)");
        return VAR_ERR_ARG;
    }
    const Sizes z = sizes_of(T, N, I, H);
    if (workspace_bytes < z.bwd_bytes) {
        VAR_SET_ERR(c, "var_gru_seq_bwd: workspace of %ld bytes, %ld needed (var_gru_seq_workspace_bytes)", workspace_bytes, z.bwd_bytes);
        return VAR_ERR_ARG;
    }
    if (misaligned(saved) || misaligned(workspace)) {
        VAR_SET_ERR(c, "var_gru_seq_bwd: saved and the workspace must be 16-byte aligned");
        return VAR_ERR_ARG;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    float* WT = (float*)w;
    float* DGI = (float*)(w + z.wt);
    float* DGH = (float*)(w + z.wt + z.dg);
    float* DHZ = (float*)(w + z.wt + 2 * z.dg);
    float* slabs = (float*)(w + z.wt + 2 * z.dg + z.dhz);
    // W_hh^T, once per call (Adam moves the weights between two minibatches: nothing packed outlives the call)
    hipLaunchKernelGGL(gru_seq_transpose_kernel, dim3(H / 32, 3 * H / 32), dim3(256), 0, s, w_hh, WT, 3 * H, H);
    VAR_HIP_CHECK(c, hipGetLastError());
    const long svs = z.rows * H, nh = (long)N * H, n3h = (long)N * 3 * H;
    const dim3 grid(H / 16, (N + 15) / 16);
    for (int t = T - 1; t >= -1; --t) {
        const int mode = t < 0 ? 2 : (t == T - 1 ? 0 : 1);
        const long tt = t < 0 ? 0 : t;                          // (mode 2 reads no row of step t)
        hipLaunchKernelGGL(gru_seq_step_bwd_kernel, grid, dim3(256), 0, s, (const float*)WT,
                           mode ? (const float*)(DGH + (t + 1) * n3h) : (const float*)nullptr,
                           mode ? masks + (long)(t + 1) * N : (const float*)nullptr, d_hT, DHZ, d_out + tt * nh, saved + tt * nh, svs, DGI + tt * n3h, DGH + tt * n3h,
                           d_hxs, N, H, mode);
        VAR_HIP_CHECK(c, hipGetLastError());
    }
    const int rows = (int)z.rows, G = 3 * H;
    int rc;
    // d_x (rows, I) = DGI (rows, 3H) W_ih (3H, I): m = i, n = row, k = j
    rc = product<false, true>(c, s, I, rows, G, w_ih, 1, I, DGI, 1, G, d_x, slabs);
    if (rc != VAR_OK) return rc;
    // d_w_ih (3H, I) = DGI^T X: m = i, n = j, k = row
    rc = product<false, false>(c, s, I, G, rows, x, 1, I, DGI, G, 1, d_w_ih, slabs);
    if (rc != VAR_OK) return rc;
    // d_w_hh (3H, H) = DGH^T H': m = k, n = j, k = row  (H' = the masked states the forward saved)
    rc = product<false, false>(c, s, H, G, rows, saved + 4 * svs, 1, H, DGH, G, 1, d_w_hh, slabs);
    if (rc != VAR_OK) return rc;
    hipLaunchKernelGGL(gru_seq_bias_kernel, dim3((G + 255) / 256, 2), dim3(256), 0, s, (const float*)DGI, (const float*)DGH, d_b_ih, d_b_hh,
                       z.rows, G);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}
