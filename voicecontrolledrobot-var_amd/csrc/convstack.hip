// The actor-critics' convolution stacks, forward and backward, as PPO.update evaluates them on a minibatch of B images:
//   kind 0  armNet_VAR.imgCNN, the 96 x 96 branch (models/RL/arm_RL_model.py:22-34): eight convolutions, three pools
//   kind 1  ai2thorNet_VAR.imgCNN (models/RL/ai2thor_RL_model.py:16-25): six convolutions, four pools
//   kind 2  the two convolutions of occupancyCNNMLP (ai2thor_RL_model.py:34-35) over a (B, 1, 9, 9) map
// every convolution 3 x 3 and followed by ReLU, "+pool" = MaxPool2d(2, 2) (include/var_hip.h has the definition).
//   var_convstack_fwd   one gather-GEMM launch per convolution (gg.h: ConvFwdP with bias and ReLU in the store), one launch per
//                       pool, one copy of the last map into `saved`.
//   var_convstack_bwd   walks the layers downwards.  Per layer: the weight gradient as a split-K gather-GEMM whose partial sums
//                       go to slabs in the caller's workspace and are added in slab order by a fold launch; the bias gradient
//                       as channel sums of the gated gradient map (partials per chunk, folded in chunk order); the data
//                       gradient (stride 1, or stride 2 by parity classes) with the ReLU gate of the layer below applied in its
//                       store, or, below a pool, the pool + ReLU backward as a launch of its own.  The pooled inputs are not
//                       saved: the backward pools the saved un-pooled map again (a function of that map alone).
// Kernel boundaries order the layers: no atomics, no spin-wait, no grid barrier.  Every split is a function of the shape alone,
// nothing packed outlives a call, equal inputs give equal bits.  Nothing reads the device.
//
// bf16 mode (flags bit 0 of the _ex entries; kinds 0 and 1, kind 2 computes in fp32 whatever the flag): every convolution product,
// in all three directions, multiplies operands rounded to bf16 (round to nearest even) and accumulates in fp32.  Everything stored
// stays fp32 and every layout stays as it is.  Forward: relu(conv(bf16(x_l), bf16(w_l)) + b_l), the bias added in fp32, x_1 the
// float image as the fp32 path forms it from bytes, pools on the stored fp32 maps.  Data gradient: conv_transpose(bf16(g_l),
// bf16(w_l)), g_l the fp32 gradient wrt layer l's pre-activation; gates and pool routing are exact selections on fp32 values.
// Weight gradient: the sum over pixels of bf16(g_l) * bf16(x_l), fp32 partial sums, slabs added in an order that depends on the
// shape alone, stored.  Bias gradient: fp32 channel sums of the unrounded g_l.  Two tiers serve it, with these semantics both:
//   tier 1  the gather-GEMM with BF = true (gg.h rounds both operands on their way from its fp32 LDS tile into
//           v_mfma_f32_32x32x16_bf16): conv 1, the stride-2 and unpadded layers, every weight gradient tier 2 does not cover
//   tier 2  img_bf16.hip's c3_kernel (forward and data gradient) and c3w_kernel (weight gradient) for the stride-1 padded layers
//           behind conv 1, where it has an instantiation of the shape; its fragment table is packed inside every call into the
//           caller's workspace
#include "gg.h"

namespace {

constexpr int kMaxConvs = 8;
constexpr int kMaxBatch = 1024;
constexpr int kFlagBf16 = 1;       // flags bit 0 of the _ex entries
// geometry ids of the 3 x 3 filters the stacks use
enum { G_S1P1 = 0, G_S2P0 = 1, G_S1P0 = 2, G_S2P1 = 3 };
typedef Geo<3, 3, 1, 1, 1, 1> GeoS1P1;
typedef Geo<3, 3, 2, 2, 0, 0> GeoS2P0;
typedef Geo<3, 3, 1, 1, 0, 0> GeoS1P0;
typedef Geo<3, 3, 2, 2, 1, 1> GeoS2P1;

struct Conv { int cin, cout, geo, pool; };
struct Stack { int n, cin, hw, small; Conv L[kMaxConvs]; };     // small: the vector-ALU kernels below, not the gather-GEMM

const Stack kStacks[3] = {
    {8, 3, 96, 0, {{3, 32, G_S1P1, 0}, {32, 32, G_S1P1, 1}, {32, 64, G_S1P1, 0}, {64, 64, G_S1P1, 1}, {64, 128, G_S1P1, 0},
                {128, 128, G_S1P1, 1}, {128, 256, G_S2P0, 0}, {256, 128, G_S1P0, 0}}},
    {6, 3, 96, 0, {{3, 32, G_S1P1, 0}, {32, 32, G_S1P1, 1}, {32, 64, G_S1P1, 1}, {64, 64, G_S1P1, 1}, {64, 128, G_S1P1, 1},
                {128, 128, G_S2P1, 0}}},
    {2, 1, 9, 1, {{1, 64, G_S2P1, 0}, {64, 32, G_S2P1, 0}}},
};

inline bool kind_ok(int kind) { return kind >= 0 && kind <= 2; }
inline int geo_stride(int g) { return g == G_S2P0 || g == G_S2P1 ? 2 : 1; }
inline int geo_pad(int g) { return g == G_S1P1 || g == G_S2P1 ? 1 : 0; }

// the maps of one stack: layer l reads (cin, hin, hin) and writes (cout, hout, hout); a pool halves what the next layer reads
struct Shapes { int hin[kMaxConvs], hout[kMaxConvs]; };
inline Shapes shapes_of(const Stack& st) {
    Shapes s{};
    int h = st.hw;
    for (int l = 0; l < st.n; ++l) {
        s.hin[l] = h;
        s.hout[l] = (h + 2 * geo_pad(st.L[l].geo) - 3) / geo_stride(st.L[l].geo) + 1;
        h = st.L[l].pool ? s.hout[l] / 2 : s.hout[l];
    }
    return s;
}
inline long act_floats(const Stack& st, const Shapes& sh, int l) { return (long)st.L[l].cout * sh.hout[l] * sh.hout[l]; }   // per image
inline long feat_floats(const Stack& st) { const Shapes sh = shapes_of(st); return act_floats(st, sh, st.n - 1); }

inline long param_floats(const Stack& st, int i) { const Conv& L = st.L[i >> 1]; return i & 1 ? L.cout : (long)L.cout * L.cin * 9; }
inline long grad_offset(const Stack& st, int i) {
    long o = 0;
    for (int k = 0; k < i; ++k) o += param_floats(st, k);
    return o;
}
inline long saved_offset(const Stack& st, long B, int j) {
    const Shapes sh = shapes_of(st);
    long o = 0;
    for (int l = 0; l < j; ++l) o += B * act_floats(st, sh, l);
    return o;
}

constexpr int kWgradKC = 32;       // both operands of a weight gradient are read along k (pixels)
constexpr int kChanChunks = 32;    // partial sums per channel of a bias gradient, whatever the shape (a chunk may be empty)
constexpr int kWideFold = 4096;    // a weight gradient of at least this many floats is folded one thread per output ...
constexpr int kWideSlabs = 128;    // ... over at most this many slabs
constexpr int kSmallImages = 8;    // images per split of the small stack's weight gradients (1024 / 8 = kWideSlabs slabs at most)

// K splits of layer l's weight gradient: about four workgroups per CU, every split at least four chunks, none empty
inline int wgrad_split(const Stack& st, const Shapes& sh, int l, long B) {
    if (st.small) return (int)((B + kSmallImages - 1) / kSmallImages);
    const int M = st.L[l].cin * 9, N = st.L[l].cout;
    const long K = B * sh.hout[l] * sh.hout[l];
    const int tiles = ((M + GG_MT - 1) / GG_MT) * ((N + 63) / 64);
    const long kchunks = (K + kWgradKC - 1) / kWgradKC;
    long ns = (1024 + tiles - 1) / tiles;
    if ((long)M * N >= kWideFold && ns > kWideSlabs) ns = kWideSlabs;   // (the fold's form depends on the layer alone)
    if (ns > kchunks / 4) ns = kchunks / 4;
    if (ns < 1) ns = 1;
    const long per = (kchunks + ns - 1) / ns;
    return (int)((kchunks + per - 1) / per);
}

// the workspace, in floats from its start (every region a multiple of 4 floats long)
struct Layout { long pooled, ga, gb, gp, slab, bpart, tab, acts, total; };
inline long up4(long n) { return (n + 3) & ~3L; }
// bf16 mode: whether layer l is one of the stride-1 padded layers behind conv 1 (tier 2's candidates)
// (-DVAR_CONVSTACK_TIER1: a tuning build that serves every layer from tier 1, to time the tiers against each other)
inline bool t2_candidate(const Stack& st, int l) {
#ifdef VAR_CONVSTACK_TIER1
    return false;
#else
    return !st.small && l > 0 && st.L[l].geo == G_S1P1;
#endif
}
inline Layout layout_of(const Stack& st, long B, bool bf = false) {
    const Shapes sh = shapes_of(st);
    long max_act = 0, max_pool = 0, max_slab = 0;
    for (int l = 0; l < st.n; ++l) {
        const long a = B * act_floats(st, sh, l);
        if (a > max_act) max_act = a;
        if (st.L[l].pool && a / 4 > max_pool) max_pool = a / 4;
        const long s = (long)wgrad_split(st, sh, l, B) * st.L[l].cin * 9 * st.L[l].cout;
        if (s > max_slab) max_slab = s;
        if (bf && t2_candidate(st, l)) {
            const long s2 = img_bf16_wgrad_slab_floats(st.L[l].cin, st.L[l].cout, sh.hout[l], (int)B);
            if (s2 > max_slab) max_slab = s2;
        }
    }
    Layout y{};
    long o = 0;
    y.pooled = o; o += up4(max_pool);
    const long fwd_base = o;
    y.ga = o; o += up4(max_act);
    y.gb = o; o += up4(max_act);
    y.gp = o; o += up4(max_pool);
    y.slab = o; o += up4(max_slab);
    y.bpart = o; o += kChanChunks * 256;
    y.tab = o; if (bf && !st.small) o += up4(img_bf16_table_bytes() / 4);      // tier 2's fragment table, packed inside every call
    y.acts = fwd_base;                                   // a forward without `saved` keeps its activations here
    const long fwd = fwd_base + up4(saved_offset(st, B, st.n));
    y.total = o > fwd ? o : fwd;
    return y;
}

// ---- element-wise kernels ---------------------------------------------------------------------------------------------------
// nn.MaxPool2d(2, 2) of (planes, H, H) maps, H even
__global__ void __launch_bounds__(256) cs_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long n, int H, int HP) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int px = (int)(i % HP), py = (int)((i / HP) % HP);
    const long plane = i / ((long)HP * HP);
    const float* q = x + plane * H * H + (long)(2 * py) * H + 2 * px;
    const float2 r0 = *(const float2*)q, r1 = *(const float2*)(q + H);
    y[i] = fmaxf(fmaxf(r0.x, r0.y), fmaxf(r1.x, r1.y));
}

// backward of ReLU followed by the pool, one thread per window: the gradient of a pooled cell goes to the first maximum of its
// window in scan order (PyTorch's choice) and is dropped where that maximum is not positive; the other three cells get zero
__global__ void __launch_bounds__(256) cs_pool_relu_bwd_kernel(const float* __restrict__ act, const float* __restrict__ gpool,
                                                               float* __restrict__ gact, long n, int H, int HP) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int px = (int)(i % HP), py = (int)((i / HP) % HP);
    const long plane = i / ((long)HP * HP);
    const long o = plane * H * H + (long)(2 * py) * H + 2 * px;
    const float2 r0 = *(const float2*)(act + o), r1 = *(const float2*)(act + o + H);
    int best = 0; float bv = r0.x;
    if (r0.y > bv) { bv = r0.y; best = 1; }
    if (r1.x > bv) { bv = r1.x; best = 2; }
    if (r1.y > bv) { bv = r1.y; best = 3; }
    const float g = bv > 0.f ? gpool[i] : 0.f;
    *(float2*)(gact + o) = make_float2(best == 0 ? g : 0.f, best == 1 ? g : 0.f);
    *(float2*)(gact + o + H) = make_float2(best == 2 ? g : 0.f, best == 3 ? g : 0.f);
}

// out = g where act > 0, else 0 (the last layer's ReLU, out of place: d_feat is the caller's)
__global__ void __launch_bounds__(256) cs_relu_gate_kernel(const float* __restrict__ g, const float* __restrict__ act,
                                                           float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = act[i] > 0.f ? g[i] : 0.f;
}

__global__ void __launch_bounds__(256) cs_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// part[chunk * C + c] = the sum of g[(b * C + c) * inner + i] over the chunk's share of {b < outer, i < inner}: a thread adds
// its elements in index order, the block's 256 sums are folded as a tree
__global__ void __launch_bounds__(256) cs_chan_sum_kernel(const float* __restrict__ g, float* __restrict__ part, int outer, int C,
                                                          int inner) {
    const int c = blockIdx.x;
    const long tot = (long)outer * inner;
    const long per = (tot + gridDim.y - 1) / gridDim.y;
    const long lo = blockIdx.y * per, hi = min(tot, lo + per);
    float acc = 0.f;
    for (long e = lo + threadIdx.x; e < hi; e += 256) {
        const long b = e / inner; const int i = (int)(e - b * inner);
        acc += g[(b * C + c) * inner + i];
    }
    __shared__ float red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long)blockIdx.y * C + c] = red[0];
}

// out[i] = sum_{s < nsplit} slabs[s * stride + i], stored: 16 outputs per workgroup, thread group g adds the slabs g, g + 16, ...
// in order and the 16 group sums are added in group order (many slabs, few outputs: conv 1's weight gradient, the bias partials)
__global__ void __launch_bounds__(256) cs_fold_kernel(float* __restrict__ out, const float* __restrict__ slabs, int n, int nsplit,
                                                      long stride) {
    const int i = blockIdx.x * 16 + (threadIdx.x & 15), g = threadIdx.x >> 4;
    float acc = 0.f;
    if (i < n)
        for (int s = g; s < nsplit; s += 16) acc += slabs[s * stride + i];
    __shared__ float red[16][17];
    red[g][threadIdx.x & 15] = acc;
    __syncthreads();
    if (g == 0 && i < n) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) v += red[k][threadIdx.x];
        out[i] = v;
    }
}
// the same for long slabs, at most kWideSlabs of them: one thread per output, the slabs added in slab order (whole-line accesses)
__global__ void __launch_bounds__(256) cs_fold_wide_kernel(float* __restrict__ out, const float* __restrict__ slabs, int n, int nsplit,
                                                           long stride) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    int s = 0;
    for (; s + 8 <= nsplit; s += 8) {                    // eight loads in flight, added in slab order
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = slabs[(s + u) * stride + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; s < nsplit; ++s) v += slabs[s * stride + i];
    out[i] = v;
}

// ---- the occupancy stack (kind 2) -----------------------------------------------------------------------------------------------
// 1 -> 64 over 9 x 9 and 64 -> 32 over 5 x 5: 25 B and 9 B output pixels, reductions of 9 and 576 -- one or two 128-row tiles of
// the gather-GEMM at the update shapes, most of them padding, and 2 MFLOP per image.  Plain vector-ALU kernels instead, one
// thread per output element, fmaf chains in a fixed order (explicit fmaf: the library is built with -ffp-contract=off).
struct SmallConv { int B, CIN, H, COUT, HO, S, P; long xb; };      // square maps, 3 x 3 filter

template <bool U8>
__device__ __forceinline__ float small_ld(const void* x, long o) {
    if (U8) return (float)((const uint8_t*)x)[o] / 255.f;
    return ((const float*)x)[o];
}

// y = relu(conv(x, w) + bias): four partial sums over ci mod 4, added as (a0 + a1) + (a2 + a3), then the bias
template <bool U8>
__global__ void __launch_bounds__(256) cs_small_fwd_kernel(const SmallConv d, const void* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)d.B * d.COUT * d.HO * d.HO) return;
    const int ox = (int)(i % d.HO), oy = (int)((i / d.HO) % d.HO), co = (int)((i / (d.HO * d.HO)) % d.COUT);
    const long b = i / ((long)d.HO * d.HO * d.COUT);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ci = 0; ci < d.CIN; ++ci)
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * d.S + ky - d.P;
            if (iy < 0 || iy >= d.H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * d.S + kx - d.P;
                if (ix < 0 || ix >= d.H) continue;
                a[ci & 3] = fmaf(small_ld<U8>(x, b * d.xb + ((long)ci * d.H + iy) * d.H + ix), w[((co * d.CIN + ci) * 3 + ky) * 3 + kx], a[ci & 3]);
            }
        }
    const float v = ((a[0] + a[1]) + (a[2] + a[3])) + bias[co];
    y[i] = v > 0.f ? v : 0.f;
}

// dx = conv_transpose(gy, w), zero where mask (the activation dx belongs to) is not positive: partial sums over co mod 4
__global__ void __launch_bounds__(256) cs_small_dgrad_kernel(const SmallConv d, const float* __restrict__ gy, const float* __restrict__ w,
                                                             const float* __restrict__ mask, float* __restrict__ dx) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)d.B * d.CIN * d.H * d.H) return;
    const int xx = (int)(i % d.H), yy = (int)((i / d.H) % d.H), ci = (int)((i / (d.H * d.H)) % d.CIN);
    const long b = i / ((long)d.H * d.H * d.CIN);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int co = 0; co < d.COUT; ++co)
        for (int ky = 0; ky < 3; ++ky) {
            const int ty = yy + d.P - ky;
            if (ty < 0 || ty % d.S || ty / d.S >= d.HO) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int tx = xx + d.P - kx;
                if (tx < 0 || tx % d.S || tx / d.S >= d.HO) continue;
                a[co & 3] = fmaf(gy[((b * d.COUT + co) * d.HO + ty / d.S) * d.HO + tx / d.S], w[((co * d.CIN + ci) * 3 + ky) * 3 + kx], a[co & 3]);
            }
        }
    const float v = (a[0] + a[1]) + (a[2] + a[3]);
    dx[i] = mask[i] > 0.f ? v : 0.f;
}

// split sz (blockIdx.y) adds its `per` images' products of one filter element in (image, oy, ox) order and stores the sum in its slab
template <bool U8>
__global__ void __launch_bounds__(256) cs_small_wgrad_kernel(const SmallConv d, const void* __restrict__ x, const float* __restrict__ gy,
                                                             float* __restrict__ slab, int per) {
    const int j = blockIdx.x * 256 + threadIdx.x, MN = d.COUT * d.CIN * 9;
    if (j >= MN) return;
    const int kx = j % 3, ky = (j / 3) % 3, ci = (j / 9) % d.CIN, co = j / (9 * d.CIN);
    const int b0 = blockIdx.y * per, b1 = min(d.B, b0 + per);
    float acc = 0.f;
    for (long b = b0; b < b1; ++b)
        for (int oy = 0; oy < d.HO; ++oy) {
            const int iy = oy * d.S + ky - d.P;
            if (iy < 0 || iy >= d.H) continue;
            for (int ox = 0; ox < d.HO; ++ox) {
                const int ix = ox * d.S + kx - d.P;
                if (ix < 0 || ix >= d.H) continue;
                acc = fmaf(small_ld<U8>(x, b * d.xb + ((long)ci * d.H + iy) * d.H + ix), gy[((b * d.COUT + co) * d.HO + oy) * d.HO + ox], acc);
            }
        }
    slab[(long)blockIdx.y * MN + j] = acc;
}

// ConvWgradP whose every split, a single one included, STORES its partial sums into its slab
template <class G, bool U8>
struct WgradSlabP : ConvWgradP<G, U8, false> {
    typedef typename ConvWgradP<G, U8, false>::CM CM;
    __device__ CM c_m(int j, int, int sz) const { return CM{this->slab + (long)sz * this->M * this->N + j}; }
    __device__ void store(const CM& cm, int n, float v, int) const { cm.q[(long)n * this->M] = v; }
};

#define CS_CHECK(c) VAR_HIP_CHECK(c, hipGetLastError())
inline dim3 g1(long n) { return dim3((unsigned)((n + 255) / 256)); }

template <class G, bool U8, bool BF>
int conv_fwd(var_ctx* c, hipStream_t s, const ConvDims& d, const void* x, const float* w, const float* bias, float* y) {
    ConvFwdP<G, U8, false> p{};
    p.M = d.B * d.HO * d.WO; p.N = d.COUT; p.K = d.CIN * G::KHW; p.nsplit = 1;
    p.d = d; p.x = x; p.w = w; p.bias = bias; p.y = y;
    return gg_launch<ConvFwdP<G, U8, false>, GG_KC, BF>(c, s, p);
}
template <class G, bool BF>
int conv_dgrad(var_ctx* c, hipStream_t s, const ConvDims& d, const float* gy, const float* w, float* dx, const float* mask) {
    if constexpr (G::SH == 2) {
        typedef ConvDgradS2P<G, false> P;
        P p{};
        p.H2 = (d.H + 1) / 2; p.W2 = (d.W + 1) / 2;
        p.inv_h2w2 = 1.f / (float)(p.H2 * p.W2); p.inv_w2 = 1.f / (float)p.W2;
        p.M = d.B * p.H2 * p.W2; p.N = d.CIN; p.K = d.COUT * P::NKY * P::NKX; p.nsplit = 1;
        p.d = d; p.gy = gy; p.w = w; p.dx = dx; p.mask = mask;
        return gg_launch<P, GG_KC, BF>(c, s, p, 4);
    } else {
        ConvDgradP<G> p{};
        p.M = d.B * d.H * d.W; p.N = d.CIN; p.K = d.COUT * G::KHW; p.nsplit = 1;
        p.d = d; p.gy = gy; p.w = w; p.dx = dx; p.mask = mask;
        return gg_launch<ConvDgradP<G>, GG_KC, BF>(c, s, p);
    }
}
template <class G, bool U8, bool BF>
int conv_wgrad(var_ctx* c, hipStream_t s, const ConvDims& d, const void* x, const float* gy, float* slab, int nsplit) {
    WgradSlabP<G, U8> p{};
    p.M = d.CIN * G::KHW; p.N = d.COUT; p.K = d.B * d.HO * d.WO; p.nsplit = nsplit;
    p.d = d; p.x = x; p.gy = gy; p.dw = nullptr; p.slab = slab;
    return gg_launch<WgradSlabP<G, U8>, kWgradKC, BF>(c, s, p);
}

int fold(var_ctx* c, hipStream_t s, float* out, const float* slabs, int n, int nsplit, long stride) {
    if (n >= kWideFold)
        hipLaunchKernelGGL(cs_fold_wide_kernel, dim3((n + 255) / 256), dim3(256), 0, s, out, slabs, n, nsplit, stride);
    else
        hipLaunchKernelGGL(cs_fold_kernel, dim3((n + 15) / 16), dim3(256), 0, s, out, slabs, n, nsplit, stride);
    CS_CHECK(c);
    return VAR_OK;
}

inline SmallConv small_of(const ConvDims& d, int stride, int pad) {
    return SmallConv{d.B, d.CIN, d.H, d.COUT, d.HO, stride, pad, d.xb};
}
int small_fwd(var_ctx* c, hipStream_t s, const SmallConv& d, bool u8, const void* x, const float* w, const float* bias, float* y) {
    const dim3 grid = g1((long)d.B * d.COUT * d.HO * d.HO);
    if (u8) hipLaunchKernelGGL(cs_small_fwd_kernel<true>, grid, dim3(256), 0, s, d, x, w, bias, y);
    else hipLaunchKernelGGL(cs_small_fwd_kernel<false>, grid, dim3(256), 0, s, d, x, w, bias, y);
    CS_CHECK(c);
    return VAR_OK;
}
int small_wgrad(var_ctx* c, hipStream_t s, const SmallConv& d, bool u8, const void* x, const float* gy, float* slab, int nsplit) {
    const dim3 grid((d.COUT * d.CIN * 9 + 255) / 256, nsplit);
    if (u8) hipLaunchKernelGGL(cs_small_wgrad_kernel<true>, grid, dim3(256), 0, s, d, x, gy, slab, kSmallImages);
    else hipLaunchKernelGGL(cs_small_wgrad_kernel<false>, grid, dim3(256), 0, s, d, x, gy, slab, kSmallImages);
    CS_CHECK(c);
    return VAR_OK;
}

// only the first layer of a stack can read bytes
#define CS_GEO1(geo, u8, CALL_U8, CALL)                                    \
    switch (geo) {                                                          \
        case G_S1P1: { typedef GeoS1P1 G; if (u8) { CALL_U8; } else { CALL; } break; } \
        case G_S2P1: { typedef GeoS2P1 G; if (u8) { CALL_U8; } else { CALL; } break; } \
        case G_S2P0: { typedef GeoS2P0 G; CALL; break; }                   \
        default: { typedef GeoS1P0 G; CALL; break; }                       \
    }
// the calls name BF: the operands rounded to bf16 (tier 1 of the bf16 mode) or not
#define CS_GEO(geo, u8, bf, CALL_U8, CALL)                                 \
    if (bf) { constexpr bool BF = true; CS_GEO1(geo, u8, CALL_U8, CALL) }  \
    else { constexpr bool BF = false; CS_GEO1(geo, u8, CALL_U8, CALL) }

inline ConvDims dims_of(const Stack& st, const Shapes& sh, int l, int B, long xb) {
    const int g = st.L[l].geo;
    ConvDims d = conv_dims(B, st.L[l].cin, sh.hin[l], sh.hin[l], st.L[l].cout, 3, 3, geo_stride(g), geo_stride(g), geo_pad(g), geo_pad(g));
    if (l == 0) d.xb = xb;
    return d;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the checks both entries share; NULL when the call is accepted
const char* common_error(int kind, const float* const* params, const void* image, int is_u8, long image_bstride, int B,
                         const void* ws, long ws_bytes, int flags, char* buf, size_t nbuf) {
    if (flags & ~kFlagBf16) { snprintf(buf, nbuf, "flags = %d: bit 0 (bf16 operands) is the only one", flags); return buf; }
    if (!kind_ok(kind)) { snprintf(buf, nbuf, "kind %d is none of 0 (arm_VAR imgCNN), 1 (ai2thor_VAR imgCNN), 2 (occupancy convolutions)", kind); return buf; }
    if (B < 1 || B > kMaxBatch) { snprintf(buf, nbuf, "B = %d is outside 1..%d", B, kMaxBatch); return buf; }
    const Stack& st = kStacks[kind];
    if (!params || !image || !ws) { snprintf(buf, nbuf, "a NULL pointer (params, image or the workspace)"); return buf; }
    for (int i = 0; i < 2 * st.n; ++i)
        if (!params[i]) { snprintf(buf, nbuf, "params[%d] is NULL (%d device pointers in var_convstack_param_floats' order)", i, 2 * st.n); return buf; }
    const long per = (long)st.cin * st.hw * st.hw;
    // the engine addresses an operand by 32-bit byte offsets from its base
    if (image_bstride < per || image_bstride * B * (is_u8 ? 1 : 4) >= (1L << 32) || image_bstride >= (1L << 31)) {
        snprintf(buf, nbuf, "image_bstride %ld: at least %ld elements, and the whole batch below 4 GB", image_bstride, per);
        return buf;
    }
    const long need = 4 * layout_of(st, B, flags & kFlagBf16).total;
    if (ws_bytes < need) {
        snprintf(buf, nbuf, "workspace of %ld bytes, %ld needed (var_convstack_workspace_bytes_ex at flags %d)", ws_bytes, need, flags);
        return buf;
    }
    return nullptr;
}

}  // namespace

extern "C" int var_convstack_n_params(int kind) { return kind_ok(kind) ? 2 * kStacks[kind].n : VAR_ERR_ARG; }
extern "C" long var_convstack_param_floats(int kind, int i) {
    if (!kind_ok(kind) || i < 0 || i >= 2 * kStacks[kind].n) return VAR_ERR_ARG;
    return param_floats(kStacks[kind], i);
}
extern "C" long var_convstack_grad_offset(int kind, int i) {
    if (!kind_ok(kind) || i < 0 || i > 2 * kStacks[kind].n) return VAR_ERR_ARG;
    return grad_offset(kStacks[kind], i);
}
extern "C" long var_convstack_saved_offset(int kind, int B, int j) {
    if (!kind_ok(kind) || B < 1 || B > kMaxBatch || j < 0 || j > kStacks[kind].n) return VAR_ERR_ARG;
    return saved_offset(kStacks[kind], B, j);
}
extern "C" long var_convstack_saved_floats(int kind, int B) {
    if (!kind_ok(kind) || B < 1 || B > kMaxBatch) return VAR_ERR_ARG;
    return saved_offset(kStacks[kind], B, kStacks[kind].n);
}
extern "C" long var_convstack_workspace_bytes_ex(int kind, int B, int flags) {
    if (!kind_ok(kind) || B < 1 || B > kMaxBatch || (flags & ~kFlagBf16)) return VAR_ERR_ARG;
    return 4 * layout_of(kStacks[kind], B, flags & kFlagBf16).total;
}
extern "C" long var_convstack_workspace_bytes(int kind, int B) { return var_convstack_workspace_bytes_ex(kind, B, 0); }

namespace {
int fwd_impl(const char* entry, var_ctx* c, void* stream, int kind, const float* const* params, const void* image, int image_is_u8,
             long image_bstride, int B, float* feat, float* saved, void* workspace, long workspace_bytes, int flags) {
    if (!c) return VAR_ERR_ARG;
    char why[256];
    if (common_error(kind, params, image, image_is_u8, image_bstride, B, workspace, workspace_bytes, flags, why, sizeof(why))) {
        VAR_SET_ERR(c, "%s: %s", entry, why);
        return VAR_ERR_ARG;
    }
    if (!feat) { VAR_SET_ERR(c, "%s: feat is NULL (only `saved` may be)", entry); return VAR_ERR_ARG; }
    if (!al16(feat) || !al16(saved) || !al16(workspace)) {
        VAR_SET_ERR(c, "%s: feat, saved and the workspace must be 16-byte aligned", entry);
        return VAR_ERR_ARG;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const Stack& st = kStacks[kind];
    const Shapes sh = shapes_of(st);
    const bool bf = (flags & kFlagBf16) && !st.small;
    const Layout lay = layout_of(st, B, flags & kFlagBf16);
    float* ws = (float*)workspace;
    float* acts = saved ? saved : ws + lay.acts;
    const void* x = image;
    for (int l = 0; l < st.n; ++l) {
        const Conv& L = st.L[l];
        const ConvDims d = dims_of(st, sh, l, B, image_bstride);
        const bool last = l == st.n - 1, u8 = l == 0 && image_is_u8;
        float* y = last ? feat : acts + saved_offset(st, B, l);
        const float *w = params[2 * l], *b = params[2 * l + 1];
        int rc = VAR_OK;
        if (st.small) {
            rc = small_fwd(c, s, small_of(d, geo_stride(L.geo), geo_pad(L.geo)), u8, x, w, b, y);
        } else {
            int t2 = 1;                                  // 1: tier 2 has no kernel of this shape
            if (bf && t2_candidate(st, l)) t2 = img_bf16_conv_shape(c, s, L.cin, L.cout, sh.hin[l], 0, (const float*)x, w, b, nullptr, y, B, ws + lay.tab);
            if (t2 != 1) rc = t2;
            else { CS_GEO(L.geo, u8, bf, (rc = conv_fwd<G, true, BF>(c, s, d, x, w, b, y)), (rc = conv_fwd<G, false, BF>(c, s, d, x, w, b, y))) }
        }
        if (rc != VAR_OK) return rc;
        x = y;
        if (L.pool) {
            const int HP = sh.hout[l] / 2;
            const long n = (long)B * L.cout * HP * HP;
            hipLaunchKernelGGL(cs_pool_fwd_kernel, g1(n), dim3(256), 0, s, y, ws + lay.pooled, n, sh.hout[l], HP);
            CS_CHECK(c);
            x = ws + lay.pooled;
        }
    }
    if (saved) {
        const long n = (long)B * feat_floats(st);
        hipLaunchKernelGGL(cs_copy_kernel, g1(n), dim3(256), 0, s, feat, saved + saved_offset(st, B, st.n - 1), n);
        CS_CHECK(c);
    }
    return VAR_OK;
}

int bwd_impl(const char* entry, var_ctx* c, void* stream, int kind, const float* const* params, const void* image, int image_is_u8,
             long image_bstride, int B, const float* saved, const float* d_feat, float* grads_flat, void* workspace,
             long workspace_bytes, float* d_saved, int flags) {
    if (!c) return VAR_ERR_ARG;
    char why[256];
    if (common_error(kind, params, image, image_is_u8, image_bstride, B, workspace, workspace_bytes, flags, why, sizeof(why))) {
        VAR_SET_ERR(c, "%s: %s", entry, why);
        return VAR_ERR_ARG;
    }
    if (!saved || !d_feat || !grads_flat) { VAR_SET_ERR(c, "%s: saved, d_feat or grads_flat is NULL", entry); return VAR_ERR_ARG; }
    if (!al16(saved) || !al16(grads_flat) || !al16(workspace) || !al16(d_saved)) {
        VAR_SET_ERR(c, "%s: saved, grads_flat, d_saved and the workspace must be 16-byte aligned", entry);
        return VAR_ERR_ARG;
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const Stack& st = kStacks[kind];
    const Shapes sh = shapes_of(st);
    const bool bf = (flags & kFlagBf16) && !st.small;
    const Layout lay = layout_of(st, B, flags & kFlagBf16);
    float* ws = (float*)workspace;
    // g_l, the gated gradient wrt convolution l's un-pooled map: the two ping-pong regions, or its place in the caller's d_saved
    auto g_of = [&](int l) { return d_saved ? d_saved + saved_offset(st, B, l) : ws + ((l & 1) ? lay.gb : lay.ga); };
    float *pooled = ws + lay.pooled, *gp = ws + lay.gp, *slab = ws + lay.slab, *bpart = ws + lay.bpart;
    {   // the last layer's ReLU
        const long n = (long)B * feat_floats(st);
        hipLaunchKernelGGL(cs_relu_gate_kernel, g1(n), dim3(256), 0, s, d_feat, saved + saved_offset(st, B, st.n - 1), g_of(st.n - 1), n);
        CS_CHECK(c);
    }
    for (int l = st.n - 1; l >= 0; --l) {
        const Conv& L = st.L[l];
        const ConvDims d = dims_of(st, sh, l, B, image_bstride);
        const float* gy = g_of(l);
        const bool u8 = l == 0 && image_is_u8;
        // the layer's input: the image, the map below, or that map pooled again
        const void* x = image;
        const float* below = l ? saved + saved_offset(st, B, l - 1) : nullptr;
        const bool pooled_in = l && st.L[l - 1].pool;
        if (l) x = below;
        if (pooled_in) {
            const long n = (long)B * L.cin * sh.hin[l] * sh.hin[l];
            hipLaunchKernelGGL(cs_pool_fwd_kernel, g1(n), dim3(256), 0, s, below, pooled, n, sh.hout[l - 1], sh.hin[l]);
            CS_CHECK(c);
            x = pooled;
        }
        const int ns = wgrad_split(st, sh, l, B), MN = L.cin * 9 * L.cout;
        int rc = VAR_OK;
        float* dw = grads_flat + grad_offset(st, 2 * l);
        if (bf && t2_candidate(st, l) && img_bf16_wgrad_slab_floats(L.cin, L.cout, sh.hin[l], B) > 0) {
            rc = img_bf16_wgrad_shape(c, s, L.cin, L.cout, sh.hin[l], (const float*)x, gy, dw, slab, B);      // (its own fold, stored)
            if (rc != VAR_OK) return rc;
        } else {
            if (st.small) {
                rc = small_wgrad(c, s, small_of(d, geo_stride(L.geo), geo_pad(L.geo)), u8, x, gy, slab, ns);
            } else {
                CS_GEO(L.geo, u8, bf, (rc = conv_wgrad<G, true, BF>(c, s, d, x, gy, slab, ns)), (rc = conv_wgrad<G, false, BF>(c, s, d, x, gy, slab, ns)))
            }
            if (rc != VAR_OK) return rc;
            rc = fold(c, s, dw, slab, MN, ns, MN);
            if (rc != VAR_OK) return rc;
        }
        const int inner = sh.hout[l] * sh.hout[l];
        hipLaunchKernelGGL(cs_chan_sum_kernel, dim3(L.cout, kChanChunks), dim3(256), 0, s, gy, bpart, B, L.cout, inner);
        CS_CHECK(c);
        rc = fold(c, s, grads_flat + grad_offset(st, 2 * l + 1), bpart, L.cout, kChanChunks, L.cout);
        if (rc != VAR_OK) return rc;
        if (!l) break;                                   // the observations carry no gradient: conv 1 has no data gradient
        float* dx = pooled_in ? gp : g_of(l - 1);
        const float* mask = pooled_in ? nullptr : below;
        const float* w = params[2 * l];
        if (st.small) {                                  // (no pool in the small stack: mask is the map below)
            const SmallConv sd = small_of(d, geo_stride(L.geo), geo_pad(L.geo));
            hipLaunchKernelGGL(cs_small_dgrad_kernel, g1((long)B * L.cin * sh.hin[l] * sh.hin[l]), dim3(256), 0, s, sd, gy, w, mask, dx);
            CS_CHECK(c);
        } else {
            int t2 = 1;
            if (bf && t2_candidate(st, l)) t2 = img_bf16_conv_shape(c, s, L.cin, L.cout, sh.hin[l], 1, gy, w, nullptr, mask, dx, B, ws + lay.tab);
            if (t2 != 1) rc = t2;
            else { CS_GEO(L.geo, false, bf, (void)0, (rc = conv_dgrad<G, BF>(c, s, d, gy, w, dx, mask))) }
        }
        if (rc != VAR_OK) return rc;
        if (pooled_in) {
            const long n = (long)B * L.cin * sh.hin[l] * sh.hin[l];
            hipLaunchKernelGGL(cs_pool_relu_bwd_kernel, g1(n), dim3(256), 0, s, below, gp, g_of(l - 1), n, sh.hout[l - 1], sh.hin[l]);
            CS_CHECK(c);
        }
    }
    return VAR_OK;
}
}  // namespace

extern "C" int var_convstack_fwd_ex(var_ctx* c, void* stream, int kind, const float* const* params, const void* image, int image_is_u8,
                                    long image_bstride, int B, float* feat, float* saved, void* workspace, long workspace_bytes,
                                    int flags) {
    return fwd_impl("var_convstack_fwd_ex", c, stream, kind, params, image, image_is_u8, image_bstride, B, feat, saved, workspace,
                    workspace_bytes, flags);
}
extern "C" int var_convstack_fwd(var_ctx* c, void* stream, int kind, const float* const* params, const void* image, int image_is_u8,
                                 long image_bstride, int B, float* feat, float* saved, void* workspace, long workspace_bytes) {
    return fwd_impl("var_convstack_fwd", c, stream, kind, params, image, image_is_u8, image_bstride, B, feat, saved, workspace,
                    workspace_bytes, 0);
}
extern "C" int var_convstack_bwd_ex(var_ctx* c, void* stream, int kind, const float* const* params, const void* image, int image_is_u8,
                                    long image_bstride, int B, const float* saved, const float* d_feat, float* grads_flat,
                                    void* workspace, long workspace_bytes, float* d_saved, int flags) {
    return bwd_impl("var_convstack_bwd_ex", c, stream, kind, params, image, image_is_u8, image_bstride, B, saved, d_feat, grads_flat,
                    workspace, workspace_bytes, d_saved, flags);
}
extern "C" int var_convstack_bwd(var_ctx* c, void* stream, int kind, const float* const* params, const void* image, int image_is_u8,
                                 long image_bstride, int B, const float* saved, const float* d_feat, float* grads_flat,
                                 void* workspace, long workspace_bytes) {
    return bwd_impl("var_convstack_bwd", c, stream, kind, params, image, image_is_u8, image_bstride, B, saved, d_feat, grads_flat,
                    workspace, workspace_bytes, nullptr, 0);
}
