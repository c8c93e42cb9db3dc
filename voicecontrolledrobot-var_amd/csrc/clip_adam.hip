// The PPO update's optimiser step (models/ppo/algo/ppo.py:89-91): torch.nn.utils.clip_grad_norm_(params, max_norm) followed by
// torch.optim.Adam(lr, betas, eps).step(), over a TABLE of tensors instead of one arena -- var_clip_adam_step, two launches:
//   opt_sumsq_kernel   every workgroup leaves the sum of squares of its share of all gradients in var_ctx::opt_part
//   opt_adam_kernel    every workgroup folds those sums in the same order (equal bits everywhere), forms the clip coefficient
//                      and applies adam_kernel's arithmetic (pack_adam.hip) to g * coef
// How the work is cut.  The segments' elements are numbered through, 0 .. E - 1, in table order.  Workgroup c owns the
// elements [c C, (c + 1) C), C = 1024 U, U = ceil(E / 2^20): at most kOptMaxWG workgroups.  In its round u = 0 .. U - 1 thread t
// takes the four elements from c C + 4 (256 u + t) on, so a wave's round covers 1 KiB per array.  Which thread adds which
// square, and in which order, is therefore a function of an element's NUMBER and of E alone -- not of where the table is cut
// into segments, nor of how a long table is cut into launches: the same tensors as one merged segment or as many small ones
// give the same bits in the norm as well as in p, m and v.  A thread's four elements are one 16-byte access per array wherever
// they lie in one segment (global_load / store_dwordx4 ask for dword alignment only, and arena offsets promise no more), and go
// one by one where a segment ends among them.
// fp32, no product contracted into an fma (-ffp-contract=off).
#include <algorithm>
#include <math.h>

#include "var_common.h"

namespace {

constexpr int kT = 256;                       // threads per workgroup
constexpr int kQuad = 4;                      // elements per thread and round
constexpr long kRound = (long)kT * kQuad;     // elements per workgroup and round
static_assert(kOptMaxWG == 1024 && kOptCarryFloats == 3 * kT, "var_common.h: the optimiser's slice of loss_buf");

struct SqTable { const float* g[VAR_OPT_MAX_SEGS]; long start[VAR_OPT_MAX_SEGS + 1]; int n; };
struct AdamTable {
    float* p[VAR_OPT_MAX_SEGS]; const float* g[VAR_OPT_MAX_SEGS]; float* m[VAR_OPT_MAX_SEGS]; float* v[VAR_OPT_MAX_SEGS];
    long start[VAR_OPT_MAX_SEGS + 1]; int n;
};
// One launch's share: the elements [e0, e1) of E, which its table's segments hold (start[0] = e0, start[n] = e1); its workgroup
// b is workgroup c0 + b of the whole.
struct Share { long e0, e1, E; int U, c0; };

// butterfly inside each wave, then the four wave sums in index order: every thread returns the same bits
__device__ __forceinline__ float block_sum(float v, float* sm4) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sm4[0] + sm4[1]) + sm4[2]) + sm4[3];
}

// the segment that holds element k (start[0] <= k < start[n]), remembered between calls: most neighbours share one
struct Cursor {
    int s; long lo, hi;
    __device__ __forceinline__ void seek(const long* start, int n, long k) {
        if (k >= lo && k < hi) return;
        int a = 0, b = n;
        while (b - a > 1) { const int mid = (a + b) >> 1; if (start[mid] <= k) a = mid; else b = mid; }
        s = a; lo = start[a]; hi = start[a + 1];
    }
};

// A pointer that has been through LDS is a generic one to the compiler; these say that it is global memory (global_load /
// global_store, not flat_*), and a vector of four floats here is dword-aligned only.
typedef __attribute__((address_space(1))) float gfloat;
typedef f32x4 __attribute__((aligned(4))) f32x4u;
typedef __attribute__((address_space(1))) f32x4u gf32x4u;
__device__ __forceinline__ f32x4 load4(const float* p) { return *(const gf32x4u*)(uintptr_t)p; }
__device__ __forceinline__ void store4(float* p, f32x4 x) { *(gf32x4u*)(uintptr_t)p = x; }
__device__ __forceinline__ float load1(const float* p) { return *(const gfloat*)(uintptr_t)p; }
__device__ __forceinline__ void store1(float* p, float x) { *(gfloat*)(uintptr_t)p = x; }

// ---- launch 1: sums of squares ----------------------------------------------------------------------------------------------
// tick: the step count, advanced here by one thread -- stream order puts this launch behind every reader of the last call's
// Adam launch and in front of this call's.  carry_in / carry_out: a workgroup whose elements begin in an earlier launch of
// the call, or go on in a later one, takes its threads' running sums from there / leaves them there instead of its sum.
__global__ void __launch_bounds__(kT) opt_sumsq_kernel(SqTable tab, Share sh, float* __restrict__ part, const float* carry_in,
                                                       float* carry_out, int* tick) {
    __shared__ long s_start[VAR_OPT_MAX_SEGS + 1];
    __shared__ const float* s_g[VAR_OPT_MAX_SEGS];
    __shared__ float sm4[4];
    const int t = threadIdx.x;
    if (t <= tab.n) s_start[t] = tab.start[t];
    if (t < tab.n) s_g[t] = tab.g[t];
    __syncthreads();
    if (tick && blockIdx.x == 0 && t == 0) tick[0] += 1;
    const long c = (long)sh.c0 + blockIdx.x, cbeg = c * sh.U * kRound;
    const long cend = cbeg + sh.U * kRound < sh.E ? cbeg + sh.U * kRound : sh.E;
    const long lo = cbeg > sh.e0 ? cbeg : sh.e0, hi = cend < sh.e1 ? cend : sh.e1;      // what this launch holds of the workgroup's
    float acc = (carry_in && cbeg < sh.e0) ? carry_in[t] : 0.f;
    Cursor cur{0, 0, 0};
    for (int u = 0; u < sh.U; ++u) {
        const long e = cbeg + ((long)u * kT + t) * kQuad;
        if (e >= hi || e + kQuad <= lo) continue;
        if (e >= lo) cur.seek(s_start, tab.n, e);
        if (e >= lo && e + kQuad <= hi && e + kQuad <= cur.hi) {
            const f32x4 x = load4(s_g[cur.s] + (e - cur.lo));
            acc += x[0] * x[0]; acc += x[1] * x[1]; acc += x[2] * x[2]; acc += x[3] * x[3];
        } else {
            for (long k = e > lo ? e : lo; k < e + kQuad && k < hi; ++k) {
                cur.seek(s_start, tab.n, k);
                const float x = load1(s_g[cur.s] + (k - cur.lo));
                acc += x * x;
            }
        }
    }
    if (carry_out && cend > sh.e1) { carry_out[t] = acc; return; }       // (the whole workgroup: no barrier is left behind)
    const float sum = block_sum(acc, sm4);
    if (t == 0) part[c] = sum;
}

// the step count of a call that has no norm launch
__global__ void opt_tick_kernel(int* step) { if (threadIdx.x == 0 && blockIdx.x == 0) step[0] += 1; }

// ---- launch 2: clip and Adam ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT) opt_adam_kernel(AdamTable tab, Share sh, const float* __restrict__ part, int n_part, float max_norm,
                                                      const float* __restrict__ lr_dev, float b1, float b2, float eps,
                                                      const int* __restrict__ step_dev, float* total_norm_out) {
    __shared__ long s_start[VAR_OPT_MAX_SEGS + 1];
    __shared__ float* s_p[VAR_OPT_MAX_SEGS];
    __shared__ const float* s_g[VAR_OPT_MAX_SEGS];
    __shared__ float* s_m[VAR_OPT_MAX_SEGS];
    __shared__ float* s_v[VAR_OPT_MAX_SEGS];
    __shared__ float sm4[4], sh_step[2];
    const int t = threadIdx.x;
    if (t <= tab.n) s_start[t] = tab.start[t];
    if (t < tab.n) { s_p[t] = tab.p[t]; s_g[t] = tab.g[t]; s_m[t] = tab.m[t]; s_v[t] = tab.v[t]; }
    if (t == 0) {
        // as adam_pack_dev_kernel (pack_adam.hip): bias corrections in double, beta^step by repeated squaring
        auto ipow = [](double b, int e) { double r = 1.0; while (e > 0) { if (e & 1) r *= b; b *= b; e >>= 1; } return r; };
        const int step = step_dev[0];                        // (already advanced by launch 1)
        sh_step[0] = (float)((double)lr_dev[0] / (1.0 - ipow((double)b1, step)));
        sh_step[1] = (float)sqrt(1.0 - ipow((double)b2, step));
    }
    float coef = 1.f;
    if (max_norm > 0.f) {
        float a = 0.f;
        for (int i = t; i < n_part; i += kT) a += part[i];
        const float total_norm = sqrtf(block_sum(a, sm4));   // (its barriers also publish the tables above)
        const float q = max_norm / (total_norm + 1e-6f);     // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0),
        coef = q > 1.f ? 1.f : q;                            // which lets a NaN through
        if (total_norm_out && blockIdx.x == 0 && t == 0) total_norm_out[0] = total_norm;
    } else {
        __syncthreads();
    }
    const float step_size = sh_step[0], bc2_sqrt = sh_step[1];
    const long c = (long)sh.c0 + blockIdx.x, cbeg = c * sh.U * kRound;
    const long cend = cbeg + sh.U * kRound < sh.E ? cbeg + sh.U * kRound : sh.E;
    const long lo = cbeg > sh.e0 ? cbeg : sh.e0, hi = cend < sh.e1 ? cend : sh.e1;
    auto adam = [&](float pi, float g0, float mo, float vo, float& pn, float& mi, float& vi) {
        const float gi = g0 * coef;
        mi = mo + (gi - mo) * (1.f - b1);                    // exp_avg.lerp_(grad, 1 - beta1)
        vi = vo * b2 + (1.f - b2) * gi * gi;                 // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        pn = pi - step_size * (mi / denom);
    };
    Cursor cur{0, 0, 0};
    for (int u = 0; u < sh.U; ++u) {
        const long e = cbeg + ((long)u * kT + t) * kQuad;
        if (e >= hi || e + kQuad <= lo) continue;
        if (e >= lo) cur.seek(s_start, tab.n, e);
        if (e >= lo && e + kQuad <= hi && e + kQuad <= cur.hi) {
            const long o = e - cur.lo;
            const f32x4 p4 = load4(s_p[cur.s] + o), g4 = load4(s_g[cur.s] + o), m4 = load4(s_m[cur.s] + o), v4 = load4(s_v[cur.s] + o);
            f32x4 pn, mn, vn;
#pragma unroll
            for (int j = 0; j < kQuad; ++j) { float a_, b_, c_; adam(p4[j], g4[j], m4[j], v4[j], a_, b_, c_); pn[j] = a_; mn[j] = b_; vn[j] = c_; }
            store4(s_m[cur.s] + o, mn);
            store4(s_v[cur.s] + o, vn);
            store4(s_p[cur.s] + o, pn);
        } else {
            for (long k = e > lo ? e : lo; k < e + kQuad && k < hi; ++k) {
                cur.seek(s_start, tab.n, k);
                const long o = k - cur.lo;
                float pn, mn, vn;
                adam(load1(s_p[cur.s] + o), load1(s_g[cur.s] + o), load1(s_m[cur.s] + o), load1(s_v[cur.s] + o), pn, mn, vn);
                store1(s_m[cur.s] + o, mn);
                store1(s_v[cur.s] + o, vn);
                store1(s_p[cur.s] + o, pn);
            }
        }
    }
}

struct Range { uintptr_t lo, hi; int seg; char which; };

}  // namespace

extern "C" int var_clip_adam_step(var_ctx* c, void* stream, const var_opt_seg* segs, int n_seg, float max_norm, const float* lr_dev,
                                  float beta1, float beta2, float eps, int* step_dev, float* total_norm_out) {
    if (!c) return VAR_ERR_ARG;
    constexpr int kMaxTable = 256;
    if (!segs || n_seg < 1 || n_seg > kMaxTable) {
        VAR_SET_ERR(c, "var_clip_adam_step: %d segments (1..%d, table not NULL)", n_seg, kMaxTable);
        return VAR_ERR_ARG;
    }
    if (!lr_dev || !step_dev || ((uintptr_t)lr_dev & 3) || ((uintptr_t)step_dev & 3) || ((uintptr_t)total_norm_out & 3)) {
        VAR_SET_ERR(c, "var_clip_adam_step: lr_dev and step_dev must not be NULL; they and total_norm_out are 4-byte aligned");
        return VAR_ERR_ARG;
    }
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f) || max_norm != max_norm) {
        VAR_SET_ERR(c, "var_clip_adam_step: beta1 %g, beta2 %g (both in [0, 1)), eps %g (>= 0), max_norm %g (not NaN)", beta1, beta2, eps,
                    max_norm);
        return VAR_ERR_ARG;
    }
    static thread_local Range r[4 * kMaxTable + 3];
    long E = 0;
    int nr = 0;
    for (int i = 0; i < n_seg; ++i) {
        const var_opt_seg& u = segs[i];
        if (!u.p || !u.g || !u.m || !u.v || u.n < 1 || u.n > (1L << 40)) {
            VAR_SET_ERR(c, "var_clip_adam_step: segment %d: a NULL pointer or n %ld (1..2^40)", i, u.n);
            return VAR_ERR_ARG;
        }
        if (((uintptr_t)u.p | (uintptr_t)u.g | (uintptr_t)u.m | (uintptr_t)u.v) & 3) {
            VAR_SET_ERR(c, "var_clip_adam_step: segment %d: a pointer is not 4-byte aligned", i);
            return VAR_ERR_ARG;
        }
        const uintptr_t bytes = sizeof(float) * (uintptr_t)u.n;
        r[nr++] = Range{(uintptr_t)u.p, (uintptr_t)u.p + bytes, i, 'p'};
        r[nr++] = Range{(uintptr_t)u.g, (uintptr_t)u.g + bytes, i, 'g'};
        r[nr++] = Range{(uintptr_t)u.m, (uintptr_t)u.m + bytes, i, 'm'};
        r[nr++] = Range{(uintptr_t)u.v, (uintptr_t)u.v + bytes, i, 'v'};
        E += u.n;
    }
    if (E > (1L << 40)) { VAR_SET_ERR(c, "var_clip_adam_step: %ld elements in all (at most 2^40)", E); return VAR_ERR_ARG; }
    // no range of the table may overlap another (nor the scalars): sorted by start, every range ends before the next begins
    r[nr++] = Range{(uintptr_t)lr_dev, (uintptr_t)lr_dev + 4, -1, 'l'};
    r[nr++] = Range{(uintptr_t)step_dev, (uintptr_t)step_dev + 4, -1, 's'};
    if (total_norm_out) r[nr++] = Range{(uintptr_t)total_norm_out, (uintptr_t)total_norm_out + 4, -1, 't'};
    std::sort(r, r + nr, [](const Range& a, const Range& b) { return a.lo < b.lo; });
    for (int i = 0; i + 1 < nr; ++i) {
        if (r[i].hi > r[i + 1].lo) {
            VAR_SET_ERR(c, "var_clip_adam_step: %c of segment %d overlaps %c of segment %d (-1: lr_dev, step_dev, total_norm_out)", r[i].which,
                        r[i].seg, r[i + 1].which, r[i + 1].seg);
            return VAR_ERR_ARG;
        }
    }
    const int U = (int)((E + (1L << 20) - 1) >> 20);             // rounds per workgroup: ceil(E / (kOptMaxWG * kRound))
    const long C = U * kRound;
    const int n_wg = (int)((E + C - 1) / C);                     // <= kOptMaxWG
    const int n_launch = (n_seg + VAR_OPT_MAX_SEGS - 1) / VAR_OPT_MAX_SEGS;
    hipStream_t s = (hipStream_t)stream;
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    const bool clip = max_norm > 0.f;
    if (!clip) {
        hipLaunchKernelGGL(opt_tick_kernel, dim3(1), dim3(64), 0, s, step_dev);
        VAR_HIP_CHECK(c, hipGetLastError());
    }
    for (int pass = clip ? 0 : 1; pass < 2; ++pass) {            // every sum-of-squares launch before any Adam launch
        long e0 = 0;
        for (int l = 0; l < n_launch; ++l) {
            const int s0 = l * VAR_OPT_MAX_SEGS, ns = std::min(VAR_OPT_MAX_SEGS, n_seg - s0);
            SqTable sq{};
            AdamTable ad{};
            long e1 = e0;
            for (int i = 0; i < ns; ++i) {
                const var_opt_seg& u = segs[s0 + i];
                sq.g[i] = ad.g[i] = u.g; ad.p[i] = u.p; ad.m[i] = u.m; ad.v[i] = u.v;
                sq.start[i] = ad.start[i] = e1;
                e1 += u.n;
            }
            sq.start[ns] = ad.start[ns] = e1;
            sq.n = ad.n = ns;
            Share sh{e0, e1, E, U, (int)(e0 / C)};
            const int grid = (int)((e1 - 1) / C) - sh.c0 + 1;
            if (pass == 0) {
                hipLaunchKernelGGL(opt_sumsq_kernel, dim3(grid), dim3(kT), 0, s, sq, sh, c->opt_part, l > 0 ? c->opt_carry + (l - 1) * kT : nullptr,
                                   l + 1 < n_launch ? c->opt_carry + l * kT : nullptr, l == 0 ? step_dev : nullptr);
            } else {
                ProfScope prof(c, s, TAG_ADAM);
                hipLaunchKernelGGL(opt_adam_kernel, dim3(grid), dim3(kT), 0, s, ad, sh, c->opt_part, n_wg, max_norm, lr_dev, beta1, beta2, eps,
                                   step_dev, l == 0 ? total_norm_out : nullptr);
            }
            VAR_HIP_CHECK(c, hipGetLastError());
            e0 = e1;
        }
    }
    return VAR_OK;
}
