// The distribution tail of Policy.act (models/ppo/model.py:59-69) as ONE launch: DiagGaussian / Categorical sampling or mode,
// the log-probability of the chosen action (models/ppo/distributions.py:7-33, 60-84), the noise from a counter-based generator
// whose step lives on the device, and the copy that carries the recurrent state into the next step's input buffer.
// Latency work: at the RL stage's 8 envs it is one workgroup; what it replaces is about a dozen torch launches on (B,2) / (B,n).
#include "var_common.h"

namespace {

constexpr int kDistThreads = 256;
constexpr int kMaxGauss = 4, kMaxCat = 16;

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter {c0..c3}, key {k0, k1}.
struct Philox4 { unsigned x[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// u = ((x >> 8) + 0.5) * 2^-24 in fp32.  The sum is exact below 2^23 and rounds to even above (the largest word gives 1.0f, the
// smallest 2^-25): ln u is finite and <= 0, and the inverse CDF below never counts past n - 1.
__device__ __forceinline__ float uniform24(unsigned x) { return ((float)(x >> 8) + 0.5f) * 0x1p-24f; }

__device__ __forceinline__ void box_muller(unsigned xa, unsigned xb, float& z0, float& z1) {
    const float r = sqrtf(-2.f * logf(uniform24(xa))), t = 6.283185307179586f * uniform24(xb);
    z0 = r * cosf(t); z1 = r * sinf(t);
}

// One thread per row; rows over workgroups.  The carry is a grid-stride copy behind the rows' work (16-byte pieces when both
// ends are aligned).  Generator: every row thread reads {key0, key1, step_lo, step_hi}; the LAST workgroup to arrive (ticket
// counter as rw_tail_kernel's, csrc/ithor_reward.hip: an atomicAdd, no spinning, no wait on another workgroup) stores step + 1
// -- every other workgroup has consumed the words before it took its ticket.  A launch of one workgroup needs no ticket.
template <int KIND>
__global__ void __launch_bounds__(kDistThreads) policy_dist_kernel(const float* __restrict__ head, const float* __restrict__ logstd, int n, int B,
                                                                 int deterministic, const float* __restrict__ noise_in,
                                                                 unsigned* rng_state, unsigned* ticket, float* __restrict__ noise_out,
                                                                 void* __restrict__ action, float* __restrict__ logp,
                                                                 const float* __restrict__ hxs_src, float* __restrict__ hxs_dst,
                                                                 long hxs_n, int hxs_vec) {
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * kDistThreads + tid;
    const bool draw = !deterministic && !noise_in;             // the built-in generator is in use
    if (row < B) {
        Philox4 w{{0u, 0u, 0u, 0u}};
        if (draw) w = philox4x32_10(rng_state[2], rng_state[3], (unsigned)row, 0u, rng_state[0], rng_state[1]);
        if (KIND == 0) {
            float z[kMaxGauss] = {0.f, 0.f, 0.f, 0.f};
            if (draw) { box_muller(w.x[0], w.x[1], z[0], z[1]); box_muller(w.x[2], w.x[3], z[2], z[3]); }
            float lp = 0.f;
#pragma unroll
            for (int d = 0; d < kMaxGauss; ++d) {
                if (d < n) {
                    const float mean = head[row * n + d], ls = logstd[d], sd = expf(ls);
                    if (!deterministic && noise_in) z[d] = noise_in[row * n + d];
                    const float a = deterministic ? mean : mean + sd * z[d];
                    const float diff = a - mean;
                    lp += -(diff * diff) / (2.f * (sd * sd)) - ls - 0.9189385332046727f;
                    ((float*)action)[row * n + d] = a;
                    if (noise_out && !deterministic) noise_out[row * n + d] = z[d];
                }
            }
            logp[row] = lp;
        } else {
            float l[kMaxCat];
            float mx = head[row * n];
            int arg = 0;
#pragma unroll
            for (int k = 0; k < kMaxCat; ++k) {
                l[k] = k < n ? head[row * n + k] : 0.f;
                if (k > 0 && k < n && l[k] > mx) { mx = l[k]; arg = k; }      // strict: the FIRST index of the maximum
            }
            float e[kMaxCat], sum = 0.f;
#pragma unroll
            for (int k = 0; k < kMaxCat; ++k) { e[k] = k < n ? expf(l[k] - mx) : 0.f; sum += e[k]; }
            int a = arg;
            if (!deterministic) {
                const float u = noise_in ? noise_in[row] : uniform24(w.x[0]);
                float cdf = 0.f;
                a = 0;
#pragma unroll
                for (int k = 0; k < kMaxCat - 1; ++k) { cdf += e[k] / sum; a += (k < n - 1 && cdf <= u) ? 1 : 0; }
                if (noise_out) noise_out[row] = u;
            }
            float la = l[0];
#pragma unroll
            for (int k = 1; k < kMaxCat; ++k) la = k == a ? l[k] : la;
            ((long long*)action)[row] = (long long)a;
            logp[row] = (la - mx) - logf(sum);
        }
    }
    if (hxs_src) {
        const long stride = (long)gridDim.x * kDistThreads, i0 = (long)blockIdx.x * kDistThreads + tid;
        const long n4 = hxs_vec ? hxs_n / 4 : 0;
        for (long i = i0; i < n4; i += stride) ((float4*)hxs_dst)[i] = ((const float4*)hxs_src)[i];
        for (long i = 4 * n4 + i0; i < hxs_n; i += stride) hxs_dst[i] = hxs_src[i];
    }
    if (!draw) return;
    if (gridDim.x > 1) {
        __shared__ int last_s;
        __syncthreads();                                       // (every row thread of this workgroup has its generator words)
        if (tid == 0) {
            last_s = atomicAdd(ticket, 1u) == gridDim.x - 1;
            if (last_s) atomicExch(ticket, 0u);
        }
        __syncthreads();
        if (!last_s) return;
    } else {
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned lo = rng_state[2] + 1u;
        rng_state[2] = lo;
        if (lo == 0u) rng_state[3] = rng_state[3] + 1u;
    }
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *p = (const char*)a, *q = (const char*)b;
    return p < q + nb && q < p + na;
}

}  // namespace

extern "C" int var_policy_dist(var_ctx* c, void* stream, int kind, const float* head, const float* logstd, int n, int B,
                               int deterministic, const float* noise_in, unsigned* rng_state, float* noise_out, void* action,
                               float* logp, const float* hxs_src, float* hxs_dst, int hidden) {
    if (!c) return VAR_ERR_ARG;
    if (kind != 0 && kind != 1) { VAR_SET_ERR(c, "var_policy_dist: kind %d (0 DiagGaussian, 1 Categorical)", kind); return VAR_ERR_ARG; }
    if (B < 1) { VAR_SET_ERR(c, "var_policy_dist: B %d < 1", B); return VAR_ERR_ARG; }
    const int nmax = kind == 0 ? kMaxGauss : kMaxCat;
    if (n < 1 || n > nmax) { VAR_SET_ERR(c, "var_policy_dist: n %d outside 1..%d", n, nmax); return VAR_ERR_ARG; }
    if (!head || !action || !logp || (kind == 0 && !logstd)) {
        VAR_SET_ERR(c, "var_policy_dist: head, action, logp%s must not be NULL", kind == 0 ? ", logstd" : "");
        return VAR_ERR_ARG;
    }
    if (!deterministic && !noise_in && !rng_state) {
        VAR_SET_ERR(c, "var_policy_dist: sampling needs noise_in or rng_state");
        return VAR_ERR_ARG;
    }
    if (hxs_src) {
        if (!hxs_dst || hidden < 1) { VAR_SET_ERR(c, "var_policy_dist: hxs_src without hxs_dst / hidden"); return VAR_ERR_ARG; }
        const size_t bytes = sizeof(float) * (size_t)B * (size_t)hidden;
        if (overlap(hxs_src, bytes, hxs_dst, bytes)) { VAR_SET_ERR(c, "var_policy_dist: hxs_dst overlaps hxs_src"); return VAR_ERR_ARG; }
    }
    VAR_HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const long hxs_n = hxs_src ? (long)B * hidden : 0;
    const int hxs_vec = hxs_src && (((uintptr_t)hxs_src | (uintptr_t)hxs_dst) & 15) == 0;
    // rows decide the grid; a long carry (large B) gets up to 8 pieces of 16 bytes per thread before the grid-stride loop turns
    long wg = ((long)B + kDistThreads - 1) / kDistThreads;
    long copy_wg = (hxs_n / 4 + 8L * kDistThreads - 1) / (8L * kDistThreads);
    if (copy_wg > 1024) copy_wg = 1024;
    if (copy_wg > wg) wg = copy_wg;
    unsigned* ticket = c->dist_ctr;                            // zero since var_init; the last workgroup of a launch re-zeroes it
    auto kern = kind == 0 ? policy_dist_kernel<0> : policy_dist_kernel<1>;
    hipLaunchKernelGGL(kern, dim3((unsigned)wg), dim3(kDistThreads), 0, s, head, logstd, n, B, deterministic, noise_in, rng_state, ticket,
                       noise_out, action, logp, hxs_src, hxs_dst, hxs_n, hxs_vec);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}
