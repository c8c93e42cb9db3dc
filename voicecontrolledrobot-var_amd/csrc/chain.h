// The small-batch MLP chain of the acting path: the Linear layers + GRU step of an actor-critic (everything after its
// convolutions) as ONE persistent launch of kChainG workgroups.  Shared by the Kuka policy (armnet.hip, armNet_VAR) and the
// iTHOR policy (ithor_policy.hip, ai2thorNet_VAR); each translation unit gets its own copy (anonymous namespace).
//
// A user describes its layer DAG with ChainBuilder: stages of jobs (one Linear layer each, input kind IN_*), buffers that
// are handed over inside the launch flagged in ChainDesc::tagged, then chain_launch().  ChainDesc::sync points at a device
// block of >= 8 words, zeroed except sync[3] = 1 (the first launch's epoch); chain_status_word() reads it.
#pragma once
#include <type_traits>

#include "var_common.h"

namespace {
// ------------------------------------------------------------------------------------------------------------------
// Small batches (the RL stage's 8 envs): everything after the convolutions as ONE persistent launch.
// 22 Linear layers + the GRU step are 12 dependent stages of tiny products (8 rows x K <= 1152 x N <= 1536): as separate
// launches they cost ~4 us each whatever they compute (45 launches, 240 us of the 435-us forward).  Here kChainG workgroups
// stay resident; a stage's inputs (<= 57 KB for 8 rows) are staged into every workgroup's LDS, a wave takes blocks of four
// output features (lanes split K: coalesced 256-B reads of the weight rows in their state_dict() layout, 8 rows x 4
// outputs of partial sums per lane, a 31-shuffle butterfly leaves one (output, row) sum per lane).  Stages are NOT separated
// by a grid barrier (round 3's first form: sc1 stores drained, counter add, counter poll, sc1 loads -- four dependent trips
// through the fabric, ~8 us per stage): the handed-off vectors carry a tag, see st_pair() below.  The polls are bounded: a
// grid that is not resident sets sync[2], every workgroup stops waiting and the outputs are NaN.
// ------------------------------------------------------------------------------------------------------------------
constexpr int kChainG = 128, kChainT = 256, kChainRows = 8, kChainNB = 4;
enum { IN_PLAIN = 0, IN_SUM, IN_CAT, IN_MASK, IN_GRU };
// out2: a second, plain copy of the output (or -1); in2: IN_SUM of three vectors, (in0 + in1) + in2 (or -1)
struct ChainJob { int w, b, K, N, kind, in0, in1, cat0, out, relu, wg0, nwg, out2, in2; };
struct ChainStage { int job0, njobs; };
constexpr int kChainMaxJobs = 28, kChainMaxStages = 12, kChainBufs = 36;
struct ChainDesc {
    const float* P;
    float* buf[kChainBufs];
    ChainJob job[kChainMaxJobs];
    ChainStage stage[kChainMaxStages];
    int nstages, B, H;
    int b_hxs, b_mask, b_hout;           // buffer ids the GRU input kind needs besides in0 (gi) / in1 (gh)
    unsigned long long tagged;           // bit i: buffer i is handed over inside the launch as (value, tag) pairs
    unsigned* sync;                      // [1] finished workgroups, [2] epoch of the last timed-out launch, [3] epoch of the next launch, [4] sticky
};
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) unsigned gu32c;

// Hand-over without a barrier: every float a stage hands to a later one travels as an 8-byte (value, tag) pair written by ONE
// 64-bit sc1 store; the tag is the launch's epoch (a device counter the last workgroup of a launch bumps: captured graphs replay
// with frozen arguments).  A consumer polls its INPUT until every pair carries the epoch -- one trip through the fabric after the
// producer's store lands, instead of drain + counter add + counter poll + load (four), and a workgroup whose inputs are complete
// runs ahead of the others.  Every internal vector is written once per launch, so the epoch alone identifies it.
typedef __attribute__((address_space(1))) unsigned long long gu64c;
__device__ __forceinline__ void st_pair(float* buf, int e, float v, unsigned tag) {
    const unsigned long long q = (unsigned long long)__builtin_bit_cast(unsigned, v) | ((unsigned long long)tag << 32);
    __hip_atomic_store((gu64c*)(buf + 2 * e), q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
constexpr unsigned kChainSpinMax = 1u << 17;

__global__ void __launch_bounds__(kChainT) mlp_chain_kernel(ChainDesc D) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int dead_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = D.B, H = D.H;
    const unsigned epoch = __hip_atomic_load((gu32c*)(D.sync + 3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid == 0) dead_s = 0;
    bool alive = true;
    PHR_INIT(5, 0);
    // this workgroup's job of a stage (jobs own ranges of workgroups, sized by their weight volume)
    auto job_of = [&](int si) {
        const ChainStage S = D.stage[si];
        int q = 0;
#pragma unroll 1
        for (int t = 1; t < S.njobs; ++t) if ((int)blockIdx.x >= D.job[S.job0 + t].wg0) q = t;
        return D.job[S.job0 + q];
    };
    // The weights do not depend on the activations: the first eight k-chunks of this wave's first item of the NEXT stage (all
    // of them for every layer but the 1152-wide one) and its bias are requested before the stage's input is polled.
    // lane -> (output, row) after the butterfly: value o * 8 + r in the even lanes
    const int lidx = ((lane >> 5) & 1) * 16 + ((lane >> 4) & 1) * 8 + ((lane >> 3) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 1) & 1);
    using NB4 = std::integral_constant<int, kChainNB>;
    float pw[8][kChainNB], pbias = 0.f;
    auto load_w = [&](auto nbc, const ChainJob& J, int o0, int kc0, float (&wv)[8][kChainNB]) {
        constexpr int NB = decltype(nbc)::value;
        const float* W = D.P + J.w;
#pragma unroll
        for (int c8 = 0; c8 < 8; ++c8) {
            const int k = kc0 + c8 * 64 + lane;
#pragma unroll
            for (int o = 0; o < NB; ++o) {                                     // (unconditional, clamped: see the staging below)
                const int kk = k < J.K ? k : J.K - 1, oo = o0 + o < J.N ? o0 + o : J.N - 1;
                wv[c8][o] = W[(long)oo * J.K + kk];
            }
        }
    };
    auto prefetch = [&](const ChainJob& J) {
        const int jw = ((int)blockIdx.x - J.wg0) * (kChainT / 64) + wave;
        if (jw * kChainNB < J.N) {
            int oo;
            load_w(NB4{}, J, jw * kChainNB, 0, pw); oo = jw * kChainNB + lidx / kChainRows;
            pbias = D.P[J.b + (oo < J.N ? oo : J.N - 1)];
        }
    };
    auto give_up = [&]() {          // a producer never delivered (the grid is not resident): outputs NaN, the event is recorded
        if (*(volatile int*)&dead_s == 0) {
            __hip_atomic_store((gu32c*)(D.sync + 2), epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // which launch (chain_status_word)
            __hip_atomic_store((gu32c*)(D.sync + 4), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // sticky
        }
        dead_s = 1;
    };
    // (once one wait of this workgroup has expired every later one gives up at its first turn: a grid that is not resident costs
    //  one bound, not one per poll)
    auto expired = [&](unsigned& spins) { return ++spins > kChainSpinMax || *(volatile int*)&dead_s != 0; };
    ChainJob J = job_of(0);
    bool mine = (int)blockIdx.x < J.wg0 + J.nwg;          // a stage may leave workgroups without a job (see split())
    if (mine) prefetch(J);
    __syncthreads();
#pragma unroll 1
    for (int si = 0; si < D.nstages; ++si) {
        if (!mine) {                                      // (workgroup-uniform; nothing to wait for: stages are not fenced)
            if (si + 1 == D.nstages) break;
            J = job_of(si + 1);
            mine = (int)blockIdx.x < J.wg0 + J.nwg;
            if (mine) prefetch(J);
            continue;
        }
        PHR(0);
        const int Kp = (J.K + 63) & ~63;
        float* xs = lds;          // two input buffers: the next stage is staged while slow waves still read this one
        const bool t0 = (D.tagged >> J.in0) & 1;          // handed-off input(s) -- IN_SUM pairs and the GRU's gi / gh are always both
        // ---- the job's input -> LDS [row][Kp], zero-padded ----
        {
            const float* a = D.buf[J.in0];
            const float* b2 = J.in1 >= 0 ? D.buf[J.in1] : nullptr;
            if (J.kind == IN_GRU) {
                // torch.nn.GRU cell (gate order r, z, n) from gi (in0) and gh (in1), both handed off: the new state is this layer's
                // input.  Two hidden units per thread and turn; a rolled loop on purpose (the code runs once per stage).
                const int kq = J.K >> 1, n2 = B * kq;
#pragma unroll 1
                for (int e = tid; e < n2; e += kChainT) {
                    const int r = e / kq, k = 2 * (e - r * kq);
                    const float2 hx = *(const float2*)(D.buf[D.b_hxs] + r * H + k);
                    const float hm = D.buf[D.b_mask][r];
                    unsigned long long q[6][2];
                    unsigned spins = 0;
                    for (;;) {
#pragma unroll
                        for (int gte = 0; gte < 3; ++gte) {
                            const int el = r * 3 * H + gte * H + k;
                            q[gte][0] = __hip_atomic_load((gu64c*)(a + 2 * el), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            q[gte][1] = __hip_atomic_load((gu64c*)(a + 2 * el + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            q[3 + gte][0] = __hip_atomic_load((gu64c*)(b2 + 2 * el), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            q[3 + gte][1] = __hip_atomic_load((gu64c*)(b2 + 2 * el + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                        unsigned bad = 0u;
#pragma unroll
                        for (int g = 0; g < 6; ++g) bad |= ((unsigned)(q[g][0] >> 32) ^ epoch) | ((unsigned)(q[g][1] >> 32) ^ epoch);
                        if (bad == 0u) break;
                        if (expired(spins)) { give_up(); break; }
                        __builtin_amdgcn_s_sleep(1);
                    }
                    float2 g3[6];
#pragma unroll
                    for (int g = 0; g < 6; ++g) g3[g] = float2{__builtin_bit_cast(float, (unsigned)q[g][0]), __builtin_bit_cast(float, (unsigned)q[g][1])};
                    const float gi_[2][3] = {{g3[0].x, g3[1].x, g3[2].x}, {g3[0].y, g3[1].y, g3[2].y}};
                    const float gh_[2][3] = {{g3[3].x, g3[4].x, g3[5].x}, {g3[3].y, g3[4].y, g3[5].y}};
                    const float hh[2] = {hx.x * hm, hx.y * hm};
                    float o[2];
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2) {
                        const float rr = 1.f / (1.f + expf(-(gi_[c2][0] + gh_[c2][0])));
                        const float z = 1.f / (1.f + expf(-(gi_[c2][1] + gh_[c2][1])));
                        const float n = tanhf(gi_[c2][2] + rr * gh_[c2][2]);
                        o[c2] = (1.f - z) * n + z * hh[c2];
                    }
                    if (blockIdx.x == J.wg0) *(float2*)(D.buf[D.b_hout] + r * H + k) = float2{o[0], o[1]};       // rnn_hxs_out
                    *(float2*)(xs + r * Kp + k) = float2{o[0], o[1]};
                }
                for (int e = tid; e < (kChainRows - B) * Kp; e += kChainT) xs[B * Kp + e] = 0.f;
            } else if ((J.K & 3) == 0) {
                const int kq = J.K >> 1, n2 = kChainRows * kq;
                if (J.K != Kp) {                                                // (a K that is not a multiple of 64: zero padding)
                    const int np = Kp - J.K;
                    for (int e = tid; e < kChainRows * np; e += kChainT) xs[(e / np) * Kp + J.K + e % np] = 0.f;
                }
                if (!t0) {
                    // kernel inputs (the convolutions' output, rnn_hxs * masks): nothing to poll.  All loads first, unconditional
                    // (addresses clamped into the buffers, values selected afterwards -- a load behind a per-lane condition becomes
                    // a branch with a wait of its own)
#pragma unroll 1
                    for (int e0 = tid; e0 < n2; e0 += 8 * kChainT) {
                        float2 v[8];
                        float hm[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            int e = e0 + i * kChainT;
                            e = e < n2 ? e : n2 - 1;
                            int r = e / kq;
                            const int k = 2 * (e - r * kq);
                            r = r < B ? r : B - 1;
                            v[i] = *(const float2*)(a + r * J.K + k);
                            hm[i] = J.kind == IN_MASK ? b2[r] : 1.f;
                        }
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const int e = e0 + i * kChainT;
                            if (e >= n2) continue;
                            const int r = e / kq, k = 2 * (e - r * kq);
                            *(float2*)(xs + r * Kp + k) = r < B ? float2{v[i].x * hm[i], v[i].y * hm[i]} : float2{0.f, 0.f};
                        }
                    }
                } else {
                    // handed-off vectors ((value, tag) pairs; IN_SUM: two of them): a turn = 8 element pairs per thread, ALL of its
                    // 64-bit atomic loads issued back to back (hipcc keeps atomic loads in program order, so anything between two of
                    // them -- a tag compare, a branch -- makes every pair wait for the previous one), then the tags are checked; a
                    // turn that is not complete yet is simply taken again
                    const bool sum = J.kind == IN_SUM;
#pragma unroll 1
                    for (int e0 = tid; e0 < n2; e0 += 8 * kChainT) {
                        unsigned long long qa[8][2], qb[8][2];
                        int el[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            int e = e0 + i * kChainT;
                            e = e < n2 ? e : n2 - 1;
                            el[i] = 2 * e;                                    // (rows beyond the batch are handed over too)
                        }
                        unsigned spins = 0;
                        for (;;) {
#pragma unroll
                            for (int i = 0; i < 8; ++i) {
                                qa[i][0] = __hip_atomic_load((gu64c*)(a + 2 * el[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                qa[i][1] = __hip_atomic_load((gu64c*)(a + 2 * el[i] + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                            if (sum) {
#pragma unroll
                                for (int i = 0; i < 8; ++i) {
                                    qb[i][0] = __hip_atomic_load((gu64c*)(b2 + 2 * el[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    qb[i][1] = __hip_atomic_load((gu64c*)(b2 + 2 * el[i] + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                }
                            } else {
#pragma unroll
                                for (int i = 0; i < 8; ++i) qb[i][0] = qb[i][1] = (unsigned long long)epoch << 32;      // value 0.f, tag ok
                            }
                            unsigned bad = 0u;
#pragma unroll
                            for (int i = 0; i < 8; ++i)
                                bad |= ((unsigned)(qa[i][0] >> 32) ^ epoch) | ((unsigned)(qa[i][1] >> 32) ^ epoch) |
                                       ((unsigned)(qb[i][0] >> 32) ^ epoch) | ((unsigned)(qb[i][1] >> 32) ^ epoch);
                            if (bad == 0u) break;
                            if (expired(spins)) { give_up(); break; }
                            __builtin_amdgcn_s_sleep(1);
                        }
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const int e = e0 + i * kChainT;
                            if (e >= n2) continue;
                            const int r = e / kq, k = 2 * (e - r * kq);
                            float2 o = float2{__builtin_bit_cast(float, (unsigned)qa[i][0]) + __builtin_bit_cast(float, (unsigned)qb[i][0]),
                                              __builtin_bit_cast(float, (unsigned)qa[i][1]) + __builtin_bit_cast(float, (unsigned)qb[i][1])};
                            if (r >= B) o = float2{0.f, 0.f};
                            *(float2*)(xs + r * Kp + k) = o;
                        }
                    }
                    if (J.in2 >= 0) {
                        // a third handed-off summand, added to the pair sum above (the same elements of the same thread: no barrier)
                        const float* c2 = D.buf[J.in2];
#pragma unroll 1
                        for (int e0 = tid; e0 < n2; e0 += 8 * kChainT) {
                            unsigned long long qc[8][2];
                            int el[8];
#pragma unroll
                            for (int i = 0; i < 8; ++i) {
                                int e = e0 + i * kChainT;
                                e = e < n2 ? e : n2 - 1;
                                el[i] = 2 * e;
                            }
                            unsigned spins = 0;
                            for (;;) {
#pragma unroll
                                for (int i = 0; i < 8; ++i) {
                                    qc[i][0] = __hip_atomic_load((gu64c*)(c2 + 2 * el[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    qc[i][1] = __hip_atomic_load((gu64c*)(c2 + 2 * el[i] + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                }
                                unsigned bad = 0u;
#pragma unroll
                                for (int i = 0; i < 8; ++i) bad |= ((unsigned)(qc[i][0] >> 32) ^ epoch) | ((unsigned)(qc[i][1] >> 32) ^ epoch);
                                if (bad == 0u) break;
                                if (expired(spins)) { give_up(); break; }
                                __builtin_amdgcn_s_sleep(1);
                            }
#pragma unroll
                            for (int i = 0; i < 8; ++i) {
                                const int e = e0 + i * kChainT;
                                if (e >= n2) continue;
                                const int r = e / kq, k = 2 * (e - r * kq);
                                if (r >= B) continue;
                                float2* d = (float2*)(xs + r * Kp + k);
                                *d = float2{d->x + __builtin_bit_cast(float, (unsigned)qc[i][0]), d->y + __builtin_bit_cast(float, (unsigned)qc[i][1])};
                            }
                        }
                    }
                }
            } else {                                                            // the two tiny first layers (K = 5: [image_feat | robot_pose], K = 3): kernel inputs
                for (int e = tid; e < kChainRows * Kp; e += kChainT) {
                    const int r = e / Kp, k = e - r * Kp;
                    float v = 0.f;
                    if (r < B && k < J.K) {
                        if (J.kind == IN_CAT) v = k < J.cat0 ? a[r * J.cat0 + k] : b2[r * (J.K - J.cat0) + k - J.cat0];
                        else v = a[r * J.K + k];
                    }
                    xs[e] = v;
                }
            }
        }
        PHR(1);
        __syncthreads();
        alive = alive && dead_s == 0;
        PHR(2);
        // ---- items: blocks of kChainNB outputs, dealt to the waves of the job's workgroups.  (Blocks of ONE output where a job has a
        //      wave per output -- a quarter of the serial work per wave -- measured: 97.5 vs 94.5 us for the chain, the second
        //      instantiation's code does not pay for itself) ----
        auto items = [&](auto nbc) {
            constexpr int NB = decltype(nbc)::value;
            const int jw = ((int)blockIdx.x - J.wg0) * (kChainT / 64) + wave, jnw = J.nwg * (kChainT / 64);
            const int nitems = (J.N + NB - 1) / NB;
            const bool tout = (D.tagged >> J.out) & 1;
            bool first = true;
#pragma unroll 1
            for (int it = jw; it < nitems; it += jnw) {
                const int o0 = it * NB;
                float acc[NB][kChainRows];
#pragma unroll
                for (int o = 0; o < NB; ++o)
#pragma unroll
                    for (int r = 0; r < kChainRows; ++r) acc[o][r] = 0.f;
                float bias = pbias;
                if (!first) { const int oo = NB == 1 ? o0 : o0 + lidx / kChainRows; bias = D.P[J.b + (oo < J.N ? oo : J.N - 1)]; }
                // weight rows stream from HBM: eight k-chunks in flight per wave
#pragma unroll 1
                for (int kc0 = 0; kc0 < Kp; kc0 += 8 * 64) {
                    float wv[8][kChainNB];
                    if (first && kc0 == 0) {
#pragma unroll
                        for (int c8 = 0; c8 < 8; ++c8)
#pragma unroll
                            for (int o = 0; o < NB; ++o) wv[c8][o] = pw[c8][o];
                    } else load_w(nbc, J, o0, kc0, wv);
#pragma unroll
                    for (int c8 = 0; c8 < 8; ++c8) {
                        const int k = kc0 + c8 * 64 + lane;
                        if (kc0 + c8 * 64 < Kp) {
#pragma unroll
                            for (int r = 0; r < kChainRows; ++r) {
                                const float xv = xs[r * Kp + k];
#pragma unroll
                                for (int o = 0; o < NB; ++o) acc[o][r] = fmaf(wv[c8][o], xv, acc[o][r]);      // (padding k: xv == 0)
                            }
                        }
                    }
                }
                // butterfly over the 64 lanes: NB x 8 values -> one (output, row) sum per lane
                float v[NB * kChainRows];
#pragma unroll
                for (int o = 0; o < NB; ++o)
#pragma unroll
                    for (int r = 0; r < kChainRows; ++r) v[o * kChainRows + r] = acc[o][r];
                // (each step with compile-time constants: a loop over (half, bit) is not unrolled by hipcc, and the array then
                //  becomes 32-way select chains -- 6 K instructions.)  The two wide steps are gfx950's lane-swap instructions
                //  (v_permlane32_swap: lanes 32-63 of one register <-> lanes 0-31 of the other, v_permlane16_swap the same for the odd /
                //  even 16-lane rows): a step is one swap + one add per pair instead of two selects + a ds_bpermute + an add; xor 8 / 2 / 1
                //  are DPP moves (row_ror:8, quad_perm); only the two xor-4 exchanges go through the LDS crossbar.
                const auto fb = [](float x) { return __builtin_bit_cast(unsigned, x); };
                const auto bf = [](unsigned x) { return __builtin_bit_cast(float, x); };
#pragma unroll
                for (int i = 0; i < 16; ++i) { const auto q = __builtin_amdgcn_permlane32_swap(fb(v[i]), fb(v[i + 16]), false, false); v[i] = bf(q[0]) + bf(q[1]); }
#pragma unroll
                for (int i = 0; i < 8; ++i) { const auto q = __builtin_amdgcn_permlane16_swap(fb(v[i]), fb(v[i + 8]), false, false); v[i] = bf(q[0]) + bf(q[1]); }
#define CHAIN_FOLD(HALF, BIT, XCHG)                                                                   \
                {                                                                                     \
                    const bool up = (lane & (BIT)) != 0;                                              \
                    _Pragma("unroll") for (int i = 0; i < (HALF); ++i) {                             \
                        const float keep = up ? v[i + (HALF)] : v[i], give = up ? v[i] : v[i + (HALF)]; \
                        v[i] = keep + XCHG(give);                                                     \
                    }                                                                                 \
                }
#define X_ROR8(x) bf((unsigned)__builtin_amdgcn_update_dpp(0, (int)fb(x), 0x128, 0xf, 0xf, false))
#define X_XOR4(x) __shfl_xor(x, 4, 64)
#define X_XOR2(x) bf((unsigned)__builtin_amdgcn_update_dpp(0, (int)fb(x), 0x4e, 0xf, 0xf, false))
#define X_XOR1(x) bf((unsigned)__builtin_amdgcn_update_dpp(0, (int)fb(x), 0xb1, 0xf, 0xf, false))
                CHAIN_FOLD(4, 8, X_ROR8) CHAIN_FOLD(2, 4, X_XOR4) CHAIN_FOLD(1, 2, X_XOR2)
                float sum;
                int o, r;
                bool writer;
                sum = v[0] + X_XOR1(v[0]);
                o = lidx / kChainRows; r = lidx % kChainRows; writer = (lane & 1) == 0;
#undef X_ROR8
#undef X_XOR4
#undef X_XOR2
#undef X_XOR1
#undef CHAIN_FOLD
                first = false;
                if (writer && o0 + o < J.N) {
                    float y = sum + bias;
                    if (J.relu) y = fmaxf(y, 0.f);
                    if (!alive) y = __builtin_nanf("");
                    // rows beyond the batch are handed over too (zeros in, bias out): a consumer polls whole vectors
                    if (tout) st_pair(D.buf[J.out], r * J.N + o0 + o, y, epoch);
                    else if (r < B) D.buf[J.out][r * J.N + o0 + o] = y;
                    if (J.out2 >= 0 && r < B) D.buf[J.out2][r * J.N + o0 + o] = y;
                }
            }
        };
        items(NB4{});
        PHR(3);
        if (si + 1 == D.nstages) break;
        J = job_of(si + 1);
        mine = (int)blockIdx.x < J.wg0 + J.nwg;
        if (mine) prefetch(J);                                      // (in flight while the next input is polled)
        __syncthreads();
        PHR(4);
    }
    PHR_FLUSH();
    // the last workgroup to finish opens the next launch's epoch (its stores are drained first: nothing of this launch can
    // carry the new tag)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned d = __hip_atomic_fetch_add((gu32c*)(D.sync + 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (d == gridDim.x - 1) {
            __hip_atomic_store((gu32c*)(D.sync + 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store((gu32c*)(D.sync + 3), epoch + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- host side: stages / jobs / workgroup ranges, the launch, the status word ----
struct ChainBuilder {
    ChainDesc& D;
    int nj = 0, ns = 0;
    long lds_max = 0;
    explicit ChainBuilder(ChainDesc& d) : D(d) {}
    void stage() { D.stage[ns].job0 = nj; D.stage[ns].njobs = 0; ++ns; }
    // a Linear layer (weight at w, bias at b in the parameter arena, K inputs, N outputs) of the current stage
    void job(int w, int b, int K, int N, int kind, int in0, int in1, int cat0, int out, int relu, int out2 = -1, int in2 = -1) {
        if (nj < kChainMaxJobs) D.job[nj] = ChainJob{w, b, K, N, kind, in0, in1, cat0, out, relu, 0, 0, out2, in2};
        D.stage[ns - 1].njobs++;
        nj++;
        const long lds_cur = (long)kChainRows * ((K + 63) & ~63);       // a workgroup stages the input of ITS job only
        if (lds_cur > lds_max) lds_max = lds_cur;
    }
    bool overflow() const { return ns > kChainMaxStages || nj > kChainMaxJobs; }
    // Workgroup ranges of a stage's jobs.  What a stage costs is its slowest wave's chain of dependent weight fetches (a block
    // of outputs = ceil(K / 512) batches of loads, ~2 us each from HBM; only a wave's first batch is requested ahead), NOT its
    // weight volume: sized by volume, the two tiny first layers (K = 5 and 3) got one workgroup each and their 64 / 32 blocks
    // took 35 us, a third of the whole chain, behind which everything else waited.  Greedy: every job starts with one
    // workgroup, the job with the longest per-wave chain gets the next one.
    void split() {
        if (overflow()) return;
        ChainStage& S = D.stage[ns - 1];
        auto chain_len = [&](const ChainJob& J, int nwg) {
            const int blocks = (J.N + kChainNB - 1) / kChainNB, waves = nwg * (kChainT / 64);
            return ((blocks + waves - 1) / waves) * ((J.K + 511) / 512);
        };
        int nwg[kChainMaxJobs] = {0};
        for (int q = 0; q < S.njobs; ++q) nwg[q] = 1;
        // (a job is never given more waves than it has blocks: an extra workgroup would only poll and stage the input once more
        //  -- the GRU stage's 196 KB per workgroup -- and the leftover workgroups skip the stage)
        auto full = [&](int q) { return nwg[q] * (kChainT / 64) >= (D.job[S.job0 + q].N + kChainNB - 1) / kChainNB; };
        for (int left = kChainG - S.njobs; left > 0; --left) {
            bool any = false;
            for (int q = 0; q < S.njobs; ++q) any = any || !full(q);
            if (!any) break;
            int worst = -1;
            for (int q = 0; q < S.njobs; ++q) {
                if (full(q)) continue;
                if (worst < 0) { worst = q; continue; }
                const int cq = chain_len(D.job[S.job0 + q], nwg[q]), cw = chain_len(D.job[S.job0 + worst], nwg[worst]);
                // ties: the job with more weight per workgroup (bandwidth is the second-order cost)
                if (cq > cw || (cq == cw && (double)D.job[S.job0 + q].K * D.job[S.job0 + q].N / nwg[q] >
                                                (double)D.job[S.job0 + worst].K * D.job[S.job0 + worst].N / nwg[worst])) worst = q;
            }
            ++nwg[worst];
        }
        int wg0 = 0;
        for (int q = 0; q < S.njobs; ++q) {
            ChainJob& J = D.job[S.job0 + q];
            J.wg0 = wg0; J.nwg = nwg[q];
            wg0 += nwg[q];
        }
    }
};

// grid: kChainG (fewer only to test the bounded waits)
inline int chain_launch(var_ctx* c, hipStream_t s, const ChainDesc& D, long lds_floats, int grid) {
    static unsigned attr = 0;      // bit d: set on device d (function attributes are per device)
    if (!(attr & var_dev_bit(c))) {
        VAR_HIP_CHECK(c, hipFuncSetAttribute((const void*)mlp_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        attr |= var_dev_bit(c);
    }
    hipLaunchKernelGGL(mlp_chain_kernel, dim3(grid), dim3(kChainT), (int)lds_floats * 4, s, D);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}

// 1 = the most recent launch timed out (its outputs are NaN), 0x40000001 = an earlier one did since the last clear, 0 = never.
// Blocking: behind the work already enqueued.
inline int chain_status_word(var_ctx* c, const unsigned* sync, unsigned* word) {
    unsigned w[8] = {0};
    VAR_HIP_CHECK(c, hipMemcpy(w, sync, sizeof(w), hipMemcpyDeviceToHost));
    // w[2]: epoch of the last launch whose waits expired; w[3]: epoch of the NEXT launch, so w[3] - 1 ran last
    *word = (w[2] != 0u && w[2] == w[3] - 1u) ? 1u : (w[4] ? 0x40000001u : 0u);
    return VAR_OK;
}
inline int chain_clear_status(var_ctx* c, unsigned* sync) {
    VAR_HIP_CHECK(c, hipDeviceSynchronize());
    const unsigned z = 0u;
    VAR_HIP_CHECK(c, hipMemcpy(sync + 2, &z, sizeof(z), hipMemcpyHostToDevice));
    VAR_HIP_CHECK(c, hipMemcpy(sync + 4, &z, sizeof(z), hipMemcpyHostToDevice));
    return VAR_OK;
}
}  // namespace
