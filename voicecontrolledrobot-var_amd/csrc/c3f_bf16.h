// The band convolutions of c3f.h (3x3 / stride 1 / pad 1 + bias + ReLU (+ 2x2 max pool), small batches) on
// v_mfma_f32_16x16x32_bf16: the acting forwards' bf16 mode (include/var_hip.h, var_*_forward_ex flags bit 0), conv 2..6 of
// armNet_VAR / conv 2..5 of ai2thorNet_VAR.  Semantics: relu(conv(bf16(x), bf16(w)) + b), operands rounded to nearest even,
// products accumulated in fp32, bias / ReLU / pool in fp32, fp32 NCHW in and out.  Same decomposition as c3f_kernel -- a workgroup
// owns a band of TR rows of one image and 16 * NCBW output channels, A = filter, B = 16 consecutive pixels, D[channel 4 (lane >> 4)
// + r][pixel lane & 15], so the epilogue and the pool tile are c3f_kernel's -- with
//   * the band rounded as it is written to LDS into a channel-innermost bf16 image: [plane of 8 channels][row][W + 2 slots of 16
//     bytes] (slot 0 and slot W + 1 of a row: the zero halo; rows outside the image: zeros selected at the LDS write), so a B
//     fragment (pixel lane & 15, channels 8 (lane >> 4) .. + 7 of a 32-channel group) is ONE ds_read_b128 and a tap an immediate
//     offset; the 16 lanes of a quarter wave read 16 consecutive slots (256 contiguous bytes) wherever a row does not end inside
//     the block;
//   * K = 32 input channels of one tap per matrix instruction: an eighth of c3f_kernel's matrix instructions, half its LDS;
//   * the filter packed by pack_item's bf16 form (16 bytes = the A fragment of one instruction: output channel lane & 15, input
//     channels 8 (lane >> 4) .. + 7) inside conv 1's launch, travelling through LDS in 32-channel chunks beside the band's;
//   * c3f_kernel's pipeline: chunk kg + 1 in registers during the products of chunk kg, written to LDS between queued matrix
//     instructions, an LDS-only barrier per chunk.
#pragma once
#include "c3f.h"

namespace c3f {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <int CIN_, int COUT_, int H_, int TR_, int NCBW_, int WCB_, bool POOL_>
struct CfgB {
    static constexpr int CIN = CIN_, COUT = COUT_, H = H_, W = H_, TR = TR_, NCBW = NCBW_, WCB = WCB_;
    static constexpr bool POOL = POOL_;
    static constexpr int PWS = W + 2, ROWS = TR + 2;                    // slots of a row: pixel x sits at slot x + 1
    static constexpr int PLANE = ROWS * PWS;                            // slots of one 8-channel plane
    static constexpr int NPX = TR * W, PBT = NPX / 16;                  // pixel blocks of the band
    static constexpr int WPB = 4 / WCB;                                 // waves along the pixel blocks
    static constexpr int NPB = (PBT + WPB - 1) / WPB, NCB = NCBW / WCB;
    static constexpr int KG = CIN / 32;                                 // 32-channel chunks = outer steps of the product loop
    static constexpr int BAND = (CIN / 8) * PLANE * 4;                  // floats (a slot is four of them)
    static constexpr int OP = NPX + 4;                                  // pool tile pitch: 4 (mod 8)
    static constexpr int OUTT = POOL ? 16 * NCBW * OP : 0;
    static constexpr int ASLOTS = NCBW * 9 * 64;                        // 16-byte A fragments of one 32-channel filter chunk
    static constexpr int BOT = BAND > OUTT ? BAND : OUTT;               // band, later the pool tile
    static constexpr int NBUF = KG > 1 ? 2 : 1;
    static constexpr int LDSF = BOT + NBUF * ASLOTS * 4;                // + the filter chunks (double buffer)
    static constexpr int BANDS = H / TR, CBG = COUT / (16 * NCBW);
    static_assert(CIN % 32 == 0 && COUT % (16 * NCBW) == 0 && H % TR == 0 && NPX % 16 == 0 && W % 4 == 0, "c3b shape");
    static_assert(NCBW % WCB == 0 && 4 % WCB == 0 && (!POOL || TR % 2 == 0), "c3b wave split");
    static_assert(LDSF * 4 <= 160 * 1024, "c3b LDS");
    static_assert((2 * PWS + 2) * 16 < 65536, "ds_read immediate offset");
};

template <class C>
__global__ void __launch_bounds__(256) c3b_kernel(const float* __restrict__ x, const u32x4* __restrict__ wp, const float* __restrict__ bias,
                                                 float* __restrict__ y, int B) {
    constexpr int CIN = C::CIN, COUT = C::COUT, H = C::H, W = C::W, TR = C::TR, PWS = C::PWS, ROWS = C::ROWS, PLANE = C::PLANE;
    constexpr int NPB = C::NPB, NCB = C::NCB, KG = C::KG, PBT = C::PBT;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    u32x4* band = (u32x4*)lds;
    u32x4* aw = (u32x4*)(lds + C::BOT);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lk = lane >> 4;
    const int tile = blockIdx.x % (B * C::BANDS), cbg = blockIdx.x / (B * C::BANDS);
    const int b = tile / C::BANDS, r0 = (tile - b * C::BANDS) * TR;
    const int wc = wave % C::WCB, wpb = wave / C::WCB;
    const int cb0 = cbg * C::NCBW + wc * NCB;                      // first 16-channel block of this wave

    // ---- stage the band: rows r0 - 1 .. r0 + TR, in chunks of 32 input channels (= one outer step of the product loop).  A unit
    //      = (plane of 8 channels, band row, four pixels): eight 16-byte loads (one per channel), four 16-byte slots.
    constexpr int Q = W / 4, CUNITS = 4 * ROWS * Q, NLD = (CUNITS + 255) / 256;
    constexpr int ASLOTS = C::ASLOTS, NLA = (ASLOTS + 255) / 256;
    const float* xb = x + (size_t)b * CIN * H * W;
    float4 sv[NLD][8];
    u32x4 sa[NLA];
    auto issue = [&](int kg) {
#pragma unroll
        for (int u = 0; u < NLA; ++u) {
            int e = tid + 256 * u;
            e = e < ASLOTS ? e : ASLOTS - 1;
            const int cbl = e / 576, rem = e - cbl * 576;
            sa[u] = wp[((size_t)(cbg * C::NCBW + cbl) * KG + kg) * 576 + rem];
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            int e = tid + 256 * u;
            e = e < CUNITS ? e : CUNITS - 1;
            const int sp = e / (ROWS * Q), rem = e - sp * (ROWS * Q), br = rem / Q, q = rem - br * Q;
            const int ir = r0 - 1 + br, irc = ir < 0 ? 0 : (ir >= H ? H - 1 : ir);
            const float* src = xb + ((size_t)(32 * kg + 8 * sp) * H + irc) * W + 4 * q;      // rows outside the image: zeroed in commit()
#pragma unroll
            for (int j = 0; j < 8; ++j) sv[u][j] = *(const float4*)(src + (size_t)j * H * W);
        }
    };
    auto commit = [&](int kg) {
#pragma unroll
        for (int u = 0; u < NLA; ++u) {
            const int e = tid + 256 * u;
            if (e < ASLOTS) aw[(kg & 1) * ASLOTS + e] = sa[u];
        }
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int e = tid + 256 * u;
            if (e < CUNITS) {
                const int sp = e / (ROWS * Q), rem = e - sp * (ROWS * Q), br = rem / Q, q = rem - br * Q;
                const int ir = r0 - 1 + br;
                const bool out = ir < 0 || ir >= H;
                u32x4* dst = band + (4 * kg + sp) * PLANE + br * PWS + 1 + 4 * q;
                const float4* v = sv[u];
                dst[0] = out ? u32x4{0u, 0u, 0u, 0u} : u32x4{pack_bf16(v[0].x, v[1].x), pack_bf16(v[2].x, v[3].x), pack_bf16(v[4].x, v[5].x), pack_bf16(v[6].x, v[7].x)};
                dst[1] = out ? u32x4{0u, 0u, 0u, 0u} : u32x4{pack_bf16(v[0].y, v[1].y), pack_bf16(v[2].y, v[3].y), pack_bf16(v[4].y, v[5].y), pack_bf16(v[6].y, v[7].y)};
                dst[2] = out ? u32x4{0u, 0u, 0u, 0u} : u32x4{pack_bf16(v[0].z, v[1].z), pack_bf16(v[2].z, v[3].z), pack_bf16(v[4].z, v[5].z), pack_bf16(v[6].z, v[7].z)};
                dst[3] = out ? u32x4{0u, 0u, 0u, 0u} : u32x4{pack_bf16(v[0].w, v[1].w), pack_bf16(v[2].w, v[3].w), pack_bf16(v[4].w, v[5].w), pack_bf16(v[6].w, v[7].w)};
            }
        }
    };
    issue(0);
    for (int e = tid; e < (CIN / 8) * ROWS; e += 256) {            // halo slots x = -1 and x = W of every row of every plane
        band[e * PWS] = u32x4{0u, 0u, 0u, 0u};
        band[e * PWS + W + 1] = u32x4{0u, 0u, 0u, 0u};
    }
    commit(0);
    if (KG > 1) issue(1);
    __builtin_amdgcn_sched_barrier(0);
    // lane constants: the slot of this lane's pixel of each block at tap (0, 0) (row-major over TR x W), in its plane of the chunk
    int va[NPB];
#pragma unroll
    for (int i = 0; i < NPB; ++i) {
        int pb = wpb * NPB + i;
        pb = pb < PBT ? pb : PBT - 1;
        const int p = pb * 16 + l15, row = p / W, col = p - row * W;
        va[i] = lk * PLANE + row * PWS + col;
    }
    f32x4 acc[NPB][NCB];
#pragma unroll
    for (int i = 0; i < NPB; ++i)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[i][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    // ---- products: K = 32 input channels per matrix instruction, 9 taps per outer step
#pragma unroll 1
    for (int kg = 0; kg < KG; ++kg) {
        const u32x4* xk = band + kg * 4 * PLANE;
        const u32x4* ak = aw + (kg & 1) * ASLOTS + (wc * NCB) * 576 + lane;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            bf16x8 a[NCB];
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) a[cb] = __builtin_bit_cast(bf16x8, ak[cb * 576 + tap * 64]);
            if (tap == 3 && kg + 1 < KG) {      // as c3f_kernel: the next chunk goes to LDS between queued matrix instructions
                commit(kg + 1);
                if (kg + 2 < KG) issue(kg + 2);
                __builtin_amdgcn_sched_barrier(0);
            }
            const int dy = tap / 3, dx = tap - 3 * dy;
            bf16x8 bv[NPB];
#pragma unroll
            for (int i = 0; i < NPB; ++i) bv[i] = __builtin_bit_cast(bf16x8, xk[va[i] + dy * PWS + dx]);
#pragma unroll
            for (int i = 0; i < NPB; ++i)
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb)
                    acc[i][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[cb], bv[i], acc[i][cb], 0, 0, 0);
        }
        // LDS-only barrier: __syncthreads() also drains vmcnt, i.e. waits for the chunk that has just been requested
        if (kg + 1 < KG) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }

    // ---- epilogue (c3f_kernel's): D[channel 4 (lane >> 4) + r][pixel lane & 15]
    if (C::POOL) __syncthreads();                                   // every wave is done with the band: the pool tile reuses it
#pragma unroll
    for (int i = 0; i < NPB; ++i) {
        const int pb = wpb * NPB + i;
        if (pb >= PBT) continue;                                    // wave-uniform
        const int p = pb * 16 + l15, row = p / W, col = p - row * W;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 16 * (cb0 + cb) + 4 * lk + r;
                float v = acc[i][cb][r] + bias[co];
                v = v > 0.f ? v : 0.f;
                if (C::POOL) lds[(16 * (wc * NCB + cb) + 4 * lk + r) * C::OP + p] = v;
                else y[(((size_t)b * COUT + co) * H + r0 + row) * W + col] = v;
            }
    }
    if (C::POOL) {
        __syncthreads();
        constexpr int HP = H / 2, WP = W / 2, TP = TR / 2, NOUT = 16 * C::NCBW * TP * WP;
        for (int e = tid; e < NOUT; e += 256) {
            const int cl = e / (TP * WP), rem = e - cl * (TP * WP), pr = rem / WP, pc = rem - pr * WP;
            const float* q = lds + cl * C::OP + (2 * pr) * W + 2 * pc;
            const float m = fmaxf(fmaxf(q[0], q[1]), fmaxf(q[W], q[W + 1]));
            y[(((size_t)b * COUT + 16 * cbg * C::NCBW + cl) * HP + r0 / 2 + pr) * WP + pc] = m;
        }
    }
}

template <class C>
int launch_bf16(var_ctx* c, hipStream_t s, const float* x, const f32x4* wp, const float* bias, float* y, int B) {
    static unsigned attr = 0;      // bit d: set on device d (function attributes are per device)
    if (!(attr & var_dev_bit(c))) {
        VAR_HIP_CHECK(c, hipFuncSetAttribute((const void*)c3b_kernel<C>, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDSF * 4));
        attr |= var_dev_bit(c);
    }
    hipLaunchKernelGGL(c3b_kernel<C>, dim3(B * C::BANDS * C::CBG), dim3(256), C::LDSF * 4, s, x, (const u32x4*)wp, bias, y, B);
    VAR_HIP_CHECK(c, hipGetLastError());
    return VAR_OK;
}
}  // namespace c3f
