// The 96 x 96 image stack on c3f.h's band kernels as the iTHOR policy (ithor_policy.hip) and the frozen encoder's reward step
// (ithor_reward.hip) both run it, and what every user of the band kernels needs: the filter-pack descriptor and the conv 1
// launch (armnet.hip too).  Include after c3f.h; actor_critic.h includes it.
#pragma once
#include "c3f_bf16.h"

namespace {

#define AC_CHECK(c) VAR_HIP_CHECK(c, hipGetLastError())
#define RUN(x) do { int r_ = (x); if (r_ != VAR_OK) return r_; } while (0)

constexpr int kBandMaxB = 64;      // up to here the image stack runs on c3f.h's band kernels; beyond, the gather-GEMM's big tiles win

// the iTHOR image stack as band kernels (c3f.h), bands / channel groups chosen for 192-256 workgroups at 8 images
using IthorC2 = c3f::Cfg<32, 32, 96, 4, 2, 1, true>;        // 96 -> pool 48: 192 workgroups
using IthorC3 = c3f::Cfg<32, 64, 48, 6, 1, 1, true>;        // 48 -> pool 24: 256
using IthorC4 = c3f::Cfg<64, 64, 24, 4, 1, 1, true>;        // 24 -> pool 12: 192
using IthorC5 = c3f::Cfg<64, 128, 12, 4, 1, 1, true>;       // 12 -> pool 6: 192
using IthorC6 = c3f::SmallCfg<128, 128, 6, 2, 3, 1>;        // stride 2 pad 1, 6 -> 3: 64
// the same bands on c3f_bf16.h's kernel (the policy's bf16 mode); kIthorBands: the band layers among the layers of the filter pack
// (bit i = conv i + 2), packed in that kernel's form under the mode
using IthorB2 = c3f::CfgB<32, 32, 96, 4, 2, 1, true>;
using IthorB3 = c3f::CfgB<32, 64, 48, 6, 1, 1, true>;
using IthorB4 = c3f::CfgB<64, 64, 24, 4, 1, 1, true>;
using IthorB5 = c3f::CfgB<64, 128, 12, 4, 1, 1, true>;
constexpr unsigned kIthorBands = 0xF;

// one band layer of a stack: the fp32 kernel, or under BF the bf16 one
template <class CF, class CB, bool BF>
inline int band(var_ctx* c, hipStream_t s, const float* x, const c3f::f32x4* wp, const float* bias, float* y, int B) {
    if constexpr (BF) return c3f::launch_bf16<CB>(c, s, x, wp, bias, y, B);
    else return c3f::launch<CF>(c, s, x, wp, bias, y, B);
}

// conv 2 .. n + 1 of an image stack for c3f::pack_item: layer i is ch[i] -> ch[i + 1], its filter at w_off[i] of the arena
inline c3f::PackDesc make_pack_desc(const int* ch, const int* w_off, int n) {
    c3f::PackDesc d{};
    d.n_layers = n;
    int f4 = 0;
    for (int i = 0; i < n; ++i) {
        d.w_off[i] = w_off[i]; d.cin[i] = ch[i]; d.cout[i] = ch[i + 1];
        d.wp_off[i] = f4; d.first[i] = f4;
        f4 += ch[i] * ch[i + 1] * 9 / 4;
    }
    d.first[n] = f4;
    return d;
}

constexpr int kFlagBf16 = 1;       // flags bit 0 of the acting forwards' _ex entries: bf16 operands in every imgCNN convolution

// The refusal of the _ex entries: any flag bit but bit 0
inline int check_flags(var_ctx* c, const char* fn, int flags) {
    if (flags & ~kFlagBf16) { VAR_SET_ERR(c, "%s: flags = %d: bit 0 (bf16 operands) is the only one", fn, flags); return VAR_ERR_ARG; }
    return VAR_OK;
}

// conv 1 (c3f.h), with wpk in the same launch the filter pack `d` of the later convolutions; bf: both with bf16 operands, the
// layers of `bfmask` (bit i: layer i of d; the band layers) packed for c3f_bf16.h's kernel
inline int conv1(var_ctx* c, hipStream_t s, const void* image, int image_is_u8, long image_bstride, const float* P, int w, int b,
                 float* y, int B, c3f::f32x4* wpk, const c3f::PackDesc& d, bool bf = false, unsigned bfmask = 0) {
    const int nconv = B * c3f::C1_BANDS, npack = wpk ? (d.first[d.n_layers] + 255) / 256 : 0;
    if (bf) {
        if (image_is_u8) hipLaunchKernelGGL((c3f::c1f_pack_kernel<true, true>), dim3(nconv + npack), dim3(256), 0, s, image, image_bstride, P, w,
                                            b, y, nconv, wpk, d, bfmask);
        else hipLaunchKernelGGL((c3f::c1f_pack_kernel<false, true>), dim3(nconv + npack), dim3(256), 0, s, image, image_bstride, P, w, b, y,
                                nconv, wpk, d, bfmask);
    } else if (image_is_u8) hipLaunchKernelGGL(c3f::c1f_pack_kernel<true>, dim3(nconv + npack), dim3(256), 0, s, image, image_bstride, P, w, b, y,
                                        nconv, wpk, d, 0u);
    else hipLaunchKernelGGL(c3f::c1f_pack_kernel<false>, dim3(nconv + npack), dim3(256), 0, s, image, image_bstride, P, w, b, y, nconv,
                            wpk, d, 0u);
    AC_CHECK(c);
    return VAR_OK;
}

}  // namespace
