// The 96 x 96 image stack on c3f.h's band kernels as the iTHOR policy (ithor_policy.hip) and the frozen encoder's reward step
// (ithor_reward.hip) both run it, and what every user of the band kernels needs: the filter-pack descriptor and the conv 1
// launch (armnet.hip too).  Include after c3f.h; actor_critic.h includes it.
#pragma once

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

// conv 1 (c3f.h), with wpk in the same launch the filter pack `d` of the later convolutions
inline int conv1(var_ctx* c, hipStream_t s, const void* image, int image_is_u8, long image_bstride, const float* P, int w, int b,
                 float* y, int B, c3f::f32x4* wpk, const c3f::PackDesc& d) {
    const int nconv = B * c3f::C1_BANDS, npack = wpk ? (d.first[d.n_layers] + 255) / 256 : 0;
    if (image_is_u8) hipLaunchKernelGGL(c3f::c1f_pack_kernel<true>, dim3(nconv + npack), dim3(256), 0, s, image, image_bstride, P, w, b, y,
                                        nconv, wpk, d);
    else hipLaunchKernelGGL(c3f::c1f_pack_kernel<false>, dim3(nconv + npack), dim3(256), 0, s, image, image_bstride, P, w, b, y, nconv,
                            wpk, d);
    AC_CHECK(c);
    return VAR_OK;
}

}  // namespace
