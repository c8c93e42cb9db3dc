// Where a clip slot's MFCC features are read from: ONE rule for the front-end that produces them (mfcc.hip) and the sound CNN
// kernels that consume them (snd_mfma.hip), so that the two can never disagree about a slot.
//
// Under a clip cache (var_mfcc_cache_bind) a slot whose length equals its pool row's cached one is SERVED: its features are the
// cache row's, bit for bit.  The copying front-end (mfcc_kernel<false, ClipCache>) delivers them into the feature buffer; the
// in-place one (mfcc_kernel<false, ClipCacheInPlace>) leaves served and empty slots of the buffer alone, and the readers take
// them from here.  A slot has exactly one source:
//   served                 cache_feats + row * frames * 40
//   lens[slot] <= 0        zeros, read from nowhere (the "empty" class)
//   anything else (live)   the feature buffer, slot * frames * 40
// Without a cache (cache_feats == nullptr) every slot resolves to the feature buffer: lens and clip_index are not read.
#pragma once
#include <stddef.h>

constexpr int kClipCoeffs = 40;

// the feature buffer is two runs of slots, as the encoder takes them: [0, split) at buf, [split, ..) at buf_hi (either may be
// null: that branch does not run).  The in-step front-end writes one block: buf_hi = buf + split * frames * 40.
struct ClipSrc {
    const float* buf;
    const float* buf_hi;
    int split;
    const int* lens;            // per slot; read only under a cache
    const int* clip_index;      // slot -> pool row (null: the slot is the row)
    const int* cache_lens;
    const float* cache_feats;   // null: no cache, every slot is read from the buffer
    int cache_rows;
    int frames;
};

// the three lookups of a slot: lens and clip_index side by side, the row's cached length behind the row
struct ClipLook { int N, row, clen; };

// UNIFORM: the slot is the same for the whole workgroup (the sound kernels) -- the lookup goes through the constant address
// space, so it is a scalar load wherever it stands; as a generic load behind a barrier it is a vector load that the compiler
// waits for on the spot, together with every other load in flight.  (The tables are not written while their readers run.)
template <bool UNIFORM>
__device__ __forceinline__ int clip_ld(const int* __restrict__ p, int i) {
    if constexpr (UNIFORM) return ((const __attribute__((address_space(4))) int*)p)[i];
    else return p[i];
}
template <bool UNIFORM = false>
__device__ __forceinline__ int clip_len_of(const int* __restrict__ lens, int slot) { return clip_ld<UNIFORM>(lens, slot); }
template <bool UNIFORM = false>
__device__ __forceinline__ int clip_row_of(const int* __restrict__ clip_index, int slot) {
    return clip_index ? clip_ld<UNIFORM>(clip_index, slot) : slot;
}
// (-1 is no length: a row outside the cache is never served)
template <bool UNIFORM = false>
__device__ __forceinline__ int clip_cached_len(const int* __restrict__ cache_lens, int cache_rows, int row) {
    return (unsigned)row < (unsigned)cache_rows ? clip_ld<UNIFORM>(cache_lens, row) : -1;
}
// THE predicate, (unsigned)row < cache_rows && N > 0 && N == cache_lens[row], on the looked-up length: clen =
// clip_cached_len(cache_lens, cache_rows, row), whose -1 for a row outside the cache equals no N > 0
__device__ __forceinline__ bool clip_served(int N, int clen) { return N > 0 && N == clen; }
__device__ __forceinline__ bool clip_empty(int N) { return N <= 0; }

__device__ __forceinline__ const float* clip_buf_ptr(const ClipSrc& cs, int slot) {
    const size_t clip = (size_t)cs.frames * kClipCoeffs;
    return slot < cs.split ? cs.buf + (size_t)slot * clip : cs.buf_hi + (size_t)(slot - cs.split) * clip;
}
// the slot's source from its lookups; nullptr = zeros
__device__ __forceinline__ const float* clip_src_from(const ClipSrc& cs, int slot, const ClipLook& k) {
    if (!cs.cache_feats) return clip_buf_ptr(cs, slot);
    if (clip_served(k.N, k.clen)) return cs.cache_feats + (size_t)k.row * cs.frames * kClipCoeffs;
    return clip_empty(k.N) ? nullptr : clip_buf_ptr(cs, slot);
}
// the sources of the workgroup-uniform slots [slot0, slot0 + n), n <= NS (the rest: nullptr): the chains side by side -- every
// slot's lens and clip_index, then every row's cached length --, two round trips for all of them
template <int NS>
__device__ __forceinline__ void clip_src_of_n(const ClipSrc& cs, int slot0, int n, const float* (&src)[NS]) {
    ClipLook k[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) k[i] = ClipLook{0, 0, -1};
    if (cs.cache_feats) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int slot = slot0 + (i < n ? i : 0);           // (a slot of the call stands in for the ones past its end)
            k[i].N = clip_len_of<true>(cs.lens, slot);
            k[i].row = clip_row_of<true>(cs.clip_index, slot);
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) k[i].clen = clip_cached_len<true>(cs.cache_lens, cs.cache_rows, k[i].row);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) src[i] = i < n ? clip_src_from(cs, slot0 + i, k[i]) : nullptr;
}
