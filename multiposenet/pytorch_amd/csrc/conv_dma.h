// conv_dma.h — what the two convolution translation units (conv_igemm.hip, conv_wgrad.hip) share: the 16-byte-operand MFMA wrapper
// and the LDS-DMA ring primitives.  Everything sits in the unnamed namespace: each unit gets its own copy.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef int i32x4_t __attribute__((ext_vector_type(4)));

// One MFMA k-step on 16-byte operands, by element type: 16x16x32 on 8 packed 16-bit values per lane, or four exact-fp32 16x16x4
// (one k per lane each) on the 4 floats.
template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    __device__ static __forceinline__ void run(f32x4_t& acc, const u32x4_t& a, const u32x4_t& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                      __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
    }
};
template <> struct Mma<f16_t> {
    __device__ static __forceinline__ void run(f32x4_t& acc, const u32x4_t& a, const u32x4_t& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    __device__ static __forceinline__ void run(f32x4_t& acc, const u32x4_t& a, const u32x4_t& b) {
        const f32x4_t fa = __builtin_bit_cast(f32x4_t, a);
        const f32x4_t fb = __builtin_bit_cast(f32x4_t, b);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[0], fb[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[1], fb[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[2], fb[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[3], fb[3], acc, 0, 0, 0);
    }
};

// LDS-DMA.  `buffer_load_dwordx4 ... lds` moves 16 bytes per lane from the buffer straight to LDS address M0 + lane * 16 (lane-linear:
// a swizzle of the tile image is applied on the SOURCE side, by choosing which chunk each lane fetches), with no staging registers and
// no ds_write pass.  A lane whose voffset + soffset lies beyond the descriptor's num_records writes ZEROS: halo taps, channel tails and
// rows past the end carry DMA_OOB (or the tensor's byte size) as their offset and need no mask.  The loads are inline asm, invisible
// to the compiler's waitcnt bookkeeping: completion is counted by hand — wait_vmcnt<N>(), N = the DMA instructions of the k-steps that
// may still be in flight — and the k-loops use the raw s_barrier, so a ring never drains inside its loop.
// (semantics pinned with tools/probe_dma.*)
__device__ __forceinline__ i32x4_t make_rsrc(const void* base, unsigned bytes) {
    const uint64_t a = (uint64_t)base;
    i32x4_t r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xffffu));
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    return r;
}

__device__ __forceinline__ void lds_dma16(unsigned voff, i32x4_t rsrc, unsigned soff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_dst) : "memory");
}

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

constexpr unsigned DMA_OOB = 0x80000000u;     // out-of-range marker for descriptors of < 2 GB (launcher checks): marker + soffset never wraps

__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ const void* rfl_ptr(const void* q) {
    const uint64_t a = (uint64_t)q;
    return (const void*)(((uint64_t)(unsigned)rfl((int)(a >> 32)) << 32) | (unsigned)rfl((int)a));
}

}  // namespace
