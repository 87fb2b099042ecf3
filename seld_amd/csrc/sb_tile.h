// sb_tile.h — the primitives of the split-bf16 kernels (gemm_sb.hip, gemm_tn_sb.hip, conv_sb.hip, conv_wgrad_sb.hip, conv_pool_sb.hip)
// and of their weight pre-passes (prep.h): the splits of an fp32 value into bf16 planes, the bf16 MFMA and the transposed LDS fragment.
// What is NOT here is the order in which a kernel issues its products and the accumulators it gives them: that order is the kernel's fp32
// summation order, i.e. its arithmetic, and stays spelled out in each kernel.
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// exact 3-way truncation split of two floats, x = hi + mid + lo (8 + 8 + 8 significant bits), packed as bf16 pairs (element 0 in the low half)
__device__ __forceinline__ void split3_pair(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    const unsigned u0 = __float_as_uint(x0), u1 = __float_as_uint(x1);
    h = __builtin_amdgcn_perm(u1, u0, 0x07060302);
    const float r0 = x0 - __uint_as_float(u0 & 0xffff0000u), r1 = x1 - __uint_as_float(u1 & 0xffff0000u);
    const unsigned v0 = __float_as_uint(r0), v1 = __float_as_uint(r1);
    m = __builtin_amdgcn_perm(v1, v0, 0x07060302);
    const float s0 = r0 - __uint_as_float(v0 & 0xffff0000u), s1 = r1 - __uint_as_float(v1 & 0xffff0000u);
    l = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302);
}

// two-plane split of two floats for the four-product form: hi = the truncated upper 16 bits, mid = the residual ROUNDED to bf16 (half up on the
// magnitude: one integer add) — with a truncated mid the dropped remainder has the sign of x for every element, and the products it would have
// carried bias every sum by the same ~2^-16 relative; rounded, it is zero-mean and the dropped terms average out over a sum
__device__ __forceinline__ void split2r_pair(float x0, float x1, unsigned& h, unsigned& m) {
    const unsigned u0 = __float_as_uint(x0), u1 = __float_as_uint(x1);
    h = __builtin_amdgcn_perm(u1, u0, 0x07060302);
    const float r0 = x0 - __uint_as_float(u0 & 0xffff0000u), r1 = x1 - __uint_as_float(u1 & 0xffff0000u);
    m = __builtin_amdgcn_perm(__float_as_uint(r1) + 0x8000u, __float_as_uint(r0) + 0x8000u, 0x07060302);
}

// bf16 single-product mode: the two floats rounded to nearest-even bf16, packed like the planes above
__device__ __forceinline__ unsigned rne_pair(float x0, float x1) { return bf16_rne_bits(x0) | (bf16_rne_bits(x1) << 16); }

// the three planes of ONE float, as the weight pre-passes write them (the high 16 bits of each plane's fp32 value).
//   one:       plane 0 is the value ROUNDED to nearest bf16 (bf16 single-product mode), which is all a ONE-form consumer reads; planes 1, 2 split
//              the residual x - plane0 exactly either way (|residual| <= an ulp of plane 0: 16 significant bits, 8 + 8), so a consumer WITHOUT a
//              ONE form (six products over all three planes) computes with the exact weights in both modes — it never reads an unwritten plane.
//   round_mid: the mid plane is rounded as in split2r_pair (a backward operand: the four-product form reads planes 0, 1 only and wants a
//              zero-mean remainder); plane 2 still completes the split exactly.
struct Planes3 { unsigned short p0, p1, p2; };
__device__ __forceinline__ Planes3 split3(float x, bool one, bool round_mid) {
    const unsigned u = one ? bf16_rne_bits(x) << 16 : __float_as_uint(x) & 0xffff0000u;
    const float r = x - __uint_as_float(u);
    const unsigned v = __float_as_uint(r) + (round_mid ? 0x8000u : 0u);
    const float s = r - __uint_as_float(v & 0xffff0000u);
    return {(unsigned short)(u >> 16), (unsigned short)(v >> 16), (unsigned short)(__float_as_uint(s) >> 16)};
}

// v_mfma_f32_32x32x16_bf16: returns acc + A B.  A: lane l holds A[i = l & 31][k = 8 (l >> 5) .. + 7]; B: lane l holds B[k = 8 (l >> 5) .. + 7][j = l & 31];
// the accumulator layout is common.h's (mfma_row)
__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 a, bf16x8 b, f32x16 acc) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0); }

// ds_read_b64_tr_b16 of a 4-row x 16-column block of an LDS image whose reduction index is the ROW: this lane's address is (row q of the
// block, 4 of its columns); it receives its own column for the 4 rows, i.e. 4 consecutive k.  Two of them make a fragment.
__device__ __forceinline__ s16x4 tr16(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}
__device__ __forceinline__ bf16x8 frag(const char* p0, const char* p1) {
    const s16x4 a = tr16(p0), b = tr16(p1);
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}
