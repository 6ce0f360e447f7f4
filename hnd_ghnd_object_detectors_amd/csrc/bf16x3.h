// The arithmetic of the emulated GEMM family (conv_bx3.hip, conv_bx3_tiled.hip, conv_bxs.hip): every fp32 value is the
// exact sum of three bf16 planes obtained by truncation, and a product is the six plane products with i + j <= 2, smallest
// terms first.  "Same bits across the family" (DESIGN section 4 rule 4) rests on every member splitting and ordering the
// products identically, so both are written HERE ONLY: the split of a pair (split_pair) and of one value (split_value: the
// pack kernels), the six products alone (mfma6: the tiled build) and with the next step's pair split between them
// (mfma6_split: the two persistent kernels' main loops).  No kernel spells the MFMA or a truncation out itself.
#pragma once
#include "common.h"

namespace hnd {

typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// two consecutive k values -> one dword per plane (x0 in the low half: the MFMA's element order): hi = top 16 bits of x,
// mid = top 16 bits of x - hi, lo = x - hi - mid (8 + 8 + 8 significant bits)
__device__ __forceinline__ void split_pair(float x0, float x1, uint32_t& hp, uint32_t& mp, uint32_t& lp) {
  const uint32_t a0 = __float_as_uint(x0), a1 = __float_as_uint(x1);
  const uint32_t h0 = a0 & 0xffff0000u, h1 = a1 & 0xffff0000u;
  const float r0 = x0 - __uint_as_float(h0), r1 = x1 - __uint_as_float(h1);
  const uint32_t m0 = __float_as_uint(r0) & 0xffff0000u, m1 = __float_as_uint(r1) & 0xffff0000u;
  const float q0 = r0 - __uint_as_float(m0), q1 = r1 - __uint_as_float(m1);
  hp = __builtin_amdgcn_perm(h1, h0, 0x07060302u);
  mp = __builtin_amdgcn_perm(m1, m0, 0x07060302u);
  lp = __builtin_amdgcn_perm(__float_as_uint(q1), __float_as_uint(q0), 0x07060302u);
}

// ... and of one value (a packed weight on its way into a plane image): the same three planes as bf16 bit patterns
__device__ __forceinline__ void split_value(float x, uint16_t& hi, uint16_t& mid, uint16_t& lo) {
  const uint32_t hb = __float_as_uint(x) & 0xffff0000u;
  const float r1 = x - __uint_as_float(hb);
  const uint32_t mb = __float_as_uint(r1) & 0xffff0000u;
  const float r2 = r1 - __uint_as_float(mb);
  hi = (uint16_t)(hb >> 16);
  mid = (uint16_t)(mb >> 16);
  lo = (uint16_t)(__float_as_uint(r2) >> 16);
}

// One 16 x 16 accumulator tile, one 32-deep k step: the six plane products, smallest terms first -- lo.hi, hi.lo, mid.mid,
// mid.hi, hi.mid, hi.hi (a = A planes hi / mid / lo, b[0 .. 2] = B planes hi / mid / lo).
__device__ __forceinline__ void mfma6(f32x4& cacc, bf8 ah, bf8 am, bf8 al, const bf8 (&b)[3]) {
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, b[0], cacc, 0, 0, 0);
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b[2], cacc, 0, 0, 0);
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b[1], cacc, 0, 0, 0);
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b[0], cacc, 0, 0, 0);
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b[1], cacc, 0, 0, 0);
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b[0], cacc, 0, 0, 0);
}

// The same six products with split_pair(x0, x1, hp, mp, lp) of the NEXT k step riding between them, statement by statement
// between sched_barriers: 96 matrix-pipe cycles with 48 free for vector issue carry the pair's 11 vector instructions.
// (split_pair's own statements, in its order: a change there is a change here.)
__device__ __forceinline__ void mfma6_split(f32x4& cacc, bf8 ah, bf8 am, bf8 al, const bf8 (&b)[3], float x0, float x1,
                                            uint32_t& hp, uint32_t& mp, uint32_t& lp) {
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, b[0], cacc, 0, 0, 0);      // smallest terms first
  const uint32_t h0 = __float_as_uint(x0) & 0xffff0000u, h1 = __float_as_uint(x1) & 0xffff0000u;
  __builtin_amdgcn_sched_barrier(0);
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b[2], cacc, 0, 0, 0);
  const float r0 = x0 - __uint_as_float(h0), r1 = x1 - __uint_as_float(h1);
  __builtin_amdgcn_sched_barrier(0);
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b[1], cacc, 0, 0, 0);
  const uint32_t m0 = __float_as_uint(r0) & 0xffff0000u, m1 = __float_as_uint(r1) & 0xffff0000u;
  __builtin_amdgcn_sched_barrier(0);
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, b[0], cacc, 0, 0, 0);
  const float q0 = r0 - __uint_as_float(m0), q1 = r1 - __uint_as_float(m1);
  __builtin_amdgcn_sched_barrier(0);
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b[1], cacc, 0, 0, 0);
  hp = __builtin_amdgcn_perm(h1, h0, 0x07060302u);
  mp = __builtin_amdgcn_perm(m1, m0, 0x07060302u);
  lp = __builtin_amdgcn_perm(__float_as_uint(q1), __float_as_uint(q0), 0x07060302u);
  __builtin_amdgcn_sched_barrier(0);
  cacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, b[0], cacc, 0, 0, 0);
}

// Launch of a pack kernel (hnd_pack_bf16x3 / hnd_pack_bf16x3s, after their own argument checks): one thread per element of
// the packed operand up to 8192 blocks of 256, a grid-stride loop beyond.  `total` travels as the kernel's last argument.
template <class Kern, class... Args>
int launch_pack(Kern kern, long long total, void* stream, const char* what, Args... args) {
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), args..., total);
  return check_launch(what);
}

}  // namespace hnd
