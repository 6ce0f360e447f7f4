// The operand split of the emulated GEMM family (conv_bx3.hip, conv_bx3_tiled.hip, conv_bxs.hip): every fp32 value is the
// exact sum of three bf16 planes obtained by truncation.  "Same bits across the family" (DESIGN section 4 rule 4) rests on
// every member splitting with these expressions.  (The main loops of bx3_kernel / bxs_kernel spell split_pair out between
// their six MFMAs, statement by statement between sched_barriers, and the pack kernels split one value at a time: keep them
// in step with it.)
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

}  // namespace hnd
