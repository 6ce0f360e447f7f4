// The arithmetic of the bottleneck quantisers, once: csrc/quant.hip (per-tensor, fixed-range and per-channel codec and fake
// quantiser) and the decoder of csrc/entropy.hip all call these functions, so their paths agree bit for bit by construction.
//
// The contract.  The codec is byte work: it must reproduce myutils.tensor_util.quantize_tensor bit for bit on identical fp32
// input (tests/test_ops_gpu.py, torch.equal on the bytes).  Every operation below is therefore a single correctly rounded
// IEEE fp32 operation in the reference's order: hipcc's __fdiv_rn / __fadd_rn / __fsub_rn / __fmul_rn are the plain
// operators, the division is the correctly rounded one (v_div_scale / fmas / fixup sequence, checked in the ISA), and EVERY
// TRANSLATION UNIT THAT INCLUDES THIS HEADER IS BUILT WITH -ffp-contract=off (csrc/Makefile), so no multiply is ever fused
// into an add.
#pragma once
#include "common.h"

namespace hnd {
namespace quant {

// zero_point + x / scale, not yet clamped: the fixed range's clip mask looks at this value
__device__ __forceinline__ float unclamped_code(float x, float scale, float zp) { return __fadd_rn(zp, __fdiv_rn(x, scale)); }

// ... NOT clipped: rint(u) inside [0, qmax] (-0 passes, a NaN does not)
__device__ __forceinline__ bool inside_range(float u, float qmax) {
  const float r = rintf(u);
  return r >= 0.f && r <= qmax;
}

// clamp_(qmin, qmax) with qmin = 0, then round_(): half to even.  The code as a float (an integer 0 ... qmax, or a NaN's NaN)
__device__ __forceinline__ float clamp_round(float u, float qmax) {
  u = u < 0.f ? 0.f : (u > qmax ? qmax : u);
  return rintf(u);
}

__device__ __forceinline__ float quantize_one(float x, float scale, float zp, float qmax) {
  return clamp_round(unclamped_code(x, scale, zp), qmax);
}

// scale * (q - zero_point); (float)(uint8_t)q == q for the integers 0 ... 255, so a code kept in a register gives the same
__device__ __forceinline__ float dequantize_one(float q, float scale, float zp) { return __fmul_rn(scale, __fsub_rn(q, zp)); }

// qp = {min, max, scale, zero_point} of the range (lo, hi).  kConstantRule is include/hnd_qchannel.h's rule for a constant
// channel (hi == lo: scale = |lo|, or 1 for a channel of zeros, so the channel is reproduced exactly); the per-tensor and
// fixed-range paths do not have it and divide by the zero scale like the reference.
template <bool kConstantRule>
__device__ __forceinline__ void write_qparams(float lo, float hi, float qmax, float* __restrict__ qp) {
  float scale;
  if (!kConstantRule || hi != lo) scale = __fdiv_rn(__fsub_rn(hi, lo), qmax);      // (max - min) / (qmax - qmin), qmin = 0
  else scale = lo != 0.f ? fabsf(lo) : 1.f;
  float zp = __fsub_rn(0.f, __fdiv_rn(lo, scale));                                 // qmin - min / scale
  zp = zp < 0.f ? 0.f : (zp > qmax ? qmax : zp);
  qp[0] = lo; qp[1] = hi; qp[2] = scale; qp[3] = truncf(zp);                       // int(zero_point)
}

// The logical NCHW order walked over an NHWC buffer of pixel stride cs: value i0 is (img, ch, pix) with plane = img * c + ch.
// I is the index type: 64-bit in the packers, 32-bit where the caller bounds numel (csrc/entropy.hip: at most 2^30).
template <class I>
struct NchwWalk {
  I img, pix, hw;
  int ch, c;
  __device__ __forceinline__ NchwWalk(I i0, I hw_, int c_) : hw(hw_), c(c_) {
    const I plane = i0 / hw;
    pix = i0 - plane * hw;
    img = plane / (I)c;
    ch = (int)(plane - img * (I)c);
  }
  __device__ __forceinline__ unsigned long long offset(int cs) const { return ((unsigned long long)img * hw + pix) * cs + ch; }
  // the next value; written as selects, not branches: a lane's step must not split the wave inside the packers' loop
  __device__ __forceinline__ void next() {
    const bool plane_end = pix + 1 == hw, image_end = plane_end && ch + 1 == c;
    pix = plane_end ? 0 : pix + 1;
    ch = image_end ? 0 : (plane_end ? ch + 1 : ch);
    img = image_end ? img + 1 : img;
  }
};

}  // namespace quant
}  // namespace hnd
