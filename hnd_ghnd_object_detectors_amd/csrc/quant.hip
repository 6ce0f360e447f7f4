// The bottleneck quantisers: include/hnd_codec.h (the codec at 1 ... 8 bits and the bit-packed payload), include/hnd_qat.h
// (the fake quantiser of the training step), include/hnd_qrange.h (the fixed, EMA-calibrated range), include/hnd_qchannel.h
// (one scale and zero point per channel) and include/hnd_qimage.h (one per image), with hnd_quantize_u8 / hnd_dequantize_u8 /
// hnd_roundtrip_f16 of hnd_hip.h.  The formulas and formats are the headers'; the arithmetic is csrc/quant_math.h, whose
// contract (single correctly rounded fp32 operations, no FMA contraction in this file) makes every path give the same bits
// for the same scale and zero point.
//
// Where a lane's scale and zero point come from is a policy type (PerTensor, PerChannel, PerImage); the fake quantiser, the
// packer and the grouped quantise / dequantise / unpack kernels are one kernel each, built per policy.  quantize /
// dequantize / unpack_dequantize exist in two lane layouts, because their exports promise different things: the per-tensor
// exports take any cs >= c with no alignment demand and run one thread per float; the per-channel and per-image exports
// (grouped_*) demand cs % 4 == 0 and aligned buffers and run one lane per (pixel, group of 4 channels) with the group
// fastest, so a wave's 16-byte accesses cover consecutive bytes and a lane KEEPS its group: its four scales and zero points
// are read once.  A pixel wider than the workgroup is walked one workgroup's worth of groups at a time.
#include "common.h"
#include "hnd_codec.h"
#include "hnd_qat.h"
#include "hnd_qchannel.h"
#include "hnd_qimage.h"
#include "hnd_qrange.h"
#include "quant_math.h"

#include <hip/hip_fp16.h>
#include <limits.h>
#include <cmath>

namespace {

using hnd::f32x4;
using namespace hnd::quant;

constexpr int kThreads = 256;            // every launch of this file but the fake quantiser's and the one-wave qparams kernels
static_assert(kThreads == 4 * 64, "minmax_kernel meets its four waves in smin[4] / smax[4]");
constexpr int kMaxBlocks = 256 * 16;
constexpr int kPartBlocks = 512;         // rows of the min / max partial in scratch, per tensor {lo, hi} and per channel [2][cs]
constexpr int kMaxC = HND_QCHANNEL_MAX_C;
constexpr int kFqRows = HND_FAKE_QUANT_TILE_ROWS;
constexpr int kFqWaves = 4;
constexpr int kImageBlocks = HND_QIMAGE_PART_BLOCKS;      // rows of the min / max partial in scratch, per image

// ---- the policies.  A policy object is the qparams of one lane's group of 4 channels (k = 0 ... 3 inside the group); its
// Table (made by stage_table) is the qparams of every channel, for the packer, whose lanes change channel as they go; where
// kTableInLds says so the workgroup has staged it in LDS and meets at a barrier before the first read.  square_sum is one step of
// the fake quantiser's sum of squares: the per-tensor statistics have always been accumulated with a fused multiply-add (the
// kernel was first built where contraction was on) and the per-channel ones with a rounded product; both are kept, because
// hnd_bn_finalize's results downstream are compared bit for bit, and they are spelled out so the build flag decides neither.
// Where the pair follows the PIXEL (PerImage) three more calls say where a lane is: set_image (the grouped kernels, whose
// grid row is the image when kImageGrid says so), begin_tile / seek_row (the fake quantiser: the tile's first global pixel,
// then its rows in ascending order) and Table::seek_image (the packer, beside NchwWalk); they are empty everywhere else.
struct PerTensor {                       // qp[2], qp[3] for every channel
  static constexpr int kPackBound = 1024;                          // the packer's launch bound (the compiler's default)
  float sc, zp;
  __device__ __forceinline__ PerTensor(const float* __restrict__ qp, int, int) : sc(qp[2]), zp(qp[3]) {}
  __device__ __forceinline__ float scale(int) const { return sc; }
  __device__ __forceinline__ float zero(int) const { return zp; }
  __device__ __forceinline__ void begin_tile(const float* __restrict__, long long, long long) const {}
  __device__ __forceinline__ void seek_row(const float* __restrict__, int) const {}
  __device__ __forceinline__ void seek_image(long long) const {}
  static __device__ __forceinline__ float square_sum(float ss, float v) { return __fmaf_rn(v, v, ss); }
  typedef PerTensor Table;                 // one pair for every channel: nothing to stage
  static constexpr bool kTableInLds = false;
  static __device__ __forceinline__ Table stage_table(const float* __restrict__ qp, int) { return PerTensor(qp, 0, 0); }
};

struct PerChannel {                      // qp[ch][4]; channels that are not real get (1, 0), unused
  static constexpr int kPackBound = kThreads;
  float sc[4], zp[4];
  __device__ __forceinline__ PerChannel(const float* __restrict__ qp, int ch0, int c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool real = ch0 + k < c;
      sc[k] = real ? qp[(ch0 + k) * 4 + 2] : 1.f;
      zp[k] = real ? qp[(ch0 + k) * 4 + 3] : 0.f;
    }
  }
  static constexpr bool kImageGrid = false;
  __device__ __forceinline__ float scale(int k) const { return sc[k]; }
  __device__ __forceinline__ float zero(int k) const { return zp[k]; }
  __device__ __forceinline__ void set_image(const float* __restrict__, long long) const {}
  __device__ __forceinline__ void begin_tile(const float* __restrict__, long long, long long) const {}
  __device__ __forceinline__ void seek_row(const float* __restrict__, int) const {}
  static __device__ __forceinline__ float square_sum(float ss, float v) { return __fadd_rn(ss, __fmul_rn(v, v)); }
  struct Table {
    const float *s_scale, *s_zp;
    __device__ __forceinline__ float scale(int ch) const { return s_scale[ch]; }
    __device__ __forceinline__ float zero(int ch) const { return s_zp[ch]; }
    __device__ __forceinline__ void seek_image(long long) const {}
  };
  static constexpr bool kTableInLds = true;
  // thread ch < c writes channel ch's pair into LDS (at most 512 bytes); the CALLER holds the barrier before any read
  static __device__ __forceinline__ Table stage_table(const float* __restrict__ qp, int c) {
    __shared__ float scale_[kMaxC], zp_[kMaxC];
    if ((int)threadIdx.x < c) {
      scale_[threadIdx.x] = qp[threadIdx.x * 4 + 2];
      zp_[threadIdx.x] = qp[threadIdx.x * 4 + 3];
    }
    return Table{scale_, zp_};
  }
};

// qp[img][4]: the pair of a lane changes with its pixel's IMAGE, every channel of a pixel shares it.  The [n] pairs are read
// through the cache, not staged in LDS: a workgroup of the grouped kernels works on ONE image (its grid row; the two floats
// are the same in every lane, loaded once per workgroup), a fake-quantiser wave's tile of 128 consecutive pixels and a
// packer lane's 8 consecutive values lie in one image or cross into the next, so each reads one or two of the n pairs --
// 8 bytes that every lane of the wave asks for at the same address, one cache line -- where staging would have every
// workgroup load all n pairs and wait at a barrier to use one of them.  The image index is never divided out per float: it
// is the grid row, or one division per tile and then a walk (seek_row), or NchwWalk's own img (Table::seek_image).
struct PerImage {
  static constexpr int kPackBound = kThreads;
  static constexpr bool kImageGrid = true;
  float sc, zp;
  long long img, hw, next;               // the fake quantiser's walk: `next` is the tile row at which image img + 1 begins
  __device__ __forceinline__ PerImage(const float* __restrict__, int, int) : sc(1.f), zp(0.f), img(0), hw(0), next(0) {}
  __device__ __forceinline__ float scale(int) const { return sc; }
  __device__ __forceinline__ float zero(int) const { return zp; }
  __device__ __forceinline__ void set_image(const float* __restrict__ qp, long long i) {
    img = i;
    sc = qp[i * 4 + 2];
    zp = qp[i * 4 + 3];
  }
  __device__ __forceinline__ void begin_tile(const float* __restrict__ qp, long long row0, long long hw_) {
    hw = hw_;
    set_image(qp, row0 / hw_);           // the one division of a tile
    next = (img + 1) * hw_ - row0;
  }
  __device__ __forceinline__ void seek_row(const float* __restrict__ qp, int r) {      // r ascending within a tile
    if (r >= next) {
      long long i = img;
      do { ++i; next += hw; } while (r >= next);
      set_image(qp, i);
    }
  }
  static __device__ __forceinline__ float square_sum(float ss, float v) { return PerTensor::square_sum(ss, v); }
  struct Table {
    const float* qp;
    long long img;
    float sc, zp;
    __device__ __forceinline__ float scale(int) const { return sc; }
    __device__ __forceinline__ float zero(int) const { return zp; }
    __device__ __forceinline__ void seek_image(long long i) {
      if (i != img) { img = i; sc = qp[i * 4 + 2]; zp = qp[i * 4 + 3]; }
    }
  };
  static constexpr bool kTableInLds = false;
  static __device__ __forceinline__ Table stage_table(const float* __restrict__ qp, int) { return Table{qp, -1, 1.f, 0.f}; }
};

// ---- min / max, per tensor: per-block min / max of the real channels, one partial {lo, hi} per workgroup
__global__ void minmax_kernel(const float* __restrict__ x, long long npix, int c, int cs, float* __restrict__ part) {
  __shared__ float smin[4], smax[4];
  float lo = INFINITY, hi = -INFINITY;
  const long long total = npix * cs;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    if ((int)(e % cs) < c) {
      const float v = x[e];
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x * 2 + 0] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    part[blockIdx.x * 2 + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  }
}

// one wave: the batch (lo, hi) from minmax_kernel's partials, then qparams.  With `state` (include/hnd_qrange.h) the batch
// range is first folded into state = {running_min, running_max, steps, 0} and the qparams are the running range's.
// Per image (kConstantRule, include/hnd_qimage.h) the grid has one such wave per image: workgroup i reduces the nblocks
// partials of image i and writes qparams[i], with the rule for a constant image.
template <bool kConstantRule>
__global__ void qparams_kernel(const float* __restrict__ part, int nblocks, float momentum, float qmax,
                               float* __restrict__ state, float* __restrict__ qp) {
  part += (size_t)blockIdx.x * nblocks * 2;
  qp += (size_t)blockIdx.x * 4;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < nblocks; i += 64) {
    lo = fminf(lo, part[i * 2]);
    hi = fmaxf(hi, part[i * 2 + 1]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  if (threadIdx.x == 0) {
    if (state != nullptr) {
      const float steps = state[2];
      if (steps != 0.f) {
        lo = __fadd_rn(state[0], __fmul_rn(momentum, __fsub_rn(lo, state[0])));
        hi = __fadd_rn(state[1], __fmul_rn(momentum, __fsub_rn(hi, state[1])));
      }
      state[0] = lo; state[1] = hi; state[2] = __fadd_rn(steps, 1.f); state[3] = 0.f;
    }
    write_qparams<kConstantRule>(lo, hi, qmax, qp);
  }
}

// ---- min / max, per image.  Launch 1 on a grid of (workgroups per image, n): workgroup (b, i) takes its share of image
// i's pixels, lanes laid out (pixel, group of 4 channels) with the group fastest, one 16-byte load per lane and pixel; only
// the groups that hold a real channel are read, and of the last group only its real channels count.  The lanes meet by
// shuffle and then in LDS; one partial {lo, hi} per workgroup, [n][gridDim.x][2] in scratch.  Launch 2 is
// qparams_kernel<true>.
__global__ void __launch_bounds__(kThreads) image_minmax_kernel(const float* __restrict__ x, long long hw, int c, int cs,
                                                                float* __restrict__ part) {
  __shared__ float smin[4], smax[4];
  x += (size_t)blockIdx.y * hw * cs;
  const int gr = (c + 3) >> 2;                                     // groups with a real channel
  float lo = INFINITY, hi = -INFINITY;
  for (int gb = 0; gb < gr; gb += kThreads) {
    const int gc = gr - gb < kThreads ? gr - gb : kThreads;
    const int slots = kThreads / gc;                               // pixels per pass
    const int gl = threadIdx.x % gc, slot = threadIdx.x / gc;
    if (slot >= slots) continue;
    const int ch0 = (gb + gl) * 4;
    for (long long p = (long long)blockIdx.x * slots + slot; p < hw; p += (long long)gridDim.x * slots) {
      const f32x4 v = *(const f32x4*)(x + p * cs + ch0);           // (ch0 + 3 < cs: cs % 4 == 0, cs >= c)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (ch0 + k < c) {
          lo = fminf(lo, v[k]);
          hi = fmaxf(hi, v[k]);
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    out[0] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    out[1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  }
}

__global__ void qrange_qparams_kernel(float lo, float hi, float qmax, float* __restrict__ qp) {
  if (blockIdx.x == 0 && threadIdx.x == 0) write_qparams<false>(lo, hi, qmax, qp);
}

// ---- min / max, per channel.  Launch 1: per-lane min / max of its four channels, lanes of the same group meet in LDS, one
// partial [2][cs] per workgroup.  Only the groups that hold a real channel are read (c <= 64: at most 16 of them, so one pass).
__global__ void __launch_bounds__(kThreads) qc_minmax_kernel(const float* __restrict__ x, long long npix, int c, int cs,
                                                             float* __restrict__ part) {
  __shared__ float red[kThreads][8];
  const int gr = (c + 3) >> 2;                                     // groups with a real channel, 1 ... 16
  const int slots = kThreads / gr;                                 // pixels per pass
  const int g = threadIdx.x % gr, slot = threadIdx.x / gr;
  float lo[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, hi[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (slot < slots) {
    for (long long p = (long long)blockIdx.x * slots + slot; p < npix; p += (long long)gridDim.x * slots) {
      const f32x4 v = *(const f32x4*)(x + p * cs + g * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lo[k] = fminf(lo[k], v[k]);
        hi[k] = fmaxf(hi[k], v[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { red[threadIdx.x][k] = lo[k]; red[threadIdx.x][4 + k] = hi[k]; }
  __syncthreads();
  for (int i = threadIdx.x; i < gr * 8; i += kThreads) {
    const int gg = i >> 3, k = i & 7;
    float acc = red[gg][k];
    for (int sl = 1; sl < slots; ++sl) {
      const float v = red[sl * gr + gg][k];
      acc = k < 4 ? fminf(acc, v) : fmaxf(acc, v);
    }
    part[((size_t)blockIdx.x * 2 + (k >> 2)) * cs + gg * 4 + (k & 3)] = acc;      // (gg * 4 + 3 < cs: cs % 4 == 0, cs >= c)
  }
}

// launch 2: the partials reduced per channel, then qparams[ch] with the header's rule for a constant channel
__global__ void __launch_bounds__(kThreads) qc_qparams_kernel(const float* __restrict__ part, int nblocks, int c, int cs,
                                                              float qmax, float* __restrict__ qp) {
  __shared__ float slo[kThreads / kMaxC][kMaxC], shi[kThreads / kMaxC][kMaxC];
  const int ch = threadIdx.x % kMaxC, sub = threadIdx.x / kMaxC;
  float lo = INFINITY, hi = -INFINITY;
  if (ch < c) {
    for (int b = sub; b < nblocks; b += kThreads / kMaxC) {
      lo = fminf(lo, part[((size_t)b * 2 + 0) * cs + ch]);
      hi = fmaxf(hi, part[((size_t)b * 2 + 1) * cs + ch]);
    }
  }
  slo[sub][ch] = lo;
  shi[sub][ch] = hi;
  __syncthreads();
  if (sub == 0 && ch < c) {
    for (int s = 1; s < kThreads / kMaxC; ++s) {
      lo = fminf(lo, slo[s][ch]);
      hi = fmaxf(hi, shi[s][ch]);
    }
    write_qparams<true>(lo, hi, qmax, qp + ch * 4);
  }
}

// ---- quantise / dequantise, one thread per float of the NHWC buffer; pad channels get 0
__global__ void quantize_kernel(const float* __restrict__ x, long long npix, int c, int cs,
                                const float* __restrict__ qp, float qmax, uint8_t* __restrict__ q) {
  const float scale = qp[2], zp = qp[3];
  const long long total = npix * cs;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    float v = 0.f;
    if ((int)(e % cs) < c) v = quantize_one(x[e], scale, zp, qmax);
    q[e] = (uint8_t)v;
  }
}

__global__ void dequantize_kernel(const uint8_t* __restrict__ q, const float* __restrict__ qp, float* __restrict__ x,
                                  long long npix, int c, int cs) {
  const float scale = qp[2], zp = qp[3];
  const long long total = npix * cs;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x)
    x[e] = ((int)(e % cs) < c) ? dequantize_one((float)q[e], scale, zp) : 0.f;
}

// the code of logical NCHW value `value` in the payload of include/hnd_codec.h: at most two bytes (bits <= 8); the second
// byte is touched only when the value reaches into it, so never past the payload's last byte
__device__ __forceinline__ float payload_code(const uint8_t* __restrict__ payload, long long value, int bits, unsigned mask) {
  const long long bit = value * bits;
  const long long byte = bit >> 3;
  const int sh = (int)(bit & 7);
  unsigned two = payload[byte];
  if (sh + bits > 8) two |= (unsigned)payload[byte + 1] << 8;
  return (float)((two >> sh) & mask);
}

__global__ void unpack_dequantize_kernel(const uint8_t* __restrict__ payload, const float* __restrict__ qp,
                                         float* __restrict__ x, long long npix, int c, long long hw, int cs, int bits) {
  const float scale = qp[2], zp = qp[3];
  const long long total = npix * cs;
  const unsigned mask = (1u << bits) - 1u;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const long long p = e / cs;
    const int ch = (int)(e - p * cs);
    float v = 0.f;
    if (ch < c) {
      const long long img = p / hw, pix = p - img * hw;
      v = dequantize_one(payload_code(payload, (img * c + ch) * hw + pix, bits, mask), scale, zp);
    }
    x[e] = v;
  }
}

// ---- the same three, one lane per (pixel, group of 4 channels), built per policy.  The grid's row y takes the npix pixels
// from pixel y * npix on: the whole tensor in one row per channel, one IMAGE per row (npix = hw) where Params::kImageGrid
// says so, so that a workgroup's pair is its row's and no lane divides an image index out.  quantise: one 16-byte load and
// one 4-byte store per lane and pixel; a group without a real channel stores 0 unread
template <class Params>
__global__ void __launch_bounds__(kThreads) grouped_quantize_kernel(const float* __restrict__ x, long long npix, int c, int cs,
                                                                    const float* __restrict__ qp, float qmax,
                                                                    uint8_t* __restrict__ q) {
  const int groups = cs >> 2;
  const long long e0 = (long long)blockIdx.y * npix * cs;
  for (int gb = 0; gb < groups; gb += kThreads) {
    const int gc = groups - gb < kThreads ? groups - gb : kThreads;
    const int slots = kThreads / gc;
    const int gl = threadIdx.x % gc, slot = threadIdx.x / gc;
    if (slot >= slots) continue;
    const int ch0 = (gb + gl) * 4;
    Params par(qp, ch0, c);
    par.set_image(qp, blockIdx.y);
    for (long long p = (long long)blockIdx.x * slots + slot; p < npix; p += (long long)gridDim.x * slots) {
      const long long e = e0 + p * cs + ch0;
      unsigned word = 0;
      if (ch0 < c) {
        const f32x4 v = *(const f32x4*)(x + e);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (ch0 + k < c) word |= (unsigned)quantize_one(v[k], par.scale(k), par.zero(k), qmax) << (8 * k);
      }
      *(unsigned*)(q + e) = word;
    }
  }
}

// dequantise: one 4-byte load and one 16-byte store per lane and pixel, 0 into the pad channels
template <class Params>
__global__ void __launch_bounds__(kThreads) grouped_dequantize_kernel(const uint8_t* __restrict__ q,
                                                                      const float* __restrict__ qp, float* __restrict__ x,
                                                                      long long npix, int c, int cs) {
  const int groups = cs >> 2;
  const long long e0 = (long long)blockIdx.y * npix * cs;
  for (int gb = 0; gb < groups; gb += kThreads) {
    const int gc = groups - gb < kThreads ? groups - gb : kThreads;
    const int slots = kThreads / gc;
    const int gl = threadIdx.x % gc, slot = threadIdx.x / gc;
    if (slot >= slots) continue;
    const int ch0 = (gb + gl) * 4;
    Params par(qp, ch0, c);
    par.set_image(qp, blockIdx.y);
    for (long long p = (long long)blockIdx.x * slots + slot; p < npix; p += (long long)gridDim.x * slots) {
      const long long e = e0 + p * cs + ch0;
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if (ch0 < c) {
        const unsigned word = *(const unsigned*)(q + e);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (ch0 + k < c) o[k] = dequantize_one((float)((word >> (8 * k)) & 255u), par.scale(k), par.zero(k));
      }
      *(f32x4*)(x + e) = o;
    }
  }
}

// unpack + dequantise: a lane writes the 16 bytes of its group of a pixel; every real channel reads its value's bits
template <class Params>
__global__ void __launch_bounds__(kThreads) grouped_unpack_dequantize_kernel(const uint8_t* __restrict__ payload,
                                                                             const float* __restrict__ qp,
                                                                             float* __restrict__ x, long long npix, int c,
                                                                             long long hw, int cs, int bits) {
  const int groups = cs >> 2;
  const long long e0 = (long long)blockIdx.y * npix * cs;
  const unsigned mask = (1u << bits) - 1u;
  for (int gb = 0; gb < groups; gb += kThreads) {
    const int gc = groups - gb < kThreads ? groups - gb : kThreads;
    const int slots = kThreads / gc;
    const int gl = threadIdx.x % gc, slot = threadIdx.x / gc;
    if (slot >= slots) continue;
    const int ch0 = (gb + gl) * 4;
    Params par(qp, ch0, c);
    par.set_image(qp, blockIdx.y);
    for (long long p = (long long)blockIdx.x * slots + slot; p < npix; p += (long long)gridDim.x * slots) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if (ch0 < c) {
        const long long img = Params::kImageGrid ? (long long)blockIdx.y : p / hw, pix = p - (Params::kImageGrid ? 0 : img * hw);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (ch0 + k < c)
            o[k] = dequantize_one(payload_code(payload, (img * c + ch0 + k) * hw + pix, bits, mask), par.scale(k), par.zero(k));
      }
      *(f32x4*)(x + e0 + p * cs + ch0) = o;
    }
  }
}

// ---- quantise + pack: the payload of include/hnd_codec.h.  Value i of the logical NCHW tensor sits in bits
// [i * bits, (i + 1) * bits) of the byte stream, LSB first.  One thread owns a GROUP of 8 consecutive values = `bits` whole
// bytes starting at byte group * bits, so no two threads share a byte and every store is a plain byte store; the last group
// holds numel % 8 values when that is not 0 and stores ceil(rem * bits / 8) bytes.  The values of a group are gathered from
// the NHWC buffer; a group may cross a row, a channel plane or an image, so the channel and the image are tracked per value.
template <class Params>
__global__ void __launch_bounds__(Params::kPackBound) quantize_pack_kernel(const float* __restrict__ x, long long numel, int c,
                                                                            long long hw, int cs, int bits,
                                                                            const float* __restrict__ qp, float qmax,
                                                                            uint8_t* __restrict__ payload) {
  typename Params::Table tab = Params::stage_table(qp, c);
  if (Params::kTableInLds) __syncthreads();
  const long long groups = (numel + 7) >> 3;
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups;
       g += (long long)gridDim.x * blockDim.x) {
    const long long i0 = g << 3;
    const int count = numel - i0 < 8 ? (int)(numel - i0) : 8;
    NchwWalk<long long> at(i0, hw, c);
    unsigned long long word = 0;
    for (int k = 0; k < count; ++k) {
      tab.seek_image(at.img);
      const float v = quantize_one(x[at.offset(cs)], tab.scale(at.ch), tab.zero(at.ch), qmax);
      word |= (unsigned long long)(unsigned)v << (k * bits);
      at.next();
    }
    const int nbytes = (count * bits + 7) >> 3;                    // `bits` for a full group
    uint8_t* dst = payload + g * bits;
    for (int b = 0; b < nbytes; ++b) dst[b] = (uint8_t)(word >> (8 * b));
  }
}

// ---- fake quantise (include/hnd_qat.h): quantise and dequantise in one pass, the code kept in a register instead of a
// byte, in place or not, with the BatchNorm partial sums of what was stored.  One WAVE per tile of kFqRows pixels, lanes
// (row, group) with the group fastest, 64 / groups rows per pass (a pixel wider than 64 groups is walked 64 groups at a
// time); the per-lane sums meet in LDS and are added in row-slot order: the fixed order of the header, no atomics.  x and y
// may be the same buffer (every float is read and written by one lane), so neither is __restrict__.  A group without a real
// channel stores 0 unread.
// include/hnd_qrange.h builds the kernel with kMask: qparams are then a caller's fixed range, values may lie outside it, and
// `mask` (when not null) receives per pixel and group one byte whose bit k says that channel 4 g + k was NOT clipped -- one
// plain byte store per lane beside its 16-byte store of y, a wave's bytes consecutive like its loads.  Pad channels and the
// high nibble are 0.
// include/hnd_qimage.h builds it with PerImage: the tiles run over the global pixel index, `hw` pixels to an image (unused
// by the other policies), and a tile that straddles two images quantises each row on its own image's pair.
template <class Params, bool kMask>
__global__ void __launch_bounds__(64 * kFqWaves) fake_quantize_kernel(const float* x, float* y, long long npix, int c,
                                                                      int cs, const float* __restrict__ qp, float qmax,
                                                                      float* __restrict__ stats, int ntiles,
                                                                      uint8_t* __restrict__ mask, long long hw) {
  __shared__ float red[kFqWaves][64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int groups = cs >> 2;
  for (int t0 = blockIdx.x * kFqWaves; t0 < ntiles; t0 += gridDim.x * kFqWaves) {      // (uniform over the block)
    const int tile = t0 + wave;
    const long long row0 = (long long)tile * kFqRows;
    const int rows = tile < ntiles ? (npix - row0 < kFqRows ? (int)(npix - row0) : kFqRows) : 0;
    for (int gb = 0; gb < groups; gb += 64) {
      const int gc = groups - gb < 64 ? groups - gb : 64;         // groups in this pass
      const int slots = 64 / gc;                                  // rows per pass
      const int gl = lane % gc, slot = lane / gc;
      const int ch0 = (gb + gl) * 4;
      Params par(qp, ch0, c);
      float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
      if (slot < slots) {
        if (rows > 0) par.begin_tile(qp, row0, hw);                // (a wave past the last tile has no image)
        for (int r = slot; r < rows; r += slots) {
          par.seek_row(qp, r);
          const long long e = (row0 + r) * cs + ch0;
          f32x4 o = {0.f, 0.f, 0.f, 0.f};
          unsigned pass = 0;
          if (ch0 < c) {
            const f32x4 v = *(const f32x4*)(x + e);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              if (ch0 + k < c) {
                const float u = unclamped_code(v[k], par.scale(k), par.zero(k));
                if (kMask) pass |= inside_range(u, qmax) ? 1u << k : 0u;
                o[k] = dequantize_one(clamp_round(u, qmax), par.scale(k), par.zero(k));
              }
            }
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            s[k] = __fadd_rn(s[k], o[k]);
            ss[k] = Params::square_sum(ss[k], o[k]);
          }
          *(f32x4*)(y + e) = o;
          if (kMask && mask != nullptr) mask[(row0 + r) * groups + gb + gl] = (uint8_t)pass;
        }
      }
      if (stats != nullptr) {                                    // (uniform over the block)
#pragma unroll
        for (int k = 0; k < 4; ++k) { red[wave][lane][k] = s[k]; red[wave][lane][4 + k] = ss[k]; }
        __syncthreads();
        if (rows > 0) {
          for (int i = lane; i < gc * 8; i += 64) {
            const int g = i >> 3, k = i & 7;
            float acc = 0.f;
            for (int sl = 0; sl < slots; ++sl) acc = __fadd_rn(acc, red[wave][sl * gc + g][k]);
            stats[((size_t)tile * 2 + (k >> 2)) * cs + (gb + g) * 4 + (k & 3)] = acc;
          }
        }
        __syncthreads();
      }
    }
  }
}

// the backward of the clipping: one thread per 4-channel group (one mask byte, one 16-byte load and store); a clipped real
// channel gets +0, everything else -- pad channels included -- keeps its bits
__global__ void qrange_mask_grad_kernel(float* __restrict__ g, const uint8_t* __restrict__ mask, long long ngroups, int c,
                                        int groups) {
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < ngroups;
       e += (long long)gridDim.x * blockDim.x) {
    const int ch0 = (int)(e % groups) * 4;
    const unsigned m = mask[e];
    f32x4 v = *(const f32x4*)(g + e * 4);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ch0 + k < c && !((m >> k) & 1u)) v[k] = 0.f;
    *(f32x4*)(g + e * 4) = v;
  }
}

__global__ void roundtrip_f16_kernel(float* x, long long n) {
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
    x[e] = __half2float(__float2half(x[e]));
}

// ---- host
inline int grid_for(long long work_items) {
  long long b = (work_items + kThreads - 1) / kThreads;
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// the grid of the grouped kernels: one pass of a workgroup takes kThreads / groups pixels
inline int pixel_grid(long long npix, int cs) {
  const int groups = cs >> 2;
  const int slots = kThreads / (groups < kThreads ? groups : kThreads);
  long long b = (npix + slots - 1) / slots;
  return (int)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

inline bool aligned(unsigned to, const void* a, const void* b = nullptr, const void* c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & (to - 1)) == 0;
}

inline float qmax_of(int bits) { return (float)((1 << bits) - 1); }

// the two launches every export that measures the batch starts with, one per flavour.  Per tensor, `state` folds the batch
// range into the running one (hnd_qrange_observe) and is null everywhere else.
void launch_qparams(const float* x, long long npix, int c, int cs, float qmax, float* qparams, float* scratch, hipStream_t s,
                    float momentum = 0.f, float* state = nullptr) {
  int nb = grid_for(npix * cs);
  if (nb > kPartBlocks) nb = kPartBlocks;
  hipLaunchKernelGGL(minmax_kernel, dim3(nb), dim3(kThreads), 0, s, x, npix, c, cs, scratch);
  hipLaunchKernelGGL(qparams_kernel<false>, dim3(1), dim3(64), 0, s, scratch, nb, momentum, qmax, state, qparams);
}

void qc_launch_qparams(const float* x, long long npix, int c, int cs, float qmax, float* qparams, float* scratch,
                       hipStream_t s) {
  const int slots = kThreads / ((c + 3) >> 2);
  long long b = (npix + slots - 1) / slots;
  const int nb = (int)(b > kPartBlocks ? kPartBlocks : b);
  hipLaunchKernelGGL(qc_minmax_kernel, dim3(nb), dim3(kThreads), 0, s, x, npix, c, cs, scratch);
  hipLaunchKernelGGL(qc_qparams_kernel, dim3(1), dim3(kThreads), 0, s, scratch, nb, c, cs, qmax, qparams);
}

// per image: workgroups per image for hw pixels when a pass of one workgroup takes `slots` of them, at most `cap`
inline int image_blocks(long long hw, int slots, int cap) {
  const long long b = (hw + slots - 1) / slots;
  return (int)(b > cap ? cap : b);
}

void image_launch_qparams(const float* x, int n, long long hw, int c, int cs, float qmax, float* qparams, float* scratch,
                          hipStream_t s) {
  const int gr = (c + 3) >> 2;
  const int nb = image_blocks(hw, kThreads / (gr < kThreads ? gr : kThreads), kImageBlocks);
  hipLaunchKernelGGL(image_minmax_kernel, dim3(nb, n), dim3(kThreads), 0, s, x, hw, c, cs, scratch);
  hipLaunchKernelGGL(qparams_kernel<true>, dim3(n), dim3(64), 0, s, scratch, nb, 0.f, qmax, (float*)nullptr, qparams);
}

// the grid of the grouped kernels per image: (workgroups per image, n), about kMaxBlocks workgroups in all
inline dim3 image_grid(int n, long long hw, int cs) {
  const int groups = cs >> 2;
  const int cap = kMaxBlocks / n;
  return dim3(image_blocks(hw, kThreads / (groups < kThreads ? groups : kThreads), cap < 1 ? 1 : cap), n);
}

void launch_quantize(const float* x, long long npix, int c, int cs, const float* qparams, float qmax, uint8_t* q,
                     hipStream_t s) {
  hipLaunchKernelGGL(quantize_kernel, dim3(grid_for(npix * cs)), dim3(kThreads), 0, s, x, npix, c, cs, qparams, qmax, q);
}

template <class Params>
void launch_pack(const float* x, int n, int h, int w, int c, int cs, int bits, const float* qparams, uint8_t* payload,
                 hipStream_t s) {
  const long long hw = (long long)h * w, numel = hw * n * c;
  hipLaunchKernelGGL(quantize_pack_kernel<Params>, dim3(grid_for((numel + 7) / 8)), dim3(kThreads), 0, s, x, numel, c, hw, cs,
                     bits, qparams, qmax_of(bits), payload);
}

template <class Params, bool kMask>
void launch_fake_quantize(const float* x, float* y, long long npix, int c, int cs, int bits, const float* qparams,
                          float* stats, int ntiles, uint8_t* mask, hipStream_t s, long long hw = 0) {
  int nb = (ntiles + kFqWaves - 1) / kFqWaves;
  if (nb > kMaxBlocks) nb = kMaxBlocks;
  hipLaunchKernelGGL((fake_quantize_kernel<Params, kMask>), dim3(nb), dim3(64 * kFqWaves), 0, s, x, y, npix, c, cs, qparams,
                     qmax_of(bits), stats, ntiles, mask, hw);
}

// hnd_quantize_bits, and hnd_quantize_u8 as its 8-bit case: the caller has checked its arguments under its own name
int quantize_bits(const char* who, const float* x, long long npix, int c, int cs, int bits, uint8_t* q, float* qparams,
                  float* scratch, void* stream) {
  hipStream_t s = hnd::as_stream(stream);
  launch_qparams(x, npix, c, cs, qmax_of(bits), qparams, scratch, s);
  launch_quantize(x, npix, c, cs, qparams, qmax_of(bits), q, s);
  return hnd::check_launch(who);
}

}  // namespace

// ---- the argument checks.  Every export keeps its own texts, so the helpers take the export's name; they read the
// export's arguments by their names (bits, npix, n, h, w, c, cs).
#define REQUIRE_POINTERS(who, all) HND_REQUIRE(all, who ": null pointer")
#define REQUIRE_BITS(who) HND_REQUIRE(bits >= 1 && bits <= 8, who ": bits %d outside 1 ... 8", bits)
// per tensor: any cs >= c; the grouped kernels (fake quantiser, fixed range) add cs % 4 == 0
#define REQUIRE_NPIX(who) HND_REQUIRE(npix > 0 && c > 0 && cs >= c, who ": bad geometry (npix > 0, c > 0, cs >= c)")
#define REQUIRE_NPIX_BY4(who) \
  HND_REQUIRE(npix > 0 && c > 0 && cs >= c && cs % 4 == 0, who ": bad geometry (npix > 0, c > 0, cs >= c, cs %% 4 == 0)")
#define REQUIRE_NHW(who) \
  HND_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && cs >= c, who ": bad geometry (n, h, w, c > 0, cs >= c)")
#define REQUIRE_NHW_BY4(who)                                               \
  HND_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && cs >= c && cs % 4 == 0, \
              who ": bad geometry (n, h, w, c > 0, cs >= c, cs %% 4 == 0)")
#define REQUIRE_TILES(who) HND_REQUIRE(ntiles > 0, who ": npix too large (the tile count must fit an int)")
// per channel
#define REQUIRE_CHANNELS(who)                                                        \
  HND_REQUIRE(c >= 1 && c <= kMaxC, who ": c %d outside 1 ... %d", c, kMaxC);         \
  HND_REQUIRE(cs >= c && cs % 4 == 0, who ": bad pixel stride %d (cs >= c, cs %% 4 == 0)", cs)
#define REQUIRE_POSITIVE_NPIX(who) HND_REQUIRE(npix > 0, who ": npix must be positive")
#define REQUIRE_POSITIVE_NHW(who) HND_REQUIRE(n > 0 && h > 0 && w > 0, who ": n, h and w must be positive")
// per image (reads hw as well; the pack / unpack exports make it from h and w first)
#define REQUIRE_IMAGES(who)                                                                                   \
  HND_REQUIRE(n >= 1 && n <= HND_QIMAGE_MAX_N, who ": n %d outside 1 ... %d", n, HND_QIMAGE_MAX_N);            \
  HND_REQUIRE(hw > 0, who ": hw (h, w) must be positive");                                                    \
  HND_REQUIRE(c > 0 && cs >= c && cs % 4 == 0, who ": bad pixel (c %d > 0, stride %d >= c, stride %% 4 == 0)", c, cs); \
  HND_REQUIRE(hw <= LLONG_MAX / cs / n, who ": too many pixels (n * hw * cs must fit an int64)")

extern "C" {

// ---- hnd_hip.h: the 8-bit codec and the fp16 link
size_t hnd_minmax_scratch_elems(void) { return 2 * kPartBlocks; }

int hnd_quantize_u8(const float* x, int64_t npix, int c, int cs, uint8_t* q, float* qparams, float* scratch,
                    void* stream) {
  HND_REQUIRE(x && q && qparams && scratch && npix > 0 && c > 0 && cs >= c, "hnd_quantize_u8: bad arguments");
  return quantize_bits("hnd_quantize_u8", x, npix, c, cs, 8, q, qparams, scratch, stream);
}

int hnd_dequantize_u8(const uint8_t* q, const float* qparams, float* x, int64_t npix, int c, int cs, void* stream) {
  HND_REQUIRE(q && qparams && x && npix > 0 && c > 0 && cs >= c, "hnd_dequantize_u8: bad arguments");
  hipLaunchKernelGGL(dequantize_kernel, dim3(grid_for((long long)npix * cs)), dim3(kThreads), 0, hnd::as_stream(stream), q,
                     qparams, x, (long long)npix, c, cs);
  return hnd::check_launch("hnd_dequantize_u8");
}

int hnd_roundtrip_f16(float* x, int64_t numel, void* stream) {
  HND_REQUIRE(x && numel > 0, "hnd_roundtrip_f16: bad arguments");
  hipLaunchKernelGGL(roundtrip_f16_kernel, dim3(grid_for(numel)), dim3(kThreads), 0, hnd::as_stream(stream), x,
                     (long long)numel);
  return hnd::check_launch("hnd_roundtrip_f16");
}

// ---- include/hnd_codec.h: the codec at 1 ... 8 bits and the bit-packed payload
int hnd_codec_abi(void) { return HND_CODEC_ABI; }

size_t hnd_codec_packed_bytes(int64_t numel, int bits) {
  if (numel <= 0 || bits < 1 || bits > 8) return 0;
  return (size_t)(numel >> 3) * bits + (size_t)(((numel & 7) * bits + 7) >> 3);      // ceil(numel * bits / 8), no overflow
}

int hnd_quantize_bits(const float* x, int64_t npix, int c, int cs, int bits, uint8_t* q, float* qparams, float* scratch,
                      void* stream) {
  REQUIRE_POINTERS("hnd_quantize_bits", x && q && qparams && scratch);
  REQUIRE_BITS("hnd_quantize_bits");
  REQUIRE_NPIX("hnd_quantize_bits");
  return quantize_bits("hnd_quantize_bits", x, npix, c, cs, bits, q, qparams, scratch, stream);
}

int hnd_quantize_pack_bits(const float* x, int n, int h, int w, int c, int cs, int bits, uint8_t* payload, float* qparams,
                           float* scratch, void* stream) {
  REQUIRE_POINTERS("hnd_quantize_pack_bits", x && payload && qparams && scratch);
  REQUIRE_BITS("hnd_quantize_pack_bits");
  REQUIRE_NHW("hnd_quantize_pack_bits");
  hipStream_t s = hnd::as_stream(stream);
  launch_qparams(x, (long long)h * w * n, c, cs, qmax_of(bits), qparams, scratch, s);
  launch_pack<PerTensor>(x, n, h, w, c, cs, bits, qparams, payload, s);
  return hnd::check_launch("hnd_quantize_pack_bits");
}

int hnd_unpack_dequantize_bits(const uint8_t* payload, const float* qparams, float* x, int n, int h, int w, int c, int cs,
                               int bits, void* stream) {
  REQUIRE_POINTERS("hnd_unpack_dequantize_bits", payload && qparams && x);
  REQUIRE_BITS("hnd_unpack_dequantize_bits");
  REQUIRE_NHW("hnd_unpack_dequantize_bits");
  const long long hw = (long long)h * w, npix = hw * n;
  hipLaunchKernelGGL(unpack_dequantize_kernel, dim3(grid_for(npix * cs)), dim3(kThreads), 0, hnd::as_stream(stream), payload,
                     qparams, x, npix, c, hw, cs, bits);
  return hnd::check_launch("hnd_unpack_dequantize_bits");
}

// ---- include/hnd_qat.h: the fake-quantised bottleneck of the training step
int hnd_qat_abi(void) { return HND_QAT_ABI; }

int hnd_fake_quantize_tiles(int64_t npix) {
  if (npix <= 0) return 0;
  const int64_t t = (npix + kFqRows - 1) / kFqRows;
  return t > INT_MAX ? 0 : (int)t;
}

int hnd_fake_quantize_bits(const float* x, float* y, int64_t npix, int c, int cs, int bits, float* qparams, float* scratch,
                           float* stats, void* stream) {
  REQUIRE_POINTERS("hnd_fake_quantize_bits", x && y && qparams && scratch);
  REQUIRE_BITS("hnd_fake_quantize_bits");
  REQUIRE_NPIX_BY4("hnd_fake_quantize_bits");
  const int ntiles = hnd_fake_quantize_tiles(npix);
  REQUIRE_TILES("hnd_fake_quantize_bits");
  HND_REQUIRE(aligned(16, x, y), "hnd_fake_quantize_bits: x and y must be 16-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  launch_qparams(x, (long long)npix, c, cs, qmax_of(bits), qparams, scratch, s);
  launch_fake_quantize<PerTensor, false>(x, y, (long long)npix, c, cs, bits, qparams, stats, ntiles, nullptr, s);
  return hnd::check_launch("hnd_fake_quantize_bits");
}

// ---- include/hnd_qrange.h: the fixed (EMA-calibrated) range
int hnd_qrange_abi(void) { return HND_QRANGE_ABI; }

int hnd_qrange_observe(const float* x, int64_t npix, int c, int cs, float momentum, int bits, float* state, float* qparams,
                       float* scratch, void* stream) {
  REQUIRE_POINTERS("hnd_qrange_observe", x && state && qparams && scratch);
  REQUIRE_BITS("hnd_qrange_observe");
  REQUIRE_NPIX_BY4("hnd_qrange_observe");
  HND_REQUIRE(momentum > 0.f && momentum <= 1.f, "hnd_qrange_observe: momentum outside (0, 1]");
  HND_REQUIRE(aligned(16, x, state, qparams), "hnd_qrange_observe: x, state and qparams must be 16-byte aligned");
  launch_qparams(x, (long long)npix, c, cs, qmax_of(bits), qparams, scratch, hnd::as_stream(stream), momentum, state);
  return hnd::check_launch("hnd_qrange_observe");
}

int hnd_qrange_qparams(float lo, float hi, int bits, float* qparams, void* stream) {
  REQUIRE_POINTERS("hnd_qrange_qparams", qparams);
  REQUIRE_BITS("hnd_qrange_qparams");
  HND_REQUIRE(std::isfinite(lo) && std::isfinite(hi) && lo < hi, "hnd_qrange_qparams: the range needs finite lo < hi");
  HND_REQUIRE(aligned(16, qparams), "hnd_qrange_qparams: qparams must be 16-byte aligned");
  hipLaunchKernelGGL(qrange_qparams_kernel, dim3(1), dim3(1), 0, hnd::as_stream(stream), lo, hi, qmax_of(bits), qparams);
  return hnd::check_launch("hnd_qrange_qparams");
}

int hnd_fake_quantize_range(const float* x, float* y, int64_t npix, int c, int cs, int bits, const float* qparams,
                            uint8_t* mask, float* stats, void* stream) {
  REQUIRE_POINTERS("hnd_fake_quantize_range", x && y && qparams);
  REQUIRE_BITS("hnd_fake_quantize_range");
  REQUIRE_NPIX_BY4("hnd_fake_quantize_range");
  const int ntiles = hnd_fake_quantize_tiles(npix);
  REQUIRE_TILES("hnd_fake_quantize_range");
  HND_REQUIRE(aligned(16, x, y, qparams), "hnd_fake_quantize_range: x, y and qparams must be 16-byte aligned");
  launch_fake_quantize<PerTensor, true>(x, y, (long long)npix, c, cs, bits, qparams, stats, ntiles, mask,
                                        hnd::as_stream(stream));
  return hnd::check_launch("hnd_fake_quantize_range");
}

int hnd_qrange_mask_grad(float* g, const uint8_t* mask, int64_t npix, int c, int cs, void* stream) {
  REQUIRE_POINTERS("hnd_qrange_mask_grad", g && mask);
  REQUIRE_NPIX_BY4("hnd_qrange_mask_grad");
  HND_REQUIRE(aligned(16, g), "hnd_qrange_mask_grad: g must be 16-byte aligned");
  const long long ngroups = (long long)npix * (cs / 4);
  hipLaunchKernelGGL(qrange_mask_grad_kernel, dim3(grid_for(ngroups)), dim3(kThreads), 0, hnd::as_stream(stream), g, mask,
                     ngroups, c, cs / 4);
  return hnd::check_launch("hnd_qrange_mask_grad");
}

int hnd_quantize_range_bits(const float* x, int64_t npix, int c, int cs, int bits, uint8_t* q, const float* qparams,
                            void* stream) {
  REQUIRE_POINTERS("hnd_quantize_range_bits", x && q && qparams);
  REQUIRE_BITS("hnd_quantize_range_bits");
  REQUIRE_NPIX_BY4("hnd_quantize_range_bits");
  HND_REQUIRE(aligned(16, x, qparams), "hnd_quantize_range_bits: x and qparams must be 16-byte aligned");
  launch_quantize(x, (long long)npix, c, cs, qparams, qmax_of(bits), q, hnd::as_stream(stream));
  return hnd::check_launch("hnd_quantize_range_bits");
}

int hnd_quantize_pack_range_bits(const float* x, int n, int h, int w, int c, int cs, int bits, uint8_t* payload,
                                 const float* qparams, void* stream) {
  REQUIRE_POINTERS("hnd_quantize_pack_range_bits", x && payload && qparams);
  REQUIRE_BITS("hnd_quantize_pack_range_bits");
  REQUIRE_NHW_BY4("hnd_quantize_pack_range_bits");
  HND_REQUIRE(aligned(16, x, qparams), "hnd_quantize_pack_range_bits: x and qparams must be 16-byte aligned");
  launch_pack<PerTensor>(x, n, h, w, c, cs, bits, qparams, payload, hnd::as_stream(stream));
  return hnd::check_launch("hnd_quantize_pack_range_bits");
}

// ---- include/hnd_qchannel.h: one (scale, zero point) per channel
int hnd_qchannel_abi(void) { return HND_QCHANNEL_ABI; }

size_t hnd_qchannel_scratch_elems(int cs) {
  if (cs <= 0 || cs % 4 != 0) return 0;
  return (size_t)kPartBlocks * 2 * (size_t)cs;
}

int hnd_qchannel_quantize_bits(const float* x, int64_t npix, int c, int cs, int bits, uint8_t* q, float* qparams,
                               float* scratch, void* stream) {
  REQUIRE_POINTERS("hnd_qchannel_quantize_bits", x && q && qparams && scratch);
  REQUIRE_BITS("hnd_qchannel_quantize_bits");
  REQUIRE_CHANNELS("hnd_qchannel_quantize_bits");
  REQUIRE_POSITIVE_NPIX("hnd_qchannel_quantize_bits");
  HND_REQUIRE(aligned(16, x) && aligned(4, q), "hnd_qchannel_quantize_bits: x must be 16-byte aligned and q 4-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  qc_launch_qparams(x, (long long)npix, c, cs, qmax_of(bits), qparams, scratch, s);
  hipLaunchKernelGGL(grouped_quantize_kernel<PerChannel>, dim3(pixel_grid(npix, cs)), dim3(kThreads), 0, s, x, (long long)npix, c, cs, qparams,
                     qmax_of(bits), q);
  return hnd::check_launch("hnd_qchannel_quantize_bits");
}

int hnd_qchannel_dequantize_u8(const uint8_t* q, const float* qparams, float* x, int64_t npix, int c, int cs, void* stream) {
  REQUIRE_POINTERS("hnd_qchannel_dequantize_u8", q && qparams && x);
  REQUIRE_CHANNELS("hnd_qchannel_dequantize_u8");
  REQUIRE_POSITIVE_NPIX("hnd_qchannel_dequantize_u8");
  HND_REQUIRE(aligned(16, x) && aligned(4, q), "hnd_qchannel_dequantize_u8: x must be 16-byte aligned and q 4-byte aligned");
  hipLaunchKernelGGL(grouped_dequantize_kernel<PerChannel>, dim3(pixel_grid(npix, cs)), dim3(kThreads), 0, hnd::as_stream(stream), q, qparams,
                     x, (long long)npix, c, cs);
  return hnd::check_launch("hnd_qchannel_dequantize_u8");
}

int hnd_qchannel_quantize_pack_bits(const float* x, int n, int h, int w, int c, int cs, int bits, uint8_t* payload,
                                    float* qparams, float* scratch, void* stream) {
  REQUIRE_POINTERS("hnd_qchannel_quantize_pack_bits", x && payload && qparams && scratch);
  REQUIRE_BITS("hnd_qchannel_quantize_pack_bits");
  REQUIRE_CHANNELS("hnd_qchannel_quantize_pack_bits");
  REQUIRE_POSITIVE_NHW("hnd_qchannel_quantize_pack_bits");
  HND_REQUIRE(aligned(16, x), "hnd_qchannel_quantize_pack_bits: x must be 16-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  qc_launch_qparams(x, (long long)h * w * n, c, cs, qmax_of(bits), qparams, scratch, s);
  launch_pack<PerChannel>(x, n, h, w, c, cs, bits, qparams, payload, s);
  return hnd::check_launch("hnd_qchannel_quantize_pack_bits");
}

int hnd_qchannel_unpack_dequantize_bits(const uint8_t* payload, const float* qparams, float* x, int n, int h, int w, int c,
                                        int cs, int bits, void* stream) {
  REQUIRE_POINTERS("hnd_qchannel_unpack_dequantize_bits", payload && qparams && x);
  REQUIRE_BITS("hnd_qchannel_unpack_dequantize_bits");
  REQUIRE_CHANNELS("hnd_qchannel_unpack_dequantize_bits");
  REQUIRE_POSITIVE_NHW("hnd_qchannel_unpack_dequantize_bits");
  HND_REQUIRE(aligned(16, x), "hnd_qchannel_unpack_dequantize_bits: x must be 16-byte aligned");
  const long long hw = (long long)h * w, npix = hw * n;
  hipLaunchKernelGGL(grouped_unpack_dequantize_kernel<PerChannel>, dim3(pixel_grid(npix, cs)), dim3(kThreads), 0, hnd::as_stream(stream),
                     payload, qparams, x, npix, c, hw, cs, bits);
  return hnd::check_launch("hnd_qchannel_unpack_dequantize_bits");
}

int hnd_qchannel_fake_quantize_bits(const float* x, float* y, int64_t npix, int c, int cs, int bits, float* qparams,
                                    float* scratch, float* stats, void* stream) {
  REQUIRE_POINTERS("hnd_qchannel_fake_quantize_bits", x && y && qparams && scratch);
  REQUIRE_BITS("hnd_qchannel_fake_quantize_bits");
  REQUIRE_CHANNELS("hnd_qchannel_fake_quantize_bits");
  REQUIRE_POSITIVE_NPIX("hnd_qchannel_fake_quantize_bits");
  const int ntiles = hnd_fake_quantize_tiles(npix);
  REQUIRE_TILES("hnd_qchannel_fake_quantize_bits");
  HND_REQUIRE(aligned(16, x, y), "hnd_qchannel_fake_quantize_bits: x and y must be 16-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  qc_launch_qparams(x, (long long)npix, c, cs, qmax_of(bits), qparams, scratch, s);
  launch_fake_quantize<PerChannel, false>(x, y, (long long)npix, c, cs, bits, qparams, stats, ntiles, nullptr, s);
  return hnd::check_launch("hnd_qchannel_fake_quantize_bits");
}

// ---- include/hnd_qimage.h: one (scale, zero point) per image
int hnd_qimage_abi(void) { return HND_QIMAGE_ABI; }

size_t hnd_qimage_scratch_elems(int n) {
  if (n < 1 || n > HND_QIMAGE_MAX_N) return 0;
  return (size_t)n * kImageBlocks * 2;
}

int hnd_qimage_quantize_bits(const float* x, int n, int64_t hw, int c, int cs, int bits, uint8_t* q, float* qparams,
                             float* scratch, void* stream) {
  REQUIRE_POINTERS("hnd_qimage_quantize_bits", x && q && qparams && scratch);
  REQUIRE_BITS("hnd_qimage_quantize_bits");
  REQUIRE_IMAGES("hnd_qimage_quantize_bits");
  HND_REQUIRE(aligned(16, x) && aligned(4, q), "hnd_qimage_quantize_bits: x must be 16-byte aligned and q 4-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  image_launch_qparams(x, n, (long long)hw, c, cs, qmax_of(bits), qparams, scratch, s);
  hipLaunchKernelGGL(grouped_quantize_kernel<PerImage>, image_grid(n, hw, cs), dim3(kThreads), 0, s, x, (long long)hw, c, cs,
                     qparams, qmax_of(bits), q);
  return hnd::check_launch("hnd_qimage_quantize_bits");
}

int hnd_qimage_dequantize_u8(const uint8_t* q, const float* qparams, float* x, int n, int64_t hw, int c, int cs,
                             void* stream) {
  REQUIRE_POINTERS("hnd_qimage_dequantize_u8", q && qparams && x);
  REQUIRE_IMAGES("hnd_qimage_dequantize_u8");
  HND_REQUIRE(aligned(16, x) && aligned(4, q), "hnd_qimage_dequantize_u8: x must be 16-byte aligned and q 4-byte aligned");
  hipLaunchKernelGGL(grouped_dequantize_kernel<PerImage>, image_grid(n, hw, cs), dim3(kThreads), 0, hnd::as_stream(stream), q,
                     qparams, x, (long long)hw, c, cs);
  return hnd::check_launch("hnd_qimage_dequantize_u8");
}

int hnd_qimage_quantize_pack_bits(const float* x, int n, int h, int w, int c, int cs, int bits, uint8_t* payload,
                                  float* qparams, float* scratch, void* stream) {
  const long long hw = h > 0 && w > 0 ? (long long)h * w : 0;
  REQUIRE_POINTERS("hnd_qimage_quantize_pack_bits", x && payload && qparams && scratch);
  REQUIRE_BITS("hnd_qimage_quantize_pack_bits");
  REQUIRE_IMAGES("hnd_qimage_quantize_pack_bits");
  HND_REQUIRE(aligned(16, x), "hnd_qimage_quantize_pack_bits: x must be 16-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  image_launch_qparams(x, n, hw, c, cs, qmax_of(bits), qparams, scratch, s);
  launch_pack<PerImage>(x, n, h, w, c, cs, bits, qparams, payload, s);
  return hnd::check_launch("hnd_qimage_quantize_pack_bits");
}

int hnd_qimage_unpack_dequantize_bits(const uint8_t* payload, const float* qparams, float* x, int n, int h, int w, int c,
                                      int cs, int bits, void* stream) {
  const long long hw = h > 0 && w > 0 ? (long long)h * w : 0;
  REQUIRE_POINTERS("hnd_qimage_unpack_dequantize_bits", payload && qparams && x);
  REQUIRE_BITS("hnd_qimage_unpack_dequantize_bits");
  REQUIRE_IMAGES("hnd_qimage_unpack_dequantize_bits");
  HND_REQUIRE(aligned(16, x), "hnd_qimage_unpack_dequantize_bits: x must be 16-byte aligned");
  hipLaunchKernelGGL(grouped_unpack_dequantize_kernel<PerImage>, image_grid(n, hw, cs), dim3(kThreads), 0,
                     hnd::as_stream(stream), payload, qparams, x, hw, c, hw, cs, bits);
  return hnd::check_launch("hnd_qimage_unpack_dequantize_bits");
}

int hnd_qimage_fake_quantize_bits(const float* x, float* y, int n, int64_t hw, int c, int cs, int bits, float* qparams,
                                  float* scratch, float* stats, void* stream) {
  REQUIRE_POINTERS("hnd_qimage_fake_quantize_bits", x && y && qparams && scratch);
  REQUIRE_BITS("hnd_qimage_fake_quantize_bits");
  REQUIRE_IMAGES("hnd_qimage_fake_quantize_bits");
  const long long npix = (long long)n * hw;
  const int ntiles = hnd_fake_quantize_tiles(npix);
  REQUIRE_TILES("hnd_qimage_fake_quantize_bits");
  HND_REQUIRE(aligned(16, x, y), "hnd_qimage_fake_quantize_bits: x and y must be 16-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  image_launch_qparams(x, n, (long long)hw, c, cs, qmax_of(bits), qparams, scratch, s);
  launch_fake_quantize<PerImage, false>(x, y, npix, c, cs, bits, qparams, stats, ntiles, nullptr, s, (long long)hw);
  return hnd::check_launch("hnd_qimage_fake_quantize_bits");
}

}  // extern "C"
