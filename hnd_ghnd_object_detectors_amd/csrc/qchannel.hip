// include/hnd_qchannel.h: the bottleneck codec and the fake quantiser with one (scale, zero point) per channel.  The formulas
// and formats are the header's; this file is the two launches that make qparams[c][4] and the one launch of every export.
// Byte work that must equal the per-tensor kernels of csrc/elementwise.hip on a single channel: the file is built without
// FMA contraction.
//
// Lane layout of every kernel but the packer: the lanes of a workgroup are laid out as (pixel, group of 4 channels) with the
// group fastest, so a wave's 16-byte loads cover consecutive bytes and a lane KEEPS its group: its four scales and zero
// points are read once and live in registers for the whole launch.  A pixel wider than the workgroup is walked one
// workgroup's worth of groups at a time.
#include "common.h"
#include "hnd_qat.h"
#include "hnd_qchannel.h"

namespace {

using hnd::f32x4;

constexpr int kThreads = 256;
constexpr int kPartBlocks = 512;         // rows of the min / max partial in scratch
constexpr int kMaxBlocks = 256 * 16;
constexpr int kMaxC = HND_QCHANNEL_MAX_C;
constexpr int kFqRows = HND_FAKE_QUANT_TILE_ROWS;
constexpr int kFqWaves = 4;

// ---- launch 1: per-lane min / max of its four channels, lanes of the same group meet in LDS, one partial [2][cs] per
// workgroup.  Only the groups that hold a real channel are read (c <= 64: at most 16 of them, so one pass).
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

// ---- launch 2: the partials reduced per channel, then qparams[ch] = {min, max, scale, zero_point} -- qparams_kernel's
// sequence (csrc/elementwise.hip) plus the header's rule for a constant channel
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
    float scale;
    if (hi != lo) scale = __fdiv_rn(__fsub_rn(hi, lo), qmax);      // (max - min) / (qmax - qmin), qmin = 0
    else scale = lo != 0.f ? fabsf(lo) : 1.f;                      // a constant channel: reproduced exactly (header)
    float zp = __fsub_rn(0.f, __fdiv_rn(lo, scale));               // qmin - min / scale
    zp = zp < 0.f ? 0.f : (zp > qmax ? qmax : zp);
    qp[ch * 4 + 0] = lo;
    qp[ch * 4 + 1] = hi;
    qp[ch * 4 + 2] = scale;
    qp[ch * 4 + 3] = truncf(zp);                                   // int(zero_point)
  }
}

// the four (scale, zero point) of the group that begins at channel ch0; channels that are not real get (1, 0), unused
__device__ __forceinline__ void lane_qparams(const float* __restrict__ qp, int ch0, int c, float (&sc)[4], float (&zp)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool real = ch0 + k < c;
    sc[k] = real ? qp[(ch0 + k) * 4 + 2] : 1.f;
    zp[k] = real ? qp[(ch0 + k) * 4 + 3] : 0.f;
  }
}

__device__ __forceinline__ float quantize_one(float v, float scale, float zp, float qmax) {
  float q = __fadd_rn(zp, __fdiv_rn(v, scale));                    // zero_point + x / scale
  q = q < 0.f ? 0.f : (q > qmax ? qmax : q);                       // clamp_(qmin, qmax)
  return rintf(q);                                                 // round_(): half to even
}

// ---- quantise: one 16-byte load and one 4-byte store per lane and pixel; a group without a real channel stores 0 unread
__global__ void __launch_bounds__(kThreads) qc_quantize_kernel(const float* __restrict__ x, long long npix, int c, int cs,
                                                               const float* __restrict__ qp, float qmax,
                                                               uint8_t* __restrict__ q) {
  const int groups = cs >> 2;
  for (int gb = 0; gb < groups; gb += kThreads) {
    const int gc = groups - gb < kThreads ? groups - gb : kThreads;
    const int slots = kThreads / gc;
    const int gl = threadIdx.x % gc, slot = threadIdx.x / gc;
    if (slot >= slots) continue;
    const int ch0 = (gb + gl) * 4;
    float sc[4], zp[4];
    lane_qparams(qp, ch0, c, sc, zp);
    for (long long p = (long long)blockIdx.x * slots + slot; p < npix; p += (long long)gridDim.x * slots) {
      const long long e = p * cs + ch0;
      unsigned word = 0;
      if (ch0 < c) {
        const f32x4 v = *(const f32x4*)(x + e);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (ch0 + k < c) word |= (unsigned)quantize_one(v[k], sc[k], zp[k], qmax) << (8 * k);
      }
      *(unsigned*)(q + e) = word;
    }
  }
}

// ---- dequantise: one 4-byte load and one 16-byte store per lane and pixel, 0 into the pad channels
__global__ void __launch_bounds__(kThreads) qc_dequantize_kernel(const uint8_t* __restrict__ q, const float* __restrict__ qp,
                                                                 float* __restrict__ x, long long npix, int c, int cs) {
  const int groups = cs >> 2;
  for (int gb = 0; gb < groups; gb += kThreads) {
    const int gc = groups - gb < kThreads ? groups - gb : kThreads;
    const int slots = kThreads / gc;
    const int gl = threadIdx.x % gc, slot = threadIdx.x / gc;
    if (slot >= slots) continue;
    const int ch0 = (gb + gl) * 4;
    float sc[4], zp[4];
    lane_qparams(qp, ch0, c, sc, zp);
    for (long long p = (long long)blockIdx.x * slots + slot; p < npix; p += (long long)gridDim.x * slots) {
      const long long e = p * cs + ch0;
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if (ch0 < c) {
        const unsigned word = *(const unsigned*)(q + e);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (ch0 + k < c) o[k] = __fmul_rn(sc[k], __fsub_rn((float)((word >> (8 * k)) & 255u), zp[k]));   // scale * (q - zp)
      }
      *(f32x4*)(x + e) = o;
    }
  }
}

// ---- quantise + pack: the payload of include/hnd_codec.h.  One thread owns a GROUP of 8 consecutive values = `bits` whole
// bytes starting at byte group * bits, so no two threads share a byte and every store is a plain byte store; the last group
// holds numel % 8 values when that is not 0 and stores ceil(rem * bits / 8) bytes.  A group may cross a row, a channel plane
// or an image, so the channel is tracked per value; the table of (scale, zero point) is staged in LDS (at most 512 bytes).
__global__ void __launch_bounds__(kThreads) qc_quantize_pack_kernel(const float* __restrict__ x, long long numel, int c,
                                                                    long long hw, int cs, int bits,
                                                                    const float* __restrict__ qp, float qmax,
                                                                    uint8_t* __restrict__ payload) {
  __shared__ float s_scale[kMaxC], s_zp[kMaxC];
  if ((int)threadIdx.x < c) {
    s_scale[threadIdx.x] = qp[threadIdx.x * 4 + 2];
    s_zp[threadIdx.x] = qp[threadIdx.x * 4 + 3];
  }
  __syncthreads();
  const long long groups = (numel + 7) >> 3;
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < groups;
       g += (long long)gridDim.x * blockDim.x) {
    const long long i0 = g << 3;
    const int count = numel - i0 < 8 ? (int)(numel - i0) : 8;
    long long plane = i0 / hw, pix = i0 - plane * hw;               // plane = img * c + ch
    long long img = plane / c;
    int ch = (int)(plane - img * c);
    unsigned long long word = 0;
    for (int k = 0; k < count; ++k) {
      const float v = quantize_one(x[(img * hw + pix) * cs + ch], s_scale[ch], s_zp[ch], qmax);
      word |= (unsigned long long)(unsigned)v << (k * bits);
      if (++pix == hw) {
        pix = 0;
        if (++ch == c) { ch = 0; ++img; }
      }
    }
    const int nbytes = (count * bits + 7) >> 3;                    // `bits` for a full group
    uint8_t* dst = payload + g * bits;
    for (int b = 0; b < nbytes; ++b) dst[b] = (uint8_t)(word >> (8 * b));
  }
}

// ---- unpack + dequantise: a lane writes the 16 bytes of its group of a pixel; every real channel reads its value's bits
// (at most two bytes: bits <= 8; the second byte is touched only when the value reaches into it, so never past the
// payload's last byte), pad channels get 0
__global__ void __launch_bounds__(kThreads) qc_unpack_dequantize_kernel(const uint8_t* __restrict__ payload,
                                                                        const float* __restrict__ qp, float* __restrict__ x,
                                                                        long long npix, int c, long long hw, int cs,
                                                                        int bits) {
  const int groups = cs >> 2;
  const unsigned mask = (1u << bits) - 1u;
  for (int gb = 0; gb < groups; gb += kThreads) {
    const int gc = groups - gb < kThreads ? groups - gb : kThreads;
    const int slots = kThreads / gc;
    const int gl = threadIdx.x % gc, slot = threadIdx.x / gc;
    if (slot >= slots) continue;
    const int ch0 = (gb + gl) * 4;
    float sc[4], zp[4];
    lane_qparams(qp, ch0, c, sc, zp);
    for (long long p = (long long)blockIdx.x * slots + slot; p < npix; p += (long long)gridDim.x * slots) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if (ch0 < c) {
        const long long img = p / hw, pix = p - img * hw;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (ch0 + k < c) {
            const long long bit = ((img * c + ch0 + k) * hw + pix) * bits;
            const long long byte = bit >> 3;
            const int sh = (int)(bit & 7);
            unsigned two = payload[byte];
            if (sh + bits > 8) two |= (unsigned)payload[byte + 1] << 8;
            o[k] = __fmul_rn(sc[k], __fsub_rn((float)((two >> sh) & mask), zp[k]));      // scale * (q - zero_point)
          }
        }
      }
      *(f32x4*)(x + p * cs + ch0) = o;
    }
  }
}

// ---- fake quantise: fake_quantize_kernel (csrc/elementwise.hip) with the scale and zero point per channel.  One WAVE per
// tile of kFqRows pixels, lanes (row, group) with the group fastest, 64 / groups rows per pass; the per-lane sums meet in LDS
// and are added in row-slot order: the fixed order of the header, no atomics.  x and y may be the same buffer (every float
// is read and written by one lane), so neither is __restrict__.
__global__ void __launch_bounds__(64 * kFqWaves) qc_fake_quantize_kernel(const float* x, float* y, long long npix, int c,
                                                                         int cs, const float* __restrict__ qp, float qmax,
                                                                         float* __restrict__ stats, int ntiles) {
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
      float sc[4], zp[4];
      lane_qparams(qp, ch0, c, sc, zp);
      float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
      if (slot < slots) {
        for (int r = slot; r < rows; r += slots) {
          const long long e = (row0 + r) * cs + ch0;
          f32x4 o = {0.f, 0.f, 0.f, 0.f};
          if (ch0 < c) {
            const f32x4 v = *(const f32x4*)(x + e);
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (ch0 + k < c)
                o[k] = __fmul_rn(sc[k], __fsub_rn(quantize_one(v[k], sc[k], zp[k], qmax), zp[k]));   // scale * (q - zp)
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            s[k] = __fadd_rn(s[k], o[k]);
            ss[k] = __fadd_rn(ss[k], __fmul_rn(o[k], o[k]));
          }
          *(f32x4*)(y + e) = o;
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

// ---- host
inline bool aligned(const void* p, unsigned a) { return (uintptr_t)p % a == 0; }

inline int pixel_grid(long long npix, int cs, int cap) {
  const int groups = cs >> 2;
  const int slots = kThreads / (groups < kThreads ? groups : kThreads);      // pixels per pass of one workgroup
  long long b = (npix + slots - 1) / slots;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// the two launches every quantising export starts with
void launch_qparams(const float* x, long long npix, int c, int cs, float qmax, float* qparams, float* scratch,
                    hipStream_t s) {
  const int slots = kThreads / ((c + 3) >> 2);
  long long b = (npix + slots - 1) / slots;
  const int nb = (int)(b > kPartBlocks ? kPartBlocks : b);
  hipLaunchKernelGGL(qc_minmax_kernel, dim3(nb), dim3(kThreads), 0, s, x, npix, c, cs, scratch);
  hipLaunchKernelGGL(qc_qparams_kernel, dim3(1), dim3(kThreads), 0, s, scratch, nb, c, cs, qmax, qparams);
}

}  // namespace

#define QC_REQUIRE_COMMON(who)                                                                                  \
  HND_REQUIRE(bits >= 1 && bits <= 8, who ": bits %d outside 1 ... 8", bits);                                   \
  HND_REQUIRE(c >= 1 && c <= kMaxC, who ": c %d outside 1 ... %d", c, kMaxC);                                    \
  HND_REQUIRE(cs >= c && cs % 4 == 0, who ": bad pixel stride %d (cs >= c, cs %% 4 == 0)", cs)

extern "C" {

int hnd_qchannel_abi(void) { return HND_QCHANNEL_ABI; }

size_t hnd_qchannel_scratch_elems(int cs) {
  if (cs <= 0 || cs % 4 != 0) return 0;
  return (size_t)kPartBlocks * 2 * (size_t)cs;
}

int hnd_qchannel_quantize_bits(const float* x, int64_t npix, int c, int cs, int bits, uint8_t* q, float* qparams,
                               float* scratch, void* stream) {
  HND_REQUIRE(x && q && qparams && scratch, "hnd_qchannel_quantize_bits: null pointer");
  QC_REQUIRE_COMMON("hnd_qchannel_quantize_bits");
  HND_REQUIRE(npix > 0, "hnd_qchannel_quantize_bits: npix must be positive");
  HND_REQUIRE(aligned(x, 16) && aligned(q, 4),
              "hnd_qchannel_quantize_bits: x must be 16-byte aligned and q 4-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  const float qmax = (float)((1 << bits) - 1);
  launch_qparams(x, (long long)npix, c, cs, qmax, qparams, scratch, s);
  hipLaunchKernelGGL(qc_quantize_kernel, dim3(pixel_grid(npix, cs, kMaxBlocks)), dim3(kThreads), 0, s, x, (long long)npix,
                     c, cs, qparams, qmax, q);
  return hnd::check_launch("hnd_qchannel_quantize_bits");
}

int hnd_qchannel_dequantize_u8(const uint8_t* q, const float* qparams, float* x, int64_t npix, int c, int cs, void* stream) {
  HND_REQUIRE(q && qparams && x, "hnd_qchannel_dequantize_u8: null pointer");
  HND_REQUIRE(c >= 1 && c <= kMaxC, "hnd_qchannel_dequantize_u8: c %d outside 1 ... %d", c, kMaxC);
  HND_REQUIRE(cs >= c && cs % 4 == 0, "hnd_qchannel_dequantize_u8: bad pixel stride %d (cs >= c, cs %% 4 == 0)", cs);
  HND_REQUIRE(npix > 0, "hnd_qchannel_dequantize_u8: npix must be positive");
  HND_REQUIRE(aligned(x, 16) && aligned(q, 4),
              "hnd_qchannel_dequantize_u8: x must be 16-byte aligned and q 4-byte aligned");
  hipLaunchKernelGGL(qc_dequantize_kernel, dim3(pixel_grid(npix, cs, kMaxBlocks)), dim3(kThreads), 0,
                     hnd::as_stream(stream), q, qparams, x, (long long)npix, c, cs);
  return hnd::check_launch("hnd_qchannel_dequantize_u8");
}

int hnd_qchannel_quantize_pack_bits(const float* x, int n, int h, int w, int c, int cs, int bits, uint8_t* payload,
                                    float* qparams, float* scratch, void* stream) {
  HND_REQUIRE(x && payload && qparams && scratch, "hnd_qchannel_quantize_pack_bits: null pointer");
  QC_REQUIRE_COMMON("hnd_qchannel_quantize_pack_bits");
  HND_REQUIRE(n > 0 && h > 0 && w > 0, "hnd_qchannel_quantize_pack_bits: n, h and w must be positive");
  HND_REQUIRE(aligned(x, 16), "hnd_qchannel_quantize_pack_bits: x must be 16-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  const float qmax = (float)((1 << bits) - 1);
  const long long hw = (long long)h * w, npix = hw * n, numel = npix * c;
  launch_qparams(x, npix, c, cs, qmax, qparams, scratch, s);
  long long nb = ((numel + 7) / 8 + kThreads - 1) / kThreads;
  if (nb > kMaxBlocks) nb = kMaxBlocks;
  hipLaunchKernelGGL(qc_quantize_pack_kernel, dim3((int)nb), dim3(kThreads), 0, s, x, numel, c, hw, cs, bits, qparams, qmax,
                     payload);
  return hnd::check_launch("hnd_qchannel_quantize_pack_bits");
}

int hnd_qchannel_unpack_dequantize_bits(const uint8_t* payload, const float* qparams, float* x, int n, int h, int w, int c,
                                        int cs, int bits, void* stream) {
  HND_REQUIRE(payload && qparams && x, "hnd_qchannel_unpack_dequantize_bits: null pointer");
  QC_REQUIRE_COMMON("hnd_qchannel_unpack_dequantize_bits");
  HND_REQUIRE(n > 0 && h > 0 && w > 0, "hnd_qchannel_unpack_dequantize_bits: n, h and w must be positive");
  HND_REQUIRE(aligned(x, 16), "hnd_qchannel_unpack_dequantize_bits: x must be 16-byte aligned");
  const long long hw = (long long)h * w, npix = hw * n;
  hipLaunchKernelGGL(qc_unpack_dequantize_kernel, dim3(pixel_grid(npix, cs, kMaxBlocks)), dim3(kThreads), 0,
                     hnd::as_stream(stream), payload, qparams, x, npix, c, hw, cs, bits);
  return hnd::check_launch("hnd_qchannel_unpack_dequantize_bits");
}

int hnd_qchannel_fake_quantize_bits(const float* x, float* y, int64_t npix, int c, int cs, int bits, float* qparams,
                                    float* scratch, float* stats, void* stream) {
  HND_REQUIRE(x && y && qparams && scratch, "hnd_qchannel_fake_quantize_bits: null pointer");
  QC_REQUIRE_COMMON("hnd_qchannel_fake_quantize_bits");
  HND_REQUIRE(npix > 0, "hnd_qchannel_fake_quantize_bits: npix must be positive");
  const int ntiles = hnd_fake_quantize_tiles(npix);
  HND_REQUIRE(ntiles > 0, "hnd_qchannel_fake_quantize_bits: npix too large (the tile count must fit an int)");
  HND_REQUIRE(aligned(x, 16) && aligned(y, 16), "hnd_qchannel_fake_quantize_bits: x and y must be 16-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  const float qmax = (float)((1 << bits) - 1);
  launch_qparams(x, (long long)npix, c, cs, qmax, qparams, scratch, s);
  int nb = (ntiles + kFqWaves - 1) / kFqWaves;
  if (nb > kMaxBlocks) nb = kMaxBlocks;
  hipLaunchKernelGGL(qc_fake_quantize_kernel, dim3(nb), dim3(64 * kFqWaves), 0, s, x, y, (long long)npix, c, cs, qparams,
                     qmax, stats, ntiles);
  return hnd::check_launch("hnd_qchannel_fake_quantize_bits");
}

}  // extern "C"
