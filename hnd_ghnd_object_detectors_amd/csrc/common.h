// Shared helpers for libhnd_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <type_traits>
#include <utility>

#include "hnd_hip.h"

namespace hnd {

void set_error(const char* fmt, ...);
int check_launch(const char* what);   // hipGetLastError -> status
int cu_count();                       // compute units of the current device (cached; 256 when the query fails)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a compile-time constant
// (register-array subscripts, inline-asm immediates)
template <int N, class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl<N>(f, std::make_integer_sequence<int, N>{});
}

// floor(x / d) for 0 <= x < 2^31 with a precomputed multiplier (d >= 1)
struct FastDiv {
  unsigned mul, shr, d;
};
inline FastDiv make_fastdiv(unsigned d) {
  FastDiv f;
  f.d = d;
  if (d == 1) { f.mul = 0; f.shr = 0; return f; }
  unsigned l = 0;
  while ((1u << l) < d) ++l;                       // l = ceil(log2 d)
  unsigned long long m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
  f.mul = (unsigned)m;
  f.shr = l;
  return f;
}
__device__ __forceinline__ unsigned fdiv(unsigned x, const FastDiv f) {
  if (f.d == 1) return x;
  unsigned t = __umulhi(x, f.mul);
  return (t + ((x - t) >> 1)) >> (f.shr - 1);
}
// GEMM row m of a convolution -> its output pixel (n, oh, ow); div_ow / div_oh = make_fastdiv of the map's ow / oh
struct RowPixel {
  unsigned n, oh, ow;
};
__device__ __forceinline__ RowPixel row_pixel(unsigned m, const FastDiv& div_ow, const FastDiv& div_oh, int ow, int oh) {
  const unsigned t = fdiv(m, div_ow), ow_ = m - t * (unsigned)ow;
  const unsigned n_ = fdiv(t, div_oh), oh_ = t - n_ * (unsigned)oh;
  return {n_, oh_, ow_};
}

// the ReLU-mask nibble of four stored values (hnd_conv_desc.mask_out / mask_bits: bit i = value i is positive)
template <class V>
__device__ __forceinline__ uint8_t relu_mask_nibble(const V v) {
  return (uint8_t)((v[0] > 0.f ? 1 : 0) | (v[1] > 0.f ? 2 : 0) | (v[2] > 0.f ? 4 : 0) | (v[3] > 0.f ? 8 : 0));
}

// Packed GEMM-operand row r (hnd_pack_weights, hnd_wino*_weights) holds output channel chan_of_row(r): inside every
// group of 64 rows the four 16-row MFMA tiles are interleaved, so the four accumulator tiles a lane of the implicit-
// GEMM kernel owns (rows 16*ni + lane%16 of its wave's 64) are four CONSECUTIVE output channels.
__host__ __device__ inline int chan_of_row(int r) { return (r & ~63) | ((r & 15) << 2) | ((r >> 4) & 3); }

// Workgroup b runs on XCD b % 8 (each XCD has its own L2).  Kernels whose neighbouring workgroups read overlapping
// data (the Winograd input transforms: tile (ty, tx) shares two of its eight columns with (ty, tx + 1)) give
// consecutive LOGICAL blocks to one XCD, so the shared part is an L2 hit instead of a second trip to HBM.  Bijective for
// any grid.  (Measured and not used for the 3x3 stride-2 max pooling: 0.64 -> 0.70 ms.)
__device__ __forceinline__ int xcd_contiguous_block() {
  const int nb = gridDim.x, b = blockIdx.x, q = nb >> 3, r = nb & 7, xcd = b & 7, slot = b >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

inline hipStream_t as_stream(void* s) { return (hipStream_t)s; }

// Launch of a kernel that needs more than 64 KB of dynamic LDS: raises the kernel's limit to `attr_bytes` once per device
// (the attribute lives on the device's function; one mask of devices per instantiation, i.e. per kernel), launches, and
// returns check_launch(what).  `what` names the launch in both error texts.
template <auto KERN, class... Args>
int launch_big_lds(dim3 grid, dim3 block, size_t lds, int attr_bytes, hipStream_t stream, const char* what, const Args&... args) {
  static std::atomic<unsigned long long> attr_set{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  if (!(attr_set.load(std::memory_order_relaxed) & bit)) {
    hipError_t e = hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, attr_bytes);
    if (e != hipSuccess) {
      set_error("hipFuncSetAttribute(%s) failed: %s", what, hipGetErrorString(e));
      return HND_ERR_LAUNCH;
    }
    attr_set.fetch_or(bit, std::memory_order_relaxed);
  }
  hipLaunchKernelGGL(KERN, grid, block, lds, stream, args...);
  return check_launch(what);
}

// The on/off (or numeric) environment switches: atoi of the value, `dflt` when unset.  Read per call: in-process A/B.
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
// ... the two switches that are off when their value BEGINS with '0' (HND_BSTREAM, HND_BXS)
inline bool env_begins_with_0(const char* name) {
  const char* e = getenv(name);
  return e && e[0] == '0';
}

// ---- host-side facts about a launch that several pickers and launches share
// more than the one centred sample per output pixel (the kernels' TAPS builds)
inline bool has_taps(const hnd_conv_desc& d) { return d.kh * d.kw > 1 || d.bh != 0 || d.bw != 0; }
// every output pixel samples inside the input (what the tap-free builds assume)
inline bool samples_inside(const hnd_conv_desc& d) {
  return (long long)(d.oh - 1) * d.sh < d.h && (long long)(d.ow - 1) * d.sw < d.w_;
}
inline long long gemm_rows(const hnd_conv_desc& d) { return (long long)d.n * d.oh * d.ow; }
// The B-resident kernels give every `bn`-column weight slice to one workgroup and the cout / bn workgroups of a TEAM to one
// XCD: the number of teams, or 0 where the slices do not divide an XCD's CUs evenly
inline int team_count(int cout, int bn) {
  const int per_xcd = cu_count() / 8, nsl = cout / bn;
  if (per_xcd < 1 || nsl < 1 || nsl > per_xcd || per_xcd % nsl != 0) return 0;
  return 8 * (per_xcd / nsl);
}

// HND_DEBUG_PICKER: the ONE switch behind which the kernel pickers' experiment / test overrides live (A/B tools and the
// bit-identity tests force a variant with it; nothing in normal use sets it).  Comma-separated keys, optionally key=value:
//   bres_all          every launch the B-resident kernels can take, not only where they were measured to win
//   bstream_all       the same for the B-streamed kernel
//   igemm_tile=0..3   block tile of the tiled kernel (128x128, 128x64, 64x128, 64x64)
//   wgrad_ring_taps   the ring weight-gradient kernel also for tap (direct 2x2) problems
//   bstream_k1024 / bstream_parity   the B-streamed kernel also for K = 1024 -> 256 launches / for stride-2 parity launches
//   bxs_wn1                          (B-streamed emulation kernel) the 256 x 64 tile also where the output has 128-column blocks
//   bx3_tiled=1 / bx3_tiled=0        (emulation, B resident) the tiled build wherever bx3_applies / never; both builds give
//                                    the same bits.  bx3_tiled_mi=1|2: its 64- or 128-row tile (tools/bench_bx3_tiled.py)
// Returns -1 when `key` is absent, its value (1 without "=value") otherwise.  Read per call: in-process A/B.
inline int debug_picker(const char* key) {
  const char* e = getenv("HND_DEBUG_PICKER");
  if (!e) return -1;
  const size_t n = strlen(key);
  for (const char* p = e; *p;) {
    const char* q = p;
    while (*q && *q != ',') ++q;
    if ((size_t)(q - p) >= n && strncmp(p, key, n) == 0 && (p[n] == ',' || p[n] == 0 || p[n] == '=')) return p[n] == '=' ? atoi(p + n + 1) : 1;
    p = *q ? q + 1 : q;
  }
  return -1;
}

#define HND_REQUIRE(cond, ...)                \
  do {                                        \
    if (!(cond)) {                            \
      hnd::set_error(__VA_ARGS__);            \
      return HND_ERR_INVALID;                 \
    }                                         \
  } while (0)

}  // namespace hnd
