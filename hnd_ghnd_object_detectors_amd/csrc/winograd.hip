// Winograd minimal filtering for the stride-1 convolutions: F(2x2 | 4x4 | 6x6, 3x3) for the pad-1 3x3 convolutions (frozen
// ResNet conv2, FPN output convs, and their data gradients) and F(4x4 | 6x6, 2x2) for the student head's 2x2 convolutions,
// their data gradients and, in the Winograd domain, their weight gradients.  Y = A^T [ (G g G^T) .* (B^T d B) ] A per
// T x T output tile, i.e. P^2 = (T + R - 1)^2 multiplies per input/output channel pair instead of (T R)^2.  The P^2
// element-wise products over channels are P^2 independent GEMMs
//     M_f [tiles x cout] = V_f [tiles x cin] * U_f^T [cin x cout]
// which run as ONE launch of the implicit-GEMM kernel (conv_igemm.hip: a 1x1 "conv" over P^2 * tiles_pad pixels whose
// weight matrix is selected per 128-row group).  This file holds the HBM-bound transforms around it: one kernel per ROLE
// (weights, input, output, dy, weight-gradient output), instantiated per scheme of winograd_schemes.h, which holds
// everything that differs between the schemes.  fp32 throughout.
#include <type_traits>

#include "common.h"
#include "winograd_schemes.h"

using namespace wino;

namespace {

constexpr int kMaxBlocks = 256 * 32;

inline int grid_for(long long work_items, int threads = 256) {
  long long b = (work_items + threads - 1) / threads;
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (int)b;
}

// The transformed product M is read exactly once, by the output transform: nontemporal loads keep it from displacing the
// output rows being written (round 4, in-step A/B: wino_output 3.61 -> 3.30 ms; nontemporal STORES of V gained nothing
// in the step -- the GEMM that follows wants V where it is).
#define HND_NT_LOAD(p) __builtin_nontemporal_load((p))

// A use of loaded values in the block that dominates a run of conditionally executed stores: hipcc's waitcnt pass
// then waits for the loads here, once, instead of in front of every store that follows.
__device__ __forceinline__ void arrive(const f32x2& a, const f32x2& b) {
  asm volatile("" ::"v"(a.x), "v"(a.y), "v"(b.x), "v"(b.y));
}

// ---------------------------------------------------------------------------------- the pieces every transform shares
template <class V> constexpr int lanes_of = sizeof(V) / sizeof(float);

template <class V> __device__ __forceinline__ V splat(float s);
template <> __device__ __forceinline__ f32x2 splat<f32x2>(float s) { return f32x2{s, s}; }
template <> __device__ __forceinline__ f32x4 splat<f32x4>(float s) { return f32x4{s, s, s, s}; }

__device__ __forceinline__ f32x2 lanes_max(f32x2 a, float f) { a.x = fmaxf(a.x, f); a.y = fmaxf(a.y, f); return a; }
__device__ __forceinline__ f32x4 lanes_max(f32x4 a, float f) {
  a.x = fmaxf(a.x, f); a.y = fmaxf(a.y, f); a.z = fmaxf(a.z, f); a.w = fmaxf(a.w, f);
  return a;
}

// first work item of a thread's grid-stride loop; XCD: blocks walk the items with hnd::xcd_contiguous_block()
template <bool XCD>
__device__ __forceinline__ long long first_item() {
  if constexpr (XCD) return hnd::xcd_contiguous_block() * (long long)blockDim.x + threadIdx.x;
  else return blockIdx.x * (long long)blockDim.x + threadIdx.x;
}

// work item e -> channel group c (fastest), tile t = (b, ty, tx)
struct TileItem {
  long long t;
  int c, tx, ty, b;
};
__device__ __forceinline__ TileItem tile_item(long long e, int cn, int th, int tw) {
  TileItem it;
  it.c = (int)(e % cn);
  it.t = e / cn;
  it.tx = (int)(it.t % tw);
  const long long q = it.t / tw;
  it.ty = (int)(q % th);
  it.b = (int)(q / th);
  return it;
}

// Optional prologue on in-bounds elements of an input transform: a = x*scale[c] + shift[c], relu.
template <class V>
struct Prologue {
  bool on;
  V ps, pb;
  float floor_;
  __device__ __forceinline__ Prologue(const float* scale, const float* shift, int relu, int c)
      : on(scale != nullptr), ps(splat<V>(1.f)), pb(splat<V>(0.f)), floor_(relu ? 0.f : -INFINITY) {
    if (on) {
      ps = *(const V*)(scale + c * lanes_of<V>);
      pb = *(const V*)(shift + c * lanes_of<V>);
    }
  }
  __device__ __forceinline__ V operator()(V a) const { return on ? lanes_max(a * ps + pb, floor_) : a; }
};

// d[j][i] (column j is one array) = f(x[b][y0 + i][x0 + j][c ...]), zero outside the h x w map
template <int N, class V, class F>
__device__ __forceinline__ void load_patch(V (&d)[N][N], const float* __restrict__ x, int b, int y0, int x0, int h, int w,
                                           int ld, int coff, F f) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int iy = y0 + i;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int ix = x0 + j;
      const bool ok = (unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w;
      const size_t off = ok ? (((size_t)b * h + iy) * w + ix) * ld + coff : 0;
      const V a = f(off);
      d[j][i] = ok ? a : splat<V>(0.f);
    }
  }
}

// dst[(i * PO + j) * fs] = (M d M^T)[i][j] for the row function `row` of M (PI -> PO): down the columns of d, then along
// the rows, straight to memory
template <int PI, int PO, class V, class Row>
__device__ __forceinline__ void transform_store(const V (&d)[PI][PI], float* __restrict__ dst, size_t fs, Row row) {
  V r[PO][PI];
#pragma unroll
  for (int j = 0; j < PI; ++j) {
    V o[PO];
    row(d[j], o);
#pragma unroll
    for (int i = 0; i < PO; ++i) r[i][j] = o[i];
  }
#pragma unroll
  for (int i = 0; i < PO; ++i) {
    V o[PO];
    row(r[i], o);
#pragma unroll
    for (int j = 0; j < PO; ++j) *(V*)(dst + (size_t)(i * PO + j) * fs) = o[j];
  }
}

// s[a][j] = (A^T m)[a][j] of the P x P GEMM results of a tile (nontemporal loads, down the columns)
template <class S>
__device__ __forceinline__ void load_at(const float* __restrict__ src, size_t fs, typename S::V (&s)[S::T][S::P]) {
  using V = typename S::V;
#pragma unroll
  for (int j = 0; j < S::P; ++j) {
    V col[S::P], o[S::T];
#pragma unroll
    for (int i = 0; i < S::P; ++i) col[i] = HND_NT_LOAD((const V*)(src + (size_t)(i * S::P + j) * fs));
    S::at(col, o);
#pragma unroll
    for (int a = 0; a < S::T; ++a) s[a][j] = o[a];
  }
}

// Per-block (s1, s2) per output channel -> stats[blockIdx][2][cout].  Threads tid and tid + k*cout/2 hold the same channel
// pair (512 % cout == 0): fold them in a fixed order.
__device__ __forceinline__ void block_stats_store(f32x2 s1, f32x2 s2, int cout, float* __restrict__ stats) {
  __shared__ float red[2][512];
  red[0][threadIdx.x * 2] = s1.x; red[0][threadIdx.x * 2 + 1] = s1.y;
  red[1][threadIdx.x * 2] = s2.x; red[1][threadIdx.x * 2 + 1] = s2.y;
  __syncthreads();
  if ((int)threadIdx.x < cout) {
    float a1 = 0.f, a2 = 0.f;
    for (int k = threadIdx.x; k < 512; k += cout) { a1 += red[0][k]; a2 += red[1][k]; }
    float* st = stats + (size_t)blockIdx.x * 2 * cout;
    st[threadIdx.x] = a1;
    st[cout + threadIdx.x] = a2;
  }
}

// ---------------------------------------------------------------------------------- weights
// U_f[co][ci] = (G g G^T)[f], g = w[co][ci] (forward) or w[ci][co] flipped (data gradient), written in the packed
// GEMM-operand layout of hnd_pack_weights: [P*P][rows_pad][kdim], K (= input channel of the GEMM) contiguous.
// GEMM rows = output channels of this conv direction, K = its input channels.
template <class S>
__global__ void wino_weights_kernel(const float* __restrict__ w, float* __restrict__ u, int cout, int cin, int dgrad,
                                    int rows, int rows_pad, int kdim) {
  constexpr int R = S::R, P = S::P;
  const long long total = (long long)rows_pad * kdim;
  const int kreal = dgrad ? cout : cin;
  const size_t fs = (size_t)rows_pad * kdim;
  for (long long e = first_item<false>(); e < total; e += (long long)gridDim.x * blockDim.x) {
    const int pr = (int)(e / kdim), k = (int)(e - (long long)pr * kdim);      // packed row pr holds channel r
    const int r = hnd::chan_of_row(pr);
    const bool ok = r < rows && k < kreal;
    float g[R][R];                          // g[j][i]: column j of the filter
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        float v = 0.f;
        if (ok) v = dgrad ? w[(((size_t)k * cin + r) * R + (R - 1 - i)) * R + (R - 1 - j)]      // w[co=k][ci=r], flipped
                          : w[(((size_t)r * cin + k) * R + i) * R + j];
        g[j][i] = v;
      }
    float t[R][P];                          // t[j][i] = (G g)[i][j]
#pragma unroll
    for (int j = 0; j < R; ++j) S::g(g[j], t[j]);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      float row[R], o[P];
#pragma unroll
      for (int j = 0; j < R; ++j) row[j] = t[j][i];
      S::g(row, o);
      float* dst = u + ((size_t)(i * P) * rows_pad + pr) * kdim + k;
#pragma unroll
      for (int j = 0; j < P; ++j) dst[(size_t)j * fs] = o[j];
    }
  }
}

// ---------------------------------------------------------------------------------- input
// V[f][t][c] = (B^T d B)[f] of the P x P input patch of tile t (rows T ty - pad .., cols T tx - pad ..), zero outside the
// image, after the optional prologue.
template <class S>
__global__ void __launch_bounds__(S::kLaunchBound)
wino_input_kernel(const float* __restrict__ x, float* __restrict__ v, const typename S::Geom g,
                  const float* __restrict__ pro_scale, const float* __restrict__ pro_shift, int pro_relu) {
  using V = typename S::V;
  constexpr int L = lanes_of<V>;
  const int cn = g.c / L;
  const long long total = (long long)g.n * g.th * g.tw * cn;
  const size_t fs = (size_t)g.tiles_pad * g.c;           // component stride
  for (long long e = first_item<S::kXcdWalk>(); e < total; e += (long long)gridDim.x * blockDim.x) {
    const TileItem it = tile_item(e, cn, g.th, g.tw);
    const Prologue<V> pro(pro_scale, pro_shift, pro_relu, it.c);
    V d[S::P][S::P];
    load_patch(d, x, it.b, S::T * it.ty - S::pad(g), S::T * it.tx - S::pad(g), g.h, g.w, g.c, it.c * L,
               [&](size_t off) { return pro(*(const V*)(x + off)); });
    transform_store<S::P, S::P>(d, v + (size_t)it.t * g.c + it.c * L, fs, [](const auto& in, auto& out) { S::bt(in, out); });
  }
}

// ---------------------------------------------------------------------------------- 3x3 output
struct WinoEpilogue {
  const float* epi_scale;
  const float* epi_shift;
  const float* res1;
  const float* mask;
  int relu;
  uint8_t* mask_out;      // F(4x4) / F(6x6): [stored value > 0] as nibbles, one byte per pixel and four channels (hnd_conv_desc.mask_out)
};

// a thread of the F(4x4) / F(6x6) output transforms owns TWO channels of a pixel: half a nibble.  The even thread of a
// pair (adjacent lanes: same tile, channels c2 * 2 and c2 * 2 + 2) fetches its neighbour's two bits and writes the byte.
// Both lanes of a pair take every branch around this call together (same tile, same pixel).
__device__ __forceinline__ void wino_store_nibble(uint8_t* mask_out, size_t off, int c2, f32x2 v) {
  const unsigned bits = (v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u);
  const unsigned other = (unsigned)__shfl_xor((int)bits, 1);
  if (!(c2 & 1)) mask_out[off >> 2] = (uint8_t)(bits | (other << 2));
}

// y[2ty+a][2tx+b][c] = epilogue( (A^T m A)[a][b] ), m = the 16 GEMM results of tile t; same epilogue order as the
// implicit-GEMM kernel: scale/shift, + res1, mask (ReLU backward), ReLU.  F(2x2,3x3) keeps an output kernel of its own:
// four channels per thread, epilogue operands read at run time, no mask_out and no interior path.
__global__ void wino_output_kernel(const float* __restrict__ m, float* __restrict__ y, const WinoGeom g, int cout,
                                   const WinoEpilogue ep) {
  using S = F23;
  const int c4n = (cout + 3) >> 2;
  const long long total = (long long)g.n * g.th * g.tw * c4n;
  const size_t fs = (size_t)g.tiles_pad * cout;
  for (long long e = first_item<false>(); e < total; e += (long long)gridDim.x * blockDim.x) {
    const TileItem it = tile_item(e, c4n, g.th, g.tw);
    const int c4 = it.c, tx = it.tx, ty = it.ty, b = it.b;
    f32x4 s[2][4];
    load_at<S>(m + (size_t)it.t * cout + c4 * 4, fs, s);
    f32x4 es = {1.f, 1.f, 1.f, 1.f}, eb = {0.f, 0.f, 0.f, 0.f};
    if (ep.epi_scale) es = *(const f32x4*)(ep.epi_scale + c4 * 4);
    if (ep.epi_shift) eb = *(const f32x4*)(ep.epi_shift + c4 * 4);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int oy = 2 * ty + a;
      f32x4 o[2];
      S::at(s[a], o);
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
        const int ox = 2 * tx + bb;
        if (oy >= g.h || ox >= g.w) continue;
        f32x4 v = o[bb] * es + eb;
        const size_t off = (((size_t)b * g.h + oy) * g.w + ox) * g.c + c4 * 4;
        if (ep.res1) v += *(const f32x4*)(ep.res1 + off);
        if (ep.mask) {
          const f32x4 k = *(const f32x4*)(ep.mask + off);
          v.x = k.x > 0.f ? v.x : 0.f; v.y = k.y > 0.f ? v.y : 0.f; v.z = k.z > 0.f ? v.z : 0.f; v.w = k.w > 0.f ? v.w : 0.f;
        }
        if (ep.relu) v = lanes_max(v, 0.f);
        *(f32x4*)(y + off) = v;
      }
    }
  }
}

// F(4x4,3x3) / F(6x6,3x3).  The epilogue operands are template parameters and tiles that lie inside the map take a
// branch-free path: with run-time `if (ptr)` operands or per-output bounds branches hipcc puts `s_waitcnt vmcnt(0)` in
// front of every store (stores count in vmcnt on gfx9), which serialises the 16 / 36 stores of a tile.
template <class S, bool RES, bool MASK>
__global__ void __launch_bounds__(S::kLaunchBound)
wino3_output_kernel(const float* __restrict__ m, float* __restrict__ y, const WinoGeom g, int cout, const WinoEpilogue ep) {
  constexpr int T = S::T;
  const int c2n = cout >> 1;
  const long long total = (long long)g.n * g.th * g.tw * c2n;
  const size_t fs = (size_t)g.tiles_pad * cout;
  for (long long e = first_item<false>(); e < total; e += (long long)gridDim.x * blockDim.x) {
    const TileItem it = tile_item(e, c2n, g.th, g.tw);
    const int c2 = it.c, tx = it.tx, ty = it.ty, b = it.b;
    f32x2 es = {1.f, 1.f}, eb = {0.f, 0.f};
    if (ep.epi_scale) es = *(const f32x2*)(ep.epi_scale + c2 * 2);
    if (ep.epi_shift) eb = *(const f32x2*)(ep.epi_shift + c2 * 2);
    f32x2 s[T][S::P];
    load_at<S>(m + (size_t)it.t * cout + c2 * 2, fs, s);
    arrive(es, eb);
    auto emit = [&](auto checked) {
      constexpr bool CHK = decltype(checked)::value;
      // interior tiles: the residual / mask rows are fetched one output row ahead of the stores that use them
      f32x2 rn[T], kn[T];
      auto fetch = [&](int a) {
        const size_t row = (((size_t)b * g.h + T * ty + a) * g.w + T * tx) * g.c + c2 * 2;
#pragma unroll
        for (int bb = 0; bb < T; ++bb) {
          if (RES) rn[bb] = *(const f32x2*)(ep.res1 + row + (size_t)bb * g.c);
          if (MASK) kn[bb] = *(const f32x2*)(ep.mask + row + (size_t)bb * g.c);
        }
      };
      if (!CHK && (RES || MASK)) fetch(0);
#pragma unroll
      for (int a = 0; a < T; ++a) {
        const int oy = T * ty + a;
        f32x2 o[T], rc[T], kc[T];
        S::at(s[a], o);
        if (!CHK && (RES || MASK)) {
#pragma unroll
          for (int bb = 0; bb < T; ++bb) { rc[bb] = rn[bb]; kc[bb] = kn[bb]; }
          if (a + 1 < T) fetch(a + 1);
        }
#pragma unroll
        for (int bb = 0; bb < T; ++bb) {
          const int ox = T * tx + bb;
          if (CHK && (oy >= g.h || ox >= g.w)) continue;
          f32x2 v = o[bb] * es + eb;
          const size_t off = (((size_t)b * g.h + oy) * g.w + ox) * g.c + c2 * 2;
          if (CHK) {
            if (RES) rc[bb] = *(const f32x2*)(ep.res1 + off);
            if (MASK) kc[bb] = *(const f32x2*)(ep.mask + off);
          }
          if (RES) v += rc[bb];
          if (MASK) { v.x = kc[bb].x > 0.f ? v.x : 0.f; v.y = kc[bb].y > 0.f ? v.y : 0.f; }
          if (ep.relu) v = lanes_max(v, 0.f);
          *(f32x2*)(y + off) = v;
          if (ep.mask_out) wino_store_nibble(ep.mask_out, off, c2, v);
        }
      }
    };
    if (T * ty + T <= g.h && T * tx + T <= g.w) emit(std::false_type{});
    else emit(std::true_type{});
  }
}

// ---------------------------------------------------------------------------------- 2x2 output
// BatchNorm BACKWARD statistics of the tensor this launch produces (BWD): when the output is the gradient g w.r.t. the output
// of a train-mode BatchNorm(+ReLU) -- the data gradient of the NEXT head conv -- the per-channel sums of
// d = g [bn(x) > 0] and d * xhat that hnd_bn_bwd_reduce would make in a pass of its own (reading g and x: 8 B per element)
// are taken here from the values in registers and one read of x (4 B per element); same [blocks][2][cout] partials,
// consumed by hnd_bn_bwd_finalize.
struct BnBwdStatsArgs {
  const float* x;                 // raw conv output the BatchNorm normalises, geometry of y
  const float* scale;             // gamma * rstd, beta - mean * gamma * rstd (the forward's folded affine: ReLU mask)
  const float* shift;
  const float* mean;
  const float* rstd;
  int relu;
};

// Output transform (+ scale/shift, ReLU) of the 2x2 Winograd conv.  With `stats`, every block also writes the partial
// (sum v, sum v^2) per output channel of the values it stored -> stats[blockIdx][2][cout]: the train-mode BatchNorm
// statistics hnd_bn_finalize consumes (ntiles = gridDim.x); BWD: the BatchNorm-backward sums above instead.  Requires
// 512 % cout == 0 so a thread keeps its channels.
template <class S, bool BWD>
__global__ void __launch_bounds__(S::kLaunchBound)
wino2_output_kernel(const float* __restrict__ m, float* __restrict__ y, const Wino2Geom g, int cout, int ldc,
                    const float* __restrict__ epi_scale, const float* __restrict__ epi_shift, int relu,
                    float* __restrict__ stats, const BnBwdStatsArgs bw) {
  constexpr int T = S::T;
  const int c2n = cout >> 1;
  const long long total = (long long)g.n * g.th * g.tw * c2n;
  const size_t fs = (size_t)g.tiles_pad * cout;
  f32x2 bsc = {1.f, 1.f}, bsh = {0.f, 0.f}, bmu = {0.f, 0.f}, brs = {1.f, 1.f};
  if (BWD) {        // (a thread's channel pair is the same in every iteration: 256 % (cout / 2) == 0)
    const int c2b = (int)(first_item<false>() % c2n);
    bsc = *(const f32x2*)(bw.scale + c2b * 2); bsh = *(const f32x2*)(bw.shift + c2b * 2);
    bmu = *(const f32x2*)(bw.mean + c2b * 2); brs = *(const f32x2*)(bw.rstd + c2b * 2);
  }
  f32x2 s1 = {0.f, 0.f}, s2 = {0.f, 0.f};
  for (long long e = first_item<false>(); e < total; e += (long long)gridDim.x * blockDim.x) {
    const TileItem it = tile_item(e, c2n, g.th, g.tw);
    const int c2 = it.c, tx = it.tx, ty = it.ty, b = it.b;
    f32x2 s[T][S::P];
    load_at<S>(m + (size_t)it.t * cout + c2 * 2, fs, s);
    f32x2 es = {1.f, 1.f}, eb = {0.f, 0.f};
    if (epi_scale) es = *(const f32x2*)(epi_scale + c2 * 2);
    if (epi_shift) eb = *(const f32x2*)(epi_shift + c2 * 2);
    arrive(es, eb);
    auto emit = [&](auto checked) {         // see wino3_output_kernel: interior tiles store without branches
      constexpr bool CHK = decltype(checked)::value;
#pragma unroll
      for (int a = 0; a < T; ++a) {
        const int oy = T * ty + a;
        f32x2 o[T];
        S::at(s[a], o);
#pragma unroll
        for (int bb = 0; bb < T; ++bb) {
          const int ox = T * tx + bb;
          if (CHK && (oy >= g.oh || ox >= g.ow)) continue;
          f32x2 v = o[bb] * es + eb;
          if (relu) v = lanes_max(v, 0.f);
          const size_t yo = (((size_t)b * g.oh + oy) * g.ow + ox) * ldc + c2 * 2;
          *(f32x2*)(y + yo) = v;
          if (BWD) {
            const f32x2 xv = *(const f32x2*)(bw.x + yo);
            f32x2 dd = v;
            if (bw.relu) {
              const f32x2 out = xv * bsc + bsh;
              dd.x = out.x > 0.f ? dd.x : 0.f;
              dd.y = out.y > 0.f ? dd.y : 0.f;
            }
            s1 += dd;
            s2 += dd * ((xv - bmu) * brs);
          } else {
            s1 += v;
            s2 += v * v;
          }
        }
      }
    };
    if (T * ty + T <= g.oh && T * tx + T <= g.ow) emit(std::false_type{});
    else emit(std::true_type{});
  }
  if (stats) block_stats_store(s1, s2, cout, stats);
}

// ---------------------------------------------------------------------------------- weight gradient: dy, output
// Z = G' dy_t G'^T of the T x T tiles of dy (F(2x2, T x T): the weight gradient in the Winograd domain, winograd_schemes.h)
template <class S>
__global__ void __launch_bounds__(S::kLaunchBound)
wino2_dy_kernel(const float* __restrict__ dy, float* __restrict__ z, const Wino2Geom g, int cout, int ldy) {
  const int c2n = cout >> 1;
  const long long total = (long long)g.n * g.th * g.tw * c2n;
  const size_t fs = (size_t)g.tiles_pad * cout;
  for (long long e = first_item<false>(); e < total; e += (long long)gridDim.x * blockDim.x) {
    const TileItem it = tile_item(e, c2n, g.th, g.tw);
    f32x2 d[S::T][S::T];
    load_patch(d, dy, it.b, S::T * it.ty, S::T * it.tx, g.oh, g.ow, ldy, it.c * 2,
               [&](size_t off) { return *(const f32x2*)(dy + off); });
    transform_store<S::T, S::P>(d, z + (size_t)it.t * cout + it.c * 2, fs, [](const auto& in, auto& out) { S::gp(in, out); });
  }
}

// dW[co][ci][i][j] = (A'^T S A')[i][j],  S_f[co][ci] at s[f*cout*cin + co*cin + ci], f = 0 .. P*P - 1
// st: s is stored [component][cin][cout] (the grouped reduction ran with its operands swapped: hnd_wino2_wgrad_output_t)
template <class S>
__global__ void wino2_wgrad_out_kernel(const float* __restrict__ s_, float* __restrict__ dw, int cout, int cin, int st) {
  constexpr int P = S::P;
  const long long total = (long long)cout * cin;
  const size_t fs = (size_t)total;
  for (long long e = first_item<false>(); e < total; e += (long long)gridDim.x * blockDim.x) {
    const float* s = s_ + (st ? (e % cin) * cout + e / cin : e) - e;
    float t[2][P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      float col[P], o[2];
#pragma unroll
      for (int i = 0; i < P; ++i) col[i] = s[(size_t)(i * P + j) * fs + e];
      S::a2t(col, o);
      t[0][j] = o[0];
      t[1][j] = o[1];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float o[2];
      S::a2t(t[i], o);
      dw[e * 4 + i * 2 + 0] = o[0];
      dw[e * 4 + i * 2 + 1] = o[1];
    }
  }
}

// ---------------------------------------------------------------------------------- fused BatchNorm-backward transforms
// BatchNorm backward "apply" fused into BOTH consumers of its result (round 4).  For the two deep decoder convs (conv6,
// conv7) the gradient w.r.t. the raw conv output, dy = k1 * d + k2 * x + k3 with d = [bn(x) > 0] * g, is read by exactly two
// kernels: the input transform of the conv's data gradient (V = B^T dy B over 7x7 patches) and the dy transform of its
// Winograd-domain weight gradient (Z = G' dy G'^T over the 6x6 tile inside that patch).  Materialising dy costs a pass
// of 12 B per element (hnd_bn_bwd_apply) plus 4 B per element in each transform; this kernel reads g and x once per patch
// and writes V and Z: 12 B per element less on the two largest tensors of the head.
// The two transforms tile different extents (data gradient: the conv INPUT, oh + 2 pad - 1; weight gradient: dy itself),
// so the launch walks the larger grid and each output exists only inside its own.
struct BnBwdTransformGeom {
  int n, oh, ow, c, pad;            // dy / g / x: [n][oh][ow][c]; pad = padding of the data-gradient correlation
  int th, tw;                       // tiles walked
  int th_d, tw_d, tiles_pad_d;      // data gradient (V)
  int th_w, tw_w, tiles_pad_w;      // weight gradient (Z)
};

__global__ void __launch_bounds__(256) wino26_bnbwd_transforms_kernel(
    const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ k123, int relu, float* __restrict__ v,
    float* __restrict__ z, const BnBwdTransformGeom q) {
  using S = F62;
  constexpr int T = S::T, P = S::P;
  const int c2n = q.c >> 1;
  const long long total = (long long)q.n * q.th * q.tw * c2n;
  const size_t fs_d = (size_t)q.tiles_pad_d * q.c, fs_w = (size_t)q.tiles_pad_w * q.c;
  for (long long e = first_item<true>(); e < total; e += (long long)gridDim.x * blockDim.x) {
    const TileItem it = tile_item(e, c2n, q.th, q.tw);
    const int c2 = it.c, tx = it.tx, ty = it.ty, b = it.b;
    const f32x2 sc = *(const f32x2*)(scale + c2 * 2), sh = *(const f32x2*)(shift + c2 * 2);
    const f32x2 k1 = *(const f32x2*)(k123 + c2 * 2), k2 = *(const f32x2*)(k123 + q.c + c2 * 2),
                k3 = *(const f32x2*)(k123 + 2 * q.c + c2 * 2);
    f32x2 d[P][P];                          // the dy patch
    load_patch(d, g, b, T * ty - q.pad, T * tx - q.pad, q.oh, q.ow, q.c, c2 * 2, [&](size_t off) {
      f32x2 dd = *(const f32x2*)(g + off);
      const f32x2 xv = *(const f32x2*)(x + off);
      if (relu) {
        const f32x2 out = xv * sc + sh;
        dd.x = out.x > 0.f ? dd.x : 0.f;
        dd.y = out.y > 0.f ? dd.y : 0.f;
      }
      return k1 * dd + k2 * xv + k3;
    });
    if (ty < q.th_w && tx < q.tw_w) {       // Z = G' dy G'^T of the 6x6 tile: patch rows / columns pad .. pad + 5
      f32x2 dt[T][T];
#pragma unroll
      for (int bb = 0; bb < T; ++bb)
#pragma unroll
        for (int a = 0; a < T; ++a) dt[bb][a] = q.pad ? d[bb + 1][a + 1] : d[bb][a];
      transform_store<T, P>(dt, z + ((size_t)((size_t)b * q.th_w + ty) * q.tw_w + tx) * q.c + c2 * 2, fs_w,
                            [](const auto& in, auto& out) { S::gp(in, out); });
    }
    if (ty < q.th_d && tx < q.tw_d)         // V = B^T dy B of the 7x7 patch
      transform_store<P, P>(d, v + ((size_t)((size_t)b * q.th_d + ty) * q.tw_d + tx) * q.c + c2 * 2, fs_d,
                            [](const auto& in, auto& out) { S::bt(in, out); });
  }
}

// ---------------------------------------------------------------------------------- host side
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// tiles of n maps of h x w outputs
inline long long tiles_of(int n, int h, int w, int tile) { return (long long)n * ceil_div(h, tile) * ceil_div(w, tile); }
inline int tiles_pad_of(int n, int h, int w, int tile) { return (int)((tiles_of(n, h, w, tile) + 127) / 128 * 128); }

inline WinoGeom wino_geom(int n, int h, int w, int c, int tile) {
  return WinoGeom{n, h, w, c, ceil_div(h, tile), ceil_div(w, tile), tiles_pad_of(n, h, w, tile)};
}

// h x w: the input (0 x 0 where the launch only sees the output side), oh x ow: the tiled extent
inline Wino2Geom wino2_geom(int n, int h, int w, int c, int oh, int ow, int pad, int tile) {
  return Wino2Geom{n, h, w, c, oh, ow, ceil_div(oh, tile), ceil_div(ow, tile), tiles_pad_of(n, oh, ow, tile), pad};
}

inline bool wino3_tile_ok(int tile) { return tile == 2 || tile == 4 || tile == 6; }
inline bool wino2_tile_ok(int tile) { return tile == 4 || tile == 6; }

// fn(scheme) for the scheme F(tile x tile, TAPS x TAPS); the tile has passed wino3_tile_ok / wino2_tile_ok
template <int TAPS, class Fn>
void with_scheme(int tile, Fn fn) {
  if constexpr (TAPS == 3) {
    if (tile == 2) fn(F23{});
    else if (tile == 4) fn(F43{});
    else fn(F63{});
  } else {
    if (tile == 4) fn(F42{});
    else fn(F62{});
  }
}

template <int TAPS>
void launch_weights(const float* weight, float* u, int cout, int cin, int dgrad, int tile, void* stream) {
  const int rows = dgrad ? cin : cout, kreal = dgrad ? cout : cin;
  const int rows_pad = (rows + 63) / 64 * 64;
  with_scheme<TAPS>(tile, [&](auto s) {
    hipLaunchKernelGGL(wino_weights_kernel<decltype(s)>, dim3(grid_for((long long)rows_pad * kreal)), dim3(256), 0,
                       hnd::as_stream(stream), weight, u, cout, cin, dgrad, rows, rows_pad, kreal);
  });
}

}  // namespace

extern "C" {

int64_t hnd_wino_tiles_pad(int n, int h, int w, int tile) {
  if (!wino3_tile_ok(tile)) return -1;
  return tiles_pad_of(n, h, w, tile);
}

int hnd_wino_weights(const float* weight, float* u, int cout, int cin, int dgrad, int tile, void* stream) {
  HND_REQUIRE(weight && u && cout > 0 && cin > 0 && (tile == 2 || tile == 4 || tile == 6),
              "hnd_wino_weights: bad arguments");
  const int kreal = dgrad ? cout : cin;
  HND_REQUIRE(kreal % 32 == 0, "hnd_wino_weights: GEMM depth %d must be a multiple of 32", kreal);
  launch_weights<3>(weight, u, cout, cin, dgrad, tile, stream);
  return hnd::check_launch("hnd_wino_weights");
}

int hnd_wino_input(const float* x, float* v, int n, int h, int w, int c, const float* pro_scale,
                   const float* pro_shift, int pro_relu, int tile, void* stream) {
  HND_REQUIRE(x && v && n > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0 && (tile == 2 || tile == 4 || tile == 6),
              "hnd_wino_input: bad arguments");
  HND_REQUIRE(pro_scale == nullptr || pro_shift != nullptr, "hnd_wino_input: pro_shift is required with pro_scale");
  const WinoGeom g = wino_geom(n, h, w, c, tile);
  with_scheme<3>(tile, [&](auto s) {
    using S = decltype(s);
    hipLaunchKernelGGL(wino_input_kernel<S>, dim3(grid_for(tiles_of(n, h, w, tile) * (c / lanes_of<typename S::V>))),
                       dim3(256), 0, hnd::as_stream(stream), x, v, g, pro_scale, pro_shift, pro_relu);
  });
  return hnd::check_launch("hnd_wino_input");
}

int hnd_wino_output(const float* m, float* y, int n, int h, int w, int cout, int ldc, const float* epi_scale,
                    const float* epi_shift, const float* res1, const float* mask, int relu, int tile, uint8_t* mask_out,
                    void* stream) {
  HND_REQUIRE(m && y && n > 0 && h > 0 && w > 0 && cout > 0 && cout % 4 == 0 && ldc >= cout && ldc % 4 == 0 &&
                  (tile == 2 || tile == 4 || tile == 6), "hnd_wino_output: bad arguments");
  HND_REQUIRE(!mask_out || (tile != 2 && cout == ldc), "hnd_wino_output: mask_out needs tile 4 / 6 and cout == ldc");
  const WinoGeom g = wino_geom(n, h, w, ldc, tile);
  const WinoEpilogue ep{epi_scale, epi_shift, res1, mask, relu, mask_out};
  const long long tiles = tiles_of(n, h, w, tile);
  hipStream_t st = hnd::as_stream(stream);
  with_scheme<3>(tile, [&](auto s) {
    using S = decltype(s);
    if constexpr (std::is_same_v<S, F23>) {
      hipLaunchKernelGGL(wino_output_kernel, dim3(grid_for(tiles * (cout / 4))), dim3(256), 0, st, m, y, g, cout, ep);
    } else {
      auto launch = [&](auto res, auto msk) {
        hipLaunchKernelGGL((wino3_output_kernel<S, decltype(res)::value, decltype(msk)::value>),
                           dim3(grid_for(tiles * (cout / 2))), dim3(256), 0, st, m, y, g, cout, ep);
      };
      if (res1 && mask) launch(std::true_type{}, std::true_type{});
      else if (res1) launch(std::true_type{}, std::false_type{});
      else if (mask) launch(std::false_type{}, std::true_type{});
      else launch(std::false_type{}, std::false_type{});
    }
  });
  return hnd::check_launch("hnd_wino_output");
}

/* ---- F(4x4, 2x2) / F(6x6, 2x2): the 2x2 convolutions of the student head; tile = 4 or 6 ---- */
int64_t hnd_wino2_tiles_pad(int n, int oh, int ow, int tile) {
  if (!wino2_tile_ok(tile)) return -1;
  return tiles_pad_of(n, oh, ow, tile);
}

int hnd_wino2_stats_blocks(int n, int oh, int ow, int cout, int tile) {
  if (!wino2_tile_ok(tile)) return -1;
  long long b = (tiles_of(n, oh, ow, tile) * (cout / 2) + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

int hnd_wino2_weights(const float* weight, float* u, int cout, int cin, int dgrad, int tile, void* stream) {
  HND_REQUIRE(weight && u && cout > 0 && cin > 0 && wino2_tile_ok(tile), "hnd_wino2_weights: bad arguments");
  const int kreal = dgrad ? cout : cin;
  HND_REQUIRE(kreal % 32 == 0, "hnd_wino2_weights: GEMM depth %d must be a multiple of 32", kreal);
  launch_weights<2>(weight, u, cout, cin, dgrad, tile, stream);
  return hnd::check_launch("hnd_wino2_weights");
}

int hnd_wino2_input(const float* x, float* v, int n, int h, int w, int c, int pad, const float* pro_scale,
                    const float* pro_shift, int pro_relu, int tile, void* stream) {
  HND_REQUIRE(x && v && n > 0 && h > 0 && w > 0 && c > 0 && c % 2 == 0 && (pad == 0 || pad == 1) &&
                  h + 2 * pad - 1 > 0 && w + 2 * pad - 1 > 0 && wino2_tile_ok(tile), "hnd_wino2_input: bad arguments");
  HND_REQUIRE(pro_scale == nullptr || pro_shift != nullptr, "hnd_wino2_input: pro_shift is required with pro_scale");
  const int oh = h + 2 * pad - 1, ow = w + 2 * pad - 1;
  const Wino2Geom g = wino2_geom(n, h, w, c, oh, ow, pad, tile);
  with_scheme<2>(tile, [&](auto s) {
    hipLaunchKernelGGL(wino_input_kernel<decltype(s)>, dim3(grid_for(tiles_of(n, oh, ow, tile) * (c / 2))), dim3(256), 0,
                       hnd::as_stream(stream), x, v, g, pro_scale, pro_shift, pro_relu);
  });
  return hnd::check_launch("hnd_wino2_input");
}

int hnd_wino2_output(const float* m, float* y, int n, int oh, int ow, int cout, int ldc, const float* epi_scale,
                     const float* epi_shift, int relu, float* stats, int tile, void* stream) {
  HND_REQUIRE(m && y && n > 0 && oh > 0 && ow > 0 && cout > 0 && cout % 2 == 0 && ldc >= cout && ldc % 2 == 0 &&
                  wino2_tile_ok(tile), "hnd_wino2_output: bad arguments");
  HND_REQUIRE(stats == nullptr || 512 % cout == 0, "hnd_wino2_output: stats need 512 %% cout == 0 (cout=%d)", cout);
  const Wino2Geom g = wino2_geom(n, 0, 0, 0, oh, ow, 0, tile);
  const int blocks = hnd_wino2_stats_blocks(n, oh, ow, cout, tile);
  with_scheme<2>(tile, [&](auto s) {
    hipLaunchKernelGGL((wino2_output_kernel<decltype(s), false>), dim3(blocks), dim3(256), 0, hnd::as_stream(stream), m, y,
                       g, cout, ldc, epi_scale, epi_shift, relu, stats, BnBwdStatsArgs{});
  });
  return hnd::check_launch("hnd_wino2_output");
}

int hnd_wino26_output_bnbwd_stats(const float* m, float* y, int n, int oh, int ow, int cout, int ldc, const float* x,
                                  const float* scale, const float* shift, const float* mean, const float* rstd,
                                  int relu_of_bn, float* partials, void* stream) {
  HND_REQUIRE(m && y && x && scale && shift && mean && rstd && partials && n > 0 && oh > 0 && ow > 0 && cout > 0 &&
                  cout % 2 == 0 && ldc >= cout && ldc % 2 == 0 && 512 % cout == 0,
              "hnd_wino26_output_bnbwd_stats: bad arguments (cout=%d must divide 512)", cout);
  const Wino2Geom g = wino2_geom(n, 0, 0, 0, oh, ow, 0, 6);
  const int blocks = hnd_wino2_stats_blocks(n, oh, ow, cout, 6);
  hipLaunchKernelGGL((wino2_output_kernel<F62, true>), dim3(blocks), dim3(256), 0, hnd::as_stream(stream), m, y, g, cout,
                     ldc, (const float*)nullptr, (const float*)nullptr, 0, partials,
                     BnBwdStatsArgs{x, scale, shift, mean, rstd, relu_of_bn});
  return hnd::check_launch("hnd_wino26_output_bnbwd_stats");
}

/* Winograd-domain weight gradient of a 2x2 head conv: z = G' dy G'^T per tile of dy [n][oh][ow][ldy] ->
 * z [(tile+1)^2][tiles_pad][cout]; after the grouped GEMMs s[f][cout][cin] = sum_t z_f[t][co] v_f[t][ci]
 * (hnd_conv2d_wgrad, groups = (tile+1)^2), hnd_wino2_wgrad_output writes dW [cout][cin][2][2]. */
int hnd_wino2_dy(const float* dy, float* z, int n, int oh, int ow, int cout, int ldy, int tile, void* stream) {
  HND_REQUIRE(dy && z && n > 0 && oh > 0 && ow > 0 && cout > 0 && cout % 2 == 0 && ldy >= cout && ldy % 2 == 0 &&
                  wino2_tile_ok(tile), "hnd_wino2_dy: bad arguments");
  const Wino2Geom g = wino2_geom(n, 0, 0, 0, oh, ow, 0, tile);
  with_scheme<2>(tile, [&](auto s) {
    hipLaunchKernelGGL(wino2_dy_kernel<decltype(s)>, dim3(grid_for(tiles_of(n, oh, ow, tile) * (cout / 2))), dim3(256), 0,
                       hnd::as_stream(stream), dy, z, g, cout, ldy);
  });
  return hnd::check_launch("hnd_wino2_dy");
}

int hnd_wino26_bnbwd_transforms(const float* g, const float* x, const float* scale, const float* shift,
                                const float* k123, int relu, int n, int oh, int ow, int c, int pad, float* v, float* z,
                                void* stream) {
  HND_REQUIRE(g && x && scale && shift && k123 && v && z && n > 0 && oh > 0 && ow > 0 && c > 0 && c % 2 == 0 &&
                  (pad == 0 || pad == 1) && oh + 2 * pad - 1 > 0 && ow + 2 * pad - 1 > 0,
              "hnd_wino26_bnbwd_transforms: bad arguments");
  const int ih = oh + 2 * pad - 1, iw = ow + 2 * pad - 1;      // extent of the data gradient's output (the conv input)
  BnBwdTransformGeom q;
  q.n = n; q.oh = oh; q.ow = ow; q.c = c; q.pad = pad;
  q.th_d = ceil_div(ih, 6); q.tw_d = ceil_div(iw, 6); q.tiles_pad_d = tiles_pad_of(n, ih, iw, 6);
  q.th_w = ceil_div(oh, 6); q.tw_w = ceil_div(ow, 6); q.tiles_pad_w = tiles_pad_of(n, oh, ow, 6);
  q.th = q.th_d > q.th_w ? q.th_d : q.th_w;
  q.tw = q.tw_d > q.tw_w ? q.tw_d : q.tw_w;
  const long long tiles = (long long)n * q.th * q.tw;
  hipLaunchKernelGGL(wino26_bnbwd_transforms_kernel, dim3(grid_for(tiles * (c / 2))), dim3(256), 0,
                     hnd::as_stream(stream), g, x, scale, shift, k123, relu, v, z, q);
  return hnd::check_launch("hnd_wino26_bnbwd_transforms");
}

int hnd_wino2_wgrad_output_t(const float* s, float* dw, int cout, int cin, int tile, int s_transposed, void* stream) {
  HND_REQUIRE(s && dw && cout > 0 && cin > 0 && wino2_tile_ok(tile), "hnd_wino2_wgrad_output: bad arguments");
  with_scheme<2>(tile, [&](auto sch) {
    hipLaunchKernelGGL(wino2_wgrad_out_kernel<decltype(sch)>, dim3(grid_for((long long)cout * cin)), dim3(256), 0,
                       hnd::as_stream(stream), s, dw, cout, cin, s_transposed ? 1 : 0);
  });
  return hnd::check_launch("hnd_wino2_wgrad_output");
}

int hnd_wino2_wgrad_output(const float* s, float* dw, int cout, int cin, int tile, void* stream) {
  return hnd_wino2_wgrad_output_t(s, dw, cout, cin, tile, 0, stream);
}

}  // extern "C"
