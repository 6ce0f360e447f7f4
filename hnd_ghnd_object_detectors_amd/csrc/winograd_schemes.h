// The minimal-filtering schemes F(m x m, r x r) of winograd.hip: one struct per scheme with what differs between them --
// the sizes, the vector a thread owns, the geometry struct of its launches, its padding, how its input transform walks
// the grid, its launch bound -- and its transform matrices as row functions out = M in over arrays of one value per
// matrix column.  A row function is applied twice per transform (down the columns, then along the rows).
//
// With -ffp-contract=fast the expression tree of a row IS its rounding: every body below keeps the grouping and the
// temporaries it was first written with (tests/wino_util.py counts the roundings of exactly these trees).
#pragma once

#include "common.h"

namespace wino {

using hnd::f32x4;
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct WinoGeom {
  int n, h, w, c;          // tensor being transformed (input: c = cin; output: c = ldc of y)
  int th, tw;              // tiles per image
  int tiles_pad;           // rows per component in V / M (multiple of 128)
};

struct Wino2Geom {
  int n, h, w, c;          // input tensor
  int oh, ow;              // output extent (h + 2q - 1)
  int th, tw, tiles_pad, pad;
};

// out = M in for a compile-time matrix: fully unrolled, zero entries vanish, +-1 become add / subtract
template <int R, int C, class V>
__device__ __forceinline__ void mat_apply(const float (&M)[R][C], const V (&in)[C], V (&out)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    V acc = in[0] * 0.f;
    bool first = true;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float m = M[r][c];
      if (m == 0.f) continue;
      const V term = m == 1.f ? in[c] : (m == -1.f ? -in[c] : in[c] * m);
      acc = first ? term : acc + term;
      first = false;
    }
    out[r] = acc;
  }
}

// ---------------------------------------------------------------------------------- 3x3, stride 1, padding 1
struct Scheme3 {
  static constexpr int R = 3;
  using Geom = WinoGeom;
  static __device__ __forceinline__ int pad(const Geom&) { return 1; }
};

// F(2x2, 3x3): 16 multiplies per 2x2 output tile instead of 36; the transforms only add / halve.  Four channels per thread.
struct F23 : Scheme3 {
  static constexpr int T = 2, P = 4, kLaunchBound = 1024;
  static constexpr bool kXcdWalk = false;
  using V = f32x4;
  template <class X> static __device__ __forceinline__ void bt(const X (&d)[4], X (&o)[4]) {
    o[0] = d[0] - d[2];
    o[1] = d[1] + d[2];
    o[2] = d[2] - d[1];
    o[3] = d[1] - d[3];
  }
  template <class X> static __device__ __forceinline__ void at(const X (&m)[4], X (&o)[2]) {
    o[0] = m[0] + m[1] + m[2];
    o[1] = m[1] - m[2] - m[3];
  }
  template <class X> static __device__ __forceinline__ void g(const X (&w)[3], X (&o)[4]) {
    o[0] = w[0];
    o[1] = 0.5f * (w[0] + w[1] + w[2]);
    o[2] = 0.5f * (w[0] - w[1] + w[2]);
    o[3] = w[2];
  }
};

// F(4x4, 3x3).  Interpolation points {0, +-1, +-2, inf}: 36 products per 4x4 output tile = 4x fewer multiplies than
// direct, and the transformed tensors inflate by 36/16 = 2.25x (F(2x2,3x3): 4x).  Two channels per thread keep the
// 6x6 patch in 72 VGPRs.
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
struct F43 : Scheme3 {
  static constexpr int T = 4, P = 6, kLaunchBound = 1024;
  static constexpr bool kXcdWalk = false;
  using V = f32x2;
  template <class X> static __device__ __forceinline__ void bt(const X (&d)[6], X (&o)[6]) {
    const X t0_ = 4.f * d[0] - 5.f * d[2] + d[4];
    const X t1_ = -4.f * (d[1] + d[2]) + d[3] + d[4];
    const X t2_ = 4.f * (d[1] - d[2]) - d[3] + d[4];
    const X t3_ = -2.f * d[1] - d[2] + 2.f * d[3] + d[4];
    const X t4_ = 2.f * d[1] - d[2] - 2.f * d[3] + d[4];
    const X t5_ = 4.f * d[1] - 5.f * d[3] + d[5];
    o[0] = t0_; o[1] = t1_; o[2] = t2_; o[3] = t3_; o[4] = t4_; o[5] = t5_;
  }
  template <class X> static __device__ __forceinline__ void at(const X (&m)[6], X (&o)[4]) {
    const X p12 = m[1] + m[2], q12 = m[1] - m[2], p34 = m[3] + m[4], q34 = m[3] - m[4];
    o[0] = m[0] + p12 + p34;
    o[1] = q12 + 2.f * q34;
    o[2] = p12 + 4.f * p34;
    o[3] = q12 + 8.f * q34 + m[5];
  }
  template <class X> static __device__ __forceinline__ void g(const X (&w)[3], X (&o)[6]) {
    const X a = w[0], b = w[1], c = w[2];
    o[0] = a * (1.f / 4.f);
    o[1] = -(a + b + c) * (1.f / 6.f);
    o[2] = (-a + b - c) * (1.f / 6.f);
    o[3] = a * (1.f / 24.f) + b * (1.f / 12.f) + c * (1.f / 6.f);
    o[4] = a * (1.f / 24.f) - b * (1.f / 12.f) + c * (1.f / 6.f);
    o[5] = c;
  }
};

// F(6x6, 3x3).  Interpolation points {0, +-1, +-2, +-1/2, inf}: 64 products per 6x6 output tile = 5.06x fewer multiplies
// than direct (F(4x4,3x3): 4x) and transformed tensors of 64/36 = 1.78x the activation (F(4x4,3x3): 2.25x) -- 21 % fewer
// GEMM flops AND 21 % fewer transform bytes than F(4x4,3x3).  fp32 error against exact convolution on post-ReLU data,
// K = 256: rel-L2 5e-6 (F(4x4,3x3): 2.6e-6; direct fp32 summation: 2e-7) -- far inside the 1e-3 parity bar.  Used
// where the 6x6 tiling wastes little (>= 50x84 maps); matrices (Cook-Toom, checked against direct correlation in
// fp64 to 3e-14):
//   B^T = [1 0 -21/4 0 21/4 0 -1 0; 0 1 1 -17/4 -17/4 1 1 0; 0 -1 1 17/4 -17/4 -1 1 0; 0 1/2 1/4 -5/2 -5/4 2 1 0;
//          0 -1/2 1/4 5/2 -5/4 -2 1 0; 0 2 4 -5/2 -5 1/2 1 0; 0 -2 4 5/2 -5 -1/2 1 0; 0 -1 0 21/4 0 -21/4 0 1]
//   G   = [1 0 0; -2/9 -2/9 -2/9; -2/9 2/9 -2/9; 1/90 1/45 2/45; 1/90 -1/45 2/45; 32/45 16/45 8/45;
//          32/45 -16/45 8/45; 0 0 1]
//   A^T = [1 1 1 1 1 1 1 0; 0 1 -1 2 -2 1/2 -1/2 0; 0 1 1 4 4 1/4 1/4 0; 0 1 -1 8 -8 1/8 -1/8 0;
//          0 1 1 16 16 1/16 1/16 0; 0 1 -1 32 -32 1/32 -1/32 1]
// The 8x8 input patch, two channels per thread, is 128 VGPRs.
struct F63 : Scheme3 {
  static constexpr int T = 6, P = 8, kLaunchBound = 256;
  static constexpr bool kXcdWalk = true;
  using V = f32x2;
  template <class X> static __device__ __forceinline__ void bt(const X (&d)[8], X (&o)[8]) {
    const X e26_ = d[2] + d[6] - 4.25f * d[4], o15_ = d[1] + d[5] - 4.25f * d[3];
    const X e3_ = 0.25f * d[2] - 1.25f * d[4] + d[6], o3_ = 0.5f * d[1] - 2.5f * d[3] + 2.f * d[5];
    const X e5_ = 4.f * d[2] - 5.f * d[4] + d[6], o5_ = 2.f * d[1] - 2.5f * d[3] + 0.5f * d[5];
    const X t0_ = d[0] - d[6] + 5.25f * (d[4] - d[2]), t7_ = d[7] - d[1] + 5.25f * (d[3] - d[5]);
    o[0] = t0_; o[1] = e26_ + o15_; o[2] = e26_ - o15_; o[3] = e3_ + o3_; o[4] = e3_ - o3_;
    o[5] = e5_ + o5_; o[6] = e5_ - o5_; o[7] = t7_;
  }
  template <class X> static __device__ __forceinline__ void at(const X (&m)[8], X (&o)[6]) {
    const X p12 = m[1] + m[2], q12 = m[1] - m[2], p34 = m[3] + m[4], q34 = m[3] - m[4], p56 = m[5] + m[6],
            q56 = m[5] - m[6];
    o[0] = m[0] + p12 + p34 + p56;
    o[1] = q12 + 2.f * q34 + 0.5f * q56;
    o[2] = p12 + 4.f * p34 + 0.25f * p56;
    o[3] = q12 + 8.f * q34 + 0.125f * q56;
    o[4] = p12 + 16.f * p34 + 0.0625f * p56;
    o[5] = q12 + 32.f * q34 + 0.03125f * q56 + m[7];
  }
  template <class X> static __device__ __forceinline__ void g(const X (&w)[3], X (&o)[8]) {
    const X a = w[0], b = w[1], c = w[2];
    o[0] = a;
    o[1] = -(a + b + c) * (2.f / 9.f);
    o[2] = (-a + b - c) * (2.f / 9.f);
    o[3] = a * (1.f / 90.f) + b * (1.f / 45.f) + c * (2.f / 45.f);
    o[4] = a * (1.f / 90.f) - b * (1.f / 45.f) + c * (2.f / 45.f);
    o[5] = a * (32.f / 45.f) + b * (16.f / 45.f) + c * (8.f / 45.f);
    o[6] = a * (32.f / 45.f) - b * (16.f / 45.f) + c * (8.f / 45.f);
    o[7] = c;
  }
};

// ---------------------------------------------------------------------------------- 2x2, stride 1, padding q in {0, 1}
// The student head's 2x2 convolutions (src/models/mimic/resnet_layer.py:43-62) and their data gradients.
// Correlation with padding q: out[y][x] = sum_ij w[i][j] in[y+i-q][x+j-q], output (h+2q-1) x (w+2q-1).  The data gradient
// of such a conv is the same correlation with flipped, transposed weights and padding 1-q.
// Weight gradient: dW[i][j] = sum over tiles of sum_ab dy_t[a][b] d_t[a+i][b+j] is the minimal-filtering problem
// F(2x2, m x m) with the dy tile in the role of the filter.  Same points => the data transform B^T d B is the V the
// forward pass already produced; the dy transform makes Z = G' dy_t G'^T (gp), (m+1)^2 grouped GEMMs reduce
// S_f[co][ci] = sum_t Z_f[t][co] V_f[t][ci] over the tiles, and dW = A'^T S A' (a2t) is a per-(co, ci) epilogue.
struct Scheme2 {
  static constexpr int R = 2;
  using Geom = Wino2Geom;
  using V = f32x2;
  static __device__ __forceinline__ int pad(const Geom& g) { return g.pad; }
};

// F(4x4, 2x2) / F(2x2, 4x4).  Points {0, 1, -1, 2, inf}: 25 products per 4x4 output tile instead of 64 (2.56x fewer),
// transformed tensors 25/16 = 1.56x.
//   A^T = [1 1 1 1 0; 0 1 -1 2 0; 0 1 1 4 0; 0 1 -1 8 1]
//   G   = [1/2 0; -1/2 -1/2; -1/6 1/6; 1/6 1/3; 0 1]
//   B^T = [2 -1 -2 1 0; 0 -2 -1 1 0; 0 2 -3 1 0; 0 -1 0 1 0; 0 2 -1 -2 1]
//   G'  = [1/2 0 0 0; -1/2 -1/2 -1/2 -1/2; -1/6 1/6 -1/6 1/6; 1/6 1/3 2/3 4/3; 0 0 0 1]
//   A'^T = [1 1 1 1 0; 0 1 -1 2 1]
struct F42 : Scheme2 {
  static constexpr int T = 4, P = 5, kLaunchBound = 1024;
  static constexpr bool kXcdWalk = false;
  template <class X> static __device__ __forceinline__ void bt(const X (&d)[5], X (&o)[5]) {
    const X t0_ = 2.f * (d[0] - d[2]) - d[1] + d[3];
    const X t1_ = -2.f * d[1] - d[2] + d[3];
    const X t2_ = 2.f * d[1] - 3.f * d[2] + d[3];
    const X t3_ = d[3] - d[1];
    const X t4_ = 2.f * (d[1] - d[3]) - d[2] + d[4];
    o[0] = t0_; o[1] = t1_; o[2] = t2_; o[3] = t3_; o[4] = t4_;
  }
  template <class X> static __device__ __forceinline__ void at(const X (&m)[5], X (&o)[4]) {
    const X p12 = m[1] + m[2], q12 = m[1] - m[2];
    o[0] = m[0] + p12 + m[3];
    o[1] = q12 + 2.f * m[3];
    o[2] = p12 + 4.f * m[3];
    o[3] = q12 + 8.f * m[3] + m[4];
  }
  template <class X> static __device__ __forceinline__ void g(const X (&w)[2], X (&o)[5]) {
    const X a = w[0], b = w[1];
    o[0] = 0.5f * a;
    o[1] = -0.5f * (a + b);
    o[2] = (b - a) * (1.f / 6.f);
    o[3] = a * (1.f / 6.f) + b * (1.f / 3.f);
    o[4] = b;
  }
  template <class X> static __device__ __forceinline__ void gp(const X (&g)[4], X (&o)[5]) {
    const X e_ = g[0] + g[2], f_ = g[1] + g[3];
    o[0] = 0.5f * g[0];
    o[1] = -0.5f * (e_ + f_);
    o[2] = (f_ - e_) * (1.f / 6.f);
    o[3] = g[0] * (1.f / 6.f) + g[1] * (1.f / 3.f) + g[2] * (2.f / 3.f) + g[3] * (4.f / 3.f);
    o[4] = g[3];
  }
  template <class X> static __device__ __forceinline__ void a2t(const X (&m)[5], X (&o)[2]) {
    o[0] = m[0] + m[1] + m[2] + m[3];
    o[1] = m[1] - m[2] + 2.f * m[3] + m[4];
  }
};

// F(6x6, 2x2) / F(2x2, 6x6).  Points {0, 1, -1, 2, -2, 1/2, inf}: 49 products per 36 outputs instead of 25 per 16 (12.9 %
// fewer GEMM flops; transformed tensors 1.36x instead of 1.56x the activation).  fp32 error against exact correlation,
// post-ReLU data, K = 256: relative L2 4.1e-6 (F(4x4,2x2): 1.7e-6).  Matrices by Cook-Toom in exact rationals (all row
// scalings 1 / prod_{l != j}(a_j - a_l) sit in G, so B^T depends on the points only and the weight-gradient problem shares
// the forward pass's V = B^T d B); checked against direct correlation in fp64 to 1e-15.
constexpr float W6_AT[6][7] = {{1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 0.f},
                               {0.f, 1.f, -1.f, 2.f, -2.f, 1.f / 2.f, 0.f},
                               {0.f, 1.f, 1.f, 4.f, 4.f, 1.f / 4.f, 0.f},
                               {0.f, 1.f, -1.f, 8.f, -8.f, 1.f / 8.f, 0.f},
                               {0.f, 1.f, 1.f, 16.f, 16.f, 1.f / 16.f, 0.f},
                               {0.f, 1.f, -1.f, 32.f, -32.f, 1.f / 32.f, 1.f}};
constexpr float W6_G[7][2] = {{-1.f / 2.f, 0.f},        {-1.f / 3.f, -1.f / 3.f}, {1.f / 9.f, -1.f / 9.f},
                              {1.f / 36.f, 1.f / 18.f}, {-1.f / 60.f, 1.f / 30.f}, {32.f / 45.f, 16.f / 45.f},
                              {0.f, 1.f}};
constexpr float W6_BT[7][7] = {{-2.f, 4.f, 5.f / 2.f, -5.f, -1.f / 2.f, 1.f, 0.f},
                               {0.f, 2.f, -2.f, -9.f / 2.f, 1.f / 2.f, 1.f, 0.f},
                               {0.f, -2.f, 6.f, -7.f / 2.f, -3.f / 2.f, 1.f, 0.f},
                               {0.f, 1.f, -3.f / 2.f, -2.f, 3.f / 2.f, 1.f, 0.f},
                               {0.f, -1.f, 5.f / 2.f, 0.f, -5.f / 2.f, 1.f, 0.f},
                               {0.f, 4.f, 0.f, -5.f, 0.f, 1.f, 0.f},
                               {0.f, -2.f, 4.f, 5.f / 2.f, -5.f, -1.f / 2.f, 1.f}};
constexpr float W6_G2[7][6] = {{-1.f / 2.f, 0.f, 0.f, 0.f, 0.f, 0.f},
                               {-1.f / 3.f, -1.f / 3.f, -1.f / 3.f, -1.f / 3.f, -1.f / 3.f, -1.f / 3.f},
                               {1.f / 9.f, -1.f / 9.f, 1.f / 9.f, -1.f / 9.f, 1.f / 9.f, -1.f / 9.f},
                               {1.f / 36.f, 1.f / 18.f, 1.f / 9.f, 2.f / 9.f, 4.f / 9.f, 8.f / 9.f},
                               {-1.f / 60.f, 1.f / 30.f, -1.f / 15.f, 2.f / 15.f, -4.f / 15.f, 8.f / 15.f},
                               {32.f / 45.f, 16.f / 45.f, 8.f / 45.f, 4.f / 45.f, 2.f / 45.f, 1.f / 45.f},
                               {0.f, 0.f, 0.f, 0.f, 0.f, 1.f}};
constexpr float W6_A2T[2][7] = {{1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 0.f}, {0.f, 1.f, -1.f, 2.f, -2.f, 1.f / 2.f, 1.f}};

struct F62 : Scheme2 {
  static constexpr int T = 6, P = 7, kLaunchBound = 256;
  static constexpr bool kXcdWalk = true;
  template <class X> static __device__ __forceinline__ void bt(const X (&d)[7], X (&o)[7]) { mat_apply(W6_BT, d, o); }
  template <class X> static __device__ __forceinline__ void at(const X (&m)[7], X (&o)[6]) { mat_apply(W6_AT, m, o); }
  template <class X> static __device__ __forceinline__ void g(const X (&w)[2], X (&o)[7]) { mat_apply(W6_G, w, o); }
  template <class X> static __device__ __forceinline__ void gp(const X (&g)[6], X (&o)[7]) { mat_apply(W6_G2, g, o); }
  template <class X> static __device__ __forceinline__ void a2t(const X (&m)[7], X (&o)[2]) { mat_apply(W6_A2T, m, o); }
};

}  // namespace wino
