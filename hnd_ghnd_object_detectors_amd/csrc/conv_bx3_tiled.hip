// Tiled build of the fp32-on-bf16-pipe emulation GEMM (conv_bx3.hip is the persistent build): one workgroup per
// (64 MI)-row x 64-column output tile, grid = tiles, several workgroups resident per CU, so that a launch with few 64-row
// chunks per team of the persistent kernel (small batches, the coarse FPN levels, layer4) still fills the chip and latency
// is hidden by occupancy instead of a hand-counted register ring.  Everything here is compiler-visible loads + LDS.
//
// SAME BITS as bx3_kernel (DESIGN section 4 rule 4) -- what that rests on:
//   * operands split by the family's one split_pair and multiplied by its one six-product step, mfma6 (bf16x3.h; the weight
//     image is the persistent build's own);
//   * the same v_mfma_f32_16x16x32_bf16 with every k value in the lane and element position it has there: lane l16 = row (A) /
//     column (B) of the 16-wide tile, lane group g4 holds k = 32 ks + 8 g4 .. + 7;
//   * per 32-k step the six products lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi, k steps ascending, a fresh accumulator per
//     256-k part;
//   * K > 256: the value the persistent build carries between its passes through y -- pass 1 acc * scale + shift (+ res1),
//     pass p (acc * scale + 0) + y -- is carried in registers here (one dispatch; an fp32 store / load round trip is exact),
//     rounded by the same expressions in the same order; mask, ReLU and the mask nibbles after the last part.
//
// Staging.  The 96 KB whole-slice stage of the persistent build would cap a CU at one workgroup; B is staged in 64-k pieces
// (3 planes x 64 columns x 64 k of bf16 = 24 KB), double-buffered (48 KB: three workgroups per CU), one barrier per piece.
// The image's XOR (chunk c of row r at c ^ (r & 15)) permutes 16-byte chunks inside aligned groups of 16, so a piece is a
// gather of whole chunks; the stage has a swizzle of its own (chunk c of row r at c ^ ((r >> 1) & 7): the 8 rows of lane
// group g4 and the 8 of g4 + 1 that one ds_read_b128 lane group holds fall on all 64 banks once).  The B piece of the NEXT piece is requested before the
// current piece's MFMAs, its A fragments as soon as the current ones are split.  Resource usage of both
// instantiations: profiles/r07_bx3_tiled_resources.txt.
#include "bf16x3.h"
#include "common.h"

namespace {

using hnd::bf8;
using hnd::f32x4;
using hnd::FastDiv;
using hnd::u32x4;

struct Bx3tArgs {
  FastDiv div_ow, div_oh;     // m -> (n, oh, ow) of the A rows
  int nsl;                    // 64-column weight slices
  int mrows;                  // M
  int cpg;                    // 64-row chunks per weight group (Winograd component), 0 = one group
  int tpg;                    // row tiles per weight group (ceil(cpg / MI)), 0 = one group
  int ngroups;                // weight groups of the image
  int res_up;                 // res1 is the exactly 2x coarser map, nearest-upsampled
};

// MI: 16-row groups per wave; the workgroup's 4 waves stack to a 64 MI-row tile on one 64-column slice.
template <int MI>
__global__ void __launch_bounds__(256, MI == 1 ? 3 : 2) bx3t_kernel(const hnd_conv_desc d, const Bx3tArgs a) {
  constexpr int NI = 4, KP = 64, PPLANE = 64 * KP, PBUF = 3 * PPLANE, NB = PBUF / 8 / 256;      // NB = 6 chunks per thread
  __shared__ __attribute__((aligned(16))) uint16_t Bs[2][PBUF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int lb = hnd::xcd_contiguous_block();       // the nsl tiles that share A rows are neighbours on one XCD
  const int rt = lb / a.nsl, slice = lb - rt * a.nsl;
  int grp = 0, row0 = rt * 64 * MI, mlim = a.mrows;
  if (a.tpg > 0) {
    grp = rt / a.tpg;
    row0 = (grp * a.cpg + (rt - grp * a.tpg) * MI) * 64;
    mlim = min((grp + 1) * a.cpg * 64, a.mrows);
  }
  const int wrow0 = row0 + wave * 16 * MI;
  const int KI = d.kdim == 128 ? 128 : 256, ppp = KI / KP, npieces = d.kdim / KP;
  const size_t slice_elems = (size_t)3 * 64 * KI;
  const int col0 = slice * 64 + l16 * 4;

  // rows past the tile's limit (a tail, or the odd last chunk of a group) are clamped in every address and never stored
  const float* ap[MI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const unsigned m = (unsigned)min(wrow0 + mi * 16 + l16, mlim - 1);
    const unsigned t = hnd::fdiv(m, a.div_ow), ow_ = m - t * (unsigned)d.ow;
    const unsigned n_ = hnd::fdiv(t, a.div_oh), oh_ = t - n_ * (unsigned)d.oh;
    const size_t pix = ((size_t)n_ * d.h + oh_ * (unsigned)d.sh) * (size_t)d.w_ + ow_ * (unsigned)d.sw;
    ap[mi] = d.x + pix * (size_t)d.cin + (size_t)(g4 * 8);
  }
  float es[NI], eb[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    es[ni] = d.epi_scale ? d.epi_scale[col0 + ni] : 1.f;
    eb[ni] = d.epi_shift ? d.epi_shift[col0 + ni] : 0.f;
  }

  u32x4 bt[NB];
  f32x4 acur[MI][2][2];      // the piece's A fragments; refilled for the next piece as soon as a k step is split
  auto load_b = [&](int pc) __attribute__((always_inline)) {
    const int part = pc / ppp, pin = pc - part * ppp;
    const uint16_t* base = d.w_bf16x3 + (((size_t)part * a.ngroups + grp) * a.nsl + slice) * slice_elems;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int idx = u * 256 + tid, plane = idx >> 9, row = (idx >> 3) & 63, cl = idx & 7;
      bt[u] = *(const u32x4*)(base + (size_t)plane * 64 * KI + row * KI + (((pin * 8 + cl) ^ (row & 15)) * 8));
    }
  };
  auto store_b = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int idx = u * 256 + tid, plane = idx >> 9, row = (idx >> 3) & 63, cl = idx & 7;
      *(u32x4*)(&Bs[buf][plane * PPLANE + row * KP + ((cl ^ ((row >> 1) & 7)) * 8)]) = bt[u];
    }
  };
  auto load_a = [&](int pc, int ksl) __attribute__((always_inline)) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      acur[mi][ksl][0] = *(const f32x4*)(ap[mi] + pc * KP + ksl * 32);
      acur[mi][ksl][1] = *(const f32x4*)(ap[mi] + pc * KP + ksl * 32 + 4);
    }
  };

  load_b(0);
  load_a(0, 0);
  load_a(0, 1);
  store_b(0);
  __syncthreads();

  f32x4 acc[MI][NI], run[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) run[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  int pin = 0, part = 0;
#pragma unroll 1
  for (int pc = 0; pc < npieces; ++pc) {
    const bool more = pc + 1 < npieces;
    if (more) load_b(pc + 1);
    if (pin == 0) {                                   // a fresh accumulator per 256-k part
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const uint16_t* B = Bs[pc & 1];
#pragma unroll
    for (int ksl = 0; ksl < 2; ++ksl) {
      bf8 ah[MI], am[MI], al[MI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        u32x4 h, m, l;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 v = acur[mi][ksl][j >> 1];
          const float x0 = (j & 1) ? v.z : v.x, x1 = (j & 1) ? v.w : v.y;
          uint32_t hp, mp, lp;
          hnd::split_pair(x0, x1, hp, mp, lp);
          h[j] = hp; m[j] = mp; l[j] = lp;
        }
        ah[mi] = __builtin_bit_cast(bf8, h);
        am[mi] = __builtin_bit_cast(bf8, m);
        al[mi] = __builtin_bit_cast(bf8, l);
      }
      if (more) load_a(pc + 1, ksl);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int row = ni * 16 + l16;
        const uint16_t* br = B + row * KP + (((ksl * 4 + g4) ^ ((row >> 1) & 7)) * 8);
        const bf8 b[3] = {*(const bf8*)(br), *(const bf8*)(br + PPLANE), *(const bf8*)(br + 2 * PPLANE)};      // hi, mid, lo
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) hnd::mfma6(acc[mi][ni], ah[mi], am[mi], al[mi], b);
      }
    }
    if (more) store_b((pc + 1) & 1);      // (last read during piece pc - 1: every wave is past the barrier that closed it)
    if (++pin == ppp) {
      // the part's end = one pass of the persistent build: x = acc * scale + shift (+ res1) first, (acc * scale + 0) + running
      // value afterwards -- the same expressions in the same order
      pin = 0;
      const bool first = part == 0;
      ++part;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          f32x4 rv = {0.f, 0.f, 0.f, 0.f};
          bool add = !first;
          if (first) {
            add = d.res1 != nullptr;
            if (add) {
              const unsigned m = (unsigned)min(wrow0 + mi * 16 + g4 * 4 + r, mlim - 1);
              size_t p = m;
              if (a.res_up) {       // pixel (n, y, x) reads (n, y / 2, x / 2) of the coarser map
                const unsigned t = hnd::fdiv(m, a.div_ow), ow_ = m - t * (unsigned)d.ow;
                const unsigned n_ = hnd::fdiv(t, a.div_oh), oh_ = t - n_ * (unsigned)d.oh;
                p = ((size_t)n_ * d.res1_h + (oh_ >> 1)) * (size_t)d.res1_w + (ow_ >> 1);
              }
              rv = *(const f32x4*)(d.res1 + p * (size_t)d.ldc + col0);
            }
          } else {
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) rv[ni] = run[mi][ni][r];
          }
#pragma unroll
          for (int ni = 0; ni < NI; ++ni) {
            float x = acc[mi][ni][r] * es[ni] + (first ? eb[ni] : 0.f);
            if (add) x += rv[ni];
            run[mi][ni][r] = x;
          }
        }
    }
    __syncthreads();
  }

  // after the last part: ReLU-backward mask, ReLU, store, mask nibbles of the stored values
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = wrow0 + mi * 16 + g4 * 4 + r;
      if (m >= mlim) continue;
      const size_t yo = (size_t)m * (size_t)d.ldc + col0;
      uint32_t mk = 0xfu;
      if (d.mask_bits) mk = d.mask_bits[yo >> 2];
      f32x4 v;
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        float x = run[mi][ni][r];
        x = ((mk >> ni) & 1u) ? x : 0.f;
        v[ni] = d.relu ? fmaxf(x, 0.f) : x;
      }
      *(f32x4*)(d.y + yo) = v;
      if (d.mask_out) d.mask_out[yo >> 2] = hnd::relu_mask_nibble(v);
    }
}

template <int MI>
int launch_bx3t_t(const hnd_conv_desc& d, hipStream_t stream) {
  Bx3tArgs a;
  a.div_ow = hnd::make_fastdiv((unsigned)d.ow);
  a.div_oh = hnd::make_fastdiv((unsigned)d.oh);
  a.nsl = d.cout / 64;
  a.mrows = (int)((long long)d.n * d.oh * d.ow);
  a.cpg = d.w_group_rows / 64;
  a.res_up = d.res1 && d.res1_mode == 1;
  const int nchunks = (a.mrows + 63) / 64;
  long long row_tiles;
  if (a.cpg > 0) {
    a.ngroups = nchunks / a.cpg;
    a.tpg = (a.cpg + MI - 1) / MI;
    row_tiles = (long long)a.ngroups * a.tpg;
  } else {
    a.ngroups = 1;
    a.tpg = 0;
    row_tiles = (nchunks + MI - 1) / MI;
  }
  const long long grid = row_tiles * a.nsl;
  if (grid <= 0 || grid >= (1ll << 31)) {
    hnd::set_error("launch_bx3_tiled: grid of %lld tiles", grid);
    return HND_ERR_INVALID;
  }
  hipLaunchKernelGGL(bx3t_kernel<MI>, dim3((unsigned)grid), dim3(256), 0, stream, d, a);
  return hnd::check_launch("hnd_conv2d_igemm(bx3 tiled)");
}

}  // namespace

namespace hnd {

// mi: bx3_build's 1 / 2 (a 64- / 128-row tile); this build takes everything bx3_applies admits.
int launch_bx3_tiled(const hnd_conv_desc& d, int mi, hipStream_t stream) {
  return mi == 1 ? launch_bx3t_t<1>(d, stream) : launch_bx3t_t<2>(d, stream);
}

}  // namespace hnd
