// include/hnd_entropy.h: the entropy-coded link payload of the bottleneck codec -- a canonical, length-limited Huffman code
// over the quantiser's codes in independently decodable chunks of 256 symbols.  The format is the header's; this file is
// the histogram, the three launches of the encoder and the one launch of the decoder.  Byte work and, in the decoder, the
// dequantise of csrc/quant_math.h, whose contract has the file built without FMA contraction.
// include/hnd_istream.h: the same format per image -- the histogram, the encoder and the decoder with the image as a grid row
// and every image's table read from device memory, on the wave and tile helpers of the kernels of hnd_entropy.h, and the one
// kernel that builds those tables from the histograms.
#include "common.h"
#include "hnd_entropy.h"
#include "hnd_istream.h"
#include "quant_math.h"

namespace {

constexpr int kChunk = 256;            // symbols per chunk
constexpr int kMaxLen = 12;            // longest code
constexpr int kChunkBytes = kChunk * kMaxLen / 8;      // 384: capacity of one chunk
constexpr long long kMaxNumel = 1ll << 30;
constexpr int kLut = 1 << kMaxLen;     // the decoder's table: the next 12 stream bits -> symbol | length << 8

// tables made on the host from the caller's code lengths; they reach the kernels by value
struct EncTable {
  uint16_t rev[256];                   // the code, bit-reversed in its length: the stream takes it least significant bit first
  uint8_t len[256];
};
struct DecTable {
  uint8_t sorted[256];                 // the symbols with a non-zero length, sorted by (length, symbol)
  uint16_t first[kMaxLen + 1];         // the code of the first symbol of every length
  uint16_t count[kMaxLen + 1];         // how many symbols have that length
  uint16_t base[kMaxLen + 1];          // where they begin in `sorted`
};

// ---- host: the table of the header, checked and turned into the two by-value forms
const char* canonical_tables(const uint8_t* lengths, int bits, EncTable* enc, DecTable* dec) {
  const int nsym = 1 << bits;
  unsigned kraft = 0;                  // in units of 2^-12
  int used = 0;
  DecTable d;
  memset(&d, 0, sizeof(d));
  for (int s = 0; s < nsym; ++s) {
    const int l = lengths[s];
    if (l > kMaxLen) return "a code length above 12";
    if (l) {
      kraft += 1u << (kMaxLen - l);
      ++used;
      ++d.count[l];
    }
  }
  if (!used) return "no non-zero code length";
  if (kraft > (1u << kMaxLen)) return "a Kraft sum above 1";
  unsigned code = 0, at = 0, next[kMaxLen + 1], slot[kMaxLen + 1];
  for (int l = 1; l <= kMaxLen; ++l) {
    d.first[l] = (uint16_t)code;
    d.base[l] = (uint16_t)at;
    next[l] = code;
    slot[l] = at;
    code = (code + d.count[l]) << 1;
    at += d.count[l];
  }
  if (enc) memset(enc, 0, sizeof(*enc));
  for (int s = 0; s < nsym; ++s) {
    const int l = lengths[s];
    if (!l) continue;
    const unsigned v = next[l]++;
    d.sorted[slot[l]++] = (uint8_t)s;
    if (enc) {
      unsigned r = 0;
      for (int b = 0; b < l; ++b) r |= ((v >> b) & 1u) << (l - 1 - b);
      enc->rev[s] = (uint16_t)r;
      enc->len[s] = (uint8_t)l;
    }
  }
  if (dec) *dec = d;
  return nullptr;
}

// ---- device
// the (at most four) symbols i0 ... i0 + 3 of the logical NCHW order, gathered from the NHWC bytes; returns how many exist
__device__ __forceinline__ int gather4(const uint8_t* __restrict__ q, unsigned i0, unsigned numel, unsigned hw, int c,
                                       int cs, unsigned sym[4]) {
  if (i0 >= numel) return 0;
  const int count = numel - i0 < 4u ? (int)(numel - i0) : 4;
  hnd::quant::NchwWalk<unsigned> at(i0, hw, c);
  for (int k = 0; k < count; ++k) {
    sym[k] = q[at.offset(cs)];
    at.next();
  }
  return count;
}

// 16 bytes of q per thread and step; each wave of the workgroup counts into an LDS histogram of its own
__global__ void __launch_bounds__(256) code_histogram_kernel(const uint8_t* __restrict__ q, unsigned long long total, int c,
                                                             int cs, unsigned nsym, unsigned* __restrict__ hist) {
  __shared__ unsigned cnt[4][256];
  for (int i = threadIdx.x; i < 4 * 256; i += 256) (&cnt[0][0])[i] = 0;
  __syncthreads();
  unsigned* mine = cnt[threadIdx.x >> 6];
  const unsigned long long nvec = total >> 4;
  for (unsigned long long v = blockIdx.x * 256ull + threadIdx.x; v < nvec; v += (unsigned long long)gridDim.x * 256ull) {
    const uint4 w = reinterpret_cast<const uint4*>(q)[v];
    const unsigned words[4] = {w.x, w.y, w.z, w.w};
    int ch = (int)((v << 4) % (unsigned)cs);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned code = (words[j >> 2] >> (8 * (j & 3))) & 255u;
      if (ch < c && code < nsym) atomicAdd(&mine[code], 1u);
      if (++ch == cs) ch = 0;
    }
  }
  if (blockIdx.x == 0) {                                            // the bytes after the last whole 16 (fewer than 16)
    const unsigned long long e = (nvec << 4) + threadIdx.x;
    if (threadIdx.x < 16 && e < total) {
      const unsigned code = q[e];
      if ((int)(e % (unsigned)cs) < c && code < nsym) atomicAdd(&mine[code], 1u);
    }
  }
  __syncthreads();
  const unsigned sum = cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
  if (sum) atomicAdd(&hist[threadIdx.x], sum);
}

// the byte count of the chunk whose symbols begin at `first` (one wave; every lane returns it); len: 256 code lengths in LDS
__device__ __forceinline__ unsigned wave_chunk_bytes(const uint8_t* __restrict__ q, unsigned first, unsigned numel, unsigned hw,
                                                     int c, int cs, const uint8_t* len, int lane) {
  unsigned sym[4], nb = 0;
  const int count = gather4(q, first + lane * 4u, numel, hw, c, cs, sym);
  for (int k = 0; k < count; ++k) nb += len[sym[k]];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nb += __shfl_xor(nb, o);
  return (nb + 7u) >> 3;
}

// launch 1 of the encoder: one wave per chunk, the chunk's byte count
__global__ void __launch_bounds__(256) chunk_bytes_kernel(const uint8_t* __restrict__ q, unsigned numel, unsigned hw, int c,
                                                          int cs, const EncTable tab, unsigned nchunks,
                                                          unsigned* __restrict__ sizes) {
  __shared__ uint8_t len[256];
  len[threadIdx.x] = tab.len[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (unsigned chunk = blockIdx.x * 4u + (threadIdx.x >> 6); chunk < nchunks; chunk += gridDim.x * 4u) {
    const unsigned nbytes = wave_chunk_bytes(q, chunk * (unsigned)kChunk, numel, hw, c, cs, len, lane);
    if (lane == 0) sizes[chunk] = nbytes;
  }
}

// launch 2: offsets = exclusive prefix sum of sizes, offsets[n] = the total.  ONE workgroup walks the array in tiles of 1024
// with a running carry: nothing waits on another workgroup.
__global__ void __launch_bounds__(1024) chunk_offsets_kernel(const unsigned* __restrict__ sizes, unsigned n,
                                                             unsigned* __restrict__ offsets) {
  __shared__ unsigned wsum[16];
  __shared__ unsigned carry_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (unsigned t0 = 0; t0 < n; t0 += 1024u) {
    const unsigned i = t0 + threadIdx.x;
    const unsigned v = i < n ? sizes[i] : 0u;
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned before = carry_s;
    for (int k = 0; k < wave; ++k) before += wsum[k];
    if (i < n) offsets[i] = before + incl - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets[n] = carry_s;
}

// launch 3: one wave per chunk.  A lane's four codes make one word of at most 48 bits; the lanes' bit counts meet in a wave
// prefix scan; the words are OR-ed into the wave's LDS staging buffer (zeroed first: the pad bits of the last byte stay 0)
// and the chunk's bytes leave lane by lane, byte i of the chunk from lane i % 64.
constexpr int kStage = kChunkBytes / 4 + 4;                         // 96 dwords and room for the shifted top of the last word

// the chunk whose symbols begin at `first`, coded to dst (one wave); code: 256 entries rev | len << 16 in LDS, st: the wave's
// staging buffer
__device__ __forceinline__ void wave_chunk_encode(const uint8_t* __restrict__ q, unsigned first, unsigned numel, unsigned hw,
                                                  int c, int cs, const unsigned* code, unsigned* st, int lane,
                                                  uint8_t* __restrict__ dst) {
  for (int i = lane; i < kStage; i += 64) st[i] = 0;
  unsigned sym[4], nb = 0;
  unsigned long long word = 0;
  const int count = gather4(q, first + lane * 4u, numel, hw, c, cs, sym);
  for (int k = 0; k < count; ++k) {
    const unsigned e = code[sym[k]];
    word |= (unsigned long long)(e & 0xFFFFu) << nb;
    nb += e >> 16;
  }
  unsigned incl = nb;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  const unsigned pos = incl - nb, nbytes = (__shfl(incl, 63) + 7u) >> 3;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");            // the zeros before the ORs (one wave: program order in LDS)
  if (nb) {
    const unsigned d = pos >> 5, sh = pos & 31u;
    const unsigned long long lo = word << sh;
    const unsigned hi = sh ? (unsigned)(word >> (64u - sh)) : 0u;
    if ((unsigned)lo) atomicOr(&st[d], (unsigned)lo);
    if ((unsigned)(lo >> 32)) atomicOr(&st[d + 1], (unsigned)(lo >> 32));
    if (hi) atomicOr(&st[d + 2], hi);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  for (unsigned i = lane; i < nbytes; i += 64) dst[i] = (uint8_t)(st[i >> 2] >> (8 * (i & 3)));
}

__global__ void __launch_bounds__(256) chunk_encode_kernel(const uint8_t* __restrict__ q, unsigned numel, unsigned hw, int c,
                                                           int cs, const EncTable tab, unsigned nchunks,
                                                           const unsigned* __restrict__ offsets,
                                                           uint8_t* __restrict__ payload) {
  __shared__ unsigned code[256];                                    // rev | len << 16
  __shared__ unsigned stage[4][kStage];
  code[threadIdx.x] = (unsigned)tab.rev[threadIdx.x] | ((unsigned)tab.len[threadIdx.x] << 16);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (unsigned chunk = blockIdx.x * 4u + wave; chunk < nchunks; chunk += gridDim.x * 4u)
    wave_chunk_encode(q, chunk * (unsigned)kChunk, numel, hw, c, cs, code, stage[wave], lane, payload + offsets[chunk]);
}

// dword `dw` of the payload; a byte at or beyond nbytes reads as 0 and is not touched
__device__ __forceinline__ unsigned payload_dword(const uint8_t* __restrict__ p, unsigned dw, unsigned nbytes) {
  if (dw < (nbytes >> 2)) return reinterpret_cast<const unsigned*>(p)[dw];
  unsigned v = 0;
  if (dw == (nbytes >> 2))
    for (unsigned b = 0; b < (nbytes & 3u); ++b) v |= (unsigned)p[dw * 4u + b] << (8 * b);
  return v;
}

constexpr int kTilePix = 2048;                         // pixels of one image per workgroup
constexpr int kTileChunks = kTilePix / kChunk + 1;     // 9: chunks one channel's 2048 symbols can overlap
constexpr int kGroup = 16;                             // channels decoded and stored together
constexpr int kSlotDwords = kChunk / 4 + 1;            // 65: a chunk's symbols, one byte each, and a dword of bank padding

// the 4096-entry table: canonical decoding of every 12-bit window.  Table: DecTable (by value) or its twin in LDS
template <typename Table>
__device__ __forceinline__ void fill_lut(const Table& tab, uint16_t* lut) {
  for (unsigned e = threadIdx.x; e < (unsigned)kLut; e += 256) {
    unsigned entry = kMaxLen << 8, v = 0;                           // no code begins here (a table with Kraft < 1): symbol 0
    for (int l = 1; l <= kMaxLen; ++l) {
      v = (v << 1) | ((e >> (l - 1)) & 1u);                         // the first l stream bits, most significant code bit first
      const unsigned d = v - tab.first[l];
      if (v >= tab.first[l] && d < tab.count[l]) {
        entry = (unsigned)tab.sorted[tab.base[l] + d] | ((unsigned)l << 8);
        break;
      }
    }
    lut[e] = (uint16_t)entry;
  }
}

// the tile of pixels p0 ... of image `img` (a whole workgroup; lut may still be in the making: the first barrier is here).
// The image's symbols are those of image `simg` of the stream whose chunk 0 has the global index `chunk0`: (img, 0) for the
// one stream of a batch, (0, img * cpi) for per-image streams.
__device__ __forceinline__ void decode_tile(const uint8_t* __restrict__ payload, unsigned payload_bytes,
                                            const unsigned* __restrict__ offsets, const uint16_t* lut, unsigned* stage,
                                            float scale, float zp, float* __restrict__ x, unsigned img, unsigned simg,
                                            unsigned chunk0, unsigned p0, unsigned hw, int c, int cs) {
  const unsigned npx = hw - p0 < (unsigned)kTilePix ? hw - p0 : (unsigned)kTilePix;
  for (int g0 = 0; g0 < c; g0 += kGroup) {
    const int gc = c - g0 < kGroup ? c - g0 : kGroup;
    __syncthreads();                                                // the table is built; the staging buffer is free again
    if ((int)threadIdx.x < gc * kTileChunks) {
      const int chg = threadIdx.x / kTileChunks, k = threadIdx.x - chg * kTileChunks;
      const unsigned s0 = (simg * (unsigned)c + g0 + chg) * hw + p0; // first symbol of this channel in the tile (< 2^30)
      const unsigned chunk = (s0 >> 8) + k;
      if (chunk <= ((s0 + npx - 1u) >> 8)) {                        // the chunk overlaps the tile, so it exists
        const unsigned o0 = offsets[chunk0 + chunk];
        unsigned dw = o0 >> 2;
        unsigned long long buf = payload_dword(payload, dw++, payload_bytes) >> (8 * (o0 & 3u));
        int have = 32 - 8 * (int)(o0 & 3u);
        unsigned* slot = stage + threadIdx.x * kSlotDwords;
        for (int j = 0; j < kChunk / 4; ++j) {                      // always 256 symbols: past a short chunk's end they are
          unsigned packed = 0;                                      // whatever zeros decode to, and nobody reads them
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            if (have < kMaxLen) {
              buf |= (unsigned long long)payload_dword(payload, dw++, payload_bytes) << have;
              have += 32;
            }
            const unsigned e = lut[(unsigned)buf & (kLut - 1)];
            packed |= (e & 255u) << (8 * b);
            buf >>= e >> 8;
            have -= (int)(e >> 8);
          }
          slot[j] = packed;
        }
      }
    }
    __syncthreads();
    const int gend = g0 + kGroup >= c ? cs : g0 + kGroup;           // the last group also clears the pad channels
    const unsigned nq = (unsigned)(gend - g0) >> 2;
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(stage);
    for (unsigned idx = threadIdx.x; idx < npx * nq; idx += 256) {
      const unsigned pix = idx / nq, qd = idx - pix * nq;
      float out[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = g0 + (int)qd * 4 + e;
        out[e] = 0.f;
        if (ch < c) {
          const unsigned s0 = (simg * (unsigned)c + ch) * hw + p0, s = s0 + pix;
          const unsigned slot = (unsigned)(ch - g0) * kTileChunks + ((s >> 8) - (s0 >> 8));
          out[e] = hnd::quant::dequantize_one((float)sb[slot * (kSlotDwords * 4) + (s & 255u)], scale, zp);
        }
      }
      float4 v4 = make_float4(out[0], out[1], out[2], out[3]);
      *reinterpret_cast<float4*>(x + ((unsigned long long)img * hw + p0 + pix) * cs + g0 + qd * 4u) = v4;
    }
  }
}

__global__ void __launch_bounds__(256) decode_dequantize_kernel(const uint8_t* __restrict__ payload, unsigned payload_bytes,
                                                                const unsigned* __restrict__ offsets, const DecTable tab,
                                                                const float* __restrict__ qp, float* __restrict__ x,
                                                                unsigned hw, int c, int cs, unsigned tiles) {
  __shared__ uint16_t lut[kLut];
  __shared__ unsigned stage[kGroup * kTileChunks * kSlotDwords];
  fill_lut(tab, lut);
  const unsigned img = blockIdx.x / tiles, p0 = (blockIdx.x - img * tiles) * (unsigned)kTilePix;
  decode_tile(payload, payload_bytes, offsets, lut, stage, qp[2], qp[3], x, img, img, 0u, p0, hw, c, cs);
}

// ---- include/hnd_istream.h: one stream, one table and one (scale, zero point) per image.  The image is blockIdx.y (the
// decoder's tiles carry it in blockIdx.x, as above); the wave and tile work is that of the kernels above.
constexpr int kMaxImages = HND_ISTREAM_MAX_N;

// the canonical tables of one image, made in LDS by its workgroup from the image's row of device code lengths
struct LdsTable {
  uint8_t len[256];                    // min(length, 12); 0 at and beyond 2^bits
  uint8_t sorted[256];                 // as DecTable
  uint16_t code[256];                  // the symbol's code
  uint16_t first[kMaxLen + 1], count[kMaxLen + 1], base[kMaxLen + 1];
};

// 256 threads.  Nothing here is validated and nothing needs to be: a length is at most 12, the counts sum to at most 256, so
// base[l] + rank < 256 for every symbol; a table whose Kraft sum exceeds 1 gives codes that are not prefix-free (and `first`
// cut to 16 bits), which changes the bytes of the stream and no address.
__device__ __forceinline__ void build_lds_table(const uint8_t* __restrict__ lengths, unsigned nsym, LdsTable& t) {
  const unsigned s = threadIdx.x;
  const unsigned mine = s < nsym ? lengths[s] : 0u;
  t.len[s] = (uint8_t)(mine < (unsigned)kMaxLen ? mine : (unsigned)kMaxLen);
  __syncthreads();
  if (s >= 1 && s <= (unsigned)kMaxLen) {
    unsigned n = 0;
    for (int k = 0; k < 256; ++k) n += t.len[k] == s;
    t.count[s] = (uint16_t)n;
  }
  __syncthreads();
  if (s == 0) {
    unsigned code = 0, at = 0;
    for (int l = 1; l <= kMaxLen; ++l) {
      t.first[l] = (uint16_t)code;
      t.base[l] = (uint16_t)at;
      code = (code + t.count[l]) << 1;
      at += t.count[l];
    }
  }
  __syncthreads();
  const unsigned l = t.len[s];
  unsigned rank = 0;                                                // among the symbols of this length: those before s
  for (unsigned k = 0; k < s; ++k) rank += t.len[k] == l;
  t.code[s] = l ? (uint16_t)(t.first[l] + rank) : (uint16_t)0;
  if (l) t.sorted[t.base[l] + rank] = (uint8_t)s;
  __syncthreads();
}

// hist[img]: grid (workgroups per image, n).  The image's bytes [b0, b1) of q begin at any multiple of 4: the 16-byte
// vectors that lie wholly inside it are loaded as vectors, the bytes before the first and after the last one (fewer than
// 16 each; fewer than 32 in all when the image holds no whole vector) one per thread by the image's first workgroup.
__global__ void __launch_bounds__(256) image_histogram_kernel(const uint8_t* __restrict__ q, unsigned long long image_bytes,
                                                              int c, int cs, unsigned nsym, unsigned* __restrict__ hist) {
  __shared__ unsigned cnt[4][256];
  for (int i = threadIdx.x; i < 4 * 256; i += 256) (&cnt[0][0])[i] = 0;
  __syncthreads();
  unsigned* mine = cnt[threadIdx.x >> 6];
  const unsigned long long b0 = blockIdx.y * image_bytes, b1 = b0 + image_bytes;
  unsigned long long v0 = (b0 + 15ull) >> 4, v1 = b1 >> 4;          // whole vectors [v0, v1) of q
  if (v0 >= v1) v0 = v1 = (b1 + 15ull) >> 4;                        // none: every byte is a head byte (v0 * 16 >= b1)
  for (unsigned long long v = v0 + blockIdx.x * 256ull + threadIdx.x; v < v1; v += (unsigned long long)gridDim.x * 256ull) {
    const uint4 w = reinterpret_cast<const uint4*>(q)[v];
    const unsigned words[4] = {w.x, w.y, w.z, w.w};
    int ch = (int)(((v << 4) - b0) % (unsigned)cs);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned code = (words[j >> 2] >> (8 * (j & 3))) & 255u;
      if (ch < c && code < nsym) atomicAdd(&mine[code], 1u);
      if (++ch == cs) ch = 0;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {                        // threads 0 ... 31: the head, 32 ... 63: the tail
    const bool tail = threadIdx.x >= 32;
    const unsigned long long lo = tail ? v1 << 4 : b0, hi = tail ? b1 : (v0 << 4 < b1 ? v0 << 4 : b1);
    const unsigned long long e = lo + (threadIdx.x & 31u);
    if (e < hi) {
      const unsigned code = q[e];
      if ((int)((e - b0) % (unsigned)cs) < c && code < nsym) atomicAdd(&mine[code], 1u);
    }
  }
  __syncthreads();
  const unsigned sum = cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
  if (sum) atomicAdd(&hist[blockIdx.y * 256u + threadIdx.x], sum);
}

// how many of the ascending a[0 ... n) are < key (or_equal: <= key)
template <typename T>
__device__ __forceinline__ unsigned count_below(const T* a, unsigned n, T key, bool or_equal) {
  unsigned lo = 0, hi = n;
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    if (a[mid] < key || (or_equal && a[mid] == key)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// lengths[img] from hist[img]: length-limited Huffman by package-merge, one workgroup per image -- the host's
// transformer.huffman_lengths without its symbol sets.  The occurring symbols, ranked by (count, symbol), are the leaves and
// level 1.  Level j + 1 is the merge, by weight, of the leaves with the packages of level j (its items paired in order, an
// odd last one dropped), a leaf before a package of equal weight: thread t places leaf t and package t by binary searches in
// the other list, and the place of every leaf in every level is kept (12 x 256 x uint16).  The walk back: the first
// k = 2 m - 2 items of level 12 are taken; a_j of the first k items of level j are leaves -- those of rank < a_j, each one
// bit longer for it -- and the other k - a_j are packages, the first 2 (k - a_j) items of level j - 1.  With the same leaf
// order and the same tie rule the merged lists are the host's, so the lengths are.  Weights are 64-bit: an item of level j
// holds a leaf at most once per level below it, so the bound is about 12 * 2^30.  The host routine falls back to the flat
// code should package-merge ever cost more than it; with a limit of 12 >= bits the flat code is one of the candidates of an
// optimal method, so that branch cannot be taken and does not exist here.
__global__ void __launch_bounds__(256) build_tables_kernel(const unsigned* __restrict__ hist, unsigned nsym,
                                                           uint8_t* __restrict__ lengths) {
  __shared__ unsigned cnt[256];
  __shared__ unsigned long long leaf[256], pack[256], list[512];
  __shared__ uint16_t place[kMaxLen][256];                          // place[j - 1][r]: where leaf r stands in level j
  __shared__ uint8_t rank_sym[256], out[256];
  __shared__ unsigned m_s;
  const unsigned t = threadIdx.x;
  const unsigned mine = t < nsym ? hist[blockIdx.x * 256u + t] : 0u;
  cnt[t] = mine;
  out[t] = 0;
  if (t == 0) m_s = 0;
  __syncthreads();
  unsigned rank = 0;
  for (unsigned k = 0; k < 256; ++k) {
    const unsigned o = cnt[k];
    rank += o && (o < mine || (o == mine && k < t));
  }
  if (mine) {
    leaf[rank] = mine;
    list[rank] = mine;
    rank_sym[rank] = (uint8_t)t;
    place[0][rank] = (uint16_t)rank;
    atomicAdd(&m_s, 1u);
  }
  __syncthreads();
  const unsigned m = m_s;
  unsigned len = m == 1 ? 1u : 0u;                                  // of the leaf of rank t
  if (m > 1) {
    unsigned n = m;                                                 // items of the newest level
    for (int j = 1; j < kMaxLen; ++j) {
      const unsigned p = n >> 1;
      if (t < p) pack[t] = list[2 * t] + list[2 * t + 1];
      __syncthreads();
      if (t < m) {
        const unsigned at = t + count_below(pack, p, leaf[t], false);
        place[j][t] = (uint16_t)at;
        list[at] = leaf[t];
      }
      if (t < p) list[t + count_below(leaf, m, pack[t], true)] = pack[t];
      n = m + p;
      __syncthreads();
    }
    unsigned k = 2 * m - 2 < n ? 2 * m - 2 : n;
    for (int j = kMaxLen - 1; j >= 0; --j) {                        // every thread walks back on its own: reads only
      const unsigned a = count_below(place[j], m, (uint16_t)k, false);
      len += t < a;
      k = 2 * (k - a);
    }
  }
  if (t < m) out[rank_sym[t]] = (uint8_t)len;
  __syncthreads();
  lengths[blockIdx.x * 256u + t] = out[t];
}

// the three kernels of the encoder and the decoder with the image as a grid row and its table from lengths[img]
__global__ void __launch_bounds__(256) image_chunk_bytes_kernel(const uint8_t* __restrict__ q, unsigned chw, unsigned hw, int c,
                                                                int cs, unsigned nsym, const uint8_t* __restrict__ lengths,
                                                                unsigned cpi, unsigned* __restrict__ sizes) {
  __shared__ uint8_t len[256];
  const unsigned img = blockIdx.y;
  const unsigned l = threadIdx.x < nsym ? lengths[img * 256u + threadIdx.x] : 0u;
  len[threadIdx.x] = (uint8_t)(l < (unsigned)kMaxLen ? l : (unsigned)kMaxLen);
  __syncthreads();
  const uint8_t* qi = q + (unsigned long long)img * hw * cs;
  const int lane = threadIdx.x & 63;
  for (unsigned chunk = blockIdx.x * 4u + (threadIdx.x >> 6); chunk < cpi; chunk += gridDim.x * 4u) {
    const unsigned nbytes = wave_chunk_bytes(qi, chunk * (unsigned)kChunk, chw, hw, c, cs, len, lane);
    if (lane == 0) sizes[img * cpi + chunk] = nbytes;
  }
}

__global__ void __launch_bounds__(256) image_chunk_encode_kernel(const uint8_t* __restrict__ q, unsigned chw, unsigned hw, int c,
                                                                 int cs, unsigned nsym, const uint8_t* __restrict__ lengths,
                                                                 unsigned cpi, const unsigned* __restrict__ offsets,
                                                                 uint8_t* __restrict__ payload) {
  __shared__ LdsTable tab;
  __shared__ unsigned code[256];                                    // rev | len << 16
  __shared__ unsigned stage[4][kStage];
  const unsigned img = blockIdx.y;
  build_lds_table(lengths + img * 256u, nsym, tab);
  {
    const unsigned l = tab.len[threadIdx.x], v = tab.code[threadIdx.x];
    unsigned r = 0;
    for (unsigned b = 0; b < l; ++b) r |= ((v >> b) & 1u) << (l - 1 - b);
    code[threadIdx.x] = r | (l << 16);
  }
  __syncthreads();
  const uint8_t* qi = q + (unsigned long long)img * hw * cs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (unsigned chunk = blockIdx.x * 4u + wave; chunk < cpi; chunk += gridDim.x * 4u)
    wave_chunk_encode(qi, chunk * (unsigned)kChunk, chw, hw, c, cs, code, stage[wave], lane,
                      payload + offsets[img * cpi + chunk]);
}

__global__ void __launch_bounds__(256) image_decode_dequantize_kernel(const uint8_t* __restrict__ payload,
                                                                      unsigned payload_bytes,
                                                                      const unsigned* __restrict__ offsets,
                                                                      const uint8_t* __restrict__ lengths, unsigned nsym,
                                                                      const float* __restrict__ qp, float* __restrict__ x,
                                                                      unsigned hw, int c, int cs, unsigned tiles,
                                                                      unsigned cpi) {
  __shared__ LdsTable tab;
  __shared__ uint16_t lut[kLut];
  __shared__ unsigned stage[kGroup * kTileChunks * kSlotDwords];
  const unsigned img = blockIdx.x / tiles, p0 = (blockIdx.x - img * tiles) * (unsigned)kTilePix;
  build_lds_table(lengths + img * 256u, nsym, tab);
  fill_lut(tab, lut);
  decode_tile(payload, payload_bytes, offsets, lut, stage, qp[img * 4u + 2], qp[img * 4u + 3], x, img, 0u, img * cpi, p0, hw,
              c, cs);
}

inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
}

inline bool good_geometry(int n, int h, int w, int c, int cs) {
  return n > 0 && h > 0 && w > 0 && c > 0 && cs >= c && cs % 4 == 0 && (long long)n * c <= kMaxNumel &&
         (long long)h * w <= kMaxNumel && (long long)n * c * ((long long)h * w) <= kMaxNumel;
}

}  // namespace

extern "C" {

int hnd_entropy_abi(void) { return HND_ENTROPY_ABI; }

int64_t hnd_entropy_chunks(int64_t numel) {
  return numel <= 0 || numel > kMaxNumel ? 0 : (numel + kChunk - 1) / kChunk;
}

size_t hnd_entropy_capacity(int64_t numel) { return (size_t)hnd_entropy_chunks(numel) * kChunkBytes; }

size_t hnd_entropy_scratch_bytes(int64_t numel) { return (size_t)hnd_entropy_chunks(numel) * sizeof(uint32_t); }

int hnd_code_histogram(const uint8_t* q, int n, int h, int w, int c, int cs, int bits, void* hist, void* stream) {
  HND_REQUIRE(q && hist, "hnd_code_histogram: null pointer");
  HND_REQUIRE(bits >= 1 && bits <= 8, "hnd_code_histogram: bits %d outside 1 ... 8", bits);
  HND_REQUIRE(good_geometry(n, h, w, c, cs),
              "hnd_code_histogram: bad geometry (n, h, w, c > 0, cs >= c, cs %% 4 == 0, n * c * h * w <= 2^30)");
  HND_REQUIRE(aligned16(q, hist), "hnd_code_histogram: q and hist must be 16-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  const unsigned long long total = (unsigned long long)n * h * w * cs;
  if (hipMemsetAsync(hist, 0, 256 * sizeof(uint32_t), s) != hipSuccess) return hnd::check_launch("hnd_code_histogram");
  unsigned long long blocks = ((total >> 4) + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
  hipLaunchKernelGGL(code_histogram_kernel, dim3((unsigned)blocks), dim3(256), 0, s, q, total, c, cs, 1u << bits,
                     (unsigned*)hist);
  return hnd::check_launch("hnd_code_histogram");
}

int hnd_entropy_encode(const uint8_t* q, int n, int h, int w, int c, int cs, int bits, const uint8_t* lengths_host,
                       uint8_t* payload, void* offsets, void* scratch, void* stream) {
  HND_REQUIRE(q && lengths_host && payload && offsets && scratch, "hnd_entropy_encode: null pointer");
  HND_REQUIRE(bits >= 1 && bits <= 8, "hnd_entropy_encode: bits %d outside 1 ... 8", bits);
  HND_REQUIRE(good_geometry(n, h, w, c, cs),
              "hnd_entropy_encode: bad geometry (n, h, w, c > 0, cs >= c, cs %% 4 == 0, n * c * h * w <= 2^30)");
  HND_REQUIRE(aligned16(q, payload, offsets) && aligned16(scratch),
              "hnd_entropy_encode: q, payload, offsets and scratch must be 16-byte aligned");
  EncTable tab;
  const char* bad = canonical_tables(lengths_host, bits, &tab, nullptr);
  HND_REQUIRE(!bad, "hnd_entropy_encode: bad table of code lengths: %s", bad);
  hipStream_t s = hnd::as_stream(stream);
  const unsigned hw = (unsigned)h * w, numel = (unsigned)n * c * hw, nchunks = (numel + kChunk - 1) / kChunk;
  unsigned blocks = (nchunks + 3) / 4;
  blocks = blocks > 2048 ? 2048 : blocks;
  hipLaunchKernelGGL(chunk_bytes_kernel, dim3(blocks), dim3(256), 0, s, q, numel, hw, c, cs, tab, nchunks, (unsigned*)scratch);
  hipLaunchKernelGGL(chunk_offsets_kernel, dim3(1), dim3(1024), 0, s, (const unsigned*)scratch, nchunks, (unsigned*)offsets);
  hipLaunchKernelGGL(chunk_encode_kernel, dim3(blocks), dim3(256), 0, s, q, numel, hw, c, cs, tab, nchunks,
                     (const unsigned*)offsets, payload);
  return hnd::check_launch("hnd_entropy_encode");
}

int hnd_entropy_decode_dequantize(const uint8_t* payload, int64_t payload_bytes, const void* offsets,
                                  const uint8_t* lengths_host, const float* qparams, float* x, int n, int h, int w, int c,
                                  int cs, int bits, void* stream) {
  HND_REQUIRE(payload && offsets && lengths_host && qparams && x, "hnd_entropy_decode_dequantize: null pointer");
  HND_REQUIRE(bits >= 1 && bits <= 8, "hnd_entropy_decode_dequantize: bits %d outside 1 ... 8", bits);
  HND_REQUIRE(good_geometry(n, h, w, c, cs),
              "hnd_entropy_decode_dequantize: bad geometry (n, h, w, c > 0, cs >= c, cs %% 4 == 0, n * c * h * w <= 2^30)");
  HND_REQUIRE(payload_bytes > 0 && payload_bytes <= (int64_t)kMaxNumel / kChunk * kChunkBytes,
              "hnd_entropy_decode_dequantize: payload_bytes %lld outside 1 ... the capacity of 2^30 values",
              (long long)payload_bytes);
  HND_REQUIRE(aligned16(payload, offsets, qparams) && aligned16(x),
              "hnd_entropy_decode_dequantize: payload, offsets, qparams and x must be 16-byte aligned");
  DecTable tab;
  const char* bad = canonical_tables(lengths_host, bits, nullptr, &tab);
  HND_REQUIRE(!bad, "hnd_entropy_decode_dequantize: bad table of code lengths: %s", bad);
  const unsigned hw = (unsigned)h * w, tiles = (hw + kTilePix - 1) / kTilePix;
  hipLaunchKernelGGL(decode_dequantize_kernel, dim3((unsigned)n * tiles), dim3(256), 0, hnd::as_stream(stream), payload,
                     (unsigned)payload_bytes, (const unsigned*)offsets, tab, qparams, x, hw, c, cs, tiles);
  return hnd::check_launch("hnd_entropy_decode_dequantize");
}

// ---- include/hnd_istream.h
int hnd_istream_abi(void) { return HND_ISTREAM_ABI; }

int64_t hnd_istream_chunks_per_image(int64_t chw) { return hnd_entropy_chunks(chw); }

size_t hnd_istream_capacity(int n, int64_t chw) { return hnd_istream_scratch_bytes(n, chw) / sizeof(uint32_t) * kChunkBytes; }

size_t hnd_istream_scratch_bytes(int n, int64_t chw) {
  if (n < 1 || n > kMaxImages || chw < 1 || chw > kMaxNumel / n) return 0;
  return (size_t)n * (size_t)hnd_entropy_chunks(chw) * sizeof(uint32_t);
}

int hnd_istream_histogram(const uint8_t* q, int n, int h, int w, int c, int cs, int bits, void* hist, void* stream) {
  HND_REQUIRE(q && hist, "hnd_istream_histogram: null pointer");
  HND_REQUIRE(bits >= 1 && bits <= 8, "hnd_istream_histogram: bits %d outside 1 ... 8", bits);
  HND_REQUIRE(good_geometry(n, h, w, c, cs) && n <= kMaxImages,
              "hnd_istream_histogram: bad geometry (n, h, w, c > 0, n <= %d, cs >= c, cs %% 4 == 0, n * c * h * w <= 2^30)",
              kMaxImages);
  HND_REQUIRE(aligned16(q, hist), "hnd_istream_histogram: q and hist must be 16-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  const unsigned long long image_bytes = (unsigned long long)h * w * cs;
  if (hipMemsetAsync(hist, 0, (size_t)n * 256 * sizeof(uint32_t), s) != hipSuccess)
    return hnd::check_launch("hnd_istream_histogram");
  unsigned long long blocks = ((image_bytes >> 4) + 255) / 256, most = 4096ull / n;
  most = most < 1 ? 1 : most;
  blocks = blocks < 1 ? 1 : (blocks > most ? most : blocks);
  hipLaunchKernelGGL(image_histogram_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, s, q, image_bytes, c, cs,
                     1u << bits, (unsigned*)hist);
  return hnd::check_launch("hnd_istream_histogram");
}

int hnd_istream_build_tables(const void* hist, int n, int bits, uint8_t* lengths, void* stream) {
  HND_REQUIRE(hist && lengths, "hnd_istream_build_tables: null pointer");
  HND_REQUIRE(bits >= 1 && bits <= 8, "hnd_istream_build_tables: bits %d outside 1 ... 8", bits);
  HND_REQUIRE(n >= 1 && n <= kMaxImages, "hnd_istream_build_tables: n %d outside 1 ... %d", n, kMaxImages);
  HND_REQUIRE(aligned16(hist), "hnd_istream_build_tables: hist must be 16-byte aligned");
  hipLaunchKernelGGL(build_tables_kernel, dim3((unsigned)n), dim3(256), 0, hnd::as_stream(stream), (const unsigned*)hist,
                     1u << bits, lengths);
  return hnd::check_launch("hnd_istream_build_tables");
}

int hnd_istream_encode(const uint8_t* q, int n, int h, int w, int c, int cs, int bits, const uint8_t* lengths,
                       uint8_t* payload, void* offsets, void* scratch, void* stream) {
  HND_REQUIRE(q && lengths && payload && offsets && scratch, "hnd_istream_encode: null pointer");
  HND_REQUIRE(bits >= 1 && bits <= 8, "hnd_istream_encode: bits %d outside 1 ... 8", bits);
  HND_REQUIRE(good_geometry(n, h, w, c, cs) && n <= kMaxImages,
              "hnd_istream_encode: bad geometry (n, h, w, c > 0, n <= %d, cs >= c, cs %% 4 == 0, n * c * h * w <= 2^30)",
              kMaxImages);
  HND_REQUIRE(aligned16(q, payload, offsets) && aligned16(scratch),
              "hnd_istream_encode: q, payload, offsets and scratch must be 16-byte aligned");
  hipStream_t s = hnd::as_stream(stream);
  const unsigned hw = (unsigned)h * w, chw = (unsigned)c * hw, cpi = (chw + kChunk - 1) / kChunk;
  unsigned blocks = (cpi + 3) / 4, most = 1024u / n;                // every workgroup builds its image's table first: few, long ones
  most = most < 1 ? 1 : most;
  blocks = blocks > most ? most : blocks;
  const dim3 grid(blocks, (unsigned)n);
  hipLaunchKernelGGL(image_chunk_bytes_kernel, grid, dim3(256), 0, s, q, chw, hw, c, cs, 1u << bits, lengths, cpi,
                     (unsigned*)scratch);
  hipLaunchKernelGGL(chunk_offsets_kernel, dim3(1), dim3(1024), 0, s, (const unsigned*)scratch, (unsigned)n * cpi,
                     (unsigned*)offsets);
  hipLaunchKernelGGL(image_chunk_encode_kernel, grid, dim3(256), 0, s, q, chw, hw, c, cs, 1u << bits, lengths, cpi,
                     (const unsigned*)offsets, payload);
  return hnd::check_launch("hnd_istream_encode");
}

int hnd_istream_decode_dequantize(const uint8_t* payload, int64_t payload_bytes, const void* offsets,
                                  const uint8_t* lengths, const float* qparams, float* x, int n, int h, int w, int c,
                                  int cs, int bits, void* stream) {
  HND_REQUIRE(payload && offsets && lengths && qparams && x, "hnd_istream_decode_dequantize: null pointer");
  HND_REQUIRE(bits >= 1 && bits <= 8, "hnd_istream_decode_dequantize: bits %d outside 1 ... 8", bits);
  HND_REQUIRE(good_geometry(n, h, w, c, cs) && n <= kMaxImages,
              "hnd_istream_decode_dequantize: bad geometry (n, h, w, c > 0, n <= %d, cs >= c, cs %% 4 == 0, "
              "n * c * h * w <= 2^30)", kMaxImages);
  // the largest call: n images of 2^30 / n values each make at most 2^22 + n chunks, so every offset fits 32 bits
  HND_REQUIRE(payload_bytes > 0 && payload_bytes <= ((int64_t)kMaxNumel / kChunk + kMaxImages) * kChunkBytes,
              "hnd_istream_decode_dequantize: payload_bytes %lld outside 1 ... the capacity of the largest call",
              (long long)payload_bytes);
  HND_REQUIRE(aligned16(payload, offsets, qparams) && aligned16(x),
              "hnd_istream_decode_dequantize: payload, offsets, qparams and x must be 16-byte aligned");
  const unsigned hw = (unsigned)h * w, tiles = (hw + kTilePix - 1) / kTilePix;
  const unsigned cpi = ((unsigned)c * hw + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(image_decode_dequantize_kernel, dim3((unsigned)n * tiles), dim3(256), 0, hnd::as_stream(stream), payload,
                     (unsigned)payload_bytes, (const unsigned*)offsets, lengths, 1u << bits, qparams, x, hw, c, cs, tiles, cpi);
  return hnd::check_launch("hnd_istream_decode_dequantize");
}

}  // extern "C"
