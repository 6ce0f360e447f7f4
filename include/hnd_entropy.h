/*
 * hnd_entropy.h -- an entropy-coded link payload for the bottleneck codec of libhnd_hip.so: a canonical, length-limited
 * Huffman code over the 2^bits quantiser codes, cut into independently decodable chunks so that both directions are data
 * parallel with no communication between workgroups.  hnd_codec.h ships exactly `bits` bits per value whatever the values
 * are; this header is the opt-in alternative for tensors whose codes are far from uniform.  Lossless: the decoder returns
 * the bits hnd_unpack_dequantize_bits returns.  An extension: the reference pickles one byte per value.
 *
 * A header of its own with a version of its own: hnd_hip.h, hnd_optim.h, hnd_codec.h, hnd_qat.h, hnd_qrange.h and their
 * versions are unchanged by it.  It declares functions only.  The conventions are those of hnd_codec.h: device pointers
 * into caller-owned buffers, `stream` is a hipStream_t passed as void*, 0 on success and a negative hnd_status otherwise,
 * hnd_last_error_string() explains.  No export synchronises with the host.
 *
 * FORMAT.
 * Symbols.  The quantised values of the LOGICAL NCHW tensor [n, c, h, w], real channels only, in index order
 *   i = ((img * c + ch) * h + y) * w + x -- the order of the packed payload of hnd_codec.h.
 * Code lengths.  `lengths` is 2^bits bytes, lengths[s] in 0 ... 12, 0 meaning symbol s does not occur.  At least one
 *   length is non-zero and the Kraft sum, sum over s of 2^(-lengths[s]), is <= 1.  A tensor with one occurring symbol gives
 *   that symbol length 1.
 * Canonical assignment.  The symbols with a non-zero length are sorted by (length, symbol); the first gets code 0 and
 *   each next one (code + 1) << (len_next - len_cur).
 * Bit stream.  Bit k of the stream is bit k % 8 of byte k / 8, as in the packed payload.  A code of length L and value v
 *   enters the stream most significant code bit first: stream bits t ... t + L - 1 are bits L - 1 ... 0 of v.
 * Chunks.  A chunk is 256 consecutive symbols; the last may be shorter; nchunks = ceil(numel / 256).  Every chunk starts on
 *   a byte boundary and the pad bits of its last byte are 0.  `offsets` is uint32[nchunks + 1], the byte offsets of the
 *   chunks in `payload`: offsets[0] = 0, offsets[nchunks] is the stream's total byte count.  `payload` has a capacity of
 *   hnd_entropy_capacity(numel) = nchunks * 384 bytes (256 symbols of 12 bits); bytes at and beyond offsets[nchunks] are
 *   not written.
 * What crosses the link: payload[0 : offsets[nchunks]], offsets, lengths, and scale and zero point from qparams:
 *   link_bytes = offsets[nchunks] + 4 * (nchunks + 1) + 2^bits + 8.
 *
 * Buffers.  q is the one-value-per-byte uint8 NHWC tensor the quantisers of hnd_codec.h / hnd_qrange.h write, pixel stride
 * `cs` bytes of which the first `c` are real channels.  x is the fp32 NHWC bottleneck buffer of the same geometry.  qparams
 * is device float[4] = {min, max, scale, zero_point}.  The 32-bit buffers are declared void*: hist is uint32_t[256], offsets
 * is uint32_t[nchunks + 1], scratch is hnd_entropy_scratch_bytes(numel) bytes (uint32_t[nchunks]: the byte count of every
 * chunk).  lengths_host is a HOST pointer to 2^bits bytes; the tables made from it travel to the kernels by value.
 *
 * hnd_code_histogram.  Counts the codes of the real channels of q into hist, which this call zeroes (a memset node) and
 * fills in ONE launch: 16-byte loads of q, counters in LDS, one flush of at most 256 global atomics per workgroup.  A byte
 * of q at or above 2^bits is counted nowhere, so the entries of hist at and above 2^bits are 0.
 *
 * hnd_entropy_encode.  THREE launches: the byte count of every chunk into scratch (one wave per chunk), their exclusive
 * prefix sum into offsets (ONE workgroup, no look-back), the stream (one wave per chunk: four symbols per lane, a wave
 * prefix scan of the lanes' bit counts, the bits OR-ed into an LDS staging buffer, the chunk's bytes stored lane by lane).
 * A symbol whose length is 0, and a byte of q at or above 2^bits, emits no bits.
 *
 * hnd_entropy_decode_dequantize.  ONE launch.  Writes scale * (q - zero_point) -- one fp32 subtraction, one fp32
 * multiplication, no FMA contraction: the bits of hnd_unpack_dequantize_bits -- into every real channel of x and 0 into
 * every pad channel, all n * h * w * cs floats.  A workgroup owns a tile of 2048 pixels of one image: it builds the
 * 4096-entry table "next 12 stream bits -> symbol, length" in LDS, one thread decodes each chunk that overlaps the tile
 * (so a chunk on a tile's edge is decoded by two workgroups), the symbols are staged in LDS, and the tile is stored as
 * 16-byte groups of four channels.  Every read of payload is inside [0, payload_bytes) (a position beyond it reads as 0)
 * and every write position comes from the tile and chunk indices alone: no content of payload or offsets can move an
 * access outside the caller's buffers.  What a malformed stream decodes to is unspecified.
 *
 * Refused with HND_ERR_INVALID before any HIP call, with the export's name in the error string: a NULL pointer, bits
 * outside 1 ... 8, a non-positive n, h, w or c, cs < c, cs % 4 != 0, n * c * h * w > 2^30, q, x, payload, offsets, hist or
 * qparams not 16-byte aligned, payload_bytes <= 0, and a table with a length above 12, a Kraft sum above 1 or no non-zero
 * length.  hnd_entropy_chunks, hnd_entropy_capacity and hnd_entropy_scratch_bytes return 0 for numel <= 0 or numel > 2^30.
 */
#ifndef HND_ENTROPY_H
#define HND_ENTROPY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HND_ENTROPY_ABI 1

int hnd_entropy_abi(void);   /* HND_ENTROPY_ABI */
int64_t hnd_entropy_chunks(int64_t numel);
size_t hnd_entropy_capacity(int64_t numel);
size_t hnd_entropy_scratch_bytes(int64_t numel);
int hnd_code_histogram(const uint8_t* q, int n, int h, int w, int c, int cs, int bits, void* hist, void* stream);
int hnd_entropy_encode(const uint8_t* q, int n, int h, int w, int c, int cs, int bits, const uint8_t* lengths_host,
                       uint8_t* payload, void* offsets, void* scratch, void* stream);
int hnd_entropy_decode_dequantize(const uint8_t* payload, int64_t payload_bytes, const void* offsets,
                                  const uint8_t* lengths_host, const float* qparams, float* x, int n, int h, int w, int c,
                                  int cs, int bits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HND_ENTROPY_H */
