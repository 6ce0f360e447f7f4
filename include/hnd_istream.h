/*
 * hnd_istream.h -- PER-IMAGE entropy streams for the bottleneck codec of libhnd_hip.so: the entropy-coded link payload of
 * hnd_entropy.h applied to every image of a batch on its own, beside the per-image scales of hnd_qimage.h, with every
 * image's code table built ON THE DEVICE.  hnd_entropy.h codes the batch as one stream under one table made on the host
 * (a histogram read-back per tensor): no image's message can be cut out of it, and image i begins in the middle of a chunk.
 * Here image i of a batched call gets the table, the bytes and the qparams it gets alone, no export synchronises with the
 * host, and what crosses the link for one image is a complete hnd_entropy.h message.  An extension: the reference has none.
 *
 * A header of its own with a version of its own: hnd_hip.h, hnd_optim.h, hnd_codec.h, hnd_qat.h, hnd_qrange.h,
 * hnd_entropy.h, hnd_qchannel.h, hnd_qimage.h and their versions are unchanged by it.  Functions only.  The conventions are
 * those of hnd_entropy.h: device pointers into caller-owned buffers, `stream` is a hipStream_t passed as void*, 0 on success
 * and a negative hnd_status otherwise, hnd_last_error_string() explains.
 *
 * FORMAT.  That of hnd_entropy.h -- the canonical code, the 12-bit limit, bytes filled least significant bit first, code
 * bits most significant first, chunks of 256 symbols on byte boundaries with zero pad bits -- per image:
 * Symbols.  The symbols of image i are the codes of its real channels in the order (ch * h + y) * w + x, chw = c * h * w of
 *   them.
 * Chunks.  cpi = hnd_istream_chunks_per_image(chw) = ceil(chw / 256) chunks per image; the last chunk of EVERY image may be
 *   short.  The global index of chunk k of image i is g = i * cpi + k.
 * offsets is uint32[n * cpi + 1], byte offsets into ONE payload buffer of capacity hnd_istream_capacity(n, chw) =
 *   n * cpi * 384 bytes: offsets[0] = 0, offsets[n * cpi] the byte count of all streams; bytes at and beyond it are not
 *   written.
 * lengths is DEVICE uint8[n][256]: row i is the table of image i, lengths[i][s] in 0 ... 12 for s < 2^bits, 0 at and beyond
 *   2^bits.
 * qparams is device float[n][4] = {min, max, scale, zero_point} per image, exactly as hnd_qimage.h writes it.
 * What crosses the link for image i: payload[offsets[i * cpi] : offsets[(i + 1) * cpi]], its cpi + 1 offsets rebased to 0,
 *   lengths[i][: 2^bits], and scale and zero point of qparams[i]:
 *   link_bytes_i = nbytes_i + 4 * (cpi + 1) + 2^bits + 8; a batch's link size is the sum over its images.
 * With n = 1 payload, offsets and lengths are what hnd_entropy_encode writes under the same table.
 *
 * Buffers.  q is the one-value-per-byte uint8 NHWC tensor hnd_qimage_quantize_bits writes, pixel stride `cs` bytes of which
 * the first `c` are real channels; x is the fp32 NHWC bottleneck buffer of the same geometry.  The 32-bit buffers are
 * declared void*: hist is uint32_t[n][256], offsets is uint32_t[n * cpi + 1], scratch is hnd_istream_scratch_bytes(n, chw)
 * bytes (uint32_t[n * cpi]: the byte count of every chunk).  1 <= n <= HND_ISTREAM_MAX_N.
 *
 * hnd_istream_histogram.  hist[i] counts the codes of the real channels of image i; the call zeroes hist (a memset node)
 * and fills it in ONE launch on a grid of (workgroups per image, n).  A byte of q at or above 2^bits, and a pad channel, is
 * counted nowhere.  An image's h * w * cs bytes need not be a multiple of 16: the whole 16-byte vectors inside an image are
 * loaded as such, the up to 15 bytes before the first and after the last one byte by byte; no load is misaligned.
 *
 * hnd_istream_build_tables.  ONE launch, one workgroup per image: lengths[i] = the code lengths of an optimal prefix code
 * of hist[i] whose longest code has 12 bits, by package-merge with the leaves ranked by (count, symbol) and a leaf before a
 * package of equal weight -- byte for byte what the host routine of the Python package (transformer.huffman_lengths) gives
 * for the same histogram.  A single occurring symbol gets length 1; an all-zero histogram gives all-zero lengths, and every
 * chunk of that image is then 0 bytes long.  Entries of hist at and beyond 2^bits are not read.
 *
 * hnd_istream_encode.  The THREE launches of hnd_entropy_encode with the image as a grid row: the byte count of every chunk
 * into scratch, their exclusive prefix sum over all n * cpi chunks into offsets (ONE workgroup), the streams.  A workgroup
 * works on one image and builds that image's canonical table in LDS from lengths[i].  lengths is device memory the export
 * cannot validate: every length is read as min(length, 12) and entries at and beyond 2^bits as 0, so no chunk exceeds 384
 * bytes whatever the table holds.  A table that is not a prefix code (a Kraft sum above 1) gives an unspecified stream, but
 * no access outside the caller's buffers.
 *
 * hnd_istream_decode_dequantize.  ONE launch: the tile decoder of hnd_entropy_decode_dequantize (a workgroup owns 2048
 * pixels of one image) with the decode table built in LDS from lengths[img], chunk indices based at img * cpi and scale and
 * zero point read from qparams[img].  Writes scale * (q - zero_point) -- one fp32 subtraction, one fp32 multiplication, no
 * FMA contraction: the bits of hnd_qimage_unpack_dequantize_bits on the same codes -- into every real channel of x and 0
 * into every pad channel, all n * h * w * cs floats.  Every read of payload is inside [0, payload_bytes) (a position beyond
 * it reads as 0), every write position comes from the tile and chunk indices alone, and the table indices are bounded by
 * construction (lengths are clamped to 12, the counts per length sum to at most 256): no content of payload, offsets or
 * lengths can move an access outside the caller's buffers.  What a malformed stream or table decodes to is unspecified.
 *
 * Refused with HND_ERR_INVALID before any HIP call, with the export's name in the error string: a NULL pointer, bits
 * outside 1 ... 8, a non-positive n, h, w or c, n > HND_ISTREAM_MAX_N, cs < c, cs % 4 != 0, n * c * h * w > 2^30, q, x,
 * payload, offsets, scratch, hist or qparams not 16-byte aligned, payload_bytes <= 0 or above the capacity of the largest
 * call.  hnd_istream_chunks_per_image returns 0 for chw <= 0 or chw > 2^30; hnd_istream_capacity and
 * hnd_istream_scratch_bytes return 0 for n outside 1 ... HND_ISTREAM_MAX_N, chw <= 0 or n * chw > 2^30.
 */
#ifndef HND_ISTREAM_H
#define HND_ISTREAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HND_ISTREAM_ABI 1
#define HND_ISTREAM_MAX_N 65535       /* images per call: the y extent of a launch grid */

int hnd_istream_abi(void);   /* HND_ISTREAM_ABI */
int64_t hnd_istream_chunks_per_image(int64_t chw);
size_t hnd_istream_capacity(int n, int64_t chw);
size_t hnd_istream_scratch_bytes(int n, int64_t chw);
int hnd_istream_histogram(const uint8_t* q, int n, int h, int w, int c, int cs, int bits, void* hist, void* stream);
int hnd_istream_build_tables(const void* hist, int n, int bits, uint8_t* lengths, void* stream);
int hnd_istream_encode(const uint8_t* q, int n, int h, int w, int c, int cs, int bits, const uint8_t* lengths,
                       uint8_t* payload, void* offsets, void* scratch, void* stream);
int hnd_istream_decode_dequantize(const uint8_t* payload, int64_t payload_bytes, const void* offsets,
                                  const uint8_t* lengths, const float* qparams, float* x, int n, int h, int w, int c,
                                  int cs, int bits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HND_ISTREAM_H */
