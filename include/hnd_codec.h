/*
 * hnd_codec.h -- the bottleneck codec of libhnd_hip.so at 1 ... 8 bits, beyond hnd_quantize_u8 / hnd_dequantize_u8
 * (hnd_hip.h): Quantizer(num_bits) / Dequantizer(num_bits) of the reference's src/structure/transformer.py:131-153 over
 * myutils tensor_util.quantize_tensor(x, num_bits) / dequantize_tensor, and a bit-packed form of the quantised tensor --
 * the payload that crosses the link between the split detector's head and tail.
 *
 * A header of its own with a version of its own: hnd_hip.h and HND_ABI_VERSION are unchanged by it.  The conventions are
 * those of hnd_hip.h: device pointers into caller-owned buffers, `stream` is a hipStream_t passed as void*, 0 on success
 * and a negative hnd_status otherwise, hnd_last_error_string() explains.
 *
 * Arithmetic (quantize_tensor with qmin = 0, qmax = 2^bits - 1; every step one correctly rounded fp32 operation in the
 * reference's order, no FMA contraction -- the kernels of hnd_quantize_u8, which take qmax as a parameter):
 *   scale      = (max - min) / qmax                 min / max over the `c` real channels of every pixel
 *   zero_point = trunc(clamp(0 - min / scale, 0, qmax))
 *   q          = rint(clamp(zero_point + x / scale, 0, qmax))          (half to even)
 *   x'         = scale * (q - zero_point)
 * max == min (a constant tensor) divides by a zero scale, as in the reference: undefined here as there.
 *
 * Buffers.  x is the fp32 NHWC bottleneck buffer, pixel stride `cs` floats, of which the first `c` are real channels and
 * the rest padding.  qparams is device float[4] = {min, max, scale, zero_point}, written by the quantising calls and read
 * by the dequantising ones.  scratch is device float[hnd_minmax_scratch_elems()] (hnd_hip.h).
 *
 * One value per byte: hnd_quantize_bits is hnd_quantize_u8 with qmax = 2^bits - 1 (bits = 8 gives its bytes and its
 * qparams): q is uint8 NHWC with stride cs, npix * cs bytes, pad channels 0.  hnd_dequantize_u8 inverts it at any width.
 *
 * PAYLOAD FORMAT (hnd_quantize_pack_bits writes it, hnd_unpack_dequantize_bits reads it).  An extension: the reference
 * pickles the one-value-per-byte tensor, so at 4 bits it still moves 8 bits per value.
 *   - the payload holds the quantised values of the LOGICAL NCHW tensor [n, c, h, w], real channels only (no padding);
 *   - values are in index order i = ((img * c + ch) * h + y) * w + x;
 *   - value i occupies bits [i * bits, (i + 1) * bits) of the byte stream, least significant bit first: bit k of the
 *     stream is bit k % 8 of byte k / 8, and bit j of value i is bit i * bits + j of the stream -- what
 *     numpy.packbits(..., bitorder='little') makes of the LSB-first bits of each value, in order;
 *   - the unused high bits of the last byte are 0;
 *   - the buffer is exactly hnd_codec_packed_bytes(n * c * h * w, bits) = ceil(n * c * h * w * bits / 8) bytes, and no
 *     byte outside it is read or written;
 *   - scale and zero point travel beside it, in qparams.
 * hnd_quantize_pack_bits runs the min/max and qparams launches of hnd_quantize_u8 and then ONE launch that quantises and
 * packs (eight consecutive values per thread, `bits` bytes per store group; the last group stores
 * ceil((numel % 8) * bits / 8) bytes).  hnd_unpack_dequantize_bits writes scale * (q - zero_point) into every real
 * channel of the NHWC buffer x and 0 into every pad channel, all n * h * w * cs floats, in one launch.
 *
 * Refused with HND_ERR_INVALID before any HIP call, with the export's name in the error string: a NULL pointer, bits
 * outside 1 ... 8, c <= 0, cs < c, npix <= 0 or a non-positive n, h or w.  hnd_codec_packed_bytes returns 0 for
 * numel <= 0 or bits outside 1 ... 8.
 */
#ifndef HND_CODEC_H
#define HND_CODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HND_CODEC_ABI 1

int hnd_codec_abi(void);   /* HND_CODEC_ABI */
size_t hnd_codec_packed_bytes(int64_t numel, int bits);
int hnd_quantize_bits(const float* x, int64_t npix, int c, int cs, int bits, uint8_t* q, float* qparams, float* scratch,
                      void* stream);
int hnd_quantize_pack_bits(const float* x, int n, int h, int w, int c, int cs, int bits, uint8_t* payload, float* qparams,
                           float* scratch, void* stream);
int hnd_unpack_dequantize_bits(const uint8_t* payload, const float* qparams, float* x, int n, int h, int w, int c, int cs,
                               int bits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HND_CODEC_H */
