/*
 * hnd_qimage.h -- PER-IMAGE scales for the bottleneck codec and the training-time fake quantiser of libhnd_hip.so: one
 * (scale, zero point) per image of the batch instead of one per tensor.  hnd_codec.h and hnd_qat.h take one min / max over
 * whatever tensor is in front of them: at batch 1 that is the image (the reference's Quantizer, the deployment case), at
 * batch N the whole batch, so an image's codes depend on its neighbours and a student trains on another quantiser than
 * the one it is deployed with.  This header is the opt-in alternative: image i of a batched call gets the bits it gets
 * alone.  No state.  The fixed range of hnd_qrange.h, the entropy coder of hnd_entropy.h, the per-channel scales of
 * hnd_qchannel.h, 16 bits and JPEG have no per-image form.  An extension: the reference has none.
 *
 * A header of its own with a version of its own: hnd_hip.h, hnd_optim.h, hnd_codec.h, hnd_qat.h, hnd_qrange.h,
 * hnd_entropy.h, hnd_qchannel.h and their versions are unchanged by it.  Functions only.  The conventions are those of
 * hnd_qchannel.h: device pointers into caller-owned buffers, `stream` is a hipStream_t passed as void*, 0 on success and a
 * negative hnd_status otherwise, hnd_last_error_string() explains.  No export synchronises with the host.
 *
 * Arithmetic.  Per image i, with qmax = 2^bits - 1; every step one correctly rounded fp32 operation in this order, no FMA
 * contraction:
 *   lo, hi     = min / max of the real channels of image i's hw pixels
 *   scale      = (hi - lo) / qmax               if hi != lo
 *              = |lo|                            if hi == lo and lo != 0
 *              = 1                               if hi == lo == 0
 *   zero_point = trunc(clamp(0 - lo / scale, 0, qmax))
 *   q          = rint(clamp(zero_point + x / scale, 0, qmax))          (half to even)
 *   x'         = scale * (q - zero_point)
 * On an image with hi != lo this is the formula of hnd_codec.h applied to that image alone: with n = 1 every export below
 * gives the bytes, the qparams, the floats and the stats of its per-tensor twin, and image i of a batched call gives what
 * the per-tensor export gives on x[i] alone.  A constant image -- a blank image is ordinary -- follows the rule
 * hnd_qchannel.h gives a constant channel and is reproduced EXACTLY, not through a zero scale: lo > 0 gives zero_point 0,
 * q 1, x' = lo; lo < 0 gives zero_point 1, q 0, x' = lo; lo = 0 gives 0.  Non-finite inputs: as in hnd_codec.h, no promise.
 *
 * Buffers.  x and y are fp32 NHWC buffers of n images of hw = h * w pixels each, pixel stride `cs` floats (cs % 4 == 0,
 * 16-byte aligned), of which the first `c` are real channels and the rest padding; 1 <= n <= HND_QIMAGE_MAX_N, c >= 1,
 * cs >= c, bits 1 ... 8.  qparams is device float[n][4] = {min, max, scale, zero_point} per image, written by the
 * quantising calls and read by the dequantising ones.  scratch is device float[hnd_qimage_scratch_elems(n)]; it needs no
 * prior fill.
 *
 * Launches.  Every quantising export begins with two: one on a grid of (workgroups per image, n) that leaves a partial
 * [n][HND_QIMAGE_PART_BLOCKS][2] of min / max in scratch (lanes laid out as (pixel, group of 4 channels), one 16-byte load per
 * lane and pixel, only the groups that hold a real channel are read), and one of one wave per image that reduces the image's
 * partials and writes qparams[i].  Min and max are exact in any order: no atomics, nothing order-dependent.  Then ONE launch
 * does the work.
 *
 * hnd_qimage_quantize_bits: q is uint8 NHWC with stride cs (4-byte aligned), n * hw * cs bytes, pad channels 0; one 16-byte
 * load and one 4-byte store per lane and pixel.  hnd_qimage_dequantize_u8 inverts it: all n * hw * cs floats of x are
 * written, pad channels 0.
 *
 * hnd_qimage_quantize_pack_bits / hnd_qimage_unpack_dequantize_bits: the PAYLOAD FORMAT IS EXACTLY THAT OF hnd_codec.h (the
 * values of the logical NCHW tensor in index order, `bits` each, least significant bit first,
 * hnd_codec_packed_bytes(n * c * h * w, bits) bytes, unused high bits of the last byte 0, no byte outside it read or
 * written); only the qparams beside it differ: 8 bytes (scale, zero point) per image cross the link instead of 8 per tensor.
 * The unpacking call writes all n * h * w * cs floats of x, pad channels 0.
 *
 * hnd_qimage_fake_quantize_bits: quantise and dequantise in one pass; y is bit-identical to hnd_qimage_quantize_bits
 * followed by hnd_qimage_dequantize_u8, all n * hw * cs floats are written, pad channels 0; y == x (in place) is allowed,
 * any other overlap is not.  stats is NULL or device float[hnd_fake_quantize_tiles(n * hw)][2][cs] (hnd_qat.h): per tile of
 * HND_FAKE_QUANT_TILE_ROWS consecutive pixels of the GLOBAL pixel index (a tile may straddle two images; each of its rows is
 * quantised on its own image's pair) and per channel (sum of y, sum of y * y), the layout hnd_bn_finalize reads; pad
 * channels 0, every row written.  The order of the additions is hnd_qat.h's, FIXED: with S = 64 / (cs / 4) row slots
 * (cs <= 256; a wider pixel is walked 64 groups of 4 channels at a time and S is 64 / the groups of the walk's step), slot s
 * adds the tile's rows s, s + S, s + 2 S, ... in ascending order onto +0 (the sum of squares with ONE fused step
 * fma(y, y, sum), as hnd_fake_quantize_bits does), and the slot sums are then added in ascending s onto +0.
 *
 * Refused with HND_ERR_INVALID before any HIP call, with the export's name in the error string: a NULL pointer (stats may
 * be NULL), bits outside 1 ... 8, n outside 1 ... HND_QIMAGE_MAX_N, a non-positive hw, h or w, c <= 0, cs < c, cs % 4 != 0,
 * so many pixels that n * hw * cs leaves an int64 or the tile count an int, x or y not 16-byte aligned, q not 4-byte
 * aligned.  hnd_qimage_scratch_elems returns 0 for n outside 1 ... HND_QIMAGE_MAX_N.
 */
#ifndef HND_QIMAGE_H
#define HND_QIMAGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HND_QIMAGE_ABI 1
#define HND_QIMAGE_MAX_N 65535        /* images per call: the y extent of a launch grid */
#define HND_QIMAGE_PART_BLOCKS 128    /* min / max partials per image in scratch */

int hnd_qimage_abi(void);   /* HND_QIMAGE_ABI */
size_t hnd_qimage_scratch_elems(int n);
int hnd_qimage_quantize_bits(const float* x, int n, int64_t hw, int c, int cs, int bits, uint8_t* q, float* qparams,
                             float* scratch, void* stream);
int hnd_qimage_dequantize_u8(const uint8_t* q, const float* qparams, float* x, int n, int64_t hw, int c, int cs,
                             void* stream);
int hnd_qimage_quantize_pack_bits(const float* x, int n, int h, int w, int c, int cs, int bits, uint8_t* payload,
                                  float* qparams, float* scratch, void* stream);
int hnd_qimage_unpack_dequantize_bits(const uint8_t* payload, const float* qparams, float* x, int n, int h, int w, int c,
                                      int cs, int bits, void* stream);
int hnd_qimage_fake_quantize_bits(const float* x, float* y, int n, int64_t hw, int c, int cs, int bits, float* qparams,
                                  float* scratch, float* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HND_QIMAGE_H */
