/*
 * hnd_qchannel.h -- PER-CHANNEL scales for the bottleneck codec and the training-time fake quantiser of libhnd_hip.so:
 * one (scale, zero point) per real channel of the bottleneck tensor instead of one per tensor.  hnd_codec.h and hnd_qat.h
 * take one min / max over all channels, so the widest channel sets the step of every other; this header is the opt-in
 * alternative for the per-batch range (min / max of the tensor in front of the call).  The fixed range of hnd_qrange.h,
 * the entropy coder of hnd_entropy.h, 16 bits and JPEG have no per-channel form.  An extension: the reference has none.
 *
 * A header of its own with a version of its own: hnd_hip.h, hnd_optim.h, hnd_codec.h, hnd_qat.h, hnd_qrange.h,
 * hnd_entropy.h and their versions are unchanged by it.  Functions only.  The conventions are those of hnd_codec.h: device
 * pointers into caller-owned buffers, `stream` is a hipStream_t passed as void*, 0 on success and a negative hnd_status
 * otherwise, hnd_last_error_string() explains.  No export synchronises with the host.
 *
 * Arithmetic.  Per real channel ch, with qmax = 2^bits - 1; every step one correctly rounded fp32 operation in this order,
 * no FMA contraction:
 *   lo, hi     = min / max of channel ch over all npix pixels
 *   scale      = (hi - lo) / qmax               if hi != lo
 *              = |lo|                            if hi == lo and lo != 0
 *              = 1                               if hi == lo == 0
 *   zero_point = trunc(clamp(0 - lo / scale, 0, qmax))
 *   q          = rint(clamp(zero_point + x / scale, 0, qmax))          (half to even)
 *   x'         = scale * (q - zero_point)
 * On a channel with hi != lo this is the formula of hnd_codec.h applied to that channel alone (with c = 1 every export
 * below gives the bytes and the qparams of its per-tensor twin).  A constant channel -- a dead channel is ordinary -- is
 * reproduced EXACTLY by the same formulas: lo > 0 gives zero_point 0, q 1, x' = lo; lo < 0 gives zero_point 1, q 0,
 * x' = lo; lo = 0 gives 0.  Non-finite inputs: as in hnd_codec.h, no promise.
 *
 * Buffers.  x and y are fp32 NHWC buffers, pixel stride `cs` floats (cs % 4 == 0, 16-byte aligned), of which the first `c`
 * are real channels and the rest padding; 1 <= c <= HND_QCHANNEL_MAX_C, cs >= c, bits 1 ... 8.  qparams is device
 * float[c][4] = {min, max, scale, zero_point} per real channel, written by the quantising calls and read by the
 * dequantising ones.  scratch is device float[hnd_qchannel_scratch_elems(cs)]; it needs no prior fill.
 *
 * Launches.  Every quantising export begins with two: one that leaves a partial [workgroup][2][cs] of per-channel min / max
 * in scratch (lanes laid out as (pixel, group of 4 channels), one 16-byte load per lane and pixel; lanes of one group meet
 * in LDS), and one small launch that reduces the partials per channel and writes qparams.  Min and max are exact in any
 * order: no atomics, nothing order-dependent.  Then ONE launch does the work.
 *
 * hnd_qchannel_quantize_bits: q is uint8 NHWC with stride cs (4-byte aligned), npix * cs bytes, pad channels 0; one 16-byte
 * load and one 4-byte store per lane and pixel.  hnd_qchannel_dequantize_u8 inverts it: all npix * cs floats of x are
 * written, pad channels 0.
 *
 * hnd_qchannel_quantize_pack_bits / hnd_qchannel_unpack_dequantize_bits: the PAYLOAD FORMAT IS EXACTLY THAT OF hnd_codec.h
 * (the values of the logical NCHW tensor in index order, `bits` each, least significant bit first,
 * hnd_codec_packed_bytes(n * c * h * w, bits) bytes, unused high bits of the last byte 0, no byte outside it read or
 * written); only the qparams beside it differ: 8 bytes (scale, zero point) per channel cross the link instead of 8 per
 * tensor.  The unpacking call writes all n * h * w * cs floats of x, pad channels 0.
 *
 * hnd_qchannel_fake_quantize_bits: quantise and dequantise in one pass; y is bit-identical to hnd_qchannel_quantize_bits
 * followed by hnd_qchannel_dequantize_u8, all npix * cs floats are written, pad channels 0; y == x (in place) is allowed,
 * any other overlap is not.  stats is NULL or device float[hnd_fake_quantize_tiles(npix)][2][cs] (hnd_qat.h): per tile of
 * HND_FAKE_QUANT_TILE_ROWS consecutive pixels and per channel (sum of y, sum of y * y), the layout hnd_bn_finalize reads;
 * pad channels 0, every row written.  The order of the additions is FIXED: with S = 64 / (cs / 4) row slots (cs <= 256; a wider
 * pixel is walked 64 groups of 4 channels at a time and S is 64 / the groups of the walk's step), slot s adds the tile's rows
 * s, s + S, s + 2 S, ... in ascending order onto +0 (y * y is rounded, then added), and the slot sums are then added in
 * ascending s onto +0.
 *
 * Refused with HND_ERR_INVALID before any HIP call, with the export's name in the error string: a NULL pointer (stats may
 * be NULL), bits outside 1 ... 8, c outside 1 ... HND_QCHANNEL_MAX_C, cs < c, cs % 4 != 0, npix <= 0 or a non-positive n, h
 * or w (or so many pixels that the tile count leaves an int), x or y not 16-byte aligned, q not 4-byte aligned.
 * hnd_qchannel_scratch_elems returns 0 for cs <= 0 or cs % 4 != 0.
 */
#ifndef HND_QCHANNEL_H
#define HND_QCHANNEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HND_QCHANNEL_ABI 1
#define HND_QCHANNEL_MAX_C 64   /* real channels */

int hnd_qchannel_abi(void);   /* HND_QCHANNEL_ABI */
size_t hnd_qchannel_scratch_elems(int cs);
int hnd_qchannel_quantize_bits(const float* x, int64_t npix, int c, int cs, int bits, uint8_t* q, float* qparams,
                               float* scratch, void* stream);
int hnd_qchannel_dequantize_u8(const uint8_t* q, const float* qparams, float* x, int64_t npix, int c, int cs, void* stream);
int hnd_qchannel_quantize_pack_bits(const float* x, int n, int h, int w, int c, int cs, int bits, uint8_t* payload,
                                    float* qparams, float* scratch, void* stream);
int hnd_qchannel_unpack_dequantize_bits(const uint8_t* payload, const float* qparams, float* x, int n, int h, int w, int c,
                                        int cs, int bits, void* stream);
int hnd_qchannel_fake_quantize_bits(const float* x, float* y, int64_t npix, int c, int cs, int bits, float* qparams,
                                    float* scratch, float* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HND_QCHANNEL_H */
