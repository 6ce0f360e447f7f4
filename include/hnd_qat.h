/*
 * hnd_qat.h -- quantisation-aware distillation in libhnd_hip.so: the bottleneck tensor fake-quantised in the TRAINING
 * step (quantise and dequantise in one pass, straight-through in the backward), so that the decoder and the layers behind
 * it are trained on the tensor the 1 ... 8-bit codec of hnd_codec.h hands them at evaluation time.  An extension: the
 * reference distils with the quantiser switched off (src/mimic_runner.py:90).
 *
 * A header of its own with a version of its own: hnd_hip.h / HND_ABI_VERSION and hnd_codec.h / HND_CODEC_ABI are unchanged
 * by it.  The conventions are those of hnd_codec.h: device pointers into caller-owned buffers, `stream` is a hipStream_t
 * passed as void*, 0 on success and a negative hnd_status otherwise, hnd_last_error_string() explains.
 *
 * Arithmetic: that of hnd_codec.h with qmax = 2^bits - 1, every step one correctly rounded fp32 operation in the
 * reference's order, no FMA contraction:
 *   scale      = (max - min) / qmax                 min / max over the `c` real channels of every pixel
 *   zero_point = trunc(clamp(0 - min / scale, 0, qmax))
 *   y          = scale * (rint(clamp(zero_point + x / scale, 0, qmax)) - zero_point)          (half to even)
 * y is bit-identical to hnd_quantize_bits followed by hnd_dequantize_u8 on the same x.
 * max == min (a constant tensor) divides by a zero scale, as in hnd_codec.h and in the reference: undefined here as there.
 *
 * Buffers.  x and y are fp32 NHWC buffers of npix pixels, pixel stride `cs` floats (cs % 4 == 0, both 16-byte aligned), of
 * which the first `c` are real channels and the rest padding; y receives 0 in every pad channel, all npix * cs floats are
 * written.  y == x (in place) is allowed; any other overlap is not.  qparams is device float[4] = {min, max, scale,
 * zero_point}, written by the call.  scratch is device float[hnd_minmax_scratch_elems()] (hnd_hip.h).
 *
 * Launches.  The min/max and qparams launches of hnd_quantize_u8, then ONE launch that reads x once (one 16-byte load per
 * 4 channels of a pixel), stores y with plain 16-byte vector stores and, when `stats` is not NULL, the BatchNorm partial
 * sums of what it stored.
 *
 * stats.  NULL, or device float[hnd_fake_quantize_tiles(npix)][2][cs]: per TILE of HND_FAKE_QUANT_TILE_ROWS consecutive
 * pixels (the last tile holds the rest) and per channel, (sum of y, sum of y * y) over the tile's pixels, fp32 -- the layout
 * hnd_bn_finalize reads, ntiles = hnd_fake_quantize_tiles(npix).  Pad channels are 0.  Every row is written: the buffer
 * needs no prior fill.  The order of the additions inside a tile is fixed (results are reproducible run to run).
 *
 * Refused with HND_ERR_INVALID before any HIP call, with the export's name in the error string: a NULL x, y, qparams or
 * scratch, bits outside 1 ... 8, c <= 0, cs < c, cs % 4 != 0, npix <= 0 (or so large that the tile count leaves an int),
 * x or y not 16-byte aligned.  hnd_fake_quantize_tiles returns 0 for npix <= 0.
 */
#ifndef HND_QAT_H
#define HND_QAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HND_QAT_ABI 1
#define HND_FAKE_QUANT_TILE_ROWS 128   /* pixels per row of `stats` */

int hnd_qat_abi(void);   /* HND_QAT_ABI */
int hnd_fake_quantize_tiles(int64_t npix);   /* rows of `stats`: ceil(npix / HND_FAKE_QUANT_TILE_ROWS) */
int hnd_fake_quantize_bits(const float* x, float* y, int64_t npix, int c, int cs, int bits, float* qparams, float* scratch,
                           float* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HND_QAT_H */
