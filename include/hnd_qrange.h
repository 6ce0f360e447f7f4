/*
 * hnd_qrange.h -- a FIXED quantisation range for the bottleneck in libhnd_hip.so: an exponential moving average of the
 * batch min / max observed during training (the range the training-time fake quantiser then clips to, with the gradient
 * zeroed where a value was clipped), and the same range as a constant of the evaluation-time codec, which then quantises
 * in ONE launch.  hnd_codec.h and hnd_qat.h take min / max from the tensor in front of them (three launches, and a
 * different range per batch size); this header is the opt-in alternative.  An extension: the reference has neither.
 *
 * A header of its own with a version of its own: hnd_hip.h, hnd_optim.h, hnd_codec.h, hnd_qat.h and their versions are
 * unchanged by it.  The conventions are those of hnd_codec.h / hnd_qat.h: device pointers into caller-owned buffers,
 * `stream` is a hipStream_t passed as void*, 0 on success and a negative hnd_status otherwise, hnd_last_error_string()
 * explains.  No export synchronises with the host.
 *
 * Arithmetic: that of hnd_codec.h with qmax = 2^bits - 1, every step one correctly rounded fp32 operation, no FMA
 * contraction.  For a range (lo, hi):
 *   scale      = (hi - lo) / qmax
 *   zero_point = trunc(clamp(0 - lo / scale, 0, qmax))
 *   u          = zero_point + x / scale
 *   code       = rint(clamp(u, 0, qmax))                                                       (half to even)
 *   y          = scale * (code - zero_point)
 *   pass       = rint(u) >= 0 && rint(u) <= qmax       (the value was not clipped; u = -0.5 passes, u = qmax + 0.5 does
 *                                                       not: qmax is odd, the tie goes to qmax + 1; a NaN does not pass)
 * qparams is device float[4] = {lo, hi, scale, zero_point} everywhere below.
 *
 * hnd_qrange_observe.  x is an fp32 NHWC buffer of npix pixels, pixel stride `cs` floats, the first `c` real.  state is
 * device float[4] = {running_min, running_max, steps, 0}; scratch is device float[hnd_minmax_scratch_elems()] (hnd_hip.h).
 * Two launches: the min / max launch of hnd_quantize_u8 into scratch, then one wave that reduces the partials to
 * (lo, hi) of the batch and folds them into state:
 *   steps == 0:  running_min = lo,  running_max = hi
 *   otherwise:   running_min = running_min + momentum * (lo - running_min)        (subtract, multiply, add: three roundings)
 *                running_max = running_max + momentum * (hi - running_max)
 *   steps += 1;  state[3] = 0
 * and writes qparams from the running pair.  `bits` only sets qmax for qparams.
 *
 * hnd_qrange_qparams.  lo, hi are HOST floats; a one-thread kernel writes qparams with the formula above, so that host and
 * device can never disagree on a rounding.
 *
 * hnd_fake_quantize_range.  hnd_fake_quantize_bits (hnd_qat.h) on caller-given qparams, which are read and not written: ONE
 * launch, no min / max launch.  x, y, stats are as in hnd_qat.h: y receives 0 in every pad channel, all npix * cs floats are
 * written, y == x is allowed, stats is NULL or device float[hnd_fake_quantize_tiles(npix)][2][cs] with the same fixed
 * order of additions.  mask is NULL or device uint8[npix][cs / 4]: bit k (0 ... 3) of byte g of a pixel is `pass` of
 * channel 4 g + k; the bits of pad channels and the high nibble are 0; every byte is written (plain byte stores, one per
 * 16-byte store of y).  A NaN in x gives a NaN in y and a 0 bit.
 *
 * hnd_qrange_mask_grad.  The backward of the clipping: in place, g[p][ch] = pass ? g[p][ch] : +0 for the real channels of
 * the fp32 NHWC buffer g (npix pixels, stride cs); pad channels keep their bits.  mask is what hnd_fake_quantize_range
 * wrote for the same geometry.
 *
 * hnd_quantize_range_bits / hnd_quantize_pack_range_bits.  The third launch of hnd_quantize_bits / hnd_quantize_pack_bits
 * (hnd_codec.h) alone, on caller-given qparams (read, not written).  q and payload have the formats of hnd_codec.h (values
 * outside the range take the codes 0 and qmax); hnd_dequantize_u8 and hnd_unpack_dequantize_bits invert them as they are.
 *
 * Refused with HND_ERR_INVALID before any HIP call, with the export's name in the error string: a NULL pointer (mask and
 * stats of hnd_fake_quantize_range may be NULL), bits outside 1 ... 8, c <= 0, cs < c, cs % 4 != 0, npix <= 0 (or a
 * non-positive n, h or w; or so large that the tile count leaves an int), x, y, g, state or qparams not 16-byte aligned, a
 * momentum outside (0, 1], and for hnd_qrange_qparams a non-finite lo or hi, or lo >= hi.
 */
#ifndef HND_QRANGE_H
#define HND_QRANGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HND_QRANGE_ABI 1

int hnd_qrange_abi(void);   /* HND_QRANGE_ABI */
int hnd_qrange_observe(const float* x, int64_t npix, int c, int cs, float momentum, int bits, float* state, float* qparams,
                       float* scratch, void* stream);
int hnd_qrange_qparams(float lo, float hi, int bits, float* qparams, void* stream);
int hnd_fake_quantize_range(const float* x, float* y, int64_t npix, int c, int cs, int bits, const float* qparams,
                            uint8_t* mask, float* stats, void* stream);
int hnd_qrange_mask_grad(float* g, const uint8_t* mask, int64_t npix, int c, int cs, void* stream);
int hnd_quantize_range_bits(const float* x, int64_t npix, int c, int cs, int bits, uint8_t* q, const float* qparams,
                            void* stream);
int hnd_quantize_pack_range_bits(const float* x, int n, int h, int w, int c, int cs, int bits, uint8_t* payload,
                                 const float* qparams, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HND_QRANGE_H */
