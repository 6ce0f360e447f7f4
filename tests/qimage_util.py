"""Shared by the tests of include/hnd_qimage.h (tests/test_qimage_cpu.py, tests/test_qimage_gpu.py,
tests/test_guard_bands_qimage_gpu.py): the input table, the reference -- oracle/myutils_r.quantize_tensor /
dequantize_tensor applied to each image z[i:i+1] ALONE, which is what the reference's Quantizer does at batch 1 -- and a
numpy-fp32 restatement of the header, constant-image rule included (the oracle divides by a zero scale there), which
tests/test_qimage_cpu.py pins to the oracle bit for bit on every non-constant image.  Everything is computed once and kept;
callers compare, they do not write.

A plain module: no fixtures, no pytest settings; importing it loads neither the library nor the launch helpers."""
import numpy as np
import torch

from oracle.myutils_r import dequantize_tensor, quantize_tensor
from tests import codec_util as CU
from tests import qat_util as QU

ROWS = 128                      # HND_FAKE_QUANT_TILE_ROWS
SHIFT = 0.3                     # codec_util.make_input's recipe that straddles zero
# (logical NCHW shape, pixel stride): the smallest shapes at which each mechanism can go wrong
SHAPES_ALL_WIDTHS = [((1, 3, 1, 2), 4),          # the n = 1 anchor
                     ((3, 1, 3, 5), 4),          # c = 1
                     ((2, 3, 5, 7), 4),          # 105 values per image: pack groups cross images, and the tail group
                     ((5, 3, 2, 3), 4)]          # several images inside one wave pass
SHAPES_TWO_WIDTHS = [((2, 3, 13, 10), 4),        # hw = 130: a stats tile straddles the image boundary
                     ((2, 6, 9, 11), 32),        # a stride far wider than c
                     ((2, 15, 3, 5), 16)]        # 15 channels
ALL_WIDTHS, TWO_WIDTHS = (1, 2, 3, 4, 5, 8), (2, 8)
CASES = [(shape, cs, bits) for shape, cs in SHAPES_ALL_WIDTHS for bits in ALL_WIDTHS] + \
        [(shape, cs, bits) for shape, cs in SHAPES_TWO_WIDTHS for bits in TWO_WIDTHS]
RMS_SHAPE, RMS_WIDTHS = (4, 3, 5, 7), (2, 4, 8)
GUARD_SHAPES, GUARD_WIDTHS = [((2, 3, 5, 7), 4), ((2, 6, 9, 11), 32)], (3, 8)
CONSTANTS = (0.75, -2.5, 0.0)   # the constant images of the header's rule

# The batch-2 fixtures whose (fixture, width) pairs were scanned for the one-step comparison with a per-image
# straight-through quantiser.  The pairs are chosen from the oracle alone (tests/test_qimage_cpu.py holds the oracle to
# them): per image the fp32 and the fp64 oracle take identical decisions, no rounding decision -- a value, or -min / scale
# -- sits within qat_util.MARGIN (1e-4 code units) of its tie, and the two images' qparams differ.
# All 32 candidate pairs (4 fixtures x widths 1 ... 8) were scanned: in every one the two oracles agree on every code and
# zero point and the images' qparams differ; 13 also keep the margin (tiny_ghnd_faster at 1 bit; tiny_hnd_faster at 1, 3, 8;
# tiny_ghnd_keypoint at 1, 3, 7, 8; tiny_ghnd_custom_hooks at 1, 3, 5, 7), the other 19 have a value 2.9e-6 ... 9.3e-5 from
# a half-integer (tiny_ghnd_custom_hooks at 8 bits keeps 6.9e-5) and are NOT used.  Of the 13, the pairs on the two fixtures
# whose step tests/test_model_gpu.py runs without special handling (the keypoint fixture draws its sizes and has a gradient
# bar of its own, the custom-hooks fixture hooks further modules), leaving out 1 bit, where an image of tiny_ghnd_faster
# quantises to the single code 0 (-min / scale = 0.57, so no value reaches one half) and the quantiser would not be at work:
# a low width and a high one on tiny_hnd_faster.  ONE_STEP_MARGINS: the measured (nearest half-integer of any value, nearest
# integer of any -min / scale) in code units, the smaller of the fp32 and the fp64 oracle, over both images.
SCAN_FIXTURES = ('tiny_ghnd_faster', 'tiny_hnd_faster', 'tiny_ghnd_keypoint', 'tiny_ghnd_custom_hooks')
ONE_STEP_CASES = [('tiny_hnd_faster', 3), ('tiny_hnd_faster', 8)]
ONE_STEP_MARGINS = {('tiny_hnd_faster', 3): (2.365e-4, 1.040e-1), ('tiny_hnd_faster', 8): (2.485e-4, 7.523e-2)}

_INPUTS, _ORACLE, _RESTATED = {}, {}, {}


def make_input(shape):
    """codec_util.make_input(shape, 0.3) with image i multiplied by 4^(i mod 4): the images' ranges differ, so a kernel
    that took the batch's range fails"""
    key = tuple(shape)
    if key not in _INPUTS:
        z = CU.make_input(shape, SHIFT).clone()
        gain = torch.tensor([4.0 ** (i % 4) for i in range(shape[0])])
        _INPUTS[key] = z * gain.view(-1, 1, 1, 1)
    return _INPUTS[key]


def with_constants(shape):
    """make_input(shape) (n >= 4) whose images 0, 1 and n - 1 are the constants 0.75, -2.5 and 0: blank images beside live
    ones"""
    z = make_input(shape).clone()
    assert shape[0] >= 4
    for i, v in zip((0, 1, shape[0] - 1), CONSTANTS):
        z[i] = v
    return z


class Quantised(object):
    """.codes (uint8 NCHW), .scale / .zero_point (fp32 tensors [n]), .lo / .hi ([n]), .dequantized (NCHW, the input's dtype),
    .qparams (fp32 [n, 4] = {min, max, scale, zero_point}), .payload (numpy uint8, the packed bytes of hnd_codec.h's format)"""

    def __init__(self, codes, lo, hi, scale, zero_point, dequantized, bits):
        self.codes, self.lo, self.hi, self.scale, self.zero_point = codes, lo, hi, scale, zero_point
        self.dequantized, self.bits = dequantized, bits
        self.qparams = torch.stack([lo, hi, scale, zero_point], 1).float()
        self.payload = CU.host_pack(codes, bits)


def oracle_per_image(z, bits):
    """the reference: quantize_tensor / dequantize_tensor on every image alone (a constant image is undefined there and
    comes out as whatever the zero scale makes of it: callers skip those)"""
    parts = [quantize_tensor(z[i:i + 1].clone(), num_bits=bits) for i in range(z.shape[0])]
    deq = torch.cat([dequantize_tensor(q) for q in parts], 0)
    col = lambda vals: torch.tensor([float(v) for v in vals], dtype=torch.float64).to(z.dtype)      # noqa: E731
    return Quantised(torch.cat([q.tensor for q in parts], 0),
                     col(z[i].min() for i in range(z.shape[0])), col(z[i].max() for i in range(z.shape[0])),
                     col(q.scale for q in parts), col(q.zero_point for q in parts), deq, bits)


def oracle(shape, bits):
    key = (tuple(shape), bits)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_per_image(make_input(shape), bits)
    return _ORACLE[key]


def restate(z, bits):
    """include/hnd_qimage.h in numpy fp32, one correctly rounded operation per step, the constant-image rule included"""
    x = z.numpy().astype(np.float32)
    f = np.float32
    qmax = f(2 ** bits - 1)
    n = x.shape[0]
    lo, hi, scale, zp = (np.empty(n, f) for _ in range(4))
    codes, deq = np.empty(x.shape, np.uint8), np.empty(x.shape, f)
    with np.errstate(all='ignore'):
        for i in range(n):
            v = x[i]
            lo[i], hi[i] = v.min(), v.max()
            if hi[i] != lo[i]:
                scale[i] = f(hi[i] - lo[i]) / qmax
            else:
                scale[i] = np.abs(lo[i]) if lo[i] != 0 else f(1)
            zp[i] = np.trunc(np.clip(f(0) - lo[i] / scale[i], f(0), qmax))
            q = np.rint(np.clip(zp[i] + v / scale[i], f(0), qmax))                    # half to even
            assert q.dtype == f
            codes[i] = q.astype(np.uint8)
            deq[i] = scale[i] * (q - zp[i])
    t = torch.from_numpy
    return Quantised(t(codes), t(lo), t(hi), t(scale), t(zp), t(deq), bits)


def restated(shape, bits):
    key = (tuple(shape), bits)
    if key not in _RESTATED:
        _RESTATED[key] = restate(make_input(shape), bits)
    return _RESTATED[key]


def restate_per_tensor(z, bits):
    """include/hnd_codec.h in numpy fp32 (one scale for the batch): the yardstick of the RMS comparison"""
    flat = restate(z.reshape(1, 1, -1, 1), bits)
    return flat.dequantized.view(z.shape)


def rms_error(z, deq):
    return float(torch.sqrt(((deq.double() - z.double()) ** 2).mean()))


def fma32(v, acc):
    """round_fp32(v * v + acc) with ONE rounding, elementwise on fp32 arrays.  v * v is exact in fp64 (48 bits); the fp64 sum
    is made exact by TwoSum and rounded to odd, after which the conversion to fp32 (29 bits fewer) rounds correctly"""
    a = v.astype(np.float64) * v.astype(np.float64)
    b = acc.astype(np.float64)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)
    even = (s.view(np.int64) & 1) == 0
    away = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, away, s).astype(np.float32)


def restate_stats(y, cs):
    """the `stats` of hnd_qimage_fake_quantize_bits for the stored buffer y [npix, cs] (fp32) over the GLOBAL pixel index, in
    the order of hnd_qat.h: per tile of 128 rows and per channel, S = 64 / (cs / 4) row slots; slot s adds rows s, s + S, ...
    in ascending order onto +0 (the sum of squares with one fused step fma(y, y, sum)), then the slot sums are added in
    ascending s onto +0.  Returns [tiles, 2, cs] fp32."""
    y = y.numpy().astype(np.float32).reshape(-1, cs)
    assert cs % 4 == 0 and cs <= 256
    slots = 64 // (cs // 4)
    npix = y.shape[0]
    nt = (npix + ROWS - 1) // ROWS
    out = np.zeros((nt, 2, cs), np.float32)
    for t in range(nt):
        blk = y[t * ROWS:(t + 1) * ROWS]
        for k in range(2):
            total = np.zeros(cs, np.float32)
            for s in range(slots):
                acc = np.zeros(cs, np.float32)
                for r in range(s, blk.shape[0], slots):
                    acc = acc + blk[r] if k == 0 else fma32(blk[r], acc)
                total = total + acc
            out[t, k] = total
    return torch.from_numpy(out)


# ---- the one-step comparison: tests/qat_util.py's estimator and preconditions, per image
def quantize_dequantize_per_image(z, bits):
    return torch.cat([dequantize_tensor(quantize_tensor(z[i:i + 1], num_bits=bits)) for i in range(z.shape[0])], 0)


def ste_per_image(z, bits):
    """the straight-through estimator: the forward value is the per-image quantise -> dequantise, the backward the identity"""
    return z + (quantize_dequantize_per_image(z, bits) - z).detach()


def decide_codes_per_image(z, bits):
    """qat_util.decide_codes on every image alone: a list of its dicts"""
    return [QU.decide_codes(z[i:i + 1], bits) for i in range(z.shape[0])]


def check_preconditions_per_image(caps32, caps64, what=''):
    """qat_util.check_preconditions on every image; returns the smallest (half-integer, integer) margins over the images and
    both oracles"""
    assert len(caps32) == len(caps64) > 0
    half, zp = [], []
    for i, (a, b) in enumerate(zip(caps32, caps64)):
        m32, m64 = QU.check_preconditions(a, b, '%s, image %d' % (what, i))
        half += [m32[0], m64[0]]
        zp += [m32[1], m64[1]]
    return min(half), min(zp)


def qparams_differ(caps):
    """the images of a capture do not share one (scale, zero point): the per-image quantiser is not the per-tensor one"""
    return len({(c['scale'], c['zero_point']) for c in caps}) > 1
