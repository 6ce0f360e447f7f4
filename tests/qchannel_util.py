"""Shared by the tests of include/hnd_qchannel.h (tests/test_qchannel_cpu.py, tests/test_qchannel_gpu.py,
tests/test_guard_bands_qchannel_gpu.py): the input table, the reference -- oracle/myutils_r.quantize_tensor /
dequantize_tensor applied to each channel z[:, ch:ch+1] ALONE, which is what "per channel" means in the reference's own
code -- and a numpy-fp32 restatement of the header, constant-channel rule included (the oracle divides by a zero scale
there), which tests/test_qchannel_cpu.py pins to the oracle bit for bit on every non-constant channel.  Everything is
computed once and kept; callers compare, they do not write.

A plain module: no fixtures, no pytest settings; importing it loads neither the library nor the launch helpers."""
import numpy as np
import torch

from oracle.myutils_r import dequantize_tensor, quantize_tensor
from tests import codec_util as CU
from tests import qat_util as QU

ROWS = 128                      # HND_FAKE_QUANT_TILE_ROWS
SHIFT = 0.3                     # codec_util.make_input's recipe that straddles zero
# (logical NCHW shape, pixel stride): the smallest shapes at which each mechanism can go wrong
SHAPES_ALL_WIDTHS = [((1, 1, 3, 5), 4),          # c = 1
                     ((1, 3, 1, 2), 4),          # one row, two pixels
                     ((2, 3, 5, 7), 4),          # 210 values: the pack tail group; hw = 35: groups cross planes and images
                     ((1, 6, 9, 11), 8)]
SHAPES_TWO_WIDTHS = [((1, 6, 9, 11), 32),        # a stride far wider than c, as on the b6 fixture
                     ((2, 15, 3, 5), 16),
                     ((1, 3, 130, 1), 4),        # npix crosses the 128-pixel stats tile
                     ((1, 64, 2, 3), 64)]        # the maximum c
ALL_WIDTHS, TWO_WIDTHS = (1, 2, 3, 4, 5, 8), (2, 8)
CASES = [(shape, cs, bits) for shape, cs in SHAPES_ALL_WIDTHS for bits in ALL_WIDTHS] + \
        [(shape, cs, bits) for shape, cs in SHAPES_TWO_WIDTHS for bits in TWO_WIDTHS]
RMS_SHAPE, RMS_WIDTHS = ((2, 15, 3, 5), 16), (2, 4, 8)
GUARD_SHAPES, GUARD_WIDTHS = [((2, 3, 5, 7), 4), ((1, 6, 9, 11), 32)], (3, 8)
CONSTANTS = (0.75, -2.5, 0.0)   # the constant channels of the header's rule

# (fixture, width) pairs of the one-step comparison with a per-channel straight-through quantiser, chosen from the oracle
# alone (tests/test_qchannel_cpu.py holds the oracle to them): per channel the fp32 and the fp64 oracle take identical
# decisions and no rounding decision -- a value, or -min / scale -- sits within qat_util.MARGIN (1e-4 code units) of its tie.
# All 16 candidate pairs (2 fixtures x widths 1 ... 8) were scanned; 9 meet the preconditions (tiny_ghnd_faster at 1, 2, 3,
# 5, 7 bits; tiny_ghnd_faster_b6 at 1, 4, 5, 6), 7 have a value 5e-5 ... 1e-4 from a half-integer and are NOT used.  Of the 9,
# a low width, a high one and the b6 fixture with the widest margins.  ONE_STEP_MARGINS: the measured (nearest half-integer
# of any value, nearest integer of any -min / scale) in code units, the smaller of the fp32 and the fp64 oracle, over all
# channels.
ONE_STEP_CASES = [('tiny_ghnd_faster', 2), ('tiny_ghnd_faster', 7), ('tiny_ghnd_faster_b6', 6)]
ONE_STEP_MARGINS = {('tiny_ghnd_faster', 2): (1.659e-4, 3.155e-1), ('tiny_ghnd_faster', 7): (5.207e-4, 3.099e-1),
                    ('tiny_ghnd_faster_b6', 6): (4.529e-4, 2.750e-2)}

_INPUTS, _ORACLE, _RESTATED = {}, {}, {}


def make_input(shape):
    """codec_util.make_input(shape, 0.3) with channel ch multiplied by 4^(ch mod 4): the channels' ranges differ"""
    key = tuple(shape)
    if key not in _INPUTS:
        z = CU.make_input(shape, SHIFT).clone()
        gain = torch.tensor([4.0 ** (ch % 4) for ch in range(shape[1])])
        _INPUTS[key] = z * gain.view(1, -1, 1, 1)
    return _INPUTS[key]


def with_constants(shape):
    """make_input(shape) (c >= 4) whose channels 0, 1 and c - 1 are the constants 0.75, -2.5 and 0: dead channels beside
    live ones"""
    z = make_input(shape).clone()
    assert shape[1] >= 4
    for ch, v in zip((0, 1, shape[1] - 1), CONSTANTS):
        z[:, ch] = v
    return z


class Quantised(object):
    """.codes (uint8 NCHW), .scale / .zero_point (fp32 tensors [c]), .lo / .hi ([c]), .dequantized (NCHW, the input's dtype),
    .qparams (fp32 [c, 4] = {min, max, scale, zero_point}), .payload (numpy uint8, the packed bytes of hnd_codec.h's format)"""

    def __init__(self, codes, lo, hi, scale, zero_point, dequantized, bits):
        self.codes, self.lo, self.hi, self.scale, self.zero_point = codes, lo, hi, scale, zero_point
        self.dequantized, self.bits = dequantized, bits
        self.qparams = torch.stack([lo, hi, scale, zero_point], 1).float()
        self.payload = CU.host_pack(codes, bits)


def oracle_per_channel(z, bits):
    """the reference: quantize_tensor / dequantize_tensor on every channel alone (a constant channel is undefined there and
    comes out as whatever the zero scale makes of it: callers skip those)"""
    parts = [quantize_tensor(z[:, ch:ch + 1].clone(), num_bits=bits) for ch in range(z.shape[1])]
    deq = torch.cat([dequantize_tensor(q) for q in parts], 1)
    col = lambda vals: torch.tensor([float(v) for v in vals], dtype=torch.float64).to(z.dtype)      # noqa: E731
    return Quantised(torch.cat([q.tensor for q in parts], 1),
                     col(z[:, ch].min() for ch in range(z.shape[1])), col(z[:, ch].max() for ch in range(z.shape[1])),
                     col(q.scale for q in parts), col(q.zero_point for q in parts), deq, bits)


def oracle(shape, bits):
    key = (tuple(shape), bits)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_per_channel(make_input(shape), bits)
    return _ORACLE[key]


def restate(z, bits):
    """include/hnd_qchannel.h in numpy fp32, one correctly rounded operation per step, the constant-channel rule included"""
    x = z.numpy().astype(np.float32)
    f = np.float32
    qmax = f(2 ** bits - 1)
    c = x.shape[1]
    lo, hi, scale, zp = (np.empty(c, f) for _ in range(4))
    codes, deq = np.empty(x.shape, np.uint8), np.empty(x.shape, f)
    with np.errstate(all='ignore'):
        for ch in range(c):
            v = x[:, ch]
            lo[ch], hi[ch] = v.min(), v.max()
            if hi[ch] != lo[ch]:
                scale[ch] = f(hi[ch] - lo[ch]) / qmax
            else:
                scale[ch] = np.abs(lo[ch]) if lo[ch] != 0 else f(1)
            zp[ch] = np.trunc(np.clip(f(0) - lo[ch] / scale[ch], f(0), qmax))
            q = np.rint(np.clip(zp[ch] + v / scale[ch], f(0), qmax))                  # half to even
            assert q.dtype == f
            codes[:, ch] = q.astype(np.uint8)
            deq[:, ch] = scale[ch] * (q - zp[ch])
    t = torch.from_numpy
    return Quantised(t(codes), t(lo), t(hi), t(scale), t(zp), t(deq), bits)


def restated(shape, bits):
    key = (tuple(shape), bits)
    if key not in _RESTATED:
        _RESTATED[key] = restate(make_input(shape), bits)
    return _RESTATED[key]


def restate_per_tensor(z, bits):
    """include/hnd_codec.h in numpy fp32 (one scale for the tensor): the yardstick of the RMS comparison"""
    flat = restate(z.reshape(1, 1, -1, 1), bits)
    return flat.dequantized.view(z.shape)


def rms_error(z, deq):
    return float(torch.sqrt(((deq.double() - z.double()) ** 2).mean()))


def restate_stats(y, cs):
    """the `stats` of hnd_qchannel_fake_quantize_bits for the stored buffer y [npix, cs] (fp32), in the header's order: per
    tile of 128 rows and per channel, S = 64 / (cs / 4) row slots; slot s adds rows s, s + S, ... in ascending order onto +0
    (y * y rounded, then added), then the slot sums are added in ascending s onto +0.  Returns [tiles, 2, cs] fp32."""
    y = y.numpy().astype(np.float32).reshape(-1, cs)
    assert cs % 4 == 0 and cs <= 256
    slots = 64 // (cs // 4)
    npix = y.shape[0]
    nt = (npix + ROWS - 1) // ROWS
    out = np.zeros((nt, 2, cs), np.float32)
    for t in range(nt):
        blk = y[t * ROWS:(t + 1) * ROWS]
        for k, vals in enumerate((blk, blk * blk)):
            total = np.zeros(cs, np.float32)
            for s in range(slots):
                acc = np.zeros(cs, np.float32)
                for r in range(s, blk.shape[0], slots):
                    acc = acc + vals[r]
                total = total + acc
            out[t, k] = total
    return torch.from_numpy(out)


# ---- the one-step comparison: tests/qat_util.py's estimator and preconditions, per channel
def quantize_dequantize_per_channel(z, bits):
    return torch.cat([dequantize_tensor(quantize_tensor(z[:, ch:ch + 1], num_bits=bits)) for ch in range(z.shape[1])], 1)


def ste_per_channel(z, bits):
    """the straight-through estimator: the forward value is the per-channel quantise -> dequantise, the backward the identity"""
    return z + (quantize_dequantize_per_channel(z, bits) - z).detach()


def decide_codes_per_channel(z, bits):
    """qat_util.decide_codes on every channel alone: a list of its dicts"""
    return [QU.decide_codes(z[:, ch:ch + 1], bits) for ch in range(z.shape[1])]


def check_preconditions_per_channel(caps32, caps64, what=''):
    """qat_util.check_preconditions on every channel; returns the smallest (half-integer, integer) margins over the channels
    and both oracles"""
    assert len(caps32) == len(caps64) > 0
    half, zp = [], []
    for ch, (a, b) in enumerate(zip(caps32, caps64)):
        m32, m64 = QU.check_preconditions(a, b, '%s, channel %d' % (what, ch))
        half += [m32[0], m64[0]]
        zp += [m32[1], m64[1]]
    return min(half), min(zp)
