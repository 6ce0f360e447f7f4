"""Shared by the tests of quantisation-aware distillation (tests/test_fake_quant_cpu.py, tests/test_fake_quant_gpu.py): the
oracle's student layer 1 restated with a straight-through fake quantiser between encoder and decoder, and the preconditions
under which a HIP step may be held to the oracle's rounding decisions.

A plain module: no fixtures, no pytest settings; importing it loads neither the library nor the launch helpers, and oracle/
is not edited -- the tests put ``make_student_layer1(bits)`` in the place of ``O.student_layer1`` with monkeypatch."""
import torch
import torch.nn.functional as F

from oracle import hnd_oracle as O
from oracle.myutils_r import quantize_tensor

MARGIN = 1e-4          # distance, in code units, every rounding decision must keep from its tie (the issue's figure)
# (fixture, width) pairs of the one-step comparison; tests/test_fake_quant_cpu.py holds the oracle alone to the
# preconditions on every pair, so the GPU comparison never hinges on a tie.  Chosen from the oracle alone: tiny_ghnd_faster
# at 4 bits has a value 9.0e-5 from a half-integer and is therefore NOT used; its nearest tie at 2 bits is 3.7e-4 away, and
# tiny_ghnd_faster_b6 (6 bottleneck channels: the 32-float pixel stride) at 4 bits keeps 4.4e-4
ONE_STEP_CASES = [('tiny_ghnd_faster', 2), ('tiny_ghnd_faster_b6', 4)]


def ste(z, bits):
    """the straight-through estimator: the forward value is quantise -> dequantise, the backward is the identity"""
    return z + (O.quantize_dequantize(z, bits) - z).detach()


def make_student_layer1(bits, capture=None, fake_quant=None):
    """O.student_layer1 with ``x = ste(x, bits)`` before the decoder when training.  capture: a dict that receives, under
    the dtype of the run, what decide_codes() makes of the unquantised bottleneck tensor.  fake_quant: a callable that
    stands in for ste (the sanity test of the estimator passes ``z + const``)."""
    fq = fake_quant if fake_quant is not None else (lambda z: ste(z, bits))

    def student_layer1(x, sd, training=True, update_buffers=True, intermediates=None, codec_bits=None, hooked=None):
        for prefix, spec in ((O.B + 'layer1.encoder.encoder.', O.ENCODER_SPEC), (O.B + 'layer1.decoder.', O.DECODER_SPEC)):
            if spec is O.DECODER_SPEC and hooked is not None:
                hooked['layer1.encoder'] = x
            if spec is O.DECODER_SPEC and codec_bits is not None and not training:
                x = O.quantize_dequantize(x, codec_bits)
            if spec is O.DECODER_SPEC and training:
                if capture is not None:
                    capture[x.dtype] = decide_codes(x.detach(), bits)
                x = fq(x)
            for op in spec:
                name = '%s%d' % (prefix, op[1])
                if op[0] == 'conv':
                    x = F.conv2d(x, sd[name + '.weight'], None, stride=1, padding=op[2])
                elif op[0] == 'bn':
                    x = O._train_bn(x, sd, name + '.', training, update_buffers)
                else:
                    x = F.relu(x)
                if intermediates is not None:
                    intermediates[name] = x
        return x
    return student_layer1


def decide_codes(z, bits):
    """the quantiser's decisions on z (oracle/myutils_r.quantize_tensor): dict(z, codes uint8, scale, zero_point, and the
    two quantities that are rounded: pre = zero_point + z / scale (round half to even) and zp_raw = -min / scale (int()))"""
    q = quantize_tensor(z.clone(), num_bits=bits)
    scale = q.scale
    return {'z': z.clone(), 'codes': q.tensor, 'scale': float(scale), 'zero_point': int(q.zero_point),
            'pre': (q.zero_point + z / scale).double(), 'zp_raw': float(0.0 - z.min() / scale), 'dtype': z.dtype}


def tie_margins(cap):
    """(distance of the nearest pre-rounding value from a half-integer, distance of -min / scale from an integer)"""
    pre = cap['pre']
    half = float(((pre - torch.floor(pre)) - 0.5).abs().min())
    zp = abs(cap['zp_raw'] - round(cap['zp_raw']))
    return half, zp


def check_preconditions(cap32, cap64, what=''):
    """the issue's preconditions: the fp32 and the fp64 oracle take the same decision for every element, and no decision
    of either sits within MARGIN of its tie"""
    assert cap32['codes'].shape == cap64['codes'].shape
    differ = int((cap32['codes'] != cap64['codes']).sum())
    assert differ == 0, '%s: %d codes differ between the fp32 and the fp64 oracle' % (what, differ)
    assert cap32['zero_point'] == cap64['zero_point'], (what, cap32['zero_point'], cap64['zero_point'])
    for cap in (cap32, cap64):
        half, zp = tie_margins(cap)
        assert half >= MARGIN, '%s (%s): a value lies %.3e from a half-integer' % (what, cap['dtype'], half)
        # (a zero point clamped to 0 or qmax is decided by the clamp, at any distance: not the case at any pair in use)
        assert zp >= MARGIN, '%s (%s): -min / scale lies %.3e from an integer' % (what, cap['dtype'], zp)
    return tie_margins(cap32), tie_margins(cap64)
