"""Shared by the tests of include/hnd_codec.h (tests/test_codec_bits_gpu.py, tests/test_guard_bands_codec_gpu.py): seeded
inputs, the oracle's answer per (input, width) computed ONCE and kept (never modified: callers compare, they do not write),
and the payload format of the header restated on the host with numpy.packbits.

A plain module: no fixtures, no pytest settings; importing it loads neither the library nor the launch helpers."""
import numpy as np
import torch

from oracle.myutils_r import dequantize_tensor, quantize_tensor

_INPUTS = {}
_REFERENCES = {}


def make_input(shape, shift):
    """logical NCHW fp32 tensor with max > min, the recipe of test_bottleneck_codec_matches_myutils_semantics: shift 0.3
    straddles zero, shift 5.0 is nearly all positive (the zeros of the pad channels must not count as the minimum)"""
    key = (tuple(shape), float(shift))
    if key not in _INPUTS:
        n, c, h, w = shape
        z = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(15 + c)) * 3 + shift
        if h * w * n == 1:
            z[0, 1:] += 2.0                                        # a single pixel still has max > min
        assert float(z.max()) > float(z.min())
        _INPUTS[key] = z
    return _INPUTS[key]


class Reference(object):
    """what oracle/myutils_r.py makes of z at `bits`: .bytes (uint8 NCHW), .scale, .zero_point (floats), .dequantized
    (fp32 NCHW), .lo / .hi (z.min() / z.max()), .payload (numpy uint8: the packed bytes of the header's format)"""

    def __init__(self, z, bits):
        q = quantize_tensor(z.clone(), num_bits=bits)
        self.bytes, self.scale, self.zero_point = q.tensor, float(q.scale), float(q.zero_point)
        self.dequantized = dequantize_tensor(q)
        self.lo, self.hi = float(z.min()), float(z.max())
        self.payload = host_pack(q.tensor, bits)


def reference(shape, shift, bits):
    key = (tuple(shape), float(shift), bits)
    if key not in _REFERENCES:
        _REFERENCES[key] = Reference(make_input(shape, shift), bits)
    return _REFERENCES[key]


def host_pack(values, bits):
    """include/hnd_codec.h, payload format: the values of the logical NCHW tensor in index order, each as its `bits` bits
    least significant first, the bit stream cut into bytes least significant bit first (zero bits fill the last byte)"""
    v = values.contiguous().view(-1).numpy()
    assert v.dtype == np.uint8 and (bits == 8 or int(v.max()) < (1 << bits))
    stream = ((v[:, None] >> np.arange(bits, dtype=np.uint8)[None, :]) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(stream, bitorder='little')


def host_unpack(payload, shape, bits):
    """the inverse of host_pack: uint8 tensor of `shape`"""
    numel = int(np.prod(shape))
    payload = np.asarray(payload, dtype=np.uint8)
    assert payload.size == (numel * bits + 7) // 8
    stream = np.unpackbits(payload, bitorder='little')
    assert not stream[numel * bits:].any(), 'the unused high bits of the last byte are not 0'
    v = (stream[:numel * bits].reshape(numel, bits).astype(np.uint16) << np.arange(bits, dtype=np.uint16)[None, :]).sum(1)
    return torch.from_numpy(v.astype(np.uint8)).view(*shape)


def nhwc_buffer(z, cs, device):
    """the NHWC fp32 buffer of stride cs the kernels read: the c real channels of z, zeros in the pad channels"""
    n, c, h, w = z.shape
    buf = torch.zeros(n, h, w, cs)
    buf[..., :c] = z.permute(0, 2, 3, 1)
    return buf.to(device)


def logical(buf, c):
    """NCHW view of the c real channels of an NHWC buffer, on the host"""
    return buf.cpu()[..., :c].permute(0, 3, 1, 2)
