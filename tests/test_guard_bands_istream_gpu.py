"""GPU: the exports of include/hnd_istream.h stay inside the buffers the header sizes -- the guard ledger of that header.

As tests/test_guard_bands_entropy_gpu.py does for include/hnd_entropy.h: every buffer of a call (the one-value-per-byte NHWC
codes, hist of exactly n * 256 words, lengths of exactly n * 256 bytes, the payload of exactly hnd_istream_capacity bytes,
offsets of exactly n * cpi + 1 words, scratch of exactly hnd_istream_scratch_bytes bytes, qparams of n * 4 floats, the NHWC
destination) is a view of exactly its stated size inside ONE tests/guard_util.Arena filled with 0xFF; the launches, then
ops.sync_check(), then arena.check() (no guard byte changed); the results are at the bit-exact bar of
tests/test_istream_gpu.py.  Only well-formed tables and streams are used.  Importing this module does not touch the GPU."""
import numpy as np
import pytest
import torch

from tests import entropy_util as EU
from tests import guard_util as G
from tests import istream_util as IU

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

LEDGER = {}          # test function name -> exports of include/hnd_istream.h whose device writes it guards


def covers(*exports):
    def deco(fn):
        LEDGER.setdefault(fn.__name__, set()).update(exports)
        return fn
    return deco


# exports that write no device memory a caller owns: nothing to guard
NO_DEVICE_OUTPUT = {
    'hnd_istream_abi': 'constant',
    'hnd_istream_chunks_per_image': 'size query',
    'hnd_istream_capacity': 'size query',
    'hnd_istream_scratch_bytes': 'size query',
}

F32, U8, I32 = torch.float32, torch.uint8, torch.int32


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


def _codes(shape, cs, bits):
    """(codes uint8 NHWC with zero pad channels, per-image flat symbols, qparams [n, 4]): the input quantised on the host,
    image i on a range of its own -- any codes do, the kernels under test start from the bytes"""
    n, c, h, w = shape
    z = IU.make_input(shape).numpy()
    qmax = np.float32((1 << bits) - 1)
    q = np.zeros((n, h, w, cs), dtype=np.uint8)
    qparams = np.zeros((n, 4), dtype=np.float32)
    for i in range(n):
        lo, hi = z[i].min(), z[i].max()
        scale = np.float32(hi - lo) / qmax
        zp = np.trunc(np.clip(-lo / scale, 0, qmax)).astype(np.float32)
        q[i, :, :, :c] = np.rint(np.clip(zp + z[i] / scale, 0, qmax)).astype(np.uint8).transpose(1, 2, 0)
        qparams[i] = (lo, hi, scale, zp)
    return q, IU.image_symbols(q, c), qparams


@covers('hnd_istream_histogram', 'hnd_istream_build_tables', 'hnd_istream_encode', 'hnd_istream_decode_dequantize')
@pytest.mark.parametrize('shape,cs,bits', IU.GUARD_CASES)
def test_every_export_stays_inside_its_buffers(ops, shape, cs, bits):
    from hnd_ghnd_object_detectors_amd.structure.transformer import huffman_lengths
    n, c, h, w = shape
    chw = c * h * w
    q_np, symbols, qp_np = _codes(shape, cs, bits)
    cpi, cap, nscratch = ops.istream_chunks_per_image(chw), ops.istream_capacity(n, chw), ops.istream_scratch_bytes(n, chw)
    assert (cpi, cap, nscratch) == (IU.chunks_per_image(chw), IU.capacity(n, chw), IU.scratch_bytes(n, chw))
    specs = [(q_np.shape, U8), ((n, 256), I32), ((n, 256), U8), ((cap,), U8), ((n * cpi + 1,), I32), ((nscratch,), U8),
             ((n, 4), F32), ((n, h, w, cs), F32)]
    arena = G.Arena(DEV, G.arena_bytes(specs))
    q = arena.load('q', torch.from_numpy(q_np))
    hist = arena.take('hist', (n, 256), I32)
    lengths = arena.take('lengths', (n, 256), U8)
    payload = arena.take('payload', (cap,), U8)
    offsets = arena.take('offsets', (n * cpi + 1,), I32)
    scratch = arena.take('scratch', (nscratch,), U8)
    qp = arena.load('qparams', torch.from_numpy(qp_np))
    x = arena.take('x', (n, h, w, cs))                                            # starts as 0xFF: every float a NaN
    ops.istream_histogram(q, c, bits, hist)
    ops.istream_build_tables(hist, bits, lengths)
    ops.istream_encode(q, c, bits, lengths, payload, offsets, scratch)
    ops.istream_decode_dequantize(payload, offsets, lengths, qp, x, c, bits)
    ops.sync_check()
    arena.check()
    assert np.array_equal(q.cpu().numpy(), q_np) and np.array_equal(qp.cpu().numpy().view(np.int32), qp_np.view(np.int32))
    got_payload, got_offsets = payload.cpu().numpy(), offsets.cpu().numpy().view(np.uint32).astype(np.int64)
    for i in range(n):
        assert np.array_equal(hist[i].cpu().numpy(), np.bincount(symbols[i], minlength=256)), i
        table = huffman_lengths(np.bincount(symbols[i], minlength=256).tolist(), bits)
        assert lengths[i].cpu().numpy().tobytes() == table + bytes(256 - len(table)), i
        want_payload, want_offsets = EU.encode(symbols[i], table)
        lo, hi = got_offsets[i * cpi], got_offsets[(i + 1) * cpi]
        assert np.array_equal(got_offsets[i * cpi:(i + 1) * cpi + 1] - lo, want_offsets), i
        assert got_payload[lo:hi].tobytes() == want_payload.tobytes(), i
    assert (got_payload[got_offsets[-1]:] == G.FILL).all()                        # nothing at or beyond the end is written
    want = np.zeros((n, h, w, cs), dtype=np.float32)
    for i in range(n):                                                            # one fp32 subtraction, one fp32 multiplication
        want[i, :, :, :c] = qp_np[i, 2] * (q_np[i, :, :, :c].astype(np.float32) - qp_np[i, 3])
    assert np.array_equal(x.cpu().numpy().view(np.int32), want.view(np.int32))
