"""GPU: the exports of include/hnd_entropy.h stay inside the buffers the header sizes -- the guard ledger of that header.

As tests/test_guard_bands_qrange_gpu.py does for include/hnd_qrange.h: every buffer of a call (the one-value-per-byte NHWC
codes, hist of exactly 256 words, the payload of exactly hnd_entropy_capacity bytes, offsets of exactly nchunks + 1 words,
scratch of exactly hnd_entropy_scratch_bytes bytes, qparams of 4 floats, the NHWC destination) is a view of exactly its stated
size inside ONE tests/guard_util.Arena filled with 0xFF; the launches, then ops.sync_check(), then arena.check() (no guard byte
changed); the results are at the bit-exact bar of tests/test_entropy_gpu.py.  Only valid streams are used.  Importing this
module does not touch the GPU."""
import numpy as np
import pytest
import torch

from tests import entropy_util as EU
from tests import guard_util as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

LEDGER = {}          # test function name -> exports of include/hnd_entropy.h whose device writes it guards


def covers(*exports):
    def deco(fn):
        LEDGER.setdefault(fn.__name__, set()).update(exports)
        return fn
    return deco


# exports that write no device memory a caller owns: nothing to guard
NO_DEVICE_OUTPUT = {
    'hnd_entropy_abi': 'constant',
    'hnd_entropy_chunks': 'size query',
    'hnd_entropy_capacity': 'size query',
    'hnd_entropy_scratch_bytes': 'size query',
}

WIDTHS = [1, 3, 8]
SHAPES = [(2, 3, 7, 13), (1, 6, 5, 52)]          # a tail chunk and chunks across channels and images | cs = 8
F32, U8, I32 = torch.float32, torch.uint8, torch.int32


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


def _codes(shape, bits):
    """(codes uint8 NHWC with zero pad channels, flat logical symbols, qparams): the normal input on a range of +-4 about
    its mean, quantised on the host -- any codes do, the kernels under test start from the bytes"""
    n, c, h, w = shape
    z = EU.make_input(shape)
    qmax = (1 << bits) - 1
    scale = np.float32(8.0) / np.float32(qmax)
    logical = np.clip(np.rint((z.numpy() + 3.6) / scale), 0, qmax).astype(np.uint8)
    q = np.zeros((n, h, w, EU.stride_of(shape)), dtype=np.uint8)
    q[..., :c] = logical.transpose(0, 2, 3, 1)
    qparams = np.array([-3.6, 4.4, scale, np.trunc(np.float32(3.6) / scale)], dtype=np.float32)
    return q, logical.reshape(-1), qparams


@covers('hnd_code_histogram')
@pytest.mark.parametrize('bits', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES)
def test_histogram_stays_inside_its_buffers(ops, shape, bits):
    q_np, symbols, _ = _codes(shape, bits)
    arena = G.Arena(DEV, G.arena_bytes([(q_np.shape, U8), ((256,), I32)]))
    q = arena.load('q', torch.from_numpy(q_np))
    hist = arena.take('hist', (256,), I32)
    ops.code_histogram(q, shape[1], bits, hist)
    ops.sync_check()
    arena.check()
    assert np.array_equal(q.cpu().numpy(), q_np)                                  # the source is read only
    assert np.array_equal(hist.cpu().numpy(), np.bincount(symbols, minlength=256))


@covers('hnd_entropy_encode', 'hnd_entropy_decode_dequantize')
@pytest.mark.parametrize('bits', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES)
def test_encoder_and_decoder_stay_inside_their_buffers(ops, shape, bits):
    n, c, h, w = shape
    q_np, symbols, qp_np = _codes(shape, bits)
    cs, numel = q_np.shape[-1], symbols.size
    lengths = EU.valid_lengths(np.bincount(symbols, minlength=1 << bits).tolist(), bits)
    nchunks, cap, nscratch = ops.entropy_chunks(numel), ops.entropy_capacity(numel), ops.entropy_scratch_bytes(numel)
    assert (nchunks, cap, nscratch) == (EU.chunks(numel), EU.capacity(numel), 4 * EU.chunks(numel))
    specs = [(q_np.shape, U8), ((cap,), U8), ((nchunks + 1,), I32), ((nscratch,), U8), ((4,), F32), ((n, h, w, cs), F32)]
    arena = G.Arena(DEV, G.arena_bytes(specs))
    q = arena.load('q', torch.from_numpy(q_np))
    payload = arena.take('payload', (cap,), U8)
    offsets = arena.take('offsets', (nchunks + 1,), I32)
    scratch = arena.take('scratch', (nscratch,), U8)
    qp = arena.load('qparams', torch.from_numpy(qp_np))
    x = arena.take('x', (n, h, w, cs))                                            # starts as 0xFF: every float a NaN
    ops.entropy_encode(q, c, bits, lengths, payload, offsets, scratch)
    ops.entropy_decode_dequantize(payload, offsets, lengths, qp, x, c, bits)
    ops.sync_check()
    arena.check()
    want_payload, want_offsets = EU.encode(symbols, lengths)
    assert np.array_equal(q.cpu().numpy(), q_np) and np.array_equal(qp.cpu().numpy().view(np.int32), qp_np.view(np.int32))
    assert np.array_equal(offsets.cpu().numpy().view(np.uint32), want_offsets)
    got = payload.cpu().numpy()
    assert got[:want_payload.size].tobytes() == want_payload.tobytes()
    assert (got[want_payload.size:] == G.FILL).all()                              # nothing at or beyond offsets[nchunks] is written
    want = np.zeros((n, h, w, cs), dtype=np.float32)
    want[..., :c] = qp_np[2] * (q_np[..., :c].astype(np.float32) - qp_np[3])     # one fp32 subtraction, one fp32 multiplication
    assert np.array_equal(x.cpu().numpy().view(np.int32), want.view(np.int32))
