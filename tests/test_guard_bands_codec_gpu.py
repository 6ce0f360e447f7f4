"""GPU: the exports of include/hnd_codec.h stay inside the buffers the header sizes -- the guard ledger of that header.

As tests/test_guard_bands_gpu.py does for include/hnd_hip.h: every buffer of a launch (the NHWC source or destination, the
one-value-per-byte q, the packed payload of exactly hnd_codec_packed_bytes bytes, qparams, scratch) is a view of exactly
its stated size inside ONE tests/guard_util.Arena filled with 0xFF; the launches, then ops.sync_check(), then
arena.check() (no guard byte changed); the source is unchanged and the results are at the byte-exact bar of
tests/test_codec_bits_gpu.py (an over-read would show in them: 0xFF is a NaN as fp32 and 255 as a byte).
tests/test_codec_bits_cpu.py holds LEDGER, with NO_DEVICE_OUTPUT, to _lib.CODEC_SYMBOLS.  Importing this module does not
touch the GPU."""
import pytest
import torch

from tests import codec_util as CU
from tests import guard_util as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

LEDGER = {}          # test function name -> exports of include/hnd_codec.h whose device writes it guards


def covers(*exports):
    def deco(fn):
        LEDGER.setdefault(fn.__name__, set()).update(exports)
        return fn
    return deco


# exports that write no device memory a caller owns: nothing to guard
NO_DEVICE_OUTPUT = {
    'hnd_codec_abi': 'constant',
    'hnd_codec_packed_bytes': 'size query',
}

SHAPES = [(1, 3, 1, 1), (1, 3, 5, 7), (2, 3, 13, 17)]       # only a tail group; a tail of one value; a tail of six
WIDTHS = [1, 3, 5, 8]
SHIFT = 0.3


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


def _qparams_ok(qp, ref):
    return [float(v) for v in qp.cpu()] == [ref.lo, ref.hi, ref.scale, ref.zero_point]


@covers('hnd_quantize_bits')
@pytest.mark.parametrize('bits', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES)
def test_quantize_bits_stays_inside_its_buffers(ops, shape, bits):
    n, c, h, w = shape
    cs = ops.chan_pad_of(c)
    z, ref = CU.make_input(shape, SHIFT), CU.reference(shape, SHIFT, bits)
    src = CU.nhwc_buffer(z, cs, 'cpu')
    f32, u8 = torch.float32, torch.uint8
    arena = G.Arena(DEV, G.arena_bytes([((n, h, w, cs), f32), ((n, h, w, cs), u8), ((4,), f32),
                                        ((ops.minmax_scratch_elems(),), f32)]))
    x = arena.load('x', src)
    q = arena.take('q', (n, h, w, cs), u8)
    qp = arena.take('qparams', (4,))
    scratch = arena.take('scratch', (ops.minmax_scratch_elems(),))
    ops.quantize_bits(x, c, bits, q, qp, scratch)
    ops.sync_check()
    arena.check()
    assert torch.equal(x.cpu(), src)                                      # the source is read only
    assert _qparams_ok(qp, ref)
    assert torch.equal(CU.logical(q, c), ref.bytes) and int(q[..., c:].max()) == 0


@covers('hnd_quantize_pack_bits')
@pytest.mark.parametrize('bits', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES)
def test_quantize_pack_bits_stays_inside_a_payload_of_exactly_the_packed_size(ops, shape, bits):
    n, c, h, w = shape
    cs = ops.chan_pad_of(c)
    z, ref = CU.make_input(shape, SHIFT), CU.reference(shape, SHIFT, bits)
    src = CU.nhwc_buffer(z, cs, 'cpu')
    nbytes = ops.codec_packed_bytes(z.numel(), bits)
    assert nbytes == (z.numel() * bits + 7) // 8
    f32, u8 = torch.float32, torch.uint8
    arena = G.Arena(DEV, G.arena_bytes([((n, h, w, cs), f32), ((nbytes,), u8), ((4,), f32),
                                        ((ops.minmax_scratch_elems(),), f32)]))
    x = arena.load('x', src)
    payload = arena.take('payload', (nbytes,), u8)
    qp = arena.take('qparams', (4,))
    scratch = arena.take('scratch', (ops.minmax_scratch_elems(),))
    ops.quantize_pack_bits(x, c, bits, payload, qp, scratch)
    ops.sync_check()
    arena.check()
    assert torch.equal(x.cpu(), src)
    assert _qparams_ok(qp, ref)
    assert payload.cpu().numpy().tobytes() == ref.payload.tobytes()


@covers('hnd_unpack_dequantize_bits')
@pytest.mark.parametrize('bits', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES)
def test_unpack_dequantize_bits_reads_the_exact_payload_and_fills_the_whole_destination(ops, shape, bits):
    n, c, h, w = shape
    cs = ops.chan_pad_of(c)
    ref = CU.reference(shape, SHIFT, bits)
    src = torch.from_numpy(ref.payload.copy())
    qp_host = torch.tensor([ref.lo, ref.hi, ref.scale, ref.zero_point], dtype=torch.float32)
    f32, u8 = torch.float32, torch.uint8
    arena = G.Arena(DEV, G.arena_bytes([((src.numel(),), u8), ((4,), f32), ((n, h, w, cs), f32)]))
    payload = arena.load('payload', src)
    qp = arena.load('qparams', qp_host)
    out = arena.take('x', (n, h, w, cs))                                  # starts as 0xFF: every float a NaN
    ops.unpack_dequantize_bits(payload, qp, out, c, bits)
    ops.sync_check()
    arena.check()
    assert torch.equal(payload.cpu(), src) and torch.equal(qp.cpu(), qp_host)
    assert not bool(torch.isnan(out).any())
    assert torch.equal(CU.logical(out, c), ref.dequantized)
    assert float(out[..., c:].abs().max()) == 0.0
