"""GPU: every export of include/hnd_qimage.h that writes device memory stays inside the buffers the header sizes -- the
guard ledger of that header (tests/test_qimage_cpu.py holds it against the header's declarations).

As tests/test_guard_bands_codec_gpu.py does for include/hnd_codec.h: every buffer of a call (the NHWC source, q of npix * cs
bytes, the payload of hnd_codec_packed_bytes bytes, qparams of n * 4 floats, scratch of hnd_qimage_scratch_elems(n)
floats, stats of hnd_fake_quantize_tiles(npix) * 2 * cs floats) is a view of exactly its stated size inside ONE
tests/guard_util.Arena filled with 0xFF; the launches, then ops.sync_check(), then arena.check() (no guard byte changed); the
results are at the bit-exact bar of tests/test_qimage_gpu.py (an over-read would show in them: 0xFF is a NaN as fp32).
Importing this module does not touch the GPU."""
import pytest
import torch

from tests import codec_util as CU
from tests import guard_util as G
from tests import qimage_util as QI

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

LEDGER = {}          # test function name -> exports of include/hnd_qimage.h whose device writes it guards


def covers(*exports):
    def deco(fn):
        LEDGER.setdefault(fn.__name__, set()).update(exports)
        return fn
    return deco


# exports that write no device memory a caller owns: nothing to guard
NO_DEVICE_OUTPUT = {
    'hnd_qimage_abi': 'constant',
    'hnd_qimage_scratch_elems': 'size query',
}

CASES = [(shape, cs, bits) for shape, cs in QI.GUARD_SHAPES for bits in QI.GUARD_WIDTHS]
PAD_GARBAGE = 1.0e6             # what the pad channels of the SOURCE hold: never counted, never copied
f32, u8 = torch.float32, torch.uint8


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


def bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def source(shape, cs):
    n, c, h, w = shape
    buf = torch.full((n, h, w, cs), PAD_GARBAGE)
    buf[..., :c] = QI.make_input(shape).permute(0, 2, 3, 1)
    return buf


@covers('hnd_qimage_quantize_bits', 'hnd_qimage_dequantize_u8')
@pytest.mark.parametrize('shape,cs,bits', CASES)
def test_quantize_and_dequantize_stay_inside_their_buffers(ops, shape, cs, bits):
    n, c, h, w = shape
    ref = QI.restated(shape, bits)
    nscratch = ops.qimage_scratch_elems(n)
    specs = [((n, h, w, cs), f32), ((n, h, w, cs), u8), ((n, 4), f32), ((nscratch,), f32), ((n, h, w, cs), f32)]
    arena = G.Arena(DEV, G.arena_bytes(specs))
    src = source(shape, cs)
    x = arena.load('x', src)
    q = arena.take('q', (n, h, w, cs), u8)
    qp = arena.take('qparams', (n, 4))
    scratch = arena.take('scratch', (nscratch,))
    out = arena.take('out', (n, h, w, cs))                                 # starts as 0xFF: every float a NaN
    ops.qimage_quantize_bits(x, c, bits, q, qp, scratch)
    ops.qimage_dequantize_u8(q, qp, out, c)
    ops.sync_check()
    arena.check()
    assert torch.equal(x.cpu(), src)                                      # the source is read only
    assert torch.equal(CU.logical(q, c), ref.codes) and torch.equal(bits_of(qp), bits_of(ref.qparams))
    assert torch.equal(bits_of(CU.logical(out, c)), bits_of(ref.dequantized))
    if cs > c:
        assert int(q[..., c:].max()) == 0 and float(out[..., c:].abs().max()) == 0.0
    assert not bool(torch.isnan(out).any())


@covers('hnd_qimage_quantize_pack_bits', 'hnd_qimage_unpack_dequantize_bits')
@pytest.mark.parametrize('shape,cs,bits', CASES)
def test_pack_and_unpack_stay_inside_their_buffers(ops, shape, cs, bits):
    n, c, h, w = shape
    ref = QI.restated(shape, bits)
    nscratch, nbytes = ops.qimage_scratch_elems(n), ops.codec_packed_bytes(n * c * h * w, bits)
    assert nbytes == ref.payload.size
    specs = [((n, h, w, cs), f32), ((nbytes,), u8), ((n, 4), f32), ((nscratch,), f32), ((n, h, w, cs), f32)]
    arena = G.Arena(DEV, G.arena_bytes(specs))
    src = source(shape, cs)
    x = arena.load('x', src)
    payload = arena.take('payload', (nbytes,), u8)
    qp = arena.take('qparams', (n, 4))
    scratch = arena.take('scratch', (nscratch,))
    out = arena.take('out', (n, h, w, cs))
    ops.qimage_quantize_pack_bits(x, c, bits, payload, qp, scratch)
    ops.qimage_unpack_dequantize_bits(payload, qp, out, c, bits)
    ops.sync_check()
    arena.check()
    assert torch.equal(x.cpu(), src)
    assert torch.equal(payload.cpu(), torch.from_numpy(ref.payload)) and torch.equal(bits_of(qp), bits_of(ref.qparams))
    assert torch.equal(bits_of(CU.logical(out, c)), bits_of(ref.dequantized))
    if cs > c:
        assert float(out[..., c:].abs().max()) == 0.0
    assert not bool(torch.isnan(out).any())


@covers('hnd_qimage_fake_quantize_bits')
@pytest.mark.parametrize('with_stats', [False, True])
@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('shape,cs,bits', CASES)
def test_fake_quantize_stays_inside_its_buffers(ops, shape, cs, bits, in_place, with_stats):
    n, c, h, w = shape
    npix = n * h * w
    ref = QI.restated(shape, bits)
    nscratch, nt = ops.qimage_scratch_elems(n), ops.fake_quantize_tiles(npix)
    specs = [((n, h, w, cs), f32), ((n, 4), f32), ((nscratch,), f32)]
    specs += [] if in_place else [((n, h, w, cs), f32)]
    specs += [((nt, 2, cs), f32)] if with_stats else []
    arena = G.Arena(DEV, G.arena_bytes(specs))
    src = source(shape, cs)
    x = arena.load('x', src)
    qp = arena.take('qparams', (n, 4))
    scratch = arena.take('scratch', (nscratch,))
    out = x if in_place else arena.take('y', (n, h, w, cs))
    stats = arena.take('stats', (nt, 2, cs)) if with_stats else None
    ops.qimage_fake_quantize_bits(x, c, bits, qp, scratch, out=None if in_place else out, stats=stats)
    ops.sync_check()
    arena.check()
    if not in_place:
        assert torch.equal(x.cpu(), src)
    assert torch.equal(bits_of(CU.logical(out, c)), bits_of(ref.dequantized))
    assert torch.equal(bits_of(qp), bits_of(ref.qparams))
    if cs > c:
        assert float(out[..., c:].abs().max()) == 0.0
    if with_stats:
        assert torch.equal(bits_of(stats), bits_of(QI.restate_stats(out.cpu().view(npix, cs), cs)))


def test_the_ledger_covers_every_export_of_the_header():
    """the rule of tests/test_guard_ledger_cpu.py for include/hnd_qimage.h: no export without a guard case"""
    from hnd_ghnd_object_detectors_amd import _lib
    covered = set().union(*LEDGER.values())
    assert len(covered) == 5 and not covered & set(NO_DEVICE_OUTPUT)
    assert covered | set(NO_DEVICE_OUTPUT) == set(_lib.QIMAGE_SYMBOLS)
