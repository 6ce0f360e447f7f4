"""GPU: hnd_fake_quantize_bits stays inside the buffers include/hnd_qat.h sizes -- the guard ledger of that header.

As tests/test_guard_bands_codec_gpu.py does for include/hnd_codec.h: every buffer of the call (the NHWC source, the
destination when it is not the source, qparams of 4 floats, scratch of hnd_minmax_scratch_elems() floats, stats of exactly
hnd_fake_quantize_tiles(npix) * 2 * cs floats) is a view of exactly its stated size inside ONE tests/guard_util.Arena filled
with 0xFF; the launches, then ops.sync_check(), then arena.check() (no guard byte changed); the results are at the bit-exact
bar of tests/test_fake_quant_gpu.py (an over-read would show in them: 0xFF is a NaN as fp32).  Importing this module does
not touch the GPU."""
import pytest
import torch

from tests import guard_util as G
from tests.test_fake_quant_gpu import SHAPES, bits_of, codec_pair, make_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

LEDGER = {}          # test function name -> exports of include/hnd_qat.h whose device writes it guards


def covers(*exports):
    def deco(fn):
        LEDGER.setdefault(fn.__name__, set()).update(exports)
        return fn
    return deco


# exports that write no device memory a caller owns: nothing to guard
NO_DEVICE_OUTPUT = {
    'hnd_qat_abi': 'constant',
    'hnd_fake_quantize_tiles': 'size query',
}

WIDTHS = [1, 3, 5, 8]


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


@covers('hnd_fake_quantize_bits')
@pytest.mark.parametrize('with_stats', [False, True])
@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('bits', WIDTHS)
@pytest.mark.parametrize('c,cs,nhw', SHAPES)
def test_fake_quantize_bits_stays_inside_its_buffers(ops, c, cs, nhw, bits, in_place, with_stats):
    n, h, w = nhw
    npix = n * h * w
    src = make_input(c, cs, nhw)
    nt = ops.fake_quantize_tiles(npix)
    f32 = torch.float32
    specs = [((n, h, w, cs), f32), ((4,), f32), ((ops.minmax_scratch_elems(),), f32)]
    specs += [] if in_place else [((n, h, w, cs), f32)]
    specs += [((nt, 2, cs), f32)] if with_stats else []
    arena = G.Arena(DEV, G.arena_bytes(specs))
    x = arena.load('x', src)
    qp = arena.take('qparams', (4,))
    scratch = arena.take('scratch', (ops.minmax_scratch_elems(),))
    out = x if in_place else arena.take('y', (n, h, w, cs))               # starts as 0xFF: every float a NaN
    stats = arena.take('stats', (nt, 2, cs)) if with_stats else None
    ref, ref_qp = codec_pair(ops, src.to(DEV), c, bits)
    ops.fake_quantize_bits(x, c, bits, qp, scratch, out=None if in_place else out, stats=stats)
    ops.sync_check()
    arena.check()
    if not in_place:
        assert torch.equal(x.cpu(), src)                                  # the source is read only
    assert torch.equal(bits_of(out), bits_of(ref)) and torch.equal(bits_of(qp), bits_of(ref_qp))
    assert float(out[..., c:].abs().max()) == 0.0
    if with_stats:
        assert not bool(torch.isnan(stats).any())                         # every row of exactly nt was written
        # (the sums themselves are held tile by tile in tests/test_fake_quant_gpu.py; here: no NaN from a guard got in)
        flat = out.double().view(npix, cs).cpu()
        err = (stats[:, 0].double().sum(0).cpu() - flat.sum(0)).abs()
        assert bool((err <= 128 * 2.0 ** -24 * flat.abs().sum(0)).all())


def test_the_ledger_covers_every_export_of_the_header():
    """the rule of tests/test_guard_ledger_cpu.py for include/hnd_qat.h: no export without a guard case"""
    from hnd_ghnd_object_detectors_amd import _lib
    covered = set().union(*LEDGER.values())
    assert covered == {'hnd_fake_quantize_bits'} and not covered & set(NO_DEVICE_OUTPUT)
    assert covered | set(NO_DEVICE_OUTPUT) == set(_lib.QAT_SYMBOLS)
