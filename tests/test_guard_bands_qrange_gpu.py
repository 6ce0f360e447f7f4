"""GPU: the exports of include/hnd_qrange.h stay inside the buffers the header sizes -- the guard ledger of that header.

As tests/test_guard_bands_qat_gpu.py does for include/hnd_qat.h: every buffer of a call (the NHWC source, the destination
when it is not the source, the clip mask of exactly npix * cs / 4 bytes, qparams and state of 4 floats, scratch of
hnd_minmax_scratch_elems() floats, stats of exactly hnd_fake_quantize_tiles(npix) * 2 * cs floats, the one-value-per-byte q,
the packed payload of exactly hnd_codec_packed_bytes bytes) is a view of exactly its stated size inside ONE
tests/guard_util.Arena filled with 0xFF; the launches, then ops.sync_check(), then arena.check() (no guard byte changed); the
results are at the bit-exact bar of tests/test_qrange_gpu.py (an over-read would show in them: 0xFF is a NaN as fp32, and
every bit of a mask byte).  Importing this module does not touch the GPU."""
import numpy as np
import pytest
import torch

from tests import guard_util as G
from tests import qrange_util as R
from tests.test_qrange_gpu import SHAPES, bits_of, literal_range, make_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

LEDGER = {}          # test function name -> exports of include/hnd_qrange.h whose device writes it guards


def covers(*exports):
    def deco(fn):
        LEDGER.setdefault(fn.__name__, set()).update(exports)
        return fn
    return deco


# exports that write no device memory a caller owns: nothing to guard
NO_DEVICE_OUTPUT = {
    'hnd_qrange_abi': 'constant',
}

WIDTHS = [1, 3, 8]
F32, U8 = torch.float32, torch.uint8


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


def _source(c, cs, npix, bits):
    lo, hi = literal_range(bits, False)
    return make_input(c, cs, npix, bits, False), lo, hi, R.qparams_np(lo, hi, bits)


@covers('hnd_fake_quantize_range', 'hnd_qrange_qparams')
@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('bits', WIDTHS)
@pytest.mark.parametrize('c,cs,npix', SHAPES)
def test_fake_quantize_range_stays_inside_its_buffers(ops, c, cs, npix, bits, in_place):
    src, lo, hi, qp_ref = _source(c, cs, npix, bits)
    nt = ops.fake_quantize_tiles(npix)
    specs = [((1, 1, npix, cs), F32), ((4,), F32), ((1, 1, npix, cs // 4), U8), ((nt, 2, cs), F32)]
    specs += [] if in_place else [((1, 1, npix, cs), F32)]
    arena = G.Arena(DEV, G.arena_bytes(specs))
    x = arena.load('x', torch.from_numpy(src).view(1, 1, npix, cs))
    qp = arena.take('qparams', (4,))
    mask = arena.take('mask', (1, 1, npix, cs // 4), U8)                  # starts as 0xFF: every bit set
    stats = arena.take('stats', (nt, 2, cs))
    out = x if in_place else arena.take('y', (1, 1, npix, cs))            # starts as 0xFF: every float a NaN
    ops.qrange_qparams(lo, hi, bits, qp)
    ops.fake_quantize_range(x, c, bits, qp, out=None if in_place else out, mask=mask, stats=stats)
    ops.sync_check()
    arena.check()
    y_ref, mask_ref, _ = R.fake_quantize_range_np(src, c, bits, qp_ref)
    if not in_place:
        assert torch.equal(bits_of(x.view(npix, cs)), bits_of(src))       # the source is read only
    assert torch.equal(bits_of(qp), bits_of(qp_ref))                      # ... and so are the qparams
    assert torch.equal(bits_of(out.view(npix, cs)), bits_of(y_ref))
    assert np.array_equal(mask.view(npix, cs // 4).cpu().numpy(), mask_ref)
    assert not bool(torch.isnan(stats).any())                             # every row of exactly nt was written
    flat = torch.from_numpy(y_ref).double()
    err = (stats[:, 0].double().sum(0).cpu() - flat.sum(0)).abs()
    assert bool((err <= 128 * 2.0 ** -24 * flat.abs().sum(0)).all())


@covers('hnd_qrange_observe')
@pytest.mark.parametrize('c,cs,npix', SHAPES)
def test_observe_stays_inside_its_buffers(ops, c, cs, npix):
    bits, momentum = 4, 0.25
    src, _, _, _ = _source(c, cs, npix, bits)
    specs = [((1, 1, npix, cs), F32), ((4,), F32), ((4,), F32), ((ops.minmax_scratch_elems(),), F32)]
    arena = G.Arena(DEV, G.arena_bytes(specs))
    x = arena.load('x', torch.from_numpy(src).view(1, 1, npix, cs))
    state = arena.take('state', (4,), fill=0)
    qp = arena.take('qparams', (4,))
    scratch = arena.take('scratch', (ops.minmax_scratch_elems(),))
    state_np = np.zeros(4, dtype=np.float32)
    for _ in range(2):
        ops.qrange_observe(x, c, bits, momentum, state, qp, scratch)
        state_np, qp_np = R.observe_np(state_np, src, c, momentum, bits)
    ops.sync_check()
    arena.check()
    assert torch.equal(bits_of(x.view(npix, cs)), bits_of(src))
    assert torch.equal(bits_of(state), bits_of(state_np)) and torch.equal(bits_of(qp), bits_of(qp_np))


@covers('hnd_qrange_mask_grad')
@pytest.mark.parametrize('c,cs,npix', SHAPES)
def test_mask_grad_stays_inside_its_buffers(ops, c, cs, npix):
    g = torch.Generator().manual_seed(c + npix)
    grad = torch.randn(1, 1, npix, cs, generator=g)
    mask_host = torch.randint(0, 256, (1, 1, npix, cs // 4), generator=g, dtype=U8)
    arena = G.Arena(DEV, G.arena_bytes([((1, 1, npix, cs), F32), ((1, 1, npix, cs // 4), U8)]))
    gd = arena.load('g', grad)
    mask = arena.load('mask', mask_host)
    ops.qrange_mask_grad(gd, mask, c)
    ops.sync_check()
    arena.check()
    keep = torch.from_numpy(R.mask_bits(mask_host.view(npix, -1).numpy(), c))
    want = grad.view(npix, cs).clone()
    want[:, :c] = torch.where(keep, want[:, :c], torch.zeros(()))
    assert torch.equal(bits_of(gd.view(npix, cs)), bits_of(want)) and torch.equal(mask.cpu(), mask_host)


@covers('hnd_quantize_range_bits', 'hnd_quantize_pack_range_bits')
@pytest.mark.parametrize('bits', WIDTHS)
@pytest.mark.parametrize('c,cs,nhw', [(3, 4, (1, 1, 1)), (3, 4, (1, 1, 129)), (5, 8, (3, 37, 41)), (12, 12, (1, 127, 1)),
                                      (258, 260, (2, 5, 13))])
def test_one_launch_codec_stays_inside_its_buffers(ops, c, cs, nhw, bits):
    from tests.codec_util import host_pack
    n, h, w = nhw
    npix = n * h * w
    src, lo, hi, qp_ref = _source(c, cs, npix, bits)
    nbytes = ops.codec_packed_bytes(npix * c, bits)
    specs = [((n, h, w, cs), F32), ((4,), F32), ((n, h, w, cs), U8), ((nbytes,), U8)]
    arena = G.Arena(DEV, G.arena_bytes(specs))
    x = arena.load('x', torch.from_numpy(src).view(n, h, w, cs))
    qp = arena.take('qparams', (4,))
    q = arena.take('q', (n, h, w, cs), U8)
    payload = arena.take('payload', (nbytes,), U8)
    ops.qrange_qparams(lo, hi, bits, qp)
    ops.quantize_range_bits(x, c, bits, q, qp)
    ops.quantize_pack_range_bits(x, c, bits, payload, qp)
    ops.sync_check()
    arena.check()
    codes = R.quantize_range_np(src, c, bits, qp_ref)
    assert torch.equal(bits_of(x.view(npix, cs)), bits_of(src)) and torch.equal(bits_of(qp), bits_of(qp_ref))
    assert np.array_equal(q.view(npix, cs).cpu().numpy(), codes)
    logical = torch.from_numpy(codes.reshape(n, h, w, cs)[..., :c]).permute(0, 3, 1, 2).contiguous()
    assert np.array_equal(payload.cpu().numpy(), host_pack(logical, bits))


def test_the_ledger_covers_every_export_of_the_header():
    """the rule of tests/test_guard_ledger_cpu.py for include/hnd_qrange.h: no export without a guard case"""
    from hnd_ghnd_object_detectors_amd import _lib
    covered = set().union(*LEDGER.values())
    assert covered == {'hnd_fake_quantize_range', 'hnd_qrange_qparams', 'hnd_qrange_observe', 'hnd_qrange_mask_grad',
                       'hnd_quantize_range_bits', 'hnd_quantize_pack_range_bits'} and not covered & set(NO_DEVICE_OUTPUT)
    assert covered | set(NO_DEVICE_OUTPUT) == set(_lib.QRANGE_SYMBOLS)
