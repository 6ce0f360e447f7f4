"""GPU: the kernels of csrc/elementwise.hip that run between the convs of a training step -- training BatchNorm, the 3x3
stride-2 max pool, the FPN helpers -- each held alone to an fp64 reference of the same fp32 inputs, at the sizes where its
code takes another path.  Tables, references and bars: tests/elementwise_util.py (held on the CPU by
tests/test_elementwise_cases_cpu.py).  A bar is an a-priori rounding bound; the assertion is worst ratio <= 1.

The ReLU gate of a BN layer is computed three times from x * scale + shift > 0 (affine_relu, bn_bwd_reduce,
bn_bwd_apply).  The relu cases place 8 % of their elements within a few ulps of a zero output and take the gate of the
REFERENCE from the mask bytes affine_relu stored for the same operands: a site that rounds differently from the forward
(an fma at one, a product and a sum at another) lets a gradient through where the forward stored 0 and misses its bar."""
import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_util as E

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
WORST = {}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


@pytest.fixture(scope='module', autouse=True)
def achieved():
    from tests.conftest import record_achieved
    record_achieved(lambda: '[elementwise vs fp64, worst |got - ref| / bound, held to 1] ' +
                    ', '.join('%s %.3f' % (k, v) for k, v in sorted(WORST.items())))
    yield


def note(key, ratio):
    print('%s: %.4f' % (key, ratio))
    if not ratio <= WORST.get(key, 0.0):           # (a NaN sticks)
        WORST[key] = ratio
    return ratio


def nhwc(t_nchw, cpad=None):
    """NCHW cpu tensor -> NHWC device tensor (channels zero-padded to cpad)."""
    t = t_nchw.permute(0, 2, 3, 1).contiguous()
    if cpad is not None and cpad != t.shape[-1]:
        t = F.pad(t, (0, cpad - t.shape[-1]))
    return t.to(DEV).contiguous()


def nchw(t_nhwc, c=None):
    t = t_nhwc.cpu()
    if c is not None:
        t = t[..., :c]
    return t.permute(0, 3, 1, 2).contiguous()


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def nan_like(t, dtype=torch.float32):
    return torch.full(tuple(t.shape), float('nan'), dtype=dtype, device=DEV)


# ---------------------------------------------------------------------------------------------------- training BN

@pytest.mark.parametrize('case', E.FINALIZE_CASES)
def test_bn_finalize(ops, case):
    ntiles, last, c, cs, running = case
    i = E.finalize_inputs(*case)
    part, gamma, beta, rm, rv = dev(i['part']), dev(i['gamma']), dev(i['beta']), dev(i['rm']), dev(i['rv'])
    nbt = torch.full((), 41, dtype=torch.int64, device=DEV)
    out = [torch.full((cs,), float('nan'), device=DEV) for _ in range(4)]
    ops.bn_finalize(part, ntiles, c, cs, i['count'], gamma, beta, rm, rv, nbt, E.MOMENTUM, E.EPS, *out)
    ops.sync_check()
    assert int(nbt) == 42
    scale, shift, mean, rstd = (t.cpu() for t in out)
    for t in (scale, shift, mean, rstd):
        assert float(t[c:].abs().sum()) == 0.0 and bool(torch.isfinite(t).all())
    got = dict(mean=mean[:c], rstd=rstd[:c], scale=scale[:c], shift=shift[:c])
    if running:
        got['rm'], got['rv'] = rm.cpu(), rv.cpu()
    ref = E.finalize_reference(i['part'], c, i['count'], i['gamma'], i['beta'], i['rm'], i['rv'])
    r = E.finalize_bars(got, ref, i['beta'])
    for k, v in r.items():
        note('bn_finalize ' + k, v)
    assert max(r.values()) <= 1.0, r


def _affine(ops, i, relu, with_mask=True):
    """device affine_relu of a bn_inputs case: (y, mask nibbles or None), on the host"""
    x = dev(i['x'])
    y = nan_like(x)
    mask = torch.full((x.shape[0], x.shape[1] // 4), 0xAA, dtype=torch.uint8, device=DEV) if with_mask else None
    ops.affine_relu(x, dev(i['scale']), dev(i['shift']), y, relu, mask)
    ops.sync_check()
    return y.cpu(), (mask.cpu() if with_mask else None)


@pytest.mark.parametrize('cs', E.STREAM_CS)
def test_affine_relu(ops, cs):
    for npix in [p for c, p in E.STREAM_CASES if c == cs]:
        for relu in (False, True):
            i = E.bn_inputs(npix, cs, cs, relu)
            for with_mask in (True, False):
                y, mask = _affine(ops, i, relu, with_mask)
                ratio, signs = E.affine_bars(y, i['x'], i['scale'], i['shift'], relu)
                note('affine_relu', ratio)
                assert ratio <= 1.0 and signs, (npix, relu, with_mask, ratio, signs)
                if with_mask:
                    assert torch.equal(mask, E.nibbles_of(y)), (npix, relu)


@pytest.mark.parametrize('n4', E.MASK_N4)
def test_relu_mask_nibbles(ops, n4):
    x = E.mask_inputs(n4)
    bits = torch.full((n4,), 0xAA, dtype=torch.uint8, device=DEV)
    ops.relu_mask_nibbles(dev(x), bits)
    ops.sync_check()
    assert torch.equal(bits.cpu(), E.nibbles_of(x.view(n4, 4)).view(-1))


def _device_gate(ops, i, relu):
    """the gate the forward stored: the mask bytes of the device's affine_relu for the same x, scale, shift"""
    if not relu:
        return None
    _, mask = _affine(ops, i, True)
    return E.gate_of(mask)


def _reduce(ops, i, relu, npix, cs):
    part = torch.full((E.bwd_ntiles(npix), 2, cs), float('nan'), device=DEV)
    assert ops.bn_bwd_ntiles(npix) == part.shape[0]
    ops.bn_bwd_reduce(dev(i['g']), dev(i['x']), dev(i['scale']), dev(i['shift']), dev(i['mean']), dev(i['rstd']), relu, part)
    ops.sync_check()
    return part.cpu()


@pytest.mark.parametrize('npix,cs', E.REDUCE_CASES)
def test_bn_bwd_reduce(ops, npix, cs):
    for relu in (False, True):
        i = E.bn_inputs(npix, cs, cs, relu)
        gate = _device_gate(ops, i, relu)
        part = _reduce(ops, i, relu, npix, cs)
        r = E.reduce_bars(part, E.reduce_reference(i['g'], i['x'], i['mean'], i['rstd'], gate), npix)
        note('bn_bwd_reduce sum d' + (' (relu: gate of the stored forward)' if relu else ''), r[0])
        note('bn_bwd_reduce sum d xhat' + (' (relu)' if relu else ''), r[1])
        assert max(r) <= 1.0, (relu, r)


@pytest.mark.parametrize('cs', E.REDUCE_REFUSED_CS)
def test_bn_bwd_reduce_refuses_a_channel_stride_it_cannot_tile(ops, cs):
    i = E.bn_inputs(3, cs, cs, False)
    part = torch.zeros(1, 2, cs, device=DEV)
    with pytest.raises(RuntimeError, match='hnd_bn_bwd_reduce'):
        ops.bn_bwd_reduce(dev(i['g']), dev(i['x']), dev(i['scale']), dev(i['shift']), dev(i['mean']), dev(i['rstd']), False,
                          part)
    ops.sync_check()
    assert float(part.abs().sum()) == 0.0


def _bwd_finalize(ops, i, part, npix, c, cs):
    dgamma, dbeta = torch.full((c,), float('nan'), device=DEV), torch.full((c,), float('nan'), device=DEV)
    k123 = torch.full((3, cs), float('nan'), device=DEV)
    ops.bn_bwd_finalize(dev(part), part.shape[0], c, cs, npix, dev(i['gamma']), dev(i['mean']), dev(i['rstd']), dgamma,
                        dbeta, k123)
    ops.sync_check()
    return dgamma.cpu(), dbeta.cpu(), k123.cpu()


@pytest.mark.parametrize('npix,c,cs', E.BWD_FINALIZE_CASES)
def test_bn_bwd_finalize(ops, npix, c, cs):
    i = E.bn_inputs(npix, cs, c, True)
    part = _reduce(ops, i, True, npix, cs)
    dgamma, dbeta, k123 = _bwd_finalize(ops, i, part, npix, c, cs)
    assert float(k123[:, c:].abs().sum()) == 0.0 and bool(torch.isfinite(k123).all())
    ref = E.bwd_finalize_reference(part, c, npix, i['gamma'], i['mean'], i['rstd'])
    r = E.bwd_finalize_bars(dict(dbeta=dbeta, dgamma=dgamma, k1=k123[0, :c], k2=k123[1, :c], k3=k123[2, :c]), ref, npix)
    for k, v in r.items():
        note('bn_bwd_finalize ' + k, v)
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize('cs', E.STREAM_CS)
def test_bn_bwd_apply(ops, cs):
    for npix in [p for c, p in E.STREAM_CASES if c == cs]:
        for relu in (False, True):
            i = E.bn_inputs(npix, cs, cs, relu)
            gate = _device_gate(ops, i, relu)
            if E.reduce_accepts(cs):           # k123 as the device's own backward finalize stored it
                _, _, k123 = _bwd_finalize(ops, i, _reduce(ops, i, relu, npix, cs), npix, cs, cs)
            else:                              # the reduce refuses this stride: the same formulas on the host, rounded once
                s1, s2, _, _ = E.reduce_reference(i['g'], i['x'], i['mean'], i['rstd'], gate)
                f = E.bwd_finalize_reference(torch.stack((s1, s2), 1), cs, npix, i['gamma'], i['mean'], i['rstd'])
                k123 = torch.stack((f['k1'], f['k2'], f['k3'])).float()
            dx = nan_like(i['x'])
            ops.bn_bwd_apply(dev(i['g']), dev(i['x']), dev(i['scale']), dev(i['shift']), dev(k123), relu, dx)
            ops.sync_check()
            ratio = E.apply_bars(dx.cpu(), E.apply_reference(i['g'], i['x'], k123, gate))
            note('bn_bwd_apply' + (' (relu: gate of the stored forward)' if relu else ''), ratio)
            assert ratio <= 1.0, (npix, relu, ratio)


@pytest.mark.parametrize('c', [12, 256])
@pytest.mark.parametrize('relu', [False, True])
def test_train_bn_end_to_end_against_torch_fp64_autograd(ops, c, relu):
    """3700 pixels: 29 statistics tiles, 4 backward tiles; the bars of test_train_bn_forward_backward, fp64 reference"""
    g = E.gen(4900 + c + int(relu))
    n, h, w = 2, 37, 50
    npix, cs = n * h * w, ops.chan_pad_of(c)
    x = torch.randn(n, c, h, w, generator=g) * 1.7 + 0.4
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    gout = torch.randn(n, c, h, w, generator=g)
    xt, gt, bt = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    rm_ref, rv_ref = rm.double(), rv.double()
    out = F.batch_norm(xt, rm_ref, rv_ref, gt, bt, True, E.f32(E.MOMENTUM), E.f32(E.EPS))
    out = F.relu(out) if relu else out
    out.backward(gout.double())

    xd = nhwc(x, cs)
    nt = ops.stats_tiles(npix)
    assert (nt, ops.bn_bwd_ntiles(npix)) == (29, 4)
    x64 = F.pad(xd.cpu().double().view(npix, cs), (0, 0, 0, nt * E.STAT_TILE - npix)).view(nt, E.STAT_TILE, cs)
    part = torch.stack((x64.sum(1), (x64 * x64).sum(1)), 1).float().to(DEV)
    gam, bet, rmd, rvd = dev(gamma), dev(beta), dev(rm), dev(rv)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    scale, shift, mean, rstd = (torch.empty(cs, device=DEV) for _ in range(4))
    ops.bn_finalize(part, nt, c, cs, npix, gam, bet, rmd, rvd, nbt, E.MOMENTUM, E.EPS, scale, shift, mean, rstd)
    y = torch.empty_like(xd)
    ops.affine_relu(xd, scale, shift, y, relu)
    gd = nhwc(gout, cs)
    bpart = torch.empty(ops.bn_bwd_ntiles(npix), 2, cs, device=DEV)
    ops.bn_bwd_reduce(gd, xd, scale, shift, mean, rstd, relu, bpart)
    dgamma, dbeta, k123 = torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.empty(3, cs, device=DEV)
    ops.bn_bwd_finalize(bpart, bpart.shape[0], c, cs, npix, gam, mean, rstd, dgamma, dbeta, k123)
    dx = torch.empty_like(xd)
    ops.bn_bwd_apply(gd, xd, scale, shift, k123, relu, dx)
    ops.sync_check()
    errs = dict(y=relerr(nchw(y, c), out.detach()), rm=relerr(rmd.cpu(), rm_ref), rv=relerr(rvd.cpu(), rv_ref),
                dgamma=relerr(dgamma.cpu(), gt.grad), dbeta=relerr(dbeta.cpu(), bt.grad), dx=relerr(nchw(dx, c), xt.grad))
    print(errs)
    assert int(nbt) == 1 and max(errs['y'], errs['rm'], errs['rv']) < 1e-5, errs
    assert max(errs['dgamma'], errs['dbeta'], errs['dx']) < 2e-5, errs
    if cs != c:
        assert float(y[..., c:].abs().max()) == 0 and float(dx[..., c:].abs().max()) == 0


# ---------------------------------------------------------------------------------------------------- max pool

def _pool(ops, x, backward=True):
    n, c, h, w = x.shape
    y_ref, tap_ref = E.pool_expected(x)
    oh, ow = y_ref.shape[2], y_ref.shape[3]
    xd = nhwc(x)
    yd = torch.full((n, oh, ow, c), float('nan'), device=DEV)
    idx = torch.full((n, oh, ow, c), 0xAA, dtype=torch.uint8, device=DEV)
    ops.maxpool_fwd(xd, yd, idx)
    ops.sync_check()
    assert E.same_bits(nchw(yd), y_ref)
    assert torch.equal(nchw(idx), tap_ref)
    if not backward:
        return
    g = E.gen(4800 + h + w)
    dy, sc = torch.randn(y_ref.shape, generator=g), torch.rand(c, generator=g) + 0.5
    dx = torch.full((n, h, w, c), float('nan'), device=DEV)
    ops.maxpool_bwd_relu_scale(nhwc(dy), idx, xd, dev(sc), dx)
    ops.sync_check()
    ratio = note('maxpool_bwd', E.pool_bwd_bars(nchw(dx), E.pool_bwd_reference(dy, tap_ref, x, sc)))
    assert ratio <= 1.0, ((n, c, h, w), ratio)


@pytest.mark.parametrize('h', E.POOL_EXTENTS)
def test_maxpool_fwd_bwd_values_taps_and_gradient(ops, h):
    """values and tap indices exact against torch's CPU scan (ties, windows of -inf only, one and two NaNs); the backward
    against fp64 with the gate (act > 0) and the argmax apart: act is not post-ReLU"""
    for n, c, hh, w in E.pool_cases():
        if hh == h:
            _pool(ops, E.pool_inputs(n, c, hh, w))


def test_maxpool_fwd_grid_stride_second_pass(ops):
    n, c, h, w = E.POOL_GRID_STRIDE_CASE
    assert E.pool_threads(n, c, h, w) > E.GRID_CAP * 256
    _pool(ops, E.pool_inputs(n, c, h, w), backward=False)


# ---------------------------------------------------------------------------------------------------- FPN helpers

@pytest.mark.parametrize('geom', E.UPSAMPLE_GEOMS)
def test_upsample_nearest_bwd(ops, geom):
    (h, w), (H, W) = geom
    for c in E.UPSAMPLE_CHANNELS:
        for n in E.UPSAMPLE_BATCHES:
            g = E.gen(5000 + H + W + c + n)
            gf, base = torch.randn(n, c, H, W, generator=g), torch.randn(n, c, h, w, generator=g)
            for acc in (False, True):
                out = nhwc(base) if acc else torch.full((n, h, w, c), float('nan'), device=DEV)
                ops.upsample_nearest_bwd(nhwc(gf), out, acc)
                ops.sync_check()
                ratio = note('upsample_nearest_bwd', E.upsample_bars(nchw(out), gf, base if acc else None, h, w))
                assert ratio <= 1.0, (c, n, acc, ratio)


@pytest.mark.parametrize('n,h,w,c', E.SUBSAMPLE_CASES)
def test_subsample2(ops, n, h, w, c):
    x = torch.randn(n, h, w, c, generator=E.gen(5100 + h + w + c))
    y = torch.full((n, (h + 1) // 2, (w + 1) // 2, c), float('nan'), device=DEV)
    ops.subsample2(dev(x), y)
    ops.sync_check()
    assert torch.equal(y.cpu(), x[:, ::2, ::2].contiguous())


@pytest.mark.parametrize('n4', E.ADD_N4)
def test_add_inplace(ops, n4):
    g = E.gen(5200 + n4 % 1000)
    x, y = torch.randn(n4 * 4, generator=g), torch.randn(n4 * 4, generator=g)
    xd = dev(x)
    ops.add_inplace(xd, dev(y))
    ops.sync_check()
    assert torch.equal(xd.cpu(), x + y)
