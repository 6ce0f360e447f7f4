"""The tiled build of the bf16x3 emulation GEMM (csrc/conv_bx3_tiled.hip) against the persistent one (csrc/conv_bx3.hip):
identical bits on everything bx3_applies admits, whichever build the picker (or HND_DEBUG_PICKER=bx3_tiled=0 / 1) chooses.

Every launch is built AND run under the same HND_DEBUG_PICKER value: the key is read per call.  Outputs are pre-filled with
NaN, mask bytes with 255.  The fp64 bar is the one of tests/test_bx3_gpu.py (e1 < 1e-6 and e1 <= 1.5 e0 + 1e-8, e0 the native
fp32 kernel's error on the same operands)."""
import contextlib
import os
import random

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from hnd_ghnd_object_detectors_amd import ops as O
    return O


@contextlib.contextmanager
def picker(value):
    """HND_DEBUG_PICKER = value (None: unset) inside the block; whatever was there before comes back afterwards"""
    old = os.environ.get('HND_DEBUG_PICKER')
    if value is None:
        os.environ.pop('HND_DEBUG_PICKER', None)
    else:
        os.environ['HND_DEBUG_PICKER'] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop('HND_DEBUG_PICKER', None)
        else:
            os.environ['HND_DEBUG_PICKER'] = old


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _nibbles(y):
    v = y.view(*y.shape[:3], y.shape[3] // 4, 4) > 0
    return (v[..., 0].to(torch.uint8) | (v[..., 1].to(torch.uint8) << 1) | (v[..., 2].to(torch.uint8) << 2)
            | (v[..., 3].to(torch.uint8) << 3))


def both_builds(ops, make, shape, mask_out=False):
    """make(y, mo) -> launch.  Runs it on the persistent and on the tiled build; asserts the builds were the ones asked for and
    that values and mask nibbles are equal bit for bit.  Returns the tiled build's (y, mo)."""
    outs = {}
    for key, want in (('bx3_tiled=0', 'persistent'), ('bx3_tiled=1', 'tiled')):
        y = torch.full(shape, float('nan'), device=DEV)
        mo = torch.full(shape[:3] + (shape[3] // 4,), 255, dtype=torch.uint8, device=DEV) if mask_out else None
        with picker(key), ops.emulation('force'):
            l = make(y, mo)
            assert l.variant == 'bx3_64' and l.build == want, (l.variant, l.build, key)
            l.run()
            ops.sync_check()
        outs[want] = (y, mo)
    (yp, mp), (yt, mt) = outs['persistent'], outs['tiled']
    assert not bool(torch.isnan(yt).any())
    assert torch.equal(yt, yp), 'tiled != persistent: %d elements differ' % int((yt != yp).sum())
    if mask_out:
        assert torch.equal(mt, mp) and torch.equal(mt, _nibbles(yt))
    return yt, mt


def native(ops, make, shape):
    y = torch.full(shape, float('nan'), device=DEV)
    with ops.emulation('off'):
        l = make(y, None)
    assert not l.variant.startswith('bx3')
    l.run()
    ops.sync_check()
    return y


def fp64_bar(y1, y0, ref):
    e0 = float((y0.cpu().double() - ref).norm() / ref.norm())
    e1 = float((y1.cpu().double() - ref).norm() / ref.norm())
    print('rel-L2 vs fp64: tiled emulation %.3e, native fp32 %.3e' % (e1, e0))
    assert e1 < 1e-6 and e1 <= 1.5 * e0 + 1e-8, (e1, e0)


SHAPES = [
    (256, 256, 4, 96, 128, 1, False), (256, 128, 8, 96, 128, 1, True), (256, 512, 8, 192, 256, 2, True),
    (128, 64, 16, 96, 128, 1, False), (256, 1024, 8, 64, 64, 1, True), (512, 256, 8, 96, 128, 1, True),
    (512, 1024, 8, 96, 128, 2, True), (1024, 256, 16, 50, 84, 1, True), (1024, 2048, 16, 50, 84, 2, True),
    (256, 256, 4, 99, 84, 1, True), (128, 64, 16, 91, 93, 1, False),          # the eleven of tests/test_bx3_gpu.py
    # the small grids the tiled build exists for (batch 4) ...
    (1024, 256, 4, 50, 84, 1, True),         # layer3.x.conv1: 263 chunks on 64 teams
    (2048, 256, 4, 25, 42, 1, False),        # fpn.inner3: 66 chunks on 64 teams
    (2048, 512, 4, 25, 42, 1, True),         # layer4.x.conv1
    (256, 64, 1, 25, 42, 1, True),           # 17 chunks (a 26-row tail) on 256 teams: fewer chunks than teams
]


@pytest.mark.parametrize('cin,cout,n,h,w,stride,epi', SHAPES)
def test_tiled_1x1_conv_equals_the_persistent_build_and_meets_the_fp64_bar(ops, cin, cout, n, h, w, stride, epi):
    g = torch.Generator().manual_seed(5 + cin + cout)
    x = torch.randn(n, cin, h, w, generator=g) * torch.exp2(torch.randn(n, 1, h, w, generator=g) * 3)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    es = torch.rand(cout, generator=g) + 0.5 if epi else None
    eb = torch.randn(cout, generator=g) if epi else None
    ref = F.conv2d(x.double(), wt.double(), None, stride)
    if epi:
        ref = F.relu(ref * es.double()[None, :, None, None] + eb.double()[None, :, None, None])
    ref = ref.permute(0, 2, 3, 1)
    xd, pk = _nhwc(x), ops.pack_weights(wt.to(DEV).contiguous())
    kw = dict(epi_scale=es.to(DEV) if epi else None, epi_shift=eb.to(DEV) if epi else None, relu=epi)
    make = lambda y, mo: ops.conv_forward(xd, pk, y, 1, stride, 0, **kw)
    yt, _ = both_builds(ops, make, tuple(ref.shape))
    fp64_bar(yt, native(ops, make, tuple(ref.shape)), ref)


@pytest.mark.parametrize('cin,cout,n,h,w', [(128, 512, 8, 96, 128), (256, 1024, 8, 64, 96), (512, 2048, 16, 32, 48),
                                            (512, 2048, 16, 25, 42), (512, 2048, 4, 25, 42)])
def test_tiled_conv3_with_residual_relu_and_mask_nibbles(ops, cin, cout, n, h, w):
    g = torch.Generator().manual_seed(9 + cin)
    x = torch.randn(n, cin, h, w, generator=g).relu()
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    es, eb = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    res = torch.randn(n, cout, h, w, generator=g)
    ref = F.relu(F.conv2d(x.double(), wt.double()) * es.double()[None, :, None, None] + eb.double()[None, :, None, None]
                 + res.double()).permute(0, 2, 3, 1)
    xd, rd, pk = _nhwc(x), _nhwc(res), ops.pack_weights(wt.to(DEV).contiguous())
    make = lambda y, mo: ops.conv_forward(xd, pk, y, 1, 1, 0, epi_scale=es.to(DEV), epi_shift=eb.to(DEV), res1=rd, relu=True,
                                          mask_out=mo)
    yt, _ = both_builds(ops, make, (n, h, w, cout), mask_out=True)
    fp64_bar(yt, native(ops, make, (n, h, w, cout)), ref)


@pytest.mark.parametrize('cin,cout,n,h,w,with_res', [
    (128, 512, 8, 96, 128, True), (256, 1024, 8, 64, 96, True), (512, 2048, 16, 32, 48, True), (512, 2048, 16, 25, 42, True),
    (1024, 256, 16, 50, 84, True), (1024, 256, 4, 50, 84, True),
    (512, 128, 16, 100, 168, False), (1024, 256, 16, 50, 84, False)])     # (K > 256: the mask alone, beside the running value)
def test_tiled_masked_data_gradient(ops, cin, cout, n, h, w, with_res):
    g = torch.Generator().manual_seed(13 + cin)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    res = torch.randn(n, cout, h, w, generator=g)
    act = torch.randn(n, cout, h, w, generator=g)
    full = F.conv2d(x.double(), wt.double()) + (res.double() if with_res else 0.0)
    ref = torch.where(act.double() > 0, full, torch.zeros((), dtype=torch.float64)).permute(0, 2, 3, 1)
    xd, rd, ad, pk = _nhwc(x), _nhwc(res), _nhwc(act), ops.pack_weights(wt.to(DEV).contiguous())
    bits = _nibbles(ad).contiguous()
    make = lambda y, mo: ops.conv_forward(xd, pk, y, 1, 1, 0, res1=rd if with_res else None, mask_bits=bits)
    yt, _ = both_builds(ops, make, (n, h, w, cout))
    fp64_bar(yt, native(ops, make, (n, h, w, cout)), ref)


@pytest.mark.parametrize('n,cin,h,w', [(8, 256, 96, 128), (4, 2048, 26, 44), (4, 1024, 50, 84)])
def test_tiled_fpn_lateral_with_the_upsampled_top_down_map(ops, n, cin, h, w):
    g = torch.Generator().manual_seed(31 + cin)
    cout = 256
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    bias = torch.randn(cout, generator=g)
    top = torch.randn(n, cout, h // 2, w // 2, generator=g)
    ref = (F.conv2d(x.double(), wt.double(), bias.double())
           + F.interpolate(top.double(), size=(h, w), mode='nearest')).permute(0, 2, 3, 1)
    xd, td, pk = _nhwc(x), _nhwc(top), ops.pack_weights(wt.to(DEV).contiguous())
    make = lambda y, mo: ops.conv_forward(xd, pk, y, 1, 1, 0, epi_shift=bias.to(DEV), res1=td, res1_up=True)
    yt, _ = both_builds(ops, make, (n, h, w, cout))
    fp64_bar(yt, native(ops, make, (n, h, w, cout)), ref)


@pytest.mark.parametrize('c,n,h,w', [(256, 4, 50, 84), (512, 4, 25, 42)])
def test_tiled_winograd_component_gemms(ops, c, n, h, w):
    """the grouped launch (w_group_rows: 64 component GEMMs over disjoint row groups) of a frozen 3x3 conv through F(6x6,3x3)"""
    g = torch.Generator().manual_seed(77 + c)
    x = torch.randn(n, c, h, w, generator=g).relu()
    wt = torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5
    xd, wd = _nhwc(x), wt.to(DEV).contiguous()

    outs = {}
    for key, want in (('bx3_tiled=0', 'persistent'), ('bx3_tiled=1', 'tiled')):
        y = torch.full((n, h, w, c), float('nan'), device=DEV)
        with picker(key), ops.emulation('force'):
            ww = ops.WinoWeights(wd, False, 6)
            nv, nm = ops.WinoConv.scratch_elems(n, h, w, c, c, 6)
            conv = ops.WinoConv(xd, ww, y, torch.empty(nv, device=DEV), torch.empty(nm, device=DEV))
            assert conv.gemm.desc.w_group_rows > 0
            assert conv.gemm.variant == 'bx3_64' and conv.gemm.build == want, (conv.gemm.variant, conv.gemm.build)
            conv.run()
            ops.sync_check()
        outs[want] = y
    assert not bool(torch.isnan(outs['tiled']).any())
    assert torch.equal(outs['tiled'], outs['persistent'])
    ref = F.conv2d(x.double(), wt.double(), None, 1, 1).permute(0, 2, 3, 1)
    e1 = float((outs['tiled'].cpu().double() - ref).norm() / ref.norm())
    assert e1 < 2e-5, e1              # (the Winograd transforms' own fp32 error dominates: tests/test_bx3_gpu.py's bound)


def test_tiled_equals_persistent_on_randomised_shapes_and_epilogues(ops):
    """seeded sweep over what bx3_applies admits, the generator of tests/test_bx3_gpu.py's sweep with K up to 2048: K 128 ...
    2048, 64 ... 1024 columns, tails of 1 ... 63 rows, M % 4 != 0, stride 1 / 2, every epilogue combination.  (With this seed
    the size filter skips none of the 40 cases; at least 30 must run.)"""
    rnd = random.Random(20261016)
    g = torch.Generator().manual_seed(99)
    done = 0
    for case in range(40):
        cin = rnd.choice([128, 256, 256, 512, 768, 1024, 1536, 2048])
        cout = rnd.choice([64, 128, 256, 512, 1024])
        stride = rnd.choice([1, 1, 1, 2])
        n = rnd.choice([2, 3, 5, 8])
        oh, ow = rnd.randrange(9, 120), rnd.choice([4 * rnd.randrange(12, 40), rnd.randrange(21, 160)])
        m = n * oh * ow
        if m * max(cin, cout) * 4 > 1.5e9:
            continue
        h, w = (oh - 1) * stride + 1 + rnd.randrange(0, stride), (ow - 1) * stride + 1 + rnd.randrange(0, stride)
        res = rnd.random() < 0.6
        relu = rnd.random() < 0.5
        mask_out = res and relu and cout % 128 == 0 and rnd.random() < 0.5
        mask_bits = (res or cin > 256) and not mask_out and rnd.random() < 0.4
        epi = rnd.random() < 0.7
        x = (torch.randn(n, h, w, cin, generator=g) * 2.0).to(DEV)
        wt = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(DEV)
        kw = dict(relu=relu)
        if epi:
            kw.update(epi_scale=(torch.rand(cout, generator=g) + 0.5).to(DEV), epi_shift=torch.randn(cout, generator=g).to(DEV))
        if res:
            kw['res1'] = torch.randn(n, oh, ow, cout, generator=g).to(DEV)
        if mask_bits:
            kw['mask_bits'] = torch.randint(0, 16, (n, oh, ow, cout // 4), generator=g, dtype=torch.uint8).to(DEV)
        pk = ops.pack_weights(wt)
        make = lambda y, mo: ops.conv_forward(x, pk, y, 1, stride, 0, mask_out=mo, **kw)
        try:
            both_builds(ops, make, (n, oh, ow, cout), mask_out=mask_out)
        except AssertionError as e:
            raise AssertionError((case, cin, cout, m, stride, res, relu, mask_out, mask_bits, epi, str(e)))
        done += 1
    print('randomised cases run:', done)
    assert done >= 30, done


def test_a_rows_bits_are_the_same_alone_and_inside_any_batch_with_the_automatic_rule(ops):
    """no HND_DEBUG_PICKER key: image 0 of a batch-1, batch-4 and batch-16 launch of layer3.x.conv1 (1024 -> 256 @ 50 x 84),
    where the rule picks by the launch's chunk count -- the same bits, and at least two different builds were in fact used"""
    g = torch.Generator().manual_seed(2026)
    cin, cout, h, w = 1024, 256, 50, 84
    x = (torch.randn(16, h, w, cin, generator=g) * 2.0).to(DEV)
    wt = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(DEV)
    es, eb = (torch.rand(cout, generator=g) + 0.5).to(DEV), torch.randn(cout, generator=g).to(DEV)
    pk = ops.pack_weights(wt)
    builds, first = {}, {}
    for n in (1, 4, 16):
        y = torch.full((n, h, w, cout), float('nan'), device=DEV)
        with picker(None), ops.emulation('force'):
            l = ops.conv_forward(x[:n].contiguous(), pk, y, 1, 1, 0, epi_scale=es, epi_shift=eb, relu=True)
            assert l.variant == 'bx3_64' and l.build in ('persistent', 'tiled'), (l.variant, l.build)
            l.run()
            ops.sync_check()
        builds[n], first[n] = l.build, y[0].clone()
    print('builds by batch:', builds)
    assert not bool(torch.isnan(first[16]).any())
    assert torch.equal(first[1], first[16]) and torch.equal(first[4], first[16])
    assert len(set(builds.values())) >= 2, builds
