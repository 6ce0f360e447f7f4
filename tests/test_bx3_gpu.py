"""fp32 emulation on the bf16 matrix pipe (csrc/conv_bx3.hip, hnd_conv_desc.w_bf16x3; VERDICT r4 item 3, the default for
the launches it covers since round 6 -- VERDICT r5 item 1).

The emulation kernel is held to an fp64 reference BESIDE the native kernel on the same operands (its error may be at most
1.5x the native one's): `ops.emulation('off')` builds the native launch, `ops.emulation('force')` the emulated one whatever
the layer policy says.  Further down: the policy itself (by layer, never by batch), identical bits of a row whatever batch /
team / tail it is computed in, and the documented non-finite / denormal behaviour through hnd_conv2d_igemm."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    from hnd_ghnd_object_detectors_amd import ops as O
    return O


@pytest.fixture(autouse=True)
def emulated_family(ops):
    """this file holds the EMULATED rounding family: the round-6 default (choice by layer), also when the suite runs under
    HND_BF16X3=0 (tests/test_ops_gpu.py is the native family's file the other way round)"""
    with ops.emulation('policy'):
        yield


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


@pytest.mark.parametrize('cin,cout,n,h,w,stride,epi', [
    (256, 256, 4, 96, 128, 1, False),        # fpn.inner0-like (without its residual)
    (256, 128, 8, 96, 128, 1, True),         # layer2.0.conv1: FrozenBN scale / shift + ReLU
    (256, 512, 8, 192, 256, 2, True),        # layer2.0.downsample: stride 2
    (128, 64, 16, 96, 128, 1, False),        # K = 128, one 64-column slice
    (256, 1024, 8, 64, 64, 1, True),         # 16 slices per team
    (512, 256, 8, 96, 128, 1, True),         # K = 512: two passes over k, the second adds the first one's partial result
    (512, 1024, 8, 96, 128, 2, True),        # layer3.0.downsample: K = 512, stride 2
    (1024, 256, 16, 50, 84, 1, True),        # layer3.x.conv1: four passes over k
    (1024, 2048, 16, 50, 84, 2, True),       # layer4.0.downsample: four passes, stride 2, M = 16 800 = 262.5 chunks (a tail)
    (256, 256, 4, 99, 84, 1, True),          # M = 33 264: the last chunk holds 48 rows
    (128, 64, 16, 91, 93, 1, False),         # M = 135 408: 2 115 chunks + 48 rows
])
def test_bx3_1x1_conv_against_fp64_beside_the_native_kernel(ops, cin, cout, n, h, w, stride, epi):
    g = torch.Generator().manual_seed(5 + cin + cout)
    x = torch.randn(n, cin, h, w, generator=g) * torch.exp2(torch.randn(n, 1, h, w, generator=g) * 3)     # wide range
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    es = torch.rand(cout, generator=g) + 0.5 if epi else None
    eb = torch.randn(cout, generator=g) if epi else None
    ref = F.conv2d(x.double(), wt.double(), None, stride)
    if epi:
        ref = F.relu(ref * es.double()[None, :, None, None] + eb.double()[None, :, None, None])
    xd, pk = _nhwc(x), ops.pack_weights(wt.to(DEV).contiguous())
    oh, ow = ref.shape[2], ref.shape[3]
    kw = dict(epi_scale=es.to(DEV) if epi else None, epi_shift=eb.to(DEV) if epi else None, relu=epi)
    y0 = torch.full((n, oh, ow, cout), float('nan'), device=DEV)
    with ops.emulation('off'):
        l0 = ops.conv_forward(xd, pk, y0, 1, stride, 0, **kw)
    assert not l0.variant.startswith('bx3')
    l0.run()
    y1 = torch.full_like(y0, float('nan'))
    with ops.emulation('force'):
        l1 = ops.conv_forward(xd, pk, y1, 1, stride, 0, **kw)
    assert l1.variant == 'bx3_64' and pk.bx3 is not None, l1.variant
    l1.run()
    ops.sync_check()
    want = ref.permute(0, 2, 3, 1)
    e0 = float((y0.cpu().double() - want).norm() / want.norm())
    e1 = float((y1.cpu().double() - want).norm() / want.norm())
    assert not bool(torch.isnan(y1).any())
    assert e1 < 1e-6 and e1 <= 1.5 * e0 + 1e-8, (e1, e0)
    y2 = torch.empty_like(y1)
    with ops.emulation('force'):
        ops.conv_forward(xd, pk, y2, 1, stride, 0, **kw).run()
    assert torch.equal(y2, y1)                        # a fixed summation order: reproducible bits
    from tests.conftest import record_achieved
    record_achieved('[bf16x3 emulation, 1x1 %d -> %d @%dx%d s%d] rel-L2 vs fp64 %.2e (native fp32 MFMA %.2e)'
                    % (cin, cout, h, w, stride, e1, e0))


@pytest.mark.parametrize('cin,cout,n,h,w', [(128, 512, 8, 96, 128), (256, 1024, 8, 64, 96), (512, 2048, 16, 32, 48),
                                            (512, 2048, 16, 25, 42)])          # layer4: M = 16 800, a 32-row tail
def test_bx3_bottleneck_conv3_with_residual_relu_and_mask_nibbles(ops, cin, cout, n, h, w):
    """conv3 of a frozen Bottleneck: FrozenBN scale / shift, + identity, ReLU, and the ReLU-mask nibbles of the stored values
    (hnd_conv_desc.mask_out) -- the residual rows travel as asm loads in the ring's in-order stream"""
    g = torch.Generator().manual_seed(9 + cin)
    x = torch.randn(n, cin, h, w, generator=g).relu()
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    es, eb = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    res = torch.randn(n, cout, h, w, generator=g)
    ref = F.relu(F.conv2d(x.double(), wt.double()) * es.double()[None, :, None, None] + eb.double()[None, :, None, None]
                 + res.double()).permute(0, 2, 3, 1)
    xd, rd, pk = _nhwc(x), _nhwc(res), ops.pack_weights(wt.to(DEV).contiguous())
    outs = {}
    for emu in (False, True):
        y = torch.full((n, h, w, cout), float('nan'), device=DEV)
        bits = torch.full((n, h, w, cout // 4), 255, dtype=torch.uint8, device=DEV)
        with ops.emulation('force' if emu else 'off'):
            l = ops.conv_forward(xd, pk, y, 1, 1, 0, epi_scale=es.to(DEV), epi_shift=eb.to(DEV), res1=rd, relu=True, mask_out=bits)
        assert (l.variant == 'bx3_64') == emu, l.variant
        l.run()
        ops.sync_check()
        outs[emu] = (y.cpu().double(), bits.cpu(), y)
    e0 = float((outs[False][0] - ref).norm() / ref.norm())
    e1 = float((outs[True][0] - ref).norm() / ref.norm())
    assert e1 < 1e-6 and e1 <= 1.5 * e0 + 1e-8, (e1, e0)
    yv = outs[True][2].view(n, h, w, cout // 4, 4)
    want = ((yv[..., 0] > 0).to(torch.uint8) | ((yv[..., 1] > 0).to(torch.uint8) << 1) | ((yv[..., 2] > 0).to(torch.uint8) << 2)
            | ((yv[..., 3] > 0).to(torch.uint8) << 3)).cpu()
    assert torch.equal(outs[True][1], want)                       # the nibbles describe the values this kernel stored
    from tests.conftest import record_achieved
    record_achieved('[bf16x3 emulation, conv3 %d -> %d + residual + ReLU + mask nibbles] rel-L2 vs fp64 %.2e (native %.2e)'
                    % (cin, cout, e1, e0))


@pytest.mark.parametrize('cin,cout,n,h,w', [(128, 512, 8, 96, 128), (256, 1024, 8, 64, 96), (512, 2048, 16, 32, 48),
                                            (512, 2048, 16, 25, 42), (1024, 256, 16, 50, 84)])
def test_bx3_masked_data_gradient_with_residual(ops, cin, cout, n, h, w):
    """conv1's data gradient in a frozen Bottleneck: W1^T g_a1 (FrozenBN scale folded into the weights) + the gradient of
    the identity path, masked by the block input's ReLU given as nibbles (hnd_conv_desc.mask_bits)"""
    g = torch.Generator().manual_seed(13 + cin)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    res = torch.randn(n, cout, h, w, generator=g)
    act = torch.randn(n, cout, h, w, generator=g)                       # the activation whose sign is the mask
    ref = torch.where(act.double() > 0, F.conv2d(x.double(), wt.double()) + res.double(),
                      torch.zeros((), dtype=torch.float64)).permute(0, 2, 3, 1)
    xd, rd, ad, pk = _nhwc(x), _nhwc(res), _nhwc(act), ops.pack_weights(wt.to(DEV).contiguous())
    av = ad.view(n, h, w, cout // 4, 4)
    bits = ((av[..., 0] > 0).to(torch.uint8) | ((av[..., 1] > 0).to(torch.uint8) << 1) | ((av[..., 2] > 0).to(torch.uint8) << 2)
            | ((av[..., 3] > 0).to(torch.uint8) << 3)).contiguous()
    errs = {}
    for emu in (False, True):
        y = torch.full((n, h, w, cout), float('nan'), device=DEV)
        with ops.emulation('force' if emu else 'off'):
            l = ops.conv_forward(xd, pk, y, 1, 1, 0, res1=rd, mask_bits=bits)
        assert (l.variant == 'bx3_64') == emu, l.variant
        l.run()
        ops.sync_check()
        errs[emu] = float((y.cpu().double() - ref).norm() / ref.norm())
    assert errs[True] < 1e-6 and errs[True] <= 1.5 * errs[False] + 1e-8, errs
    from tests.conftest import record_achieved
    record_achieved('[bf16x3 emulation, masked data gradient %d -> %d + residual, mask nibbles] rel-L2 vs fp64 %.2e (native %.2e)'
                    % (cin, cout, errs[True], errs[False]))


@pytest.mark.parametrize('cin,cout,n,h,w', [(512, 128, 16, 100, 168), (1024, 256, 16, 50, 84)])
def test_bx3_conv3_data_gradient_masked_by_nibbles_made_from_the_activation(ops, cin, cout, n, h, w):
    """conv3's data gradient of a frozen Bottleneck: g_a2 = [a2 > 0] W3^T g (K = 4 x planes: passes over k, the mask in the last
    one beside the partial result).  The nibbles come from hnd_relu_mask_nibbles(a2) (byte-exact against torch), the result
    equals the native kernel's fp32-mask launch within the emulation's error."""
    g = torch.Generator().manual_seed(17 + cin)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    act = torch.randn(n, cout, h, w, generator=g).relu()                # a2: post-ReLU, half of it exact zeros
    ref = torch.where(act.double() > 0, F.conv2d(x.double(), wt.double()), torch.zeros((), dtype=torch.float64)).permute(0, 2, 3, 1)
    xd, ad, pk = _nhwc(x), _nhwc(act), ops.pack_weights(wt.to(DEV).contiguous())
    bits = ops.mask_nibbles_like(ad)
    ops.relu_mask_nibbles(ad, bits)
    av = ad.view(n, h, w, cout // 4, 4) > 0
    want_bits = (av[..., 0].to(torch.uint8) | (av[..., 1].to(torch.uint8) << 1) | (av[..., 2].to(torch.uint8) << 2)
                 | (av[..., 3].to(torch.uint8) << 3))
    assert torch.equal(bits, want_bits)
    y0 = torch.full((n, h, w, cout), float('nan'), device=DEV)
    with ops.emulation('off'):
        l0 = ops.conv_forward(xd, pk, y0, 1, 1, 0, mask=ad)
    l0.run()
    y1 = torch.full_like(y0, float('nan'))
    with ops.emulation('force'):
        l1 = ops.conv_forward(xd, pk, y1, 1, 1, 0, mask_bits=bits)
    assert l1.variant == 'bx3_64' and not l0.variant.startswith('bx3'), (l0.variant, l1.variant)
    l1.run()
    ops.sync_check()
    e0 = float((y0.cpu().double() - ref).norm() / ref.norm())
    e1 = float((y1.cpu().double() - ref).norm() / ref.norm())
    assert torch.equal(y1 == 0, y0 == 0) or float(((y1 == 0) != (y0 == 0)).float().mean()) < 1e-6
    assert e1 < 1e-6 and e1 <= 1.5 * e0 + 1e-8, (e1, e0)
    from tests.conftest import record_achieved
    record_achieved('[bf16x3 emulation, conv3 data gradient %d -> %d, nibbles of a2] rel-L2 vs fp64 %.2e (native, fp32 mask %.2e)'
                    % (cin, cout, e1, e0))


def test_bx3_randomised_shapes_and_epilogues_against_the_native_kernel(ops):
    """seeded sweep over what bx3_applies admits: K in {128 ... 1024} (1 - 4 passes), 64 ... 1024 columns, ANY row count (tails
    of 1 ... 63 rows, M % 4 != 0, fewer chunks than teams), stride 1 / 2, every epilogue combination -- each beside the native kernel on the same operands (the two
    agree to the two roundings: every element within 3e-5 of the result's rms -- achieved 7e-6), twice for reproducible bits.  Hand-counted waits
    that were wrong for ONE combination of tail / passes / operands would show here as garbage, not as a small error."""
    import random
    rnd = random.Random(20261004)
    g = torch.Generator().manual_seed(99)
    done = 0
    for case in range(40):
        cin = rnd.choice([128, 256, 256, 512, 768, 1024])
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
        bits_in = None
        if mask_bits:
            bits_in = torch.randint(0, 16, (n, oh, ow, cout // 4), generator=g, dtype=torch.uint8).to(DEV)
            kw['mask_bits'] = bits_in
        pk = ops.pack_weights(wt)
        outs = []
        for emu in (False, True, True):
            y = torch.full((n, oh, ow, cout), float('nan'), device=DEV)
            mo = torch.full((n, oh, ow, cout // 4), 255, dtype=torch.uint8, device=DEV) if mask_out else None
            with ops.emulation('force' if emu else 'off'):
                l = ops.conv_forward(x, pk, y, 1, stride, 0, mask_out=mo, **kw)
            assert l.variant.startswith('bx3') == emu, (case, cin, cout, m, stride, res, relu, mask_out, mask_bits, l.variant)
            l.run()
            outs.append((y, mo))
        ops.sync_check()
        (y0, m0), (y1, m1), (y2, m2) = outs
        rms = float(y0.double().pow(2).mean().sqrt()) + 1e-30
        err = float((y1.double() - y0.double()).abs().max()) / rms
        assert not bool(torch.isnan(y1).any()) and err < 3e-5, (case, cin, cout, m, stride, res, relu, mask_out, mask_bits, err)
        assert torch.equal(y1, y2) and (m1 is None or torch.equal(m1, m2))
        if mask_out:        # the nibbles describe the values stored beside them
            yv = y1.view(n, oh, ow, cout // 4, 4) > 0
            want = (yv[..., 0].to(torch.uint8) | (yv[..., 1].to(torch.uint8) << 1) | (yv[..., 2].to(torch.uint8) << 2)
                    | (yv[..., 3].to(torch.uint8) << 3))
            assert torch.equal(m1, want)
        done += 1
    assert done >= 30, done
    from tests.conftest import record_achieved
    record_achieved('[bf16x3 emulation] %d randomised shape / epilogue cases agree with the native kernel within 3e-5 rms per element' % done)


def test_bx3_fpn_lateral_with_the_upsampled_top_down_map(ops):
    """FeaturePyramidNetwork inner block (torchvision 0.4.2 ops/feature_pyramid_network.py via
    /root/reference/src/models/org/rcnn.py:399-414): 1x1 conv + bias + F.interpolate(coarser, size=..., mode='nearest')"""
    g = torch.Generator().manual_seed(31)
    n, cin, cout, h, w = 8, 256, 256, 96, 128
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    bias = torch.randn(cout, generator=g)
    top = torch.randn(n, cout, h // 2, w // 2, generator=g)
    ref = (F.conv2d(x.double(), wt.double(), bias.double()) + F.interpolate(top.double(), size=(h, w), mode='nearest')).permute(0, 2, 3, 1)
    xd, td, pk = _nhwc(x), _nhwc(top), ops.pack_weights(wt.to(DEV).contiguous())
    errs = {}
    for emu in (False, True):
        y = torch.full((n, h, w, cout), float('nan'), device=DEV)
        with ops.emulation('force' if emu else 'off'):
            l = ops.conv_forward(xd, pk, y, 1, 1, 0, epi_shift=bias.to(DEV), res1=td, res1_up=True)
        assert (l.variant == 'bx3_64') == emu, l.variant
        l.run()
        ops.sync_check()
        errs[emu] = float((y.cpu().double() - ref).norm() / ref.norm())
    assert errs[True] < 1e-6 and errs[True] <= 1.5 * errs[False] + 1e-8, errs
    from tests.conftest import record_achieved
    record_achieved('[bf16x3 emulation, FPN lateral 256 -> 256 + upsampled top-down map] rel-L2 vs fp64 %.2e (native %.2e)'
                    % (errs[True], errs[False]))


@pytest.mark.parametrize('c,n,h,w', [(256, 8, 96, 132), (128, 8, 102, 168), (512, 16, 48, 66)])
def test_bx3_winograd_component_gemms_match_the_native_path(ops, c, n, h, w):
    """a frozen 3x3 conv through F(6x6,3x3): the 64 component GEMMs on the emulation vs on the native kernel; both held to
    the direct fp64 convolution"""
    g = torch.Generator().manual_seed(77 + c)
    x = torch.randn(n, c, h, w, generator=g).relu()
    wt = torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5
    ref = F.conv2d(x.double(), wt.double(), None, 1, 1).permute(0, 2, 3, 1)
    xd, wd = _nhwc(x), wt.to(DEV).contiguous()
    outs = {}
    for emu in (False, True):
        ww = ops.WinoWeights(wd, False, 6)
        nv, nm = ops.WinoConv.scratch_elems(n, h, w, c, c, 6)
        v, m = torch.empty(nv, device=DEV), torch.empty(nm, device=DEV)
        y = torch.full((n, h, w, c), float('nan'), device=DEV)
        with ops.emulation('force' if emu else 'off'):
            conv = ops.WinoConv(xd, ww, y, v, m)
        assert (conv.gemm.variant == 'bx3_64') == emu, conv.gemm.variant
        conv.run()
        ops.sync_check()
        outs[emu] = y.cpu().double()
    e0 = float((outs[False] - ref).norm() / ref.norm())
    e1 = float((outs[True] - ref).norm() / ref.norm())
    assert e1 < 2e-5 and e1 <= 1.5 * e0, (e1, e0)                 # (the Winograd transforms' own fp32 error dominates)
    from tests.conftest import record_achieved
    record_achieved('[bf16x3 emulation, F(6x6,3x3) %d ch @%dx%d] rel-L2 vs the direct fp64 conv %.2e (native %.2e)' % (c, h, w, e1, e0))


LAYERS = [   # (cin, cout, h, w, stride): 1x1 launches of the frozen layers and the FPN at 800x1344 (and two that stay native)
    (256, 128, 200, 336, 1), (512, 128, 100, 168, 1), (128, 512, 100, 168, 1), (1024, 256, 50, 84, 1), (256, 1024, 50, 84, 1),
    (512, 2048, 25, 42, 1), (2048, 512, 25, 42, 1), (256, 256, 200, 336, 1), (2048, 256, 25, 42, 1), (256, 512, 200, 336, 2),
]


def test_bx3_choice_and_image_depend_on_the_layer_and_never_on_the_batch(ops):
    """whether a launch runs on the emulation is decided by hnd_bf16x3_recommended from the rows ONE
    image contributes, the depth and the output channels; the batch of the launch changes nothing -- also for row counts
    that are no multiple of 64 or of 4 (25 x 42 = 1050 rows per image) and for fewer chunks than teams (batch 1)."""
    picked = []
    for cin, cout, h, w, stride in LAYERS:
        wt = torch.randn(cout, cin, 1, 1).to(DEV) / cin ** 0.5
        pk = ops.pack_weights(wt)
        assert ops.bx3_on() and pk.bx3 is None and pk.bxs is None       # no image before a launch asks for one
        oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
        variants = set()
        for n in (1, 2, 3, 16):
            x = torch.empty(n, h, w, cin, device=DEV)
            y = torch.empty(n, oh, ow, cout, device=DEV)
            variants.add(ops.conv_forward(x, pk, y, 1, stride, 0, relu=True).variant.startswith('bx3'))
        assert len(variants) == 1, (cin, cout, h, w, variants)
        assert variants.pop() == ops.bx3_recommended(oh * ow, cin, cout)
        picked.append(ops.bx3_recommended(oh * ow, cin, cout))
        assert (pk.bx3 is not None) == picked[-1], (cin, cout, h, w)          # an image only where the policy picked it
    assert any(picked) and not all(picked), picked
    # Winograd component GEMMs fold the batch into their row count: the launch states rows per image itself
    wd = (torch.randn(256, 256, 3, 3) / 48).to(DEV)
    ww = ops.WinoWeights(wd, False, 6)
    vs = set()
    for n in (1, 2, 16):
        nv, nm = ops.WinoConv.scratch_elems(n, 50, 84, 256, 256, 6)
        conv = ops.WinoConv(torch.empty(n, 50, 84, 256, device=DEV), ww, torch.empty(n, 50, 84, 256, device=DEV),
                            torch.empty(nv, device=DEV), torch.empty(nm, device=DEV))
        vs.add(conv.gemm.variant)
    assert vs == {'bx3_64'} and ww.bx3 is not None and ww.bxs is None, vs


@pytest.mark.parametrize('cin,cout,h,w,stride,epi', [
    (256, 128, 100, 168, 1, 'relu'), (512, 2048, 25, 42, 1, 'res_relu_bits'), (1024, 256, 50, 84, 1, 'relu'),
    (2048, 512, 25, 42, 1, 'mask'), (256, 512, 67, 131, 2, 'none'), (128, 512, 37, 75, 1, 'res_mask')])
def test_bx3_rows_have_the_same_bits_alone_and_inside_any_batch(ops, cin, cout, h, w, stride, epi):
    """'same bits within a family' (VERDICT r5 item 1(d)): the emulated result of an image's rows does not depend on where the
    rows sit in the launch -- which team / wave / chunk computes them, how many passes run beside them, whether they end in
    a clamped tail (M % 64 != 0, M % 4 != 0) -- because every row's k chain is the same fixed order.  Image i of a batch
    of 5 == the same image alone == the same image as the last of 3, bit for bit."""
    g = torch.Generator().manual_seed(41 + cin + cout)
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = (torch.randn(5, h, w, cin, generator=g) * 2.0).to(DEV)
    res = torch.randn(5, oh, ow, cout, generator=g).to(DEV)
    bits = torch.randint(0, 16, (5, oh, ow, cout // 4), generator=g, dtype=torch.uint8).to(DEV)
    wt = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(DEV)
    es, eb = (torch.rand(cout, generator=g) + 0.5).to(DEV), torch.randn(cout, generator=g).to(DEV)
    pk = ops.pack_weights(wt)

    def run(sel):
        xs, n = x[sel].contiguous(), len(sel)
        y = torch.full((n, oh, ow, cout), float('nan'), device=DEV)
        kw = dict(epi_scale=es, epi_shift=eb)
        mo = None
        if epi in ('relu', 'res_relu_bits'):
            kw['relu'] = True
        if epi in ('res_relu_bits', 'res_mask'):
            kw['res1'] = res[sel].contiguous()
        if epi == 'res_relu_bits':
            mo = torch.full((n, oh, ow, cout // 4), 255, dtype=torch.uint8, device=DEV)
            kw['mask_out'] = mo
        if epi in ('mask', 'res_mask'):
            kw['mask_bits'] = bits[sel].contiguous()
        with ops.emulation('force'):
            l = ops.conv_forward(xs, pk, y, 1, stride, 0, **kw)
        assert l.variant == 'bx3_64', l.variant
        l.run()
        ops.sync_check()
        return y, mo

    y5, m5 = run([0, 1, 2, 3, 4])
    assert not bool(torch.isnan(y5).any())
    for sel in ([0], [3], [4], [1, 2, 4]):
        ys, ms = run(sel)
        for j, i in enumerate(sel):
            assert torch.equal(ys[j], y5[i]), (sel, i)
            assert ms is None or torch.equal(ms[j], m5[i])


def _rowsum_abs(x, wt):
    return x.abs().double().flatten(0, 2) @ wt.abs().double().flatten(1).t()


def test_weight_images_are_made_by_the_first_launch_and_follow_every_repack(ops):
    """A packed operand has no pre-split image until a launch descriptor asks for one (a re-pack makes none); attaching makes
    it from the CURRENT weights, and from then on every re-pack refreshes it in place -- also one made while the emulation
    is off -- so the launch always computes with the current weights, bit for bit what a freshly packed operand gives.
    The Winograd operands (grouped: one matrix per component GEMM) follow the same rule."""
    g = torch.Generator().manual_seed(5)
    for k, cin, cout, h, w, pad in ((1, 256, 128, 40, 64, 0), (2, 64, 128, 41, 65, 1)):
        x = torch.randn(2, h, w, cin, generator=g).to(DEV)
        wt = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(DEV)
        oh, ow = ops.conv_out_size(h, k, 1, pad), ops.conv_out_size(w, k, 1, pad)
        y, y_ref = torch.empty(2, oh, ow, cout, device=DEV), torch.empty(2, oh, ow, cout, device=DEV)

        def fresh():
            with ops.emulation('force'):
                launch = ops.conv_forward(x, ops.pack_weights(wt), y_ref, k, 1, pad)
            launch.run()
            ops.sync_check()
            return launch.variant, y_ref.clone()

        pk = ops.pack_weights(wt)
        assert pk.bx3 is None and pk.bxs is None                # no launch has asked: no image
        wt.mul_(1.5).add_(0.01)                                 # an optimizer step
        pk.repack()
        assert pk.bx3 is None and pk.bxs is None                # a re-pack makes none
        with ops.emulation('force'):
            launch = ops.conv_forward(x, pk, y, k, 1, pad)      # attaching makes it from the current weights
        img = pk.bx3 if k == 1 else pk.bxs
        assert img is not None
        launch.run()
        ops.sync_check()
        variant, want = fresh()
        assert launch.variant == variant and variant.startswith('bx3' if k == 1 else 'bxs'), (launch.variant, variant)
        assert torch.equal(y, want)
        wt.mul_(0.5).sub_(0.02)                                 # the next step: the re-pack refreshes the image itself
        with ops.emulation('off'):
            pk.repack()
        assert (pk.bx3 if k == 1 else pk.bxs) is img
        launch.run()
        ops.sync_check()
        assert torch.equal(y, fresh()[1])
    # F(6x6,3x3) and F(6x6,2x2) weights, 256 deep: the launch built under 'force', the weights changed, the re-pack made
    # while the emulation is off -- the launch must not go on with the old image
    c, n, h, w = 256, 2, 30, 42
    x = torch.randn(n, h, w, c, generator=g).to(DEV)
    for make, k in ((ops.WinoWeights, 3), (ops.Wino2Weights, 2)):
        wt = (torch.randn(c, c, k, k, generator=g) / (c * k * k) ** 0.5).to(DEV)

        oh, ow = (h, w) if k == 3 else (h + 1, w + 1)          # (the 2x2 conv with padding 1)

        def build(ww, out):
            if k == 3:
                nv, nm = ops.WinoConv.scratch_elems(n, h, w, c, c, 6)
                return ops.WinoConv(x, ww, out, torch.empty(nv, device=DEV), torch.empty(nm, device=DEV))
            nv, nm = ops.Wino2Conv.scratch_elems(n, oh, ow, c, c, 6)
            return ops.Wino2Conv(x, ww, out, torch.empty(nv, device=DEV), torch.empty(nm, device=DEV), 1)

        ww = make(wt, False, 6)
        assert ww.bx3 is None and ww.bxs is None
        y, y_ref = torch.empty(n, oh, ow, c, device=DEV), torch.empty(n, oh, ow, c, device=DEV)
        with ops.emulation('force'):
            conv = build(ww, y)
        img = ww.bx3
        assert conv.gemm.variant == 'bx3_64' and img is not None and ww.bxs is None, conv.gemm.variant
        wt.mul_(1.5).add_(0.01)
        with ops.emulation('off'):
            ww.repack()
        assert ww.bx3 is img
        conv.run()
        with ops.emulation('force'):
            ref = build(make(wt, False, 6), y_ref)
        assert ref.gemm.variant == conv.gemm.variant
        ref.run()
        ops.sync_check()
        assert not bool(torch.isnan(y).any()) and torch.equal(y, y_ref), make.__name__


def test_bx3_non_finite_inputs_are_loud_and_denormals_behave_as_documented(ops):
    """VERDICT r5 item 1(b), through hnd_conv2d_igemm (include/hnd_hip.h, hnd_conv_desc.w_bf16x3 'DEVIATIONS'):
    (i) an Inf / -Inf / NaN anywhere in an A row makes EVERY output of that row non-finite -- never a finite value -- and
    leaves every other row's bits alone; a non-finite weight does the same to its output channel;
    (ii) tiny operands (the header's bounds: |x| < 2^-126 may count as zero, 2^-126 <= |x| < 2^-110 may lose their mid / lo
    planes, anything larger is exact): asserted at ~10x the ACHIEVED figures -- 9e-6 of sum |a||b| in the middle range, 3.4e-2
    for denormal inputs (the pipe keeps their hi plane), 3e-7 above 2^-110; native fp32 MFMA: 4e-7 ... 5e-6."""
    g = torch.Generator().manual_seed(1234)
    n, h, w, cin, cout = 2, 64, 96, 256, 256
    x = torch.randn(n, h, w, cin, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / 16
    xd = x.to(DEV)

    def run(xt, wtt, emu=True):
        pk = ops.pack_weights(wtt.to(DEV).contiguous())
        y = torch.full((n, h, w, cout), 7.0, device=DEV)
        with ops.emulation('force' if emu else 'off'):
            l = ops.conv_forward(xt, pk, y, 1, 1, 0)
        assert l.variant.startswith('bx3') == emu
        l.run()
        ops.sync_check()
        return y.view(-1, cout)

    clean = run(xd, wt)
    assert bool(torch.isfinite(clean).all())
    # (i) A rows.  rows 5 / 4097 / 9000 (a different chunk, wave and lane group each), one bad element per row
    bad = {5: (17, float('inf')), 4097: (200, float('-inf')), 9000: (255, float('nan')), 12287: (0, float('inf'))}
    xb = xd.clone().view(-1, cin)
    for r, (k, v) in bad.items():
        xb[r, k] = v
    yb = run(xb.view(n, h, w, cin), wt)
    rows = torch.tensor(sorted(bad), device=DEV)
    assert not bool(torch.isfinite(yb[rows]).any()), 'a finite value came out of a row that holds Inf / NaN'
    keep = torch.ones(yb.shape[0], dtype=torch.bool, device=DEV)
    keep[rows] = False
    assert torch.equal(yb[keep], clean[keep])                          # nobody else's bits move
    yn = run(xb.view(n, h, w, cin), wt, emu=False)
    assert not bool(torch.isfinite(yn[rows]).any())                      # (the native kernel: non-finite there too, +-Inf / NaN)
    # an exact-zero weight column meets the Inf: 0 * Inf is NaN in fp32 as well
    # (i') a non-finite weight: its whole output channel
    wb = wt.clone()
    wb[3, 100, 0, 0] = float('inf')
    wb[130, 7, 0, 0] = float('nan')
    yw = run(xd, wb)
    cols = torch.tensor([3, 130], device=DEV)
    assert not bool(torch.isfinite(yw[:, cols]).any())
    kc = torch.ones(cout, dtype=torch.bool, device=DEV)
    kc[cols] = False
    assert torch.equal(yw[:, kc], clean[:, kc])
    # (ii) tiny operands
    from tests.conftest import record_achieved
    for name, scale, frac in (('2^-126 <= |x| < 2^-110', 2.0 ** -118, 1e-4), ('denormal |x| < 2^-126', 2.0 ** -130, 0.35),
                              ('|x| >= 2^-110 (exact planes; partial products near 2^-126)', 2.0 ** -100, 3e-6)):
        xt = (x.sign() * (x.abs().clamp(2.0 ** -6, 8.0)) * scale)
        if name.startswith('denormal'):
            assert float(xt.abs().max()) < 2.0 ** -126
        ref = (xt.double().flatten(0, 2) @ wt.double().flatten(1).t())
        bound = _rowsum_abs(xt, wt)
        ye = run(xt.to(DEV), wt).cpu().double()
        assert bool(torch.isfinite(ye).all())
        worst = float(((ye - ref).abs() / bound).max())
        assert worst <= frac * 1.001, (name, worst, frac)
        yn_ = run(xt.to(DEV), wt, emu=False).cpu().double()
        record_achieved('[bf16x3 emulation, tiny operands %s] worst |y - exact| / sum|a||b| = %.2e (documented bound %.1e; '
                        'native fp32 MFMA %.2e)' % (name, worst, frac, float(((yn_ - ref).abs() / bound).max())))
    record_achieved('[bf16x3 emulation, non-finite] Inf / -Inf / NaN in 4 A rows and 2 weight rows: every dependent output '
                    'non-finite, every other output bit-identical to the clean run')


def test_full_size_reference_fixture_passes_with_the_emulation_switched_off():
    """HND_BF16X3=0 -- native fp32 MFMA everywhere, the `value_native_fp32` leg of bench.py -- stays a supported build: the
    reference-made full-size fixture (batch 4, 3x800x1333; maps, loss terms, gradient fingerprints, parameters after Adam)
    under the ordinary bars.  (The default build runs the same test in tests/test_model_gpu.py.)"""
    env = dict(os.environ, HND_BF16X3='0')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-m', 'gpu',
                        'tests/test_model_gpu.py::test_full_size_step_matches_reference_checksums',
                        '-k', 'full_ghnd_faster_b4 or full_hnd_faster_b2'], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=1500)
    text = r.stdout.decode()
    assert r.returncode == 0, text[-3000:]
    from tests.conftest import record_achieved
    for line in text.splitlines():
        if line.startswith('[full size'):
            record_achieved('[HND_BF16X3=0, native fp32 MFMA] ' + line)
