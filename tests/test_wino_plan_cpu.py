"""CPU: the plan entries of the Winograd launches -- ops.WinoConv, ops.Wino2Conv (forward, and the data gradient with the
BatchNorm-backward sums), ops.Wino2InputTransform + ops.Wino2Wgrad (operands swapped and not) and ops.wino26_bnbwd_step --
held to literals: every (tag, kernel, variant, flops, alg_flops, hbm_bytes) of launches() / step(), tiles_pad, the shapes
of the v / m / z views and scratch_elems, at the smallest geometries with a ragged last tile, for every tile size.

The literals of EXPECT were recorded by running observe() below on the commit BEFORE the launch classes were folded into
one base class (four hand-written classes then), never from what the present classes print: a change to the launch
classes that moves one byte count, label, kernel pick or view shape fails here.

Building a launch runs nothing: the descriptors, the library's size and dispatch queries and the views work on host
tensors, so this file needs the library and no device (the queries assume the 256 compute units of the MI355X where they
find none).  The weight operands are ops.PackedWeight stand-ins of the shape ops.WinoWeights / ops.Wino2Weights make
(whose transforms do need a device), as in tests/test_guard_bands_gpu.py.  tests/test_wino_gpu.py holds the values."""
import pytest
import torch

N, HW = 2, 8                    # the 2x2 cases: 8x8 inputs -> 7x7 (pad 0) / 9x9 (pad 1) outputs, ragged for tiles 4 and 6


@pytest.fixture(scope='module')
def ops():
    from hnd_ghnd_object_detectors_amd import ops as o
    return o


def weights(ops, k, cout, cin, tile, dgrad=False):
    """the operand of ops.WinoWeights (k = 3) / ops.Wino2Weights (k = 2) of a [cout, cin, k, k] weight, left unfilled"""
    rows, depth = (cin, cout) if dgrad else (cout, cin)
    ncomp, rows_pad = (tile + k - 1) ** 2, (rows + 63) // 64 * 64
    ww = ops.PackedWeight(buf(ncomp * rows_pad * depth), rows, depth, depth, groups=ncomp, group_stride=rows_pad * depth)
    ww.tile, ww.ncomp, ww.depth, ww.K, ww.dgrad = tile, ncomp, depth, k, dgrad
    return ww


def buf(*shape):
    return torch.zeros(shape)


def entries(pairs):
    return [(tag, getattr(l, 'kernel', None), l.variant, l.flops, l.alg_flops, getattr(l, 'hbm_bytes', None))
            for l, tag in pairs]


def views(launch, *names):
    return {k: tuple(getattr(launch, k).shape) for k in names}


def conv_case(l, scratch):
    """what a WinoConv / Wino2Conv holds: its plan, sizes and views, and the grouping of its component GEMMs"""
    d = l.gemm.desc
    return dict(plan=entries(l.launches('t')), tiles_pad=l.tiles_pad, scratch=scratch, geom=tuple(l.geom), cout=l.cout,
                gemm=(d.ow, d.w_group_rows, d.w_group_stride), **views(l, 'v', 'm'))


WGRAD_FIELDS = ('w_', 'ow', 'cin', 'cin_real', 'cout', 'ldy', 'groups', 'x_group_stride', 'dy_group_stride', 'dw_group_stride')


def wgrad_case(ops, wg):
    """what a Wino2Wgrad holds: its plan, the grouped split-K descriptor and the workspace that descriptor asks for"""
    return dict(plan=entries(wg.launches('t')), wgrad_geom=tuple(wg.geom), swapped=wg.swapped, tile=wg.tile,
                z=tuple(wg.z.shape), desc=tuple(getattr(wg.gemm.desc, f) for f in WGRAD_FIELDS),
                workspace=ops.wgrad_workspace_of(wg.gemm.desc))


def wino_conv(ops, tile):
    """WinoConv, N = 2, 7x7, 32 -> 32, with a residual and (tiles 4 / 6) mask_out: every term of the output bytes"""
    n, h, c = 2, 7, 32
    ww = weights(ops, 3, c, c, tile)
    nv, nm = ops.WinoConv.scratch_elems(n, h, h, c, c, tile)
    y = buf(n, h, h, c)
    l = ops.WinoConv(buf(n, h, h, c), ww, y, buf(nv), buf(nm), pro_scale=buf(c), epi_shift=buf(c), res1=buf(n, h, h, c),
                     relu=True, mask_out=ops.mask_nibbles_like(y) if tile != 2 else None)
    return dict(conv_case(l, (nv, nm)), pro_shift=tuple(l.pro[1].shape))


def wino2_forward(ops, tile, pad, cin=64, cout=128, stats=True):
    n, o = N, HW + 2 * pad - 1
    ww = weights(ops, 2, cout, cin, tile)
    nv, nm = ops.Wino2Conv.scratch_elems(n, o, o, cin, cout, tile)
    st = buf(ops.Wino2Conv.stats_blocks(n, o, o, cout, tile), 2, cout) if stats else None
    return ops.Wino2Conv(buf(n, HW, HW, cin), ww, buf(n, o, o, cout), buf(nv), buf(nm), pad, pro_scale=buf(cin),
                         pro_relu=True, stats=st), (nv, nm)


def wino2_conv(ops, tile, pad):
    """Wino2Conv forward, N = 2, 8x8 input, 64 -> 128, BN(+ReLU) prologue without a shift, statistics"""
    l, scratch = wino2_forward(ops, tile, pad)
    return dict(conv_case(l, scratch), pad=l.pad, pro_shift=tuple(l.pro[1].shape))


def wino2_dgrad(ops, with_sums=True):
    """the data gradient of the pad-0 conv above at tile 6: dy [2, 7, 7, 128] -> dx [2, 8, 8, 64], with the
    BatchNorm-backward partial sums of dx from the output transform"""
    n, cin, cout, o = N, 64, 128, HW - 1
    wd = weights(ops, 2, cout, cin, 6, dgrad=True)
    nv, nm = ops.Wino2Conv.scratch_elems(n, HW, HW, cout, cin, 6)
    dx = buf(n, HW, HW, cin)
    part = buf(ops.Wino2Conv.stats_blocks(n, HW, HW, cin, 6), 2, cin)
    bwd = (buf(n, HW, HW, cin), buf(cin), buf(cin), buf(cin), buf(cin), True, part) if with_sums else None
    return ops.Wino2Conv(buf(n, o, o, cout), wd, dx, buf(nv), buf(nm), 1, bwd_stats=bwd), (nv, nm)


def wino2_dgrad_sums(ops):
    l, scratch = wino2_dgrad(ops)
    return dict(conv_case(l, scratch), pad=l.pad)


def wgrad_under(ops, swap, *args):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('HND_WGRAD_SWAP', '1' if swap else '0')
        return ops.Wino2Wgrad(*args)


def wino2_wgrad(ops, swap):
    """Wino2InputTransform + Wino2Wgrad, N = 2, 8x8 input, pad 1, 64 -> 256, tile 6, under HND_WGRAD_SWAP = 1 / 0: this
    shape is the ring kernel's as it stands, so neither setting exchanges its operands"""
    n, cin, cout, o = N, 64, 256, HW + 1
    nv = ops.Wino2InputTransform.scratch_elems(n, o, o, cin, 6)
    own = ops.Wino2InputTransform(buf(n, HW, HW, cin), buf(nv), 1, cout, 6, pro_scale=buf(cin))
    nz = ops.Wino2Conv.scratch_elems(n, o, o, cin, cout, 6)[1]
    wg = wgrad_under(ops, swap, own, buf(n, o, o, cout), buf(cout, cin, 2, 2), buf(nz), buf(49 * cout * cin))
    return dict(wgrad_case(ops, wg), step=entries([own.step('t')]), tiles_pad=own.tiles_pad, scratch=(nv, nz),
                geom=tuple(own.geom), own_tile=own.tile, pro_shift=tuple(own.pro[1].shape), v=tuple(own.v.shape))


def wino2_wgrad_64_rows(ops, swap):
    """Wino2Wgrad on the V of a Wino2Conv forward, 256 -> 64 (same input, pad 1, tile 6): 64 output channels, the shape
    whose operands HND_WGRAD_SWAP = 1 exchanges for the ring kernel"""
    n, cin, cout, o = N, 256, 64, HW + 1
    fwd, scratch = wino2_forward(ops, 6, 1, cin, cout, stats=False)
    wg = wgrad_under(ops, swap, fwd, buf(n, o, o, cout), buf(cout, cin, 2, 2), buf(scratch[1]), buf(49 * cout * cin))
    return wgrad_case(ops, wg)


def bnbwd_step(ops):
    """wino26_bnbwd_step over the dy [2, 7, 7, 128] of the pad-0 64 -> 128 conv: the tile-6 forward's weight gradient and
    the data gradient above"""
    fwd, _ = wino2_forward(ops, 6, 0, stats=False)
    n, c, o = N, 128, HW - 1
    nz = ops.Wino2Conv.scratch_elems(n, o, o, 64, c, 6)[1]
    g = buf(n, o, o, c)
    wg = ops.Wino2Wgrad(fwd, g, buf(c, 64, 2, 2), buf(nz), buf(49 * c * 64))
    dg, _ = wino2_dgrad(ops, with_sums=False)
    step = ops.wino26_bnbwd_step(g, buf(n, o, o, c), buf(c), buf(c), buf(3, c), True, dg, wg)
    return dict(wgrad_case(ops, wg), step=entries([(step, 't')]))


def observe(ops):
    r = {}
    for tile in (2, 4, 6):
        r['WinoConv tile %d' % tile] = wino_conv(ops, tile)
    for pad in (0, 1):
        for tile in (4, 6):
            r['Wino2Conv pad %d tile %d' % (pad, tile)] = wino2_conv(ops, tile, pad)
    r['Wino2Conv dgrad bwd_stats'] = wino2_dgrad_sums(ops)
    for swap in (1, 0):
        r['Wino2Wgrad own 64 -> 256 HND_WGRAD_SWAP %d' % swap] = wino2_wgrad(ops, swap)
        r['Wino2Wgrad fwd 256 -> 64 HND_WGRAD_SWAP %d' % swap] = wino2_wgrad_64_rows(ops, swap)
    r['bnbwd_step'] = bnbwd_step(ops)
    return r


# recorded on the commit before the refactor (see the module docstring)
EXPECT = {'Wino2Conv dgrad bwd_stats': {'cout': 64,
                               'gemm': (6272, 128, 8192),
                               'geom': (2, 7, 7, 128, 8, 8),
                               'm': (1, 1, 6272, 64),
                               'pad': 1,
                               'plan': [('t.wino_in', 'wino2_input', 'transform', 0, 0, 250880),
                                        ('t', None, 'igemm_64x64', 6422528, 8388608, None),
                                        ('t.wino_out', 'wino2_output', 'transform', 0, 0, 165888)],
                               'scratch': (802816, 401408),
                               'tiles_pad': 128,
                               'v': (1, 1, 6272, 128)},
 'Wino2Conv pad 0 tile 4': {'cout': 128,
                            'gemm': (3200, 128, 8192),
                            'geom': (2, 8, 8, 64, 7, 7),
                            'm': (1, 1, 3200, 128),
                            'pad': 0,
                            'plan': [('t.wino_in', 'wino2_input', 'transform', 0, 0, 83968),
                                     ('t', None, 'igemm_64x64', 3276800, 6422528, None),
                                     ('t.wino_out', 'wino2_output', 'transform', 0, 0, 152576)],
                            'pro_shift': (64,),
                            'scratch': (204800, 409600),
                            'tiles_pad': 128,
                            'v': (1, 1, 3200, 64)},
 'Wino2Conv pad 0 tile 6': {'cout': 128,
                            'gemm': (6272, 128, 8192),
                            'geom': (2, 8, 8, 64, 7, 7),
                            'm': (1, 1, 6272, 128),
                            'pad': 0,
                            'plan': [('t.wino_in', 'wino2_input', 'transform', 0, 0, 133120),
                                     ('t', None, 'igemm_64x64', 6422528, 6422528, None),
                                     ('t.wino_out', 'wino2_output', 'transform', 0, 0, 250880)],
                            'pro_shift': (64,),
                            'scratch': (401408, 802816),
                            'tiles_pad': 128,
                            'v': (1, 1, 6272, 64)},
 'Wino2Conv pad 1 tile 4': {'cout': 128,
                            'gemm': (3200, 128, 8192),
                            'geom': (2, 8, 8, 64, 9, 9),
                            'm': (1, 1, 3200, 128),
                            'pad': 1,
                            'plan': [('t.wino_in', 'wino2_input', 'transform', 0, 0, 147968),
                                     ('t', None, 'igemm_64x64', 7372800, 10616832, None),
                                     ('t.wino_out', 'wino2_output', 'transform', 0, 0, 313344)],
                            'pro_shift': (64,),
                            'scratch': (204800, 409600),
                            'tiles_pad': 128,
                            'v': (1, 1, 3200, 64)},
 'Wino2Conv pad 1 tile 6': {'cout': 128,
                            'gemm': (6272, 128, 8192),
                            'geom': (2, 8, 8, 64, 9, 9),
                            'm': (1, 1, 6272, 128),
                            'pad': 1,
                            'plan': [('t.wino_in', 'wino2_input', 'transform', 0, 0, 133120),
                                     ('t', None, 'igemm_64x64', 6422528, 10616832, None),
                                     ('t.wino_out', 'wino2_output', 'transform', 0, 0, 283648)],
                            'pro_shift': (64,),
                            'scratch': (401408, 802816),
                            'tiles_pad': 128,
                            'v': (1, 1, 6272, 64)},
 'Wino2Wgrad fwd 256 -> 64 HND_WGRAD_SWAP 0': {'desc': (8, 8, 256, 256, 64, 64, 49, 32768, 8192, 16384),
                                               'plan': [('t.wino_dy', 'wino2_dy', 'transform', 0, 0, 141824),
                                                        ('t', None, 'wgrad_m64', 12845056, 21233664, None),
                                                        ('t.wino_out', 'wino2_wgrad_output', 'transform', 0, 0, 3473408)],
                                               'swapped': False,
                                               'tile': 6,
                                               'wgrad_geom': (2, 9, 9, 64, 64, 256),
                                               'workspace': 3211264,
                                               'z': (401408,)},
 'Wino2Wgrad fwd 256 -> 64 HND_WGRAD_SWAP 1': {'desc': (8, 8, 64, 64, 256, 256, 49, 8192, 32768, 16384),
                                               'plan': [('t.wino_dy', 'wino2_dy', 'transform', 0, 0, 141824),
                                                        ('t', None, 'wgrad_ring', 12845056, 21233664, None),
                                                        ('t.wino_out', 'wino2_wgrad_output', 'transform', 0, 0, 3473408)],
                                               'swapped': True,
                                               'tile': 6,
                                               'wgrad_geom': (2, 9, 9, 64, 64, 256),
                                               'workspace': 6422528,
                                               'z': (401408,)},
 'Wino2Wgrad own 64 -> 256 HND_WGRAD_SWAP 0': {'desc': (8, 8, 64, 64, 256, 256, 49, 8192, 32768, 16384),
                                               'geom': (2, 8, 8, 64, 9, 9),
                                               'own_tile': 6,
                                               'plan': [('t.wino_dy', 'wino2_dy', 'transform', 0, 0, 567296),
                                                        ('t', None, 'wgrad_ring', 12845056, 21233664, None),
                                                        ('t.wino_out', 'wino2_wgrad_output', 'transform', 0, 0, 3473408)],
                                               'pro_shift': (64,),
                                               'scratch': (401408, 1605632),
                                               'step': [('t.wino_in', 'wino2_input', 'transform', 0, 0, 133120)],
                                               'swapped': False,
                                               'tile': 6,
                                               'tiles_pad': 128,
                                               'v': (1, 1, 6272, 64),
                                               'wgrad_geom': (2, 9, 9, 256, 256, 64),
                                               'workspace': 6422528,
                                               'z': (1605632,)},
 'Wino2Wgrad own 64 -> 256 HND_WGRAD_SWAP 1': {'desc': (8, 8, 64, 64, 256, 256, 49, 8192, 32768, 16384),
                                               'geom': (2, 8, 8, 64, 9, 9),
                                               'own_tile': 6,
                                               'plan': [('t.wino_dy', 'wino2_dy', 'transform', 0, 0, 567296),
                                                        ('t', None, 'wgrad_ring', 12845056, 21233664, None),
                                                        ('t.wino_out', 'wino2_wgrad_output', 'transform', 0, 0, 3473408)],
                                               'pro_shift': (64,),
                                               'scratch': (401408, 1605632),
                                               'step': [('t.wino_in', 'wino2_input', 'transform', 0, 0, 133120)],
                                               'swapped': False,
                                               'tile': 6,
                                               'tiles_pad': 128,
                                               'v': (1, 1, 6272, 64),
                                               'wgrad_geom': (2, 9, 9, 256, 256, 64),
                                               'workspace': 6422528,
                                               'z': (1605632,)},
 'WinoConv tile 2': {'cout': 32,
                     'gemm': (2048, 128, 2048),
                     'geom': (2, 7, 7, 32),
                     'm': (1, 1, 2048, 32),
                     'plan': [('t.wino_in', 'wino_input', 'transform', 0, 0, 78080),
                              ('t', None, 'igemm_64x64', 1048576, 1806336, None),
                              ('t.wino_out', 'wino_output', 'transform', 0, 0, 90624)],
                     'pro_shift': (32,),
                     'scratch': (65536, 65536),
                     'tiles_pad': 128,
                     'v': (1, 1, 2048, 32)},
 'WinoConv tile 4': {'cout': 32,
                     'gemm': (4608, 128, 2048),
                     'geom': (2, 7, 7, 32),
                     'm': (1, 1, 4608, 32),
                     'plan': [('t.wino_in', 'wino_input', 'transform', 0, 0, 49408),
                              ('t', None, 'igemm_64x64', 589824, 1806336, None),
                              ('t.wino_out', 'wino_output', 'transform', 0, 0, 62736)],
                     'pro_shift': (32,),
                     'scratch': (147456, 147456),
                     'tiles_pad': 128,
                     'v': (1, 1, 4608, 32)},
 'WinoConv tile 6': {'cout': 32,
                     'gemm': (8192, 128, 2048),
                     'geom': (2, 7, 7, 32),
                     'm': (1, 1, 8192, 32),
                     'plan': [('t.wino_in', 'wino_input', 'transform', 0, 0, 78080),
                              ('t', None, 'igemm_64x64', 1048576, 1806336, None),
                              ('t.wino_out', 'wino_output', 'transform', 0, 0, 91408)],
                     'pro_shift': (32,),
                     'scratch': (262144, 262144),
                     'tiles_pad': 128,
                     'v': (1, 1, 8192, 32)},
 'bnbwd_step': {'desc': (8, 8, 64, 64, 128, 128, 49, 8192, 16384, 8192),
                'plan': [('t.wino_dy', 'wino2_dy', 'transform', 0, 0, 250880),
                         ('t', None, 'wgrad_m128', 6422528, 6422528, None),
                         ('t.wino_out', 'wino2_wgrad_output', 'transform', 0, 0, 1736704)],
                'step': [('t', 'wino2_bnbwd_fused', 'transform', 0, 0, 501760)],
                'swapped': False,
                'tile': 6,
                'wgrad_geom': (2, 7, 7, 128, 128, 64),
                'workspace': 3211264,
                'z': (802816,)}}


@pytest.fixture(scope='module')
def observed(ops):
    with ops.emulation('off'):
        return observe(ops)


def test_every_case_has_its_literals(observed):
    assert sorted(observed) == sorted(EXPECT)


@pytest.mark.parametrize('case', sorted(EXPECT))
def test_winograd_plan_is_the_recorded_one(observed, case):
    assert observed[case] == EXPECT[case], (case, observed[case])
