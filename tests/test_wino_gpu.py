"""GPU: the Winograd path of csrc/winograd.hip against an fp64 reference, element by element.

The cases are the tables of tests/wino_util.py (tests/test_wino_cases_cpu.py holds their coverage conditions, the host
arithmetic and the teeth without a GPU).  Every forward / data-gradient case: NaN into the output, the scratch and the
statistics, launch through ops.WinoConv / ops.Wino2Conv, and hold the stored values to BOTH bars of wino_util.bars -- the
relative-to-max bar of tests/test_ops_gpu.py (< 1e-4 for tile 2, < 2e-4 for tiles 4 and 6) and, element by element,
|got - y64| <= (K + T) 2^-24 Bw + 1e-30 -- then the exact bits: mask_out nibbles of the values actually stored, the lanes
beyond cout (zeros up to the launch's own rounding of cout, untouched NaN beyond it), the rows of V in [tiles, tiles_pad)
(untouched NaN), and a second launch with the same bits.  Every buffer a launch writes is a view of a guard_util.Arena: a
store outside it damages a guard band."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_util as U
from tests import guard_util as G
from tests import wino_util as W

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
WORST = {}                              # (k, tile, direction) -> [ratio, case]


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


@pytest.fixture(autouse=True)
def native_family(ops):
    with ops.emulation('off'):
        yield


@pytest.fixture(scope='module', autouse=True)
def achieved():
    from tests.conftest import record_achieved
    record_achieved(lambda: '\n'.join('[Winograd vs fp64, k %d tile %d %-5s] worst |got - ref| / ((K + T) 2^-24 Bw) %.3f (held to 1) at %s'
                                      % (key + tuple(WORST[key])) for key in sorted(WORST)))
    yield


def note(key, ratio, what):
    w = WORST.setdefault(key, [0.0, ''])
    if ratio > w[0]:
        w[0], w[1] = ratio, what


def to_nhwc(t_nchw, lanes):
    t = t_nchw.permute(0, 2, 3, 1)
    if t.shape[-1] != lanes:
        t = F.pad(t, (0, lanes - t.shape[-1]))
    return t.contiguous().to(DEV)


def vec(v, lanes):
    return F.pad(v, (0, lanes - v.numel())).to(DEV)


class Conv(object):
    """one forward / data-gradient case as a launch: the operands on the device, NaN canaries in everything it writes"""

    def __init__(self, ops, c, t):
        e = U.epi_of(c.epi)
        self.c, self.ldc = c, W.lanes_out(c) if 'bwd' in e else W.ldc_of(c)
        ldc = self.ldc
        x = to_nhwc(t['x'], c.cin)
        wp = t['wp'].to(DEV).contiguous()
        cls, wcls = (ops.WinoConv, ops.WinoWeights) if c.k == 3 else (ops.Wino2Conv, ops.Wino2Weights)
        ww = wcls(wp, dgrad=c.dgrad, tile=c.tile)
        nv, nm = cls.scratch_elems(c.n, c.oh, c.ow, c.cin, c.cout, c.tile)
        blocks, lo = W.stats_blocks(c), W.lanes_out(c)
        specs = [((nv,), torch.float32), ((nm,), torch.float32), ((c.n, c.oh, c.ow, ldc), torch.float32),
                 ((blocks, 2, lo), torch.float32), ((c.n, c.oh, c.ow, ldc // 4), torch.uint8)]
        self.arena = G.Arena(DEV, G.arena_bytes(specs))
        self.v, self.m, self.y = [self.arena.take(n_, sh) for n_, (sh, _) in zip(('v', 'm', 'y'), specs)]
        kw = dict(pro_relu=c.pro in ('relu', W.SCALE_RELU), relu='relu' in e)
        if 'ps' in t:
            kw['pro_scale'] = vec(t['ps'], c.cin)
        if 'pb' in t:
            kw['pro_shift'] = vec(t['pb'], c.cin)
        if 'es' in e:
            kw['epi_scale'] = vec(t['es'], ldc)
        if 'eb' in e:
            kw['epi_shift'] = vec(t['eb'], ldc)
        self.stats = self.mask_out = None
        if c.k == 3:
            for name, key in (('r1', 'res1'), ('mask', 'mask')):
                if name in e:
                    kw[key] = to_nhwc(t[name], ldc)
            if 'mout' in e:
                self.mask_out = kw['mask_out'] = self.arena.take('mask_out', specs[4][0], torch.uint8)
            self.launch = cls(x, ww, self.y, self.v, self.m, **kw)
        else:
            if 'stats' in e:
                assert cls.stats_blocks(c.n, c.oh, c.ow, W.lanes_out(c), c.tile) == W.stats_blocks(c)
                self.stats = kw['stats'] = self.arena.take('stats', specs[3][0])
            if 'bwd' in e:
                self.stats = self.arena.take('stats', specs[3][0])
                kw['bwd_stats'] = (to_nhwc(t['bx'], ldc), vec(t['bsc'], ldc), vec(t['bsh'], ldc), vec(t['bmu'], ldc),
                                   vec(t['brs'], ldc), 'lin' not in e, self.stats)
            self.launch = cls(x, ww, self.y, self.v, self.m, c.pad, **kw)
        assert self.launch.tiles_pad == c.tiles_pad

    def run(self, ops):
        """NaN into everything the launch writes, launch, wait -> copies of (y, stats, mask_out)"""
        for b in (self.y, self.v, self.m, self.stats):
            if b is not None:
                b.fill_(NAN)
        if self.mask_out is not None:
            self.mask_out.fill_(0xA5)
        self.launch.run()
        ops.sync_check()
        self.arena.check()
        # the input transform writes the rows of its own tiles and nothing else of V
        v = self.v.view(self.c.ncomp, self.c.tiles_pad, self.c.cin)
        assert not bool(torch.isnan(v[:, :self.c.tiles]).any()) and bool(torch.isnan(v[:, self.c.tiles:]).all())
        return (self.y.clone(), None if self.stats is None else self.stats.clone(),
                None if self.mask_out is None else self.mask_out.clone())


def hold_conv(ops, c, t, y64, bw, key):
    """every assertion of a forward / data-gradient case; y64 / bw on any device"""
    e = U.epi_of(c.epi)
    conv = Conv(ops, c, t)
    y, stats, mout = conv.run(ops)
    got = y[..., :c.cout].permute(0, 3, 1, 2).to(y64.device)
    assert not bool(torch.isnan(got).any()), 'NaN in the logical region'
    k_t = W.t_of(c.k, c.tile)
    rel, ratio = W.bars(got, y64, bw, c.cin, k_t)
    note(key, ratio, W.case_id(c))
    print('%s: relative to max %.3e, ratio to the element-wise bound %.4f' % (W.case_id(c), rel, ratio))
    assert rel < W.rel_bar(c.tile), (W.case_id(c), rel)
    assert ratio <= 1.0, (W.case_id(c), ratio)
    # the lanes beyond cout: zero weight rows up to the launch's own rounding of cout, nothing written beyond it
    lo = W.lanes_out(c)
    assert torch.equal(y[..., c.cout:lo], torch.zeros_like(y[..., c.cout:lo]))
    assert bool(torch.isnan(y[..., lo:]).all())
    if mout is not None:
        assert torch.equal(mout, U.nibbles(y))
    if 'stats' in e:
        assert not bool(torch.isnan(stats).any())
        sums = stats.double().sum(0)[:, :c.cout].to(y64.device)
        r1, r2 = U.stats_bars(sums, y64, bw, c.cin + k_t - 8, c.n * c.oh * c.ow)
        print('%s: statistics, ratios to their bounds %.4f %.4f' % (W.case_id(c), r1, r2))
        assert r1 <= 1.0 and r2 <= 1.0, (W.case_id(c), r1, r2)
    if 'bwd' in e:
        assert not bool(torch.isnan(stats).any())
        s64, lim = W.bwd_stats_reference(c, t, y64, bw)
        r = ((stats.double().sum(0).to(y64.device) - s64).abs() / lim).amax(1)
        print('%s: BN-backward sums, ratios to their bounds %.4f %.4f' % (W.case_id(c), float(r[0]), float(r[1])))
        assert float(r.max()) <= 1.0, (W.case_id(c), r)
    again = conv.run(ops)
    assert torch.equal(again[0][..., :lo], y[..., :lo])
    for a, b in zip(again[1:], (stats, mout)):
        assert b is None or torch.equal(a, b)


CONV_PARAMS = [pytest.param(key, c, id='%s-%s' % (key[2], W.case_id(c))) for key, cases in W.TABLES.items() for c in cases]


@pytest.mark.parametrize('key,c', CONV_PARAMS)
def test_winograd_conv_holds_to_fp64_element_by_element(ops, key, c):
    t, y64, bw = W.conv_case(c)
    hold_conv(ops, c, t, y64, bw, key)


@pytest.mark.parametrize('c', W.OVER_CASES, ids=W.case_id)
def test_transforms_walk_their_grid_stride_loop_a_second_time(ops, c):
    """more work items than kMaxBlocks * 256 in the input AND the output transform (wino_util.conv_work), or, for
    hnd_wino26_output_bnbwd_stats, than its 2048 blocks cover; the operands are drawn and the fp64 reference is computed on
    the device"""
    t = W.over_inputs(c, DEV)
    y64, bw = W.reference(c, t)
    hold_conv(ops, c, t, y64, bw, (c.k, c.tile, 'over' + (' bwd' if c is W.OVER_BWD else '')))


def test_a_depth_below_32_is_refused_by_the_wrappers(ops):
    w3 = torch.zeros(32, W.REFUSED_DEPTH, 3, 3, device=DEV)
    w2 = torch.zeros(32, W.REFUSED_DEPTH, 2, 2, device=DEV)
    for build in (lambda: ops.WinoWeights(w3, tile=4), lambda: ops.Wino2Weights(w2, tile=4),
                  lambda: ops.WinoWeights(w3.transpose(0, 1).contiguous(), dgrad=True, tile=2)):
        with pytest.raises(AssertionError, match='GEMM depth that is a multiple of 32'):
            build()


@pytest.mark.parametrize('tile', [4, 6])
def test_statistics_of_a_cout_that_does_not_divide_512_are_refused(ops, tile):
    c = W.case(2, tile, False, 1, 32, tile, tile, 96, 0, epi='stats')
    t = W.make_inputs(c)
    ww = ops.Wino2Weights(t['wp'].to(DEV).contiguous(), tile=tile)
    nv, nm = ops.Wino2Conv.scratch_elems(c.n, c.oh, c.ow, c.cin, c.cout, tile)
    y = torch.full((c.n, c.oh, c.ow, 96), NAN, device=DEV)
    stats = torch.full((W.stats_blocks(c), 2, 96), NAN, device=DEV)
    conv = ops.Wino2Conv(to_nhwc(t['x'], 32), ww, y, torch.zeros(nv, device=DEV), torch.zeros(nm, device=DEV), 0, stats=stats)
    with pytest.raises(RuntimeError, match='stats need 512 % cout == 0'):
        conv._run_output()
    ops.sync_check()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(stats).all())


@pytest.mark.parametrize('c,route,alias', W.WGRAD_CASES, ids=lambda v: W.case_id(v) if isinstance(v, W.Case) else str(v))
def test_winograd_weight_gradient_holds_to_fp64(ops, c, route, alias):
    """ops.Wino2Wgrad from a Wino2Conv forward ('fwd'; z aliasing the forward's m scratch or not) and from a
    Wino2InputTransform ('own'): dW against the fp64 weight gradient under (tiles + T) 2^-24 Bw, twice with the same bits"""
    t = W.wgrad_inputs(c)
    dw64, bw = W.wgrad_reference(c, t)
    x = to_nhwc(t['x'], c.cin)
    kw = dict(pro_relu=c.pro in ('relu', W.SCALE_RELU))
    if 'ps' in t:
        kw['pro_scale'] = vec(t['ps'], c.cin)
    if 'pb' in t:
        kw['pro_shift'] = vec(t['pb'], c.cin)
    nv, nm = ops.Wino2Conv.scratch_elems(c.n, c.oh, c.ow, c.cin, c.cout, c.tile)
    nz, ns = c.ncomp * c.tiles_pad * c.cout, c.ncomp * c.cout * c.cin
    specs = [((n_,), torch.float32) for n_ in (nv, nm, nz, ns)] + [((c.cout, c.cin, 2, 2), torch.float32)]
    arena = G.Arena(DEV, G.arena_bytes(specs))
    v, m, z_own, s, dw = [arena.take(name, sh) for name, (sh, _) in zip(('v', 'm', 'z', 's', 'dw'), specs)]
    if route == 'fwd':
        ww = ops.Wino2Weights(t['wp'].to(DEV).contiguous(), tile=c.tile)
        y = torch.empty(c.n, c.oh, c.ow, c.cout, device=DEV)
        fwd = ops.Wino2Conv(x, ww, y, v, m, c.pad, **kw)
        fwd.run()
    else:
        assert nv == ops.Wino2InputTransform.scratch_elems(c.n, c.oh, c.ow, c.cin, c.tile)
        fwd = ops.Wino2InputTransform(x, v, c.pad, c.cout, c.tile, **kw)
        fwd._run_input()
    z = m if alias else z_own
    wg = ops.Wino2Wgrad(fwd, to_nhwc(t['dy'], c.cout), dw, z, s)
    assert wg.swapped == W.wgrad_swapped(c), (wg.swapped, wg.variant)
    outs = []
    for _ in range(2):
        for b in (z, s, dw):
            b.fill_(NAN)
        wg.run()
        ops.sync_check()
        arena.check()
        zz = z[:nz].view(c.ncomp, c.tiles_pad, c.cout)
        assert not bool(torch.isnan(zz[:, :c.tiles]).any()) and bool(torch.isnan(zz[:, c.tiles:]).all())
        outs.append(dw.cpu().clone())
    assert not bool(torch.isnan(outs[0]).any())
    rel, ratio = W.bars(outs[0], dw64, bw, c.tiles, W.t_wgrad(c.tile))
    note((2, c.tile, 'wgrad'), ratio, W.case_id(c))
    print('%s %s%s: relative to max %.3e, ratio to the element-wise bound %.4f' % (W.case_id(c), route, ' swapped' if wg.swapped else '', rel, ratio))
    assert rel < 2e-4, rel
    assert ratio <= 1.0, ratio
    assert torch.equal(outs[0], outs[1])


def hold_bnbwd(ops, n, oh, ow, c, pad, relu, t, ref):
    from hnd_ghnd_object_detectors_amd import _lib
    L = _lib.load()
    walked, tiles_d, tiles_w = W.bnbwd_tiles(n, oh, ow, pad)
    tp_d, tp_w = int(L.hnd_wino2_tiles_pad(n, oh + 2 * pad - 1, ow + 2 * pad - 1, 6)), int(L.hnd_wino2_tiles_pad(n, oh, ow, 6))
    assert (tp_d, tp_w) == (U.round_up(tiles_d, 128), U.round_up(tiles_w, 128))
    g, x = [t[k].permute(0, 2, 3, 1).contiguous().to(DEV) for k in ('g', 'x')]
    sc, sh, k123 = t['scale'].to(DEV), t['shift'].to(DEV), t['k123'].to(DEV).contiguous()
    specs = [((49 * tp_d * c,), torch.float32), ((49 * tp_w * c,), torch.float32)]
    arena = G.Arena(DEV, G.arena_bytes(specs))
    v, z = arena.take('v', specs[0][0]), arena.take('z', specs[1][0])
    outs = []
    for _ in range(2):
        v.fill_(NAN)
        z.fill_(NAN)
        _lib.check(L.hnd_wino26_bnbwd_transforms(g.data_ptr(), x.data_ptr(), sc.data_ptr(), sh.data_ptr(), k123.data_ptr(),
                                                 int(relu), n, oh, ow, c, pad, v.data_ptr(), z.data_ptr(), ops.stream_ptr()),
                   'hnd_wino26_bnbwd_transforms')
        ops.sync_check()
        arena.check()
        # each output exists only inside its own grid: the rows beyond it keep their NaN
        assert bool(torch.isnan(v.view(49, tp_d, c)[:, tiles_d:]).all()) and bool(torch.isnan(z.view(49, tp_w, c)[:, tiles_w:]).all())
        outs.append((v.view(49, tp_d, c)[:, :tiles_d].clone(), z.view(49, tp_w, c)[:, :tiles_w].clone()))
    v64, vmag, z64, zmag = ref
    for name, got, r64, mag, k_t in (('V', outs[0][0], v64, vmag, W.t_v()), ('Z', outs[0][1], z64, zmag, W.t_z())):
        got = got.to(r64.device)
        assert got.shape == r64.shape and not bool(torch.isnan(got).any()), name
        ratio = float(((got.double() - r64).abs() / (k_t * W.U24 * mag + 1e-30)).max())
        note((2, 6, 'bnbwd ' + name), ratio, '%d-%d-%d-%d-%d-%d' % (n, oh, ow, c, pad, relu))
        print('%s: ratio to the element-wise bound %.4f' % (name, ratio))
        assert ratio <= 1.0, (name, ratio)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize('n,oh,ow,c,pad,relu', W.BNBWD_CASES)
def test_fused_bn_backward_transforms_hold_to_fp64(ops, n, oh, ow, c, pad, relu):
    """hnd_wino26_bnbwd_transforms: V and Z against the fp64 transforms of dy = k1 [scale x + shift > 0] g + k2 x + k3,
    element by element under T 2^-24 |B^T| |dy|_mag |B| (Z: |G'| |dy|_mag |G'|^T); with pad 0 the data gradient's grid is the
    smaller of the two"""
    t = W.bnbwd_inputs(n, oh, ow, c, pad, relu)
    hold_bnbwd(ops, n, oh, ow, c, pad, relu, t, W.bnbwd_reference(t, pad, relu))


def test_fused_bn_backward_transforms_walk_their_loop_a_second_time(ops):
    n, oh, ow, c, pad, relu = W.BNBWD_OVER
    gen = torch.Generator(device=DEV).manual_seed(62000)
    t = dict(g=torch.randn(n, oh, ow, c, generator=gen, device=DEV).permute(0, 3, 1, 2),
             x=torch.randn(n, oh, ow, c, generator=gen, device=DEV).permute(0, 3, 1, 2),
             scale=torch.rand(c, generator=gen, device=DEV) + 0.5, shift=torch.randn(c, generator=gen, device=DEV) * 0.5,
             k123=torch.randn(3, c, generator=gen, device=DEV) * 0.5)
    pre = t['x'].double() * t['scale'].double()[None, :, None, None] + t['shift'].double()[None, :, None, None]
    t['x'] = torch.where(pre.abs() < 1e-3, t['x'] + 0.5, t['x'])          # (|scale| >= 0.5: the moved elements are decided)
    hold_bnbwd(ops, n, oh, ow, c, pad, relu, t, W.bnbwd_reference(t, pad, relu))


# --------------------------------------------------------------------------------------------------------- transforms without a GEMM, alone

def alone(ops, name, launch, out_spec):
    """launch twice into a NaN-filled arena view -> the first result, after asking the second for the same bits"""
    arena = G.Arena(DEV, G.arena_bytes([out_spec]))
    out = arena.take('out', out_spec[0])
    got = []
    for _ in range(2):
        out.fill_(NAN)
        from hnd_ghnd_object_detectors_amd import _lib
        _lib.check(launch(out), name)
        ops.sync_check()
        arena.check()
        got.append(out.clone())
    assert torch.equal(got[0], got[1])
    return got[0]


def hold_alone(key, what, got, r64, mag, k_t):
    assert got.shape == r64.shape and not bool(torch.isnan(got).any())
    ratio = float(((got.double() - r64).abs() / (k_t * W.U24 * mag + 1e-30)).max())
    note(key, ratio, what)
    print('%s %s: ratio to the element-wise bound %.4f' % (key, what, ratio))
    assert ratio <= 1.0, (key, what, ratio)


@pytest.mark.parametrize('k,tile,dgrad', W.OVER_WEIGHTS)
def test_weight_transforms_walk_their_loop_a_second_time(ops, k, tile, dgrad):
    """hnd_wino_weights / hnd_wino2_weights alone on round_up(rows, 64) * depth > kMaxBlocks * 256 work items: U against
    the fp64 G g G^T of the channel each packed row holds, under (2 r(G) + 8) 2^-24 |G| |g| |G|^T"""
    from hnd_ghnd_object_detectors_amd import _lib
    L = _lib.load()
    rows, depth = W.OVER_ROWS, W.OVER_DEPTH
    gen = torch.Generator(device=DEV).manual_seed(63000 + 10 * k + tile)
    cout, cin = (depth, rows) if dgrad else (rows, depth)
    w = torch.randn(cout, cin, k, k, generator=gen, device=DEV)
    fn = L.hnd_wino_weights if k == 3 else L.hnd_wino2_weights
    ncomp = (tile + k - 1) ** 2
    u = alone(ops, 'weights', lambda out: fn(w.data_ptr(), out.data_ptr(), cout, cin, int(dgrad), tile, ops.stream_ptr()),
              ((ncomp, rows, depth), torch.float32))
    u64, mag = W.weights_reference(w, k, tile, dgrad)
    chan = torch.tensor([W.chan_of_row(r) for r in range(rows)], device=DEV)
    hold_alone((k, tile, 'over U'), 'dgrad' if dgrad else 'fwd', u, u64[:, chan], mag[:, chan], W.t_u(k, tile))


@pytest.mark.parametrize('tile,st', W.OVER_WGRAD_OUT)
def test_weight_gradient_output_transform_walks_its_loop_a_second_time(ops, tile, st):
    """hnd_wino2_wgrad_output_t alone on cout * cin > kMaxBlocks * 256, S as [comp][cout][cin] and transposed"""
    from hnd_ghnd_object_detectors_amd import _lib
    L = _lib.load()
    cout, cin, ncomp = W.OVER_ROWS, W.OVER_DEPTH, (tile + 1) ** 2
    gen = torch.Generator(device=DEV).manual_seed(64000 + tile + st)
    s = torch.randn(ncomp, cout, cin, generator=gen, device=DEV)
    stored = s.transpose(1, 2).contiguous() if st else s
    dw = alone(ops, 'wgrad_output', lambda out: L.hnd_wino2_wgrad_output_t(stored.data_ptr(), out.data_ptr(), cout, cin, tile, st,
                                                                          ops.stream_ptr()), ((cout, cin, 2, 2), torch.float32))
    dw64, mag = W.wgrad_out_reference(s, tile)
    hold_alone((2, tile, 'over dW'), 'transposed' if st else 'plain', dw, dw64, mag, W.t_dw(tile))


@pytest.mark.parametrize('n,oh,ow,cout,tile', W.OVER_DY)
def test_dy_transforms_walk_their_loop_a_second_time(ops, n, oh, ow, cout, tile):
    """hnd_wino2_dy alone on tiles * cout / 2 > kMaxBlocks * 256: Z against the fp64 G' dy G'^T; the rows of Z beyond the tiles
    keep their NaN"""
    from hnd_ghnd_object_detectors_amd import _lib
    L = _lib.load()
    gen = torch.Generator(device=DEV).manual_seed(65000 + tile)
    dy = torch.randn(n, oh, ow, cout, generator=gen, device=DEV)
    tiles = n * ((oh + tile - 1) // tile) * ((ow + tile - 1) // tile)
    tp, ncomp = U.round_up(tiles, 128), (tile + 1) ** 2
    assert tp == int(L.hnd_wino2_tiles_pad(n, oh, ow, tile))
    z = alone(ops, 'dy', lambda out: L.hnd_wino2_dy(dy.data_ptr(), out.data_ptr(), n, oh, ow, cout, cout, tile, ops.stream_ptr()),
              ((ncomp, tp, cout), torch.float32))
    assert bool(torch.isnan(z[:, tiles:]).all())
    z64, mag = W.dy_reference(dy.permute(0, 3, 1, 2), tile)
    hold_alone((2, tile, 'over Z'), 'dy', z[:, :tiles], z64, mag, W.t_z(tile))
