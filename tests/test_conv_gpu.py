"""GPU: every native forward / data-gradient kernel and build of hnd_conv2d_igemm against an fp64 reference, element by element.

The cases are the tables of tests/conv_util.py (tests/test_conv_cases_cpu.py holds their routing and coverage without a
GPU).  Every case: build the launch under its switches, ask refresh_variant() for the kernel, launch on a NaN-filled output,
compare with fp64 under BOTH bars of conv_util.bars -- relative to the largest element < 1e-4 (the project's bar for
fp32-MFMA convs) and, element by element, |got - y64| <= (K + 8) 2^-24 B64 + 1e-30, which holds for any summation order and
catches an error confined to small elements (a wrong tap at a border, a padded column leaking into a tail tile, a parity
class writing one row too many, a dropped shift on a small-shift channel) -- then launch again and ask for the same bits.
Where the header documents a second kernel as bit-identical (thin_n4, stem7_lds, the B-resident and B-streamed builds
against the tiled kernel) both run and their bits are compared.  The fp64 reference is computed on the CPU, or, for the
B-resident / relay rows whose CPU convolution takes over a second (conv_util.heavy: all 1x1), by torch in fp64 on the device."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_util as U

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
WORST = {k: [0.0, 0.0, 0] for k in U.KERNELS}       # kernel -> [relative to max, ratio to the element-wise bound, launches]
POINTERS = ('pro_scale', 'pro_shift', 'epi_scale', 'epi_shift', 'res1', 'res2', 'mask', 'stats', 'mask_bits', 'mask_out')


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
    for k in U.KERNELS:
        record_achieved(lambda k=k: '[conv forward / data gradient vs fp64, %-16s %3d launches] worst relative to max %.2e (held to '
                        '1e-4), worst |got - ref| / ((K + 8) 2^-24 B64) %.3f (held to 1)' % (k + ',', WORST[k][2], WORST[k][0], WORST[k][1]))
    yield


def switches(monkeypatch, env):
    for s in U.SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def hold(got, y64, b64, k, variant, what):
    """both bars, after the figures are on record"""
    rel, ratio = U.bars(got, y64, b64, k)
    w = WORST[U.kernel_of(variant)]
    w[0], w[1], w[2] = max(w[0], rel), max(w[1], ratio), w[2] + 1
    print('%s %s: relative to max %.3e, ratio to the element-wise bound %.4f' % (variant, what, rel, ratio))
    assert rel < 1e-4, (variant, what, rel)
    assert ratio <= 1.0, (variant, what, ratio)


def to_nhwc(t_nchw, lanes, value=0.0):
    """NHWC device tensor with `lanes` channel lanes (the padding lanes hold `value`)"""
    t = t_nchw.permute(0, 2, 3, 1)
    if t.shape[-1] != lanes:
        t = F.pad(t, (0, lanes - t.shape[-1]), value=value)
    return t.contiguous().to(DEV)


def vec(v, lanes):
    return F.pad(v, (0, lanes - v.numel())).to(DEV)


def check_desc(l, fields):
    got = {n: getattr(l.desc, n) for n in fields if n != 'ptrs'}
    assert got == {n: v for n, v in fields.items() if n != 'ptrs'}, got
    assert {n for n in POINTERS if getattr(l.desc, n) is not None} == set(fields['ptrs']), fields['ptrs']


class Forward(object):
    """one forward case built as a launch: the operands on the device, NaN-filled outputs"""

    def __init__(self, ops, c, t, lane_value=0.0):
        f, e = U.fwd_fields(c), U.epi_of(c.epi)
        self.case, self.fields, self.width = c, f, c.cout if c.ldc else f['ldc']
        x = to_nhwc(t['x'], f['cin'], lane_value)
        pw = ops.pack_weights(t['w'].to(DEV).contiguous(), chan_pad=f['cin'])
        self.y = torch.empty(c.n, f['oh'], f['ow'], f['ldc'], device=DEV)
        kw = dict(pro_relu=bool(f['pro_relu']), relu=bool(f['relu']))
        if 'ps' in t:
            kw['pro_scale'] = vec(t['ps'], f['cin'])
        if 'pb' in t:
            kw['pro_shift'] = vec(t['pb'], f['cin'])
        if 'es' in e:
            kw['epi_scale'] = vec(t['es'], f['cout'])
        if 'eb' in e:
            kw['epi_shift'] = vec(t['eb'], f['cout'])
        for name, key in (('r1', 'res1'), ('r2', 'res2'), ('mask', 'mask')):
            if name in e:
                kw[key] = to_nhwc(t[name], f['ldc'])
        kw['res1_up'] = 'up' in e
        self.stats = self.mask_out = None
        if 'stats' in e:
            self.stats = kw['stats'] = torch.empty(ops.stats_tiles(U.rows_of(c)), 2, f['cout'], device=DEV)
        if 'mout' in e:
            self.mask_out = kw['mask_out'] = torch.empty(c.n, f['oh'], f['ow'], f['ldc'] // 4, dtype=torch.uint8, device=DEV)
        if c.ldc:
            kw['cout'] = c.cout
        self.launch = ops.conv_forward(x, pw, self.y, (c.kh, c.kw), c.stride, c.pad, **kw)

    def run(self, ops):
        """NaN into everything the launch writes, launch, wait -> (y, stats, mask_out) copies"""
        self.y.fill_(NAN)
        if self.stats is not None:
            self.stats.fill_(NAN)
        if self.mask_out is not None:
            self.mask_out.fill_(0xAA)
        self.launch.run()
        ops.sync_check()
        return (self.y.clone(), None if self.stats is None else self.stats.clone(),
                None if self.mask_out is None else self.mask_out.clone())


def reference_of(c):
    """(y64, B64, K, M): on the CPU (shared with the CPU file), or in fp64 on the device for the heavy rows"""
    if not U.heavy(c):
        return U.fwd_case(c)[1:]
    t = {k: v.to(DEV) for k, v in U.fwd_inputs(c).items()}
    return U.fwd_reference(c, t) + (c.kh * c.kw * c.cin, U.rows_of(c))


def run_forward(ops, monkeypatch, env, c, variant, ref=None, lane_value=0.0, what=''):
    """the whole procedure for one forward case on one kernel -> (first y, the Forward)"""
    switches(monkeypatch, env)
    y64, b64, k, m = ref if ref is not None else reference_of(c)
    fw = Forward(ops, c, U.fwd_inputs(c), lane_value)
    l = fw.launch
    l.refresh_variant()
    if variant is None:                                 # whichever block tile the cost model picks
        assert l.variant in U.TILE_NAMES, l.variant
    else:
        assert l.variant == variant, (l.variant, variant)
    variant = l.variant
    check_desc(l, fw.fields)
    y, stats, mask_out = fw.run(ops)
    written = y[..., :c.cout]
    assert not bool(torch.isnan(written).any()), (variant, c, what)
    if c.ldc:                                           # lanes beyond an explicit cout are not the launch's: they keep their NaN
        assert bool(torch.isnan(y[..., c.cout:]).all()), (variant, c)
    else:                                               # zero weight rows: exact zeros
        assert not bool((y[..., c.cout:] != 0).any()), (variant, c)
    got = written.permute(0, 3, 1, 2)
    hold(got if y64.is_cuda else got.cpu(), y64, b64, k, variant, '%s %s' % (U.case_id(c), what))
    if stats is not None:
        assert bool(torch.isfinite(stats).all())
        r1, r2 = U.stats_bars(stats.double().sum(0)[:, :c.cout].cpu(), y64, b64, k, m)
        print('%s %s: statistics sum %.4f, sum of squares %.4f of their bounds' % (variant, U.case_id(c), r1, r2))
        assert r1 <= 1.0 and r2 <= 1.0, (variant, c, r1, r2)
    if mask_out is not None:
        assert torch.equal(mask_out, U.nibbles(y)), (variant, c)
    again = fw.run(ops)
    assert torch.equal(y[..., :fw.width], again[0][..., :fw.width]), (variant, c, what)
    assert stats is None or torch.equal(stats, again[1])
    assert mask_out is None or torch.equal(mask_out, again[2])
    return y[..., :fw.width], fw


# --------------------------------------------------------------------------------------------------------- A .. C

@pytest.mark.parametrize('case', U.TILED_CASES, ids=U.case_id)
def test_tiled_kernel_on_every_block_tile(ops, case, monkeypatch):
    """csrc/conv_igemm.hip igemm_kernel<128x128 | 128x64 | 64x128 | 64x64>, with and without the prologue: a single output
    pixel, maps smaller than the kernel, pad = k - 1, rows around the 64- and 128-row tiles, channel tails, k = 1 .. 7 at
    both strides, rectangular kernels, every fused form, statistics of a nearly empty tile, mask nibbles"""
    seen = {}
    for tile in range(4):
        variant = U.tiled_variant(case, tile)
        if variant not in seen:
            seen[variant] = run_forward(ops, monkeypatch, U.tiled_env(tile), case, variant, what='tile %d' % tile)[1]
        else:                                           # a fall-back of the override names a build that already ran: ask the
            switches(monkeypatch, U.tiled_env(tile))    # library, on the device, that this tile code does fall back to it
            seen[variant].launch.refresh_variant()
            assert seen[variant].launch.variant == variant, (case, tile, seen[variant].launch.variant, variant)


@pytest.mark.parametrize('row', U.C4_CASES, ids=lambda r: U.case_id(r[0]) if isinstance(r, tuple) else None)
def test_four_lane_tile(ops, row, monkeypatch):
    """igemm_kernel<128, 64, 32, CIN4>: cin 3 and a genuine cin 4 at k = 2 and, kept off the stem kernel, k = 7"""
    case, env, variant = row
    run_forward(ops, monkeypatch, env, case, variant)


@pytest.mark.parametrize('row', U.STEM_CASES, ids=lambda r: '-'.join(str(v) for v in r if v != ''))
def test_stem_kernel_below_and_across_one_tile(ops, row, monkeypatch):
    """csrc/conv_stem.hip stem7_kernel: maps below its 8 x 32 output tile, one row / one column beyond it, odd and even
    extents; with HND_STEM7=0 the 4-lane tile gives the same bits"""
    case = U.stem_case(row)
    stem, _ = run_forward(ops, monkeypatch, {}, case, 'stem7_lds')
    generic, _ = run_forward(ops, monkeypatch, {'HND_STEM7': '0'}, case, 'igemm_c4_128x64', what='stem off')
    assert torch.equal(stem, generic), case


@pytest.mark.parametrize('row', U.THIN_CASES, ids=lambda r: U.case_id(r[0]) if isinstance(r, tuple) else None)
def test_thin_kernel_and_the_tiled_kernel_on_the_same_descriptor(ops, row, monkeypatch):
    """csrc/conv_igemm.hip thin_n_kernel: 1 .. 4 output channels, k = 1 / 2, both strides and pads, 1 / 127 / 128 / 129
    pixels around its block, every prologue form, statistics, residuals, the kdim = 4096 limit taken and 4352 refused;
    HND_THIN_N=0 gives the same bits on the MFMA tiles"""
    case, taken = row
    thin, _ = run_forward(ops, monkeypatch, {}, case, 'thin_n4' if taken else None)
    tiled, _ = run_forward(ops, monkeypatch, {'HND_THIN_N': '0'}, case, None, what='thin off')
    assert torch.equal(thin, tiled), case


# --------------------------------------------------------------------------------------------------------- D, E

@pytest.mark.parametrize('row', U.BRES_CASES, ids=lambda r: U.case_id(r[0]) + '-%d-wave' % r[3][0] if isinstance(r, tuple) else None)
def test_b_resident_builds_at_their_smallest_size(ops, row, monkeypatch):
    """csrc/conv_bres.hip: one case per instantiated build of the 8-wave and the one-wave kernel, each at the fewest rows
    bres_variant accepts with a ragged last chunk; the tiled kernel gives the same bits"""
    case, env, variant, build = row
    ref = reference_of(case)
    bres, _ = run_forward(ops, monkeypatch, env, case, variant, ref=ref, what='build %r' % (build,))
    tiled, _ = run_forward(ops, monkeypatch, U.BRES_OFF_ENV, case, None, ref=ref, what='bres off')
    assert torch.equal(bres, tiled), case


@pytest.mark.parametrize('row', U.BSTREAM_CASES, ids=lambda r: U.case_id(r[0]) if isinstance(r, tuple) else None)
def test_b_streamed_builds_with_and_without_the_relay(ops, row, monkeypatch):
    """csrc/conv_bstream.hip: both wave-column builds with and without taps and prologue at K = 256 / 384 / 1152; the relay
    rows run twice on one workspace and once without any; the tiled kernel gives the same bits"""
    case, variant, relay = row
    ref = reference_of(case)
    first, fw = run_forward(ops, monkeypatch, U.BSTREAM_ENV, case, variant, ref=ref)
    assert (fw.launch.relay is not None) == relay and (fw.launch.desc.relay_ws is not None) == relay
    if relay:                                           # (run_forward launched twice on fw.launch.relay)
        fw.launch.desc.relay_ws = None
        assert torch.equal(first, fw.run(ops)[0][..., :fw.width]), (case, 'without a workspace')
        assert ops._L.hnd_relay_timeouts(0) == 0
    tiled, _ = run_forward(ops, monkeypatch, U.BSTREAM_OFF_ENV, case, None, ref=ref, what='bstream off')
    assert torch.equal(first, tiled), case


# --------------------------------------------------------------------------------------------------------- F

def run_dgrad(ops, monkeypatch, c, index, lane_value=0.0):
    """the whole procedure for one data-gradient case -> dx (host, NCHW over the real channels)"""
    t, dx64, b64, kmap = U.dgrad_case(c)
    o, ldy, ldc = U.opts_of(c.opts), U.lanes(c.cout), U.lanes(c.cin)
    dy = to_nhwc(t['dy'], ldy, lane_value)
    start = to_nhwc(t['base'], ldc) if 'acc' in o else torch.full((c.n, c.h, c.w, ldc), NAN, device=DEV)
    dx = start.clone()
    kw = {}
    if 'pro' in o:
        kw['pro_scale'] = vec(t['s'], ldy)
    if 'fold' in o:
        kw['fold_scale'] = t['s'].to(DEV)
    if 'mask' in o:
        kw['mask'] = to_nhwc(t['mask'], ldc)
    if 'bits' in o:
        kw['mask_bits'] = U.nibbles(to_nhwc(t['mask'], ldc))
    plan = U.dgrad_plan(c, index)
    switches(monkeypatch, U.DGRAD_ENV)
    launches, _ = ops.conv_dgrad(dy, t['w'].to(DEV).contiguous(), dx, c.k, c.stride, c.pad, accumulate='acc' in o, **kw)
    assert len(launches) == len(plan)
    outs = []
    for _ in range(2):
        dx.copy_(start)
        for l, (ph, pw, fields, env, variant) in zip(launches, plan):
            switches(monkeypatch, env)
            l.refresh_variant()
            assert l.variant == variant, (c, ph, pw, l.variant, variant)
            check_desc(l, fields)
            l.run()
        ops.sync_check()
        outs.append(dx.cpu())
    got = outs[0][..., :c.cin].permute(0, 3, 1, 2)
    assert not bool(torch.isnan(got).any()), c
    assert not bool((outs[0][..., c.cin:] != 0).any()), c
    for variant in dict.fromkeys(p[4] for p in plan):
        rows = [p for p in plan if p[4] == variant]
        sel = torch.zeros(c.h, c.w, dtype=torch.bool)
        for ph, pw, _, _, _ in rows:
            sel[ph::c.stride, pw::c.stride] = True
        hold(got[:, :, sel], dx64[:, :, sel], b64[:, :, sel], kmap.expand_as(dx64)[:, :, sel], variant, '%s data gradient' % U.case_id(c))
    idle = U.untouched(c)
    if 'acc' in o:
        # pixels of tap-less parities are not written at all and keep the base's bits; pixels no output pixel reads inside
        # a written parity are base + 0 (the base's value; -0.0 may come back as +0.0), or 0 where the mask is off
        keep, expect = ~U.written_map(c), t['base']
        assert torch.equal(got[:, :, keep].view(torch.int32), expect[:, :, keep].view(torch.int32)), c
        if 'mask' in t:
            expect = torch.where((t['mask'] > 0) | keep, expect, torch.zeros_like(expect))
        assert torch.equal(got[:, :, idle & ~keep], expect[:, :, idle & ~keep]), c
    elif bool(idle.any()):                              # input rows / columns no output pixel reads: exact zeros
        assert not bool((got[:, :, idle] != 0).any()), c
    assert torch.equal(outs[0], outs[1]), c
    return outs[0]


@pytest.mark.parametrize('index', range(len(U.DGRAD_CASES)), ids=lambda i: U.case_id(U.DGRAD_CASES[i]))
def test_data_gradient_through_conv_dgrad(ops, index, monkeypatch):
    """ops.conv_dgrad: every k / stride / pad of the strided forward rows on odd and even maps, leftover rows and columns
    written as exact zeros over NaN, tap-less parities left to the base, an empty parity class, dx in 4 lanes on thin_n4 /
    the tiled kernel / the 4-lane tile, the folded scale and the prologue form, mask floats and nibbles"""
    run_dgrad(ops, monkeypatch, U.DGRAD_CASES[index], index)


# --------------------------------------------------------------------------------------------------------- G

@pytest.mark.parametrize('row', U.PAD_LANE_FWD, ids=lambda r: U.case_id(r[0]) if isinstance(r, tuple) else None)
def test_padding_lanes_of_x_never_reach_y(ops, row, monkeypatch):
    """include/hnd_hip.h stores cin_real channels in 4 or a multiple of 32 lanes and asks no caller to zero the rest: the packed
    operand has zero columns there, so y is the same bit for bit when those lanes hold 3e4"""
    case, env, variant = row
    assert U.lanes(case.cin) > case.cin
    clean, _ = run_forward(ops, monkeypatch, env, case, variant, what='zero padding lanes')
    dirty, _ = run_forward(ops, monkeypatch, env, case, variant, lane_value=U.PAD_LANE_VALUE, what='padding lanes 3e4')
    assert torch.equal(clean, dirty), case


@pytest.mark.parametrize('index', range(len(U.PAD_LANE_DGRAD)), ids=lambda i: U.case_id(U.PAD_LANE_DGRAD[i]))
def test_padding_lanes_of_dy_never_reach_dx(ops, index, monkeypatch):
    """... and the data gradient's input: dy lanes beyond cout (3 in 4, 12 in 32, 100 in 128)"""
    case, at = U.PAD_LANE_DGRAD[index], len(U.DGRAD_CASES) + index
    assert U.lanes(case.cout) > case.cout
    assert torch.equal(run_dgrad(ops, monkeypatch, case, at), run_dgrad(ops, monkeypatch, case, at, U.PAD_LANE_VALUE)), case
