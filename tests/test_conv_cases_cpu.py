"""CPU: the forward / data-gradient case tables of tests/conv_util.py, held before anyone has a GPU.

* every row reaches the kernel its table names under its switches: hnd_conv2d_igemm_tile / _build / _workspace read pointer
  VALUES only and answer without a device (256 compute units assumed), as in tests/test_conv_picker_cpu.py;
* coverage conditions keep the tables from quietly shrinking or growing: every tile code but the unused 10 and the emulated
  13 - 15, every instantiated B-resident and B-streamed build, every prologue form and epilogue operand on two kernels,
  tables D and E at the smallest size their kernels accept;
* the fp64 reference equals torch's fp64 conv2d / autograd, and a result with one border tap or one small epi_shift dropped
  fails the element-wise bar while passing the relative-to-max one;
* torch's own fp32 CPU convolution of every case stays under both bars: the bound is derived, and this is the room it
  leaves a correct fp32 result.  Left out here (their CPU convolution takes about a second or more; conv_util.heavy: above
  1.2e9 multiply-adds): the B-resident rows of K >= 256 and those of 16330 rows at K = 128, and the 257-tile relay row of the
  B-streamed table.  The K = 64 and the one-wave K = 128 B-resident rows and the 256-tile relay row are held here."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_util as U


@pytest.fixture(scope='module')
def ask():
    """ask(switches, fields) -> (tile code, build, workspace bytes), with the switches set for that call only"""
    import __graft_entry__ as g
    g.build()
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    names = [n for n, _ in _lib.ConvDesc._fields_]
    ptr = dict((n, 0x100000 * (i + 1)) for i, n in enumerate(names))          # distinct 16-byte aligned pointer values
    saved = {s: os.environ.get(s) for s in U.SWITCHES}

    def query(env, fields):
        d = _lib.ConvDesc()
        for n, v in fields.items():
            if n != 'ptrs':
                setattr(d, n, int(v))
        for n in ('x', 'w', 'y') + tuple(fields['ptrs']):
            setattr(d, n, ptr[n])
        for s in U.SWITCHES:
            os.environ.pop(s, None)
        os.environ.update(env)
        ref = ctypes.byref(d)
        return int(lib.hnd_conv2d_igemm_tile(ref)), int(lib.hnd_conv2d_igemm_build(ref)), int(lib.hnd_conv2d_igemm_workspace(ref))

    try:
        yield query
    finally:
        for s in U.SWITCHES:
            os.environ.pop(s, None)
        os.environ.update({s: v for s, v in saved.items() if v is not None})


# --------------------------------------------------------------------------------------------------------- routing

def test_every_row_reaches_the_kernel_its_table_names(ask):
    routes = U.routing()
    assert len(routes) > 400
    wrong, reached = [], set()
    for label, env, fields, variant, relay in routes:
        tile, build, ws = ask(env, fields)
        reached.add(tile)
        ok = tile == U.TILE_CODE[variant] if variant else 0 <= tile <= 3          # None: whichever block tile the model picks
        if fields['cin'] == 4:
            ok = ok and (tile == 9) == (variant == 'stem7_lds')
        if not ok or build != 0 or (ws > 0) != relay:
            wrong.append((label, env, variant, tile, build, ws))
    assert not wrong, wrong
    assert reached == set(range(10)) | {11, 12}               # every code but the unused 10 and the emulated 13 .. 15


def test_the_b_resident_table_holds_every_build_at_its_smallest_size(ask):
    seen = set()
    for c, env, variant, build in U.BRES_CASES:
        f = U.fwd_fields(c)
        waves, wn, kq = build
        assert variant == ('bres_' if waves == 8 else 'bres2_') + str(64 * wn) and f['kdim'] == 64 * kq == f['cin'], (c, build)
        assert (env.get('HND_BRES2') == '0') == (waves == 8) and env['HND_DEBUG_PICKER'] == 'bres_all' and env['HND_BSTREAM'] == '0'
        low = U.bres_min_rows(f['cout'], wn, waves)
        assert low <= U.rows_of(c) < low + 64 and U.rows_of(c) % 64 != 0, (c, low)          # the last chunk is ragged
        fewer = dict(f, n=1, h=1, w_=U.rows_of(c) - 64, oh=1, ow=U.rows_of(c) - 64, yh=1, yw=U.rows_of(c) - 64, sh=1, sw=1,
                     res1_mode=0, res1_h=0, res1_w=0)
        assert ask(env, dict(f, n=1, h=1, w_=U.rows_of(c), oh=1, ow=U.rows_of(c), yh=1, yw=U.rows_of(c), sh=1, sw=1,
                             res1_mode=0, res1_h=0, res1_w=0))[0] == U.TILE_CODE[variant]
        assert 0 <= ask(env, fewer)[0] <= 3, (c, 'takes 64 rows fewer: not the smallest size')
        seen.add(build)
    assert seen == U.BRES_BUILDS, seen ^ U.BRES_BUILDS
    eight = [c for c, _, _, b in U.BRES_CASES if b[0] == 8]
    assert [c for c in eight if c.stride == 2 and c.h % 2 == 1]
    assert [c for c in eight if U.epi_of(c.epi) >= {'r1'} and 'up' not in c.epi] and [c for c in eight if 'up' in c.epi]
    assert [c for c in eight if 'mask' in c.epi and c.pro != 'none']
    one = [c for c, _, _, b in U.BRES_CASES if b[0] == 1]
    assert [c for c in one if 'r1' in c.epi] and [c for c in one if c.pro != 'none']


def test_the_b_streamed_table_holds_both_builds_in_their_four_forms_and_the_relay(ask):
    forms = set()
    for c, variant, relay in U.BSTREAM_CASES:
        f = U.fwd_fields(c)
        taps = c.kh * c.kw > 1 or c.pad != 0
        forms.add((variant, taps, c.pro != 'none'))
        assert f['kdim'] in (256, 384, 1152) and (U.bstream_tiles(c) >= U.COMPUTE_UNITS) == relay
        assert relay or U.rows_of(c) <= 2 * 8 * 9
        if taps:
            assert c.cin == 128 and (c.kh, c.kw, c.pad) == (3, 3, 1) and (c.h, c.w) in ((5, 7), (8, 9))
    assert forms == {(v, t, p) for v in ('bstream_64', 'bstream_128') for t in (False, True) for p in (False, True)}
    assert {c.stride for c, _, _ in U.BSTREAM_CASES if c.kh == 3} == {1, 2}
    assert {U.fwd_fields(c)['kdim'] for c, _, _ in U.BSTREAM_CASES} == {256, 384, 1152}
    # K = 256 is the kernel's minimum: the same launch at K = 128 is not taken
    c = U.BSTREAM_CASES[1][0]
    assert ask(U.BSTREAM_ENV, U.fwd_fields(c))[0] == 11 and ask(U.BSTREAM_ENV, U.fwd_fields(c._replace(cin=128)))[0] <= 3
    # the first relay row is the smallest launch with a workspace; the second splits tiles between workgroups
    small, split = [c for c, _, relay in U.BSTREAM_CASES if relay]
    f = U.fwd_fields(small)
    flat = dict(f, n=1, h=1, w_=U.rows_of(small), oh=1, ow=U.rows_of(small), yh=1, yw=U.rows_of(small))
    assert U.bstream_tiles(small) == U.COMPUTE_UNITS and ask(U.BSTREAM_ENV, flat)[2] > 0
    fewer = dict(flat, w_=flat['w_'] - 64, ow=flat['ow'] - 64, yw=flat['yw'] - 64)
    assert ask(U.BSTREAM_ENV, fewer)[::2] == (11, 0)
    assert (U.bstream_tiles(split) * (U.fwd_fields(split)['kdim'] // 128)) % U.COMPUTE_UNITS != 0


def forward_rows():
    """(kernel, case) of every forward launch of tables A .. E"""
    out = [(U.kernel_of(U.tiled_variant(c, t)), c) for c in U.TILED_CASES for t in range(4)]
    out += [(v, c) for c, _, v in U.C4_CASES] + [('stem7_lds', U.stem_case(r)) for r in U.STEM_CASES]
    out += [('thin_n4', c) for c, taken in U.THIN_CASES if taken]
    out += [(U.kernel_of(v), c) for c, _, v, _ in U.BRES_CASES] + [(U.kernel_of(v), c) for c, v, _ in U.BSTREAM_CASES]
    return out


def test_every_prologue_form_and_epilogue_operand_runs_on_two_kernels():
    rows = forward_rows()
    assert {k for k, _ in rows} == set(U.KERNELS)
    for form in U.ALL_FORMS:
        assert len({k for k, c in rows if c.pro == form}) >= 2, form
    for operand in U.EPI_OPERANDS:
        on = {k for k, c in rows if operand in U.epi_of(c.epi)}
        assert len(on) >= 2, (operand, on)


def test_the_tiled_table_keeps_the_geometries_nobody_ran():
    cases = U.TILED_CASES
    assert len(set(cases)) == len(cases) and len(cases) >= 60
    m = [U.rows_of(c) for c in cases]
    assert {1, 63, 64, 65, 127, 128, 129} <= set(m)
    assert {c.kh for c in cases if m[cases.index(c)] == 1} >= {1, 3, 7}                     # a single output pixel
    assert [c for c in cases if c.h < c.kh and c.w < c.kw] and [c for c in cases if (c.h, c.w, c.kh, c.pad) == (2, 1, 5, 2)]
    assert {c.kh for c in cases if c.pad == c.kh - 1 and c.kh == c.kw and c.kh > 1} >= {2, 3}
    assert {c.cout for c in cases if c.ldc is None} >= set(U.COUTS) and [c for c in cases if c.ldc and c.cout < c.ldc]
    assert {c.cin for c in cases} >= {32, 96, 160}
    assert {(c.kh, c.stride) for c in cases if c.kh == c.kw} >= {(k, s) for k in (1, 2, 3, 4, 5, 7) for s in (1, 2)}
    assert [c for c in cases if c.stride == 2 and c.pad == 0 and (c.h - c.kh) % 2 == 1]    # rows no output pixel touches
    assert [c for c in cases if c.stride == 2 and c.pad == 0 and (c.w - c.kw) % 2 == 1]
    assert {(c.kh, c.kw) for c in cases} >= {(1, 3), (3, 1)}
    assert {c.pro for c in cases} == set(U.ALL_FORMS)
    epis = {c.epi for c in cases}
    assert {'es', 'eb', 'r1', 'r1+r2', 'r1+up', 'mask', 'mask+relu', 'stats'} <= epis and [e for e in epis if 'mout' in e]
    up = [c for c in cases if 'up' in c.epi][0]
    assert U.fwd_fields(up)['oh'] % 2 == 1 and U.fwd_fields(up)['ow'] % 2 == 1 and (U.fwd_fields(up)['res1_h'], U.fwd_fields(up)['res1_w']) == (5, 7)
    assert [c for c in cases if 'stats' in c.epi and U.rows_of(c) == 129 and c.cout % 128 == 0]
    # the override's fall-backs: all four tiles where nothing forbids them, and each fall-back taken somewhere
    assert {U.tiled_variant(c, t) for c in cases for t in range(4)} == set(U.TILE_NAMES)
    assert U.tiled_name(0, 64) == 'igemm_128x64' and U.tiled_name(2, 100) == 'igemm_64x64' and U.tiled_name(3, 128, stats=True) == 'igemm_128x64'
    assert U.tiled_name(1, 128, mask_out=True) == 'igemm_128x128' and U.tiled_name(3, 128, mask_out=True) == 'igemm_64x128'


def test_the_small_kernel_tables_keep_their_edges():
    th, tw = U.STEM_TILE
    ext = [(U.fwd_fields(U.stem_case(r))['oh'], U.fwd_fields(U.stem_case(r))['ow'], r) for r in U.STEM_CASES]
    assert [1 for oh, ow, r in ext if oh < th and ow < tw] and [1 for oh, ow, r in ext if oh == 1]
    assert [1 for oh, ow, r in ext if ow == tw + 1] and [1 for oh, ow, r in ext if oh == th + 1]
    assert {r[1] for _, _, r in ext} == {3, 4} and {r[2] % 2 for _, _, r in ext} == {0, 1} == {r[3] % 2 for _, _, r in ext}
    c4 = [c for c, _, _ in U.C4_CASES]
    assert {(c.cin, c.kh) for c in c4} >= {(3, 2), (4, 2), (3, 7), (4, 7)}
    assert all(U.fwd_fields(c)['kdim'] > c.kh * c.kw * 4 for c in c4)
    thin = [c for c, taken in U.THIN_CASES if taken]
    assert {c.cout for c in thin} == {1, 2, 3, 4} and {c.cin for c in thin} >= {64, 128}
    assert {(c.kh, c.stride, c.pad) for c in thin} >= {(1, 1, 0), (1, 1, 1), (1, 2, 0), (1, 2, 1), (2, 1, 0), (2, 1, 1), (2, 2, 0), (2, 2, 1)}
    assert {U.rows_of(c) for c in thin} >= {1, 127, 128, 129}
    assert {c.pro for c in thin} == set(U.ALL_FORMS) and [c for c in thin if 'stats' in c.epi] and [c for c in thin if 'r1' in c.epi]
    kd = {U.fwd_fields(c)['kdim']: taken for c, taken in U.THIN_CASES if c.cin > 1000}
    assert kd == {4096: True, 4352: False}


def test_the_data_gradient_table_keeps_its_edges():
    cases = U.DGRAD_CASES
    assert len(set(cases)) == len(cases)
    for k, s, p in {(c.kh, c.stride, c.pad) for c in U.TILED_CASES if c.stride == 2 and c.kh == c.kw}:
        ext = {(c.h % 2, c.w % 2) for c in cases if (c.k, c.stride, c.pad) == (k, s, p)}
        assert {e[0] for e in ext} == {0, 1} == {e[1] for e in ext}, (k, s, p)
    assert [c for c in cases if (c.h, c.k, c.stride, c.pad) == (8, 3, 2, 0)] and [c for c in cases if (c.h, c.k, c.stride, c.pad) == (9, 4, 2, 0)]
    assert all(bool(U.untouched(c).any()) for c in cases if c.stride == 2 and c.pad == 0 and (c.h - c.k) % 2 == 1)
    assert [c for c in cases if c.k == 1 and c.stride == 2 and 'acc' in c.opts]
    assert [c for c in cases if c.h == 1 and c.stride == 2] and [c for c in cases if c.w == 1 and c.stride == 2]
    assert all(len(U.dgrad_launches(c)) == 2 for c in cases if 1 in (c.h, c.w) and c.stride == 2)
    assert [c for c in cases if (c.k, c.stride, c.pad, c.cin) == (7, 2, 3, 32)]
    kernels = {v for i, c in enumerate(cases) if c.cin <= 4 for _, _, _, _, v in U.dgrad_plan(c, i)}
    assert kernels >= {'thin_n4', 'igemm_c4_128x64'} and kernels & set(U.TILE_NAMES)
    opts = {c.opts for c in cases}
    assert {'fold', 'pro', 'mask', 'bits'} <= opts
    fold, pro = [c for c in cases if c.opts == 'fold'][0], [c for c in cases if c.opts == 'pro' and c.cin == 32][0]
    assert fold[:8] == pro[:8]
    assert {v for i, c in enumerate(cases) for _, _, _, _, v in U.dgrad_plan(c, i)} >= {'igemm_128x64', 'igemm_64x64'}
    # the strided-output epilogue (y_sh = 2, one launch per parity) on all four block tiles
    assert {v for i, c in enumerate(cases) for _, _, f, _, v in U.dgrad_plan(c, i) if f['y_sh'] == 2} >= set(U.TILE_NAMES)
    # with 'acc', pixels no output pixel reads inside a parity class that IS written: base + 0
    assert [c for c in cases if 'acc' in c.opts and bool((U.untouched(c) & U.written_map(c)).any())]
    assert [c for c in cases if 'acc' in c.opts and 'mask' in c.opts and bool((U.untouched(c) & U.written_map(c)).any())]


# --------------------------------------------------------------------------------------------------------- the reference

@pytest.mark.parametrize('case', [U.fwd(2, 32, 7, 9, 5, 3, 2, 1, pro='relu', epi='es+eb+r1+r2+mask+relu'),
                                  U.fwd(1, 64, 6, 5, 8, 1, 2, 0, pro=U.SCALE_RELU, epi='eb'),
                                  U.fwd(2, 3, 9, 13, 6, (3, 1), 1, 1, pro='shift', epi='r1+up')], ids=U.case_id)
def test_the_forward_reference_is_torch_fp64_of_the_same_expression(case):
    t, y64, b64, k, m = U.fwd_case(case)
    f = U.fwd_fields(case)
    assert y64.dtype == b64.dtype == torch.float64 and tuple(y64.shape) == tuple(b64.shape) == (case.n, case.cout, f['oh'], f['ow'])
    assert k == case.kh * case.kw * case.cin and m == case.n * f['oh'] * f['ow']
    a = t['x'].double()
    a = a * t['ps'].double()[None, :, None, None] + (t['pb'].double()[None, :, None, None] if 'pb' in t else 0.0)
    want = F.conv2d(F.relu(a) if f['pro_relu'] else a, t['w'].double(), None, case.stride, case.pad)
    want = want * (t['es'].double()[None, :, None, None] if 'es' in t else 1.0) + (t['eb'].double()[None, :, None, None] if 'eb' in t else 0.0)
    if 'r1' in t:
        r1 = t['r1'].double()
        want = want + (r1 if r1.shape == want.shape else r1[:, :, (torch.arange(f['oh']) * r1.shape[2]) // f['oh']][..., (torch.arange(f['ow']) * r1.shape[3]) // f['ow']])
    if 'r2' in t:
        want = want + t['r2'].double()
    if 'mask' in t:
        want = want * (t['mask'] > 0)
    if f['relu']:
        want = F.relu(want)
    assert float((y64 - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((b64 >= y64.abs() * (1 - 1e-12)).all())                  # every term by absolute value: it bounds |y|


@pytest.mark.parametrize('case', [U.dg(2, 32, 9, 10, 5, 3, 2, 1, 'fold'), U.dg(1, 3, 8, 8, 6, 3, 2, 0, 'acc+pro+mask'),
                                  U.dg(2, 32, 6, 7, 8, 2, 1, 1)], ids=U.case_id)
def test_the_data_gradient_reference_is_torch_fp64_autograd(case):
    t, dx64, b64, kmap = U.dgrad_case(case)
    x = torch.zeros(case.n, case.cin, case.h, case.w, dtype=torch.float64, requires_grad=True)
    s = t['s'].double()[None, :, None, None] if 's' in t else 1.0
    F.conv2d(x, t['w'].double(), None, case.stride, case.pad).backward(t['dy'].double() * s)
    want = x.grad + (t['base'].double() if 'base' in t else 0.0)
    if 'mask' in t:
        want = want * ((t['mask'] > 0) | ~U.written_map(case))
    assert float((dx64 - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((b64 >= dx64.abs() * (1 - 1e-12)).all())
    taps = {(ph, pw): f['kh'] * f['kw'] for ph, pw, f in U.dgrad_launches(case)}
    for (ph, pw), n_taps in taps.items():
        assert bool((kmap[0, 0, ph::case.stride, pw::case.stride] == n_taps * case.cout).all())
    if 'acc' not in case.opts:
        assert bool((dx64[:, :, U.untouched(case)] == 0).all()) and bool((b64[:, :, U.untouched(case)] == 0).all())


def test_a_dropped_border_tap_and_a_dropped_small_shift_fail_the_second_bar_only():
    """what the relative-to-max bar cannot see: one channel of the epilogue scale is 1e4 times the others (a BatchNorm weight
    does that), so the largest element is far above everything a fault in another channel can move"""
    case = U.fwd(2, 32, 5, 7, 64, 3, 1, 1, epi='es+eb')
    t = dict(U.fwd_inputs(case))
    t['es'] = t['es'].clone()
    t['es'][0] *= 1e4
    y64, b64 = U.fwd_reference(case, t)
    k, good = case.kh * case.kw * case.cin, U.fwd_fp32(case, t)
    rel, ratio = U.bars(good, y64, b64, k)
    assert rel < 1e-4 and ratio <= 1.0, (rel, ratio)
    # tap (0, 0) of the last output pixel of image 0 (it reads the in-bounds input pixel (h - 2, w - 2)) is dropped
    tap = torch.einsum('c,oc->o', t['x'][0, :, case.h - 2, case.w - 2], t['w'][:, :, 0, 0]) * t['es']
    bad = good.clone()
    bad[0, 1:, -1, -1] -= tap[1:]
    rel, ratio = U.bars(bad, y64, b64, k)
    assert rel < 1e-4 and ratio > 1.0, (rel, ratio)
    # epi_shift of channel 1 (1e-3, conv_util.fwd_inputs) is dropped
    assert abs(float(t['eb'][1])) == pytest.approx(1e-3)
    bad = good.clone()
    bad[:, 1] -= t['eb'][1]
    rel, ratio = U.bars(bad, y64, b64, k)
    assert rel < 1e-4 and ratio > 1.0, (rel, ratio)


# --------------------------------------------------------------------------------------------------------- room

def hold(worst, what, got, y64, b64, k):
    rel, ratio = U.bars(got, y64, b64, k)
    worst[0], worst[1] = max(worst[0], rel), max(worst[1], ratio)
    assert rel < 1e-4 and ratio <= 1.0, (what, rel, ratio)


def test_torch_fp32_on_the_cpu_stays_under_both_bars_on_every_case():
    worst, count = [0.0, 0.0], 0
    rows = [c for _, c in forward_rows() if not U.heavy(c)] + [c for c, _, _ in U.PAD_LANE_FWD] + [c for c, taken in U.THIN_CASES if not taken]
    for c in dict.fromkeys(rows):
        t, y64, b64, k, m = U.fwd_case(c)
        y32 = U.fwd_fp32(c, t)
        hold(worst, c, y32, y64, b64, k)
        if 'stats' in c.epi:
            r1, r2 = U.stats_bars(torch.stack([y32.sum((0, 2, 3)), (y32 * y32).sum((0, 2, 3))]), y64, b64, k, m)
            assert r1 <= 1.0 and r2 <= 1.0, (c, r1, r2)
        count += 1
    for c in U.DGRAD_CASES + U.PAD_LANE_DGRAD:
        t, dx64, b64, kmap = U.dgrad_case(c)
        hold(worst, c, U.dgrad_fp32(c, t), dx64, b64, kmap)
        count += 1
    left_out = [c for _, c in forward_rows() if U.heavy(c)]
    assert count > 140 and left_out and all(c in [r[0] for r in U.BRES_CASES] + [r[0] for r in U.BSTREAM_CASES] for c in left_out)
    print('torch fp32 CPU vs fp64 over %d cases: worst relative to max %.3e (held to 1e-4), worst |got - ref| / ((K + 8) 2^-24 B64) '
          '%.4f (held to 1)' % (count, worst[0], worst[1]))
