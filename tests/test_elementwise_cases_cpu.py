"""CPU: the case tables, references and bars of tests/elementwise_util.py, held before anyone has a GPU.

1. every fp64 reference equals torch's fp64 autograd of the same expression to 1e-12;
2. the bars are attainable: a plain fp32 CPU computation of each operation stays at ratio <= 1 on every case, the near-zero
   placement included (the gate of the stand-in comes from its own stored forward, as on the device);
3. the bars bite: one injected fault per kernel pushes the ratio above 1;
4. the tables reach every branch the kernels of csrc/elementwise.hip have, by a restatement of each branch condition, so
   they cannot quietly shrink."""
import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_util as E


def relmax(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


# ---------------------------------------------------------------------------------------------------- 1. references

@pytest.mark.parametrize('relu', [False, True])
def test_bn_references_are_torch_fp64_autograd_of_batch_norm(relu):
    """finalize -> affine -> reduce -> backward finalize -> apply, chained in fp64 with nothing rounded in between,
    against F.batch_norm (+ ReLU) and its autograd in fp64.  The partials are unrounded fp64 tile sums here; the channel
    whose variance is 0 up to fp64 cancellation (CLAMP_CH: rstd there amplifies 1e-13 to 1e-8) is left out."""
    g = E.gen(1)
    npix, c = 2 * 1024 + 37, 12
    keep = [i for i in range(c) if i != E.CLAMP_CH]
    x = (torch.randn(npix, c, generator=g, dtype=torch.float64) * 1.7 + 0.4)
    x[:, E.CONST_CH], x[:, E.CLAMP_CH] = 0.5, 37.25
    gamma = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(c, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(c, generator=g, dtype=torch.float64), torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    gout = torch.randn(npix, c, generator=g, dtype=torch.float64)

    xt, gt, bt = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm_t, rv_t = rm.clone(), rv.clone()
    out = F.batch_norm(xt, rm_t, rv_t, gt, bt, True, E.f32(E.MOMENTUM), E.f32(E.EPS))
    out = F.relu(out) if relu else out
    out.backward(gout)

    nt = (npix + E.STAT_TILE - 1) // E.STAT_TILE
    x3 = F.pad(x, (0, 0, 0, nt * E.STAT_TILE - npix)).view(nt, E.STAT_TILE, c)
    part = torch.stack((x3.sum(1), (x3 * x3).sum(1)), 1)
    fin = E.finalize_reference(part, c, npix, gamma, beta, rm, rv)
    assert relmax(fin['rm'], rm_t) < 1e-12 and relmax(fin['rv'][keep], rv_t[keep]) < 1e-12
    assert relmax(fin['mean'], x.mean(0)) < 1e-12 and relmax(fin['var'][keep], x.var(0, unbiased=False)[keep]) < 1e-12
    y = E.affine_reference(x, fin['scale'], fin['shift'], relu)
    assert relmax(y[:, keep], out.detach()[:, keep]) < 1e-12
    gate = (y > 0) if relu else None
    s1, s2, _, _ = E.reduce_reference(gout, x, fin['mean'], fin['rstd'], gate)
    bf = E.bwd_finalize_reference(torch.stack((s1, s2), 1), c, npix, gamma, fin['mean'], fin['rstd'])
    assert relmax(bf['dbeta'][keep], bt.grad[keep]) < 1e-12 and relmax(bf['dgamma'][keep], gt.grad[keep]) < 1e-12
    dx, _ = E.apply_reference(gout, x, torch.stack((bf['k1'], bf['k2'], bf['k3'])), gate)
    assert relmax(dx[:, keep], xt.grad[:, keep]) < 1e-12


def test_pool_references_are_torch_autograd_and_the_kernels_scan_rule():
    for n, c, h, w in [(2, 4, 7, 9), (1, 8, 16, 17), (2, 4, 1, 1), (1, 4, 2, 3), (1, 4, 33, 5)]:
        g = E.gen(h * 100 + w)
        x = E.pool_inputs(n, c, h, w, False)
        y, tap = E.pool_expected(x)
        xt = x.double().requires_grad_(True)
        dy = torch.randn(y.shape, generator=g)
        sc = torch.rand(c, generator=g) + 0.5
        F.max_pool2d(xt, 3, 2, 1).backward(dy.double())
        ref, _ = E.pool_bwd_reference(dy, tap, x, sc)
        want = xt.grad * (x > 0) * sc.double()[None, :, None, None]
        assert relmax(ref, want) < 1e-12
        # the scan rule of the kernel, restated, is torch's: values and taps, with -inf windows and NaNs
        xs = E.pool_inputs(n, c, h, w)
        ys, taps = E.pool_expected(xs)
        got_y, got_tap = E.pool_scan(xs)
        assert E.same_bits(got_y, ys) and torch.equal(got_tap, taps)
    xs = E.pool_inputs(1, 8, 16, 17)
    ys, _ = E.pool_expected(xs)
    assert bool(torch.isnan(ys).any()) and bool(torch.isinf(ys).any()) and bool((ys[torch.isfinite(ys)] < 0).any())


def test_upsample_reference_is_the_integer_rule_on_the_listed_geometries():
    for (h, w), (H, W) in E.UPSAMPLE_GEOMS:
        g = torch.randn(2, 4, H, W, generator=E.gen(H + W), dtype=torch.float64)
        ref = E.upsample_reference(g, h, w)
        assert relmax(E.upsample_standin(g, h, w, dtype=torch.float64), ref) < 1e-12


def test_the_index_rule_of_the_kernel_equals_torchs_on_the_fpn_domain_and_not_beyond():
    """the kernel reads coarse floor(Y h / H) in integers, torch floorf(Y * (float)h / (float)H): the same index for every
    fine pixel when H < 1500 and h is ceil(H / 2), floor(H / 2) or H; not for (h, H) = (820, 1122)"""
    for H in range(1, E.INDEX_RULE_LIMIT):
        for h in E.fpn_coarse_extents(H):
            assert torch.equal(E.nearest_src_exact(H, h), E.nearest_src_float(H, h)), (h, H)
    h, H = E.INDEX_RULE_COUNTEREXAMPLE
    assert not torch.equal(E.nearest_src_exact(H, h), E.nearest_src_float(H, h))
    # ... and nearest_src_float is what F.interpolate does
    for h, H in [E.INDEX_RULE_COUNTEREXAMPLE, (25, 49), (7, 13)]:
        src = F.interpolate(torch.arange(h, dtype=torch.float32).view(1, 1, h, 1), size=(H, 1), mode='nearest')
        assert torch.equal(src.view(-1).long(), E.nearest_src_float(H, h))


# ---------------------------------------------------------------------------------------------------- 2, 3. bars

def _fin_got(i, drop=None):
    return E.finalize_standin(i['part'], i['gamma'].numel(), i['count'], i['gamma'], i['beta'], i['rm'], i['rv'],
                              drop_tile=drop)


@pytest.mark.parametrize('case', E.FINALIZE_CASES)
def test_finalize_bars_hold_for_the_standin_and_catch_a_dropped_tile(case):
    ntiles, last, c, cs, running = case
    i = E.finalize_inputs(*case)
    ref = E.finalize_reference(i['part'], c, i['count'], i['gamma'], i['beta'], i['rm'], i['rv'])
    r = E.finalize_bars(_fin_got(i), ref, i['beta'])
    assert set(r) == ({'mean', 'rstd', 'scale', 'shift', 'rm', 'rv'} if running else {'mean', 'rstd', 'scale', 'shift'})
    assert max(r.values()) <= 1.0, r
    # the special channels are what they claim to be, on the rounded partials
    assert float(ref['raw_var'][E.CONST_CH]) == 0.0 and float(ref['rstd'][E.CONST_CH]) == 1.0 / E.f32(E.EPS) ** 0.5
    assert float(ref['raw_var'][E.CLAMP_CH]) < -E.EPS          # without the clamp: the square root of a negative number
    if i['count'] > 1000:
        assert 8.0 < float(ref['mean'][E.FAR_CH] * ref['rstd'][E.FAR_CH]) < 12.0
    if ntiles > 1:
        bad = E.finalize_bars(_fin_got(i, drop=ntiles // 2), ref, i['beta'])
        assert bad['mean'] > 1.0 and bad['shift'] > 1.0, bad


def _stored_gate(i, relu):
    """the stand-in's own stored forward decides the gate, as the device's mask does"""
    if not relu:
        return None
    return E.gate_of(E.nibbles_of(E.affine_standin(i['x'], i['scale'], i['shift'], True)))


def _fp64_gate(i):
    return E.affine_reference(i['x'], i['scale'], i['shift'], False) > 0


@pytest.mark.parametrize('cs,npix', E.STREAM_CASES)
@pytest.mark.parametrize('relu', [False, True])
def test_affine_and_apply_bars_hold_for_the_standin_and_catch_their_faults(cs, npix, relu):
    i = E.bn_inputs(npix, cs, cs, relu)
    y = E.affine_standin(i['x'], i['scale'], i['shift'], relu)
    ratio, signs = E.affine_bars(y, i['x'], i['scale'], i['shift'], relu)
    assert ratio <= 1.0 and signs, (ratio, signs)
    assert torch.equal(E.gate_of(E.nibbles_of(y)), y > 0)
    gate = _stored_gate(i, relu)
    k123 = torch.stack((i['gamma'] * i['rstd'], -i['gamma'] * i['rstd'] * 0.01, i['shift'] * 0.1))
    ref = E.apply_reference(i['g'], i['x'], k123, gate)
    assert E.apply_bars(E.apply_standin(i['g'], i['x'], k123, gate), ref) <= 1.0
    if cs > 4:
        at = (npix // 2) * (cs // 4) + 3                       # a lane that reads the next channel group
        bad, _ = E.affine_bars(E.affine_standin(i['x'], i['scale'], i['shift'], relu, wrong_group_at=at), i['x'],
                               i['scale'], i['shift'], relu)
        assert bad > 1.0
        assert E.apply_bars(E.apply_standin(i['g'], i['x'], k123, gate, wrong_group_at=at), ref) > 1.0
    if relu and i['near'].sum() > 50:
        # a gate taken from the fp64 sign, not from the stored forward, flips near-zero elements: orders above the bar
        assert bool((_fp64_gate(i) != gate)[i['near']].any())
        assert E.apply_bars(E.apply_standin(i['g'], i['x'], k123, _fp64_gate(i)), ref) > 100.0


@pytest.mark.parametrize('npix,cs', E.REDUCE_CASES)
@pytest.mark.parametrize('relu', [False, True])
def test_reduce_bars_hold_for_the_standin_and_catch_their_faults(npix, cs, relu):
    i = E.bn_inputs(npix, cs, cs, relu)
    gate = _stored_gate(i, relu)
    ref = E.reduce_reference(i['g'], i['x'], i['mean'], i['rstd'], gate)
    r = E.reduce_bars(E.reduce_standin(i['g'], i['x'], i['mean'], i['rstd'], gate), ref, npix)
    assert max(r) <= 1.0, r
    if not relu:                                               # the last pixel of the (partial) last tile skipped
        bad = E.reduce_bars(E.reduce_standin(i['g'], i['x'], i['mean'], i['rstd'], None, skip_pixel=npix - 1), ref, npix)
        assert max(bad) > 1.0, bad
    if relu and i['near'].sum() > 50:
        bad = E.reduce_bars(E.reduce_standin(i['g'], i['x'], i['mean'], i['rstd'], _fp64_gate(i)), ref, npix)
        assert max(bad) > 1.0, bad


@pytest.mark.parametrize('npix,c,cs', E.BWD_FINALIZE_CASES)
def test_bwd_finalize_bars_hold_for_the_standin_and_catch_a_dropped_tile(npix, c, cs):
    i = E.bn_inputs(npix, cs, c, True)
    gate = _stored_gate(i, True)
    part = E.reduce_standin(i['g'], i['x'], i['mean'], i['rstd'], gate)
    ref = E.bwd_finalize_reference(part, c, npix, i['gamma'], i['mean'], i['rstd'])
    r = E.bwd_finalize_bars(E.bwd_finalize_standin(part, c, npix, i['gamma'], i['mean'], i['rstd']), ref, npix)
    assert max(r.values()) <= 1.0, r
    if part.shape[0] > 1:
        bad = E.bwd_finalize_bars(E.bwd_finalize_standin(part, c, npix, i['gamma'], i['mean'], i['rstd'], drop_tile=1),
                                  ref, npix)
        assert bad['dbeta'] > 1.0 and bad['k3'] > 1.0, bad


def test_pool_checks_hold_for_the_standin_and_catch_a_tap_off_by_one():
    for n, c, h, w in [(1, 4, 15, 17), (3, 68, 3, 16), (1, 4, 1, 1), (3, 4, 2, 33)]:
        g = E.gen(5 * h + w)
        x = E.pool_inputs(n, c, h, w)
        y, tap = E.pool_expected(x)
        dy, sc = torch.randn(y.shape, generator=g), torch.rand(c, generator=g) + 0.5
        ref = E.pool_bwd_reference(dy, tap, x, sc)
        assert E.pool_bwd_bars(E.pool_bwd_standin(dy, tap, x, sc), ref) <= 1.0
        # gate and argmax apart: argmax pixels whose gate is shut, open gates that are no argmax
        assert bool(((ref[1] == 0) & (x > 0)).any()) or h * w == 1
    x = E.pool_inputs(1, 4, 15, 17)
    y, tap = E.pool_expected(x)
    dy, sc = torch.ones(y.shape), torch.ones(4)
    ref = E.pool_bwd_reference(dy, tap, x, sc)
    open_windows = torch.nonzero((y > 0) & (tap % 3 < 2))
    bad = tap.clone()
    b, ch, oy, ox = open_windows[0].tolist()
    bad[b, ch, oy, ox] += 1
    assert not torch.equal(bad, tap) and E.pool_bwd_bars(E.pool_bwd_standin(dy, bad, x, sc), ref) > 1.0


@pytest.mark.parametrize('geom', E.UPSAMPLE_GEOMS)
def test_upsample_bars_hold_for_the_standin_and_catch_a_missed_row(geom):
    (h, w), (H, W) = geom
    g = E.gen(3 * H + W)
    gf, base = torch.randn(2, 4, H, W, generator=g), torch.randn(2, 4, h, w, generator=g)
    assert E.upsample_bars(E.upsample_standin(gf, h, w), gf, None, h, w) <= 1.0
    assert E.upsample_bars(E.upsample_standin(gf, h, w, base), gf, base, h, w) <= 1.0
    bad = E.upsample_standin(gf, h, w, base, miss_row_of=(h - 1, w // 2))
    assert E.upsample_bars(bad, gf, base, h, w) > 1.0


# ---------------------------------------------------------------------------------------------------- 4. coverage

def test_finalize_table_reaches_every_branch_of_bn_finalize_kernel():
    cases = E.FINALIZE_CASES
    assert {c[0] for c in cases} == set(E.FINALIZE_NTILES) == {1, 63, 64, 65, 192, 193, 256, 257, 449, 1000}
    for nt in E.FINALIZE_NTILES:                       # every class with a padded and an unpadded channel stride
        assert {c[2] == c[3] for c in cases if c[0] == nt} == {True, False}, nt
    assert {(c[2], c[3]) for c in cases} == {(3, 4), (12, 32), (40, 64), (64, 64), (80, 96), (256, 256)}
    lanes = {nt: [E.finalize_lane_passes(nt, t0) for t0 in range(64)] for nt in E.FINALIZE_NTILES}
    assert all(p == 0 for nt in (1, 63, 64, 65, 192) for p, _ in lanes[nt])          # the unrolled loop never entered
    assert lanes[193][0] == (1, 0) and all(p == 0 for p, _ in lanes[193][1:])         # ... by the first lane only
    assert (1, 3) in lanes[449] and max(p for p, _ in lanes[1000]) >= 3               # a remainder after a pass; several
    assert any(r == 0 and nt > 1 for nt in (1, 63) for _, r in lanes[nt])             # lanes with no tile at all
    assert {c[4] for c in cases if c[2] == c[3]} == {True, False} == {c[4] for c in cases if c[2] != c[3]}
    assert any(c[0] == 1 and c[1] == 1 for c in cases)                                # count == 1
    assert any(c[2] % 16 and c[2] > 16 and c[3] > c[2] for c in cases)                # a 16-channel block straddles c
    assert any(c[1] < E.STAT_TILE and c[0] > 1 for c in cases)


def test_stream_tables_reach_both_paths_and_every_size_class():
    assert {cs for cs, _ in E.STREAM_CASES} == set(E.STREAM_CS) == {4, 32, 64, 96, 256, 2048}
    assert {cs for cs in E.STREAM_CS if not E.stream_fixed(cs)} == {96, 2048} and 2048 // 4 > 256
    for cs in E.STREAM_CS:
        n4s = [npix * (cs // 4) for c, npix in E.STREAM_CASES if c == cs]
        if cs // 4 <= 128:
            assert any(v < 256 for v in n4s), cs
            assert any(1024 < v < 2048 and v % 256 for v in n4s), cs
        else:                                           # n4 is a multiple of 512: neither class exists
            assert any(v < E.CHUNK for v in n4s) and any(E.CHUNK < v < 2 * E.CHUNK for v in n4s)
        assert any(v > 4 * E.CHUNK and v % E.CHUNK for v in n4s), cs
        assert all(v <= E.CHUNK_CAP * E.CHUNK // 64 for v in n4s)       # nowhere near the cap of grid_for_chunks
    assert all(n4 <= E.CHUNK_CAP * E.CHUNK // 64 for n4 in E.MASK_N4) and E.MASK_N4 == (1, 255, 256, 1025)


def test_reduce_tables_reach_every_row_count_tile_class_and_refusal():
    assert {cs for _, cs in E.REDUCE_CASES} == {4, 32, 64, 128, 256, 512, 1024}
    assert {256 // (cs // 4) for _, cs in E.REDUCE_CASES} == {256, 32, 16, 8, 4, 2, 1}
    assert all(E.reduce_accepts(cs) for _, cs in E.REDUCE_CASES)
    assert not any(E.reduce_accepts(cs) for cs in E.REDUCE_REFUSED_CS) and E.REDUCE_REFUSED_CS == (96, 2048)
    for cs in (4, 32, 64):
        assert {n for n, c in E.REDUCE_CASES if c == cs} >= {1, 1023, 1024, 1025, 2 * 1024 + 37}
    over = [(n, cs) for n, cs in E.REDUCE_CASES if E.bwd_ntiles(n) > 64]
    assert over == [(65 * 1024 + 5, 4)] and E.bwd_ntiles(over[0][0]) == 66           # 65 full tiles and one of 5 pixels
    assert any(E.bwd_ntiles(n) > 64 and c < cs for n, c, cs in E.BWD_FINALIZE_CASES)
    assert any(c == cs for _, c, cs in E.BWD_FINALIZE_CASES) and any(cs - c >= 4 for _, c, cs in E.BWD_FINALIZE_CASES)
    assert all(E.reduce_accepts(cs) for _, _, cs in E.BWD_FINALIZE_CASES)
    for npix, cs in E.REDUCE_CASES:                     # the near-zero placement is there, and is near zero
        if npix * cs < 2000:
            continue
        i = E.bn_inputs(npix, cs, cs, True)
        assert float(i['near'].float().mean()) >= 0.05
        out = E.affine_reference(i['x'], i['scale'], i['shift'], False)[i['near']]
        lim = 10 * E.U * i['shift'].double().abs().expand(npix, cs)[i['near']]
        assert bool((out.abs() <= lim).all()) and bool((i['g'][i['near']].abs() >= 0.5).all())


def test_pool_and_fpn_tables_reach_every_strip_count_and_both_grid_strides():
    cases = E.pool_cases()
    assert {(h, w) for _, _, h, w in cases} == {(h, w) for h in E.POOL_EXTENTS for w in E.POOL_EXTENTS}
    assert E.POOL_EXTENTS == (1, 2, 3, 15, 16, 17, 33) and [E.pool_out(h) for h in (15, 16, 17, 33)] == [8, 8, 9, 17]
    strips = {(E.pool_out(h) + E.POOL_STRIP - 1) // E.POOL_STRIP for _, _, h, _ in cases}
    assert strips == {1, 2, 3}
    for h in E.POOL_EXTENTS:
        assert {(n, c) for n, c, hh, _ in cases if hh == h} == {(n, c) for n in E.POOL_BATCHES for c in E.POOL_CHANNELS}
    assert any((c // 4) & (c // 4 - 1) for _, c, _, _ in cases)                        # c / 4 no power of two
    assert all(E.pool_threads(*c) <= E.GRID_CAP * 256 for c in cases)
    n, c, h, w = E.POOL_GRID_STRIDE_CASE
    assert E.GRID_CAP * 256 < E.pool_threads(n, c, h, w) < 1.01 * E.GRID_CAP * 256 and n * h * w * (c // 4) < 2 ** 31
    assert E.ADD_N4 == (1, 255, 256, 4096 * 256 + 3) and E.ADD_N4[-1] > E.GRID_CAP * 256
    assert E.UPSAMPLE_GEOMS == [((7, 9), (14, 18)), ((7, 9), (13, 17)), ((7, 9), (7, 9)), ((1, 1), (2, 1)),
                                ((25, 42), (50, 84)), ((25, 42), (49, 83))]
    assert E.UPSAMPLE_CHANNELS == (4, 36, 256) and E.UPSAMPLE_BATCHES == (1, 2)
    assert {(h % 2, w % 2) for _, h, w, _ in E.SUBSAMPLE_CASES} >= {(0, 0), (1, 1), (1, 0), (0, 1)}
    assert {c for _, _, _, c in E.SUBSAMPLE_CASES} == {4, 68}
