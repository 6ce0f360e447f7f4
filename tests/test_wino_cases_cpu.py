"""No GPU: the case tables of tests/wino_util.py reach every edge they claim, the host arithmetic of the Winograd wrappers
equals the restatement's own tiling, the restated matrices ARE the algorithm (fp64 Winograd against fp64 direct), the bar is
reachable (the fp32 restatement stays under half of it) and has teeth (four planted bugs exceed it; two of them stay under
the relative-to-max bar of tests/test_ops_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_util as U
from tests import wino_util as W

KEYS = list(W.TABLES)


@pytest.fixture(scope='module')
def ops():
    from hnd_ghnd_object_detectors_amd import ops as o               # loads the library; no device is touched
    return o


# --------------------------------------------------------------------------------------------------------- coverage

@pytest.mark.parametrize('key', KEYS, ids=str)
def test_every_table_reaches_every_edge(key):
    k, tile, direction = key
    cases = W.TABLES[key]
    assert all((c.k, c.tile, c.dgrad) == (k, tile, direction == 'dgrad') for c in cases)
    assert len(set(cases)) == len(cases)
    for pad in ((1,) if k == 3 else (0, 1)):
        sub = [c for c in cases if c.pad == pad]
        # a 2x2 correlation with padding 1 has no output extent of 1 (its input would be empty)
        want = set(W.EXTENT_CLASSES) - ({'one'} if (k, pad) == (2, 1) else set())
        assert set().union(*(W.extent_classes(c.oh, tile) for c in sub)) >= want
        assert set().union(*(W.extent_classes(c.ow, tile) for c in sub)) >= want
        if 'one' in want:
            assert any((c.oh, c.ow) == (1, tile + 1) for c in sub) and any((c.oh, c.ow) == (tile + 1, 1) for c in sub)
        assert {c.n for c in sub} >= {1, 3}
        assert {W.pad_class(c) for c in sub} >= {'below', 'on', 'above'}
        assert any(c.th * tile > c.oh and c.tw * tile > c.ow for c in sub)           # a corner tile partial in both directions
        assert any(c.quiet for c in sub)
    assert {c.cin for c in cases} >= {32, 64, 96, 256} and {c.cout for c in cases} >= {32, 64, 96, 256}
    assert any(c.cout == 1 for c in cases)                  # the smallest count the wrappers accept: a lane of exact zeros beside it
    forms = {(c.pro, c.epi) for c in cases}
    if key[::2] == (3, 'fwd'):
        assert forms >= {(p, W._epi3(tile, e)) for p in W.PRO_FORMS for e in W.EPI3}
        assert any(c.cout < 32 for c in cases) and any(c.cout % 32 and c.cout > 32 for c in cases)
    if key[::2] == (3, 'dgrad'):
        assert forms >= set(W.DGRAD3_FORMS)
        assert len({(c.oh, c.ow) for c in cases}) >= len(W.extents(tile))
    if key[::2] == (2, 'fwd'):
        assert forms >= {('relu', 'stats'), ('relu', '')}
    if key[::2] == (2, 'dgrad'):
        assert ('none', '') in forms and (tile == 4 or {('none', 'bwd'), ('none', 'bwd+lin')} <= forms)
    for c in cases:                                                   # what the wrappers and the library ask of a launch
        e = U.epi_of(c.epi)
        assert c.cin % 32 == 0
        assert not e & {'stats', 'bwd'} or (k == 2 and 512 % W.lanes_out(c) == 0)
        assert 'bwd' not in e or (tile == 6 and c.dgrad and e <= {'bwd', 'lin'} and W.lanes_out(c) == c.cout)
        assert 'mout' not in e or (k == 3 and tile != 2 and c.cout == W.ldc_of(c))
        assert not e & {'r1', 'mask', 'mout'} or k == 3


def test_only_the_over_cap_cases_walk_a_grid_stride_loop_twice():
    assert W.CAP == 256 * 32 * 256
    assert [(c.k, c.tile) for c in W.OVER_CASES] == list(W.KINDS) + [(2, 6)] and W.OVER_CASES[-1] is W.OVER_BWD
    c = W.OVER_BWD                      # hnd_wino26_output_bnbwd_stats: its own 2048 blocks, one tile row fewer fits them
    assert c.dgrad and c.epi == 'bwd' and W.conv_work(c)['wino2_output'][0] > W.CAP_WINO2_OUTPUT == W.conv_work(c)['wino2_output'][1]
    assert W.conv_work(c._replace(oh=c.oh - 6))['wino2_output'][0] <= W.CAP_WINO2_OUTPUT and W.stats_blocks(c) == 2048
    for c in W.OVER_CASES[:-1]:
        work = W.conv_work(c)
        assert len(work) == 2 and all(items > cap for items, cap in work.values()), (c, work)
        # the smallest such extent: one tile row fewer stays under the cap of the input transform
        fewer = W.conv_work(c._replace(oh=c.oh - c.tile))
        assert min(items - cap for items, cap in fewer.values() if cap == W.CAP) <= 0, fewer
        assert c.cin in (32, 64) and c.cout in (32, 64)
    for c in W.ALL_CASES + [w[0] for w in W.WGRAD_CASES]:
        assert all(items <= cap for items, cap in W.conv_work(c).values()), c
    for c, _, _ in W.WGRAD_CASES:
        assert W.work_items('wino2_dy', tiles=c.tiles, c=c.cout) <= W.CAP
        assert W.work_items('wino2_wgrad_out', cout=c.cout, cin=c.cin) <= W.CAP
    for n, oh, ow, ch, pad, relu in W.BNBWD_CASES:
        assert W.work_items('wino26_bnbwd', tiles=W.bnbwd_tiles(n, oh, ow, pad)[0], c=ch) <= W.CAP
    # the transforms launched alone: just above the cap, and the next smaller shape under it
    assert {(k, t) for k, t, _ in W.OVER_WEIGHTS} == set(W.KINDS) and {d for _, _, d in W.OVER_WEIGHTS} == {False, True}
    assert W.work_items('wino_weights', rows=W.OVER_ROWS, depth=W.OVER_DEPTH) > W.CAP
    assert W.work_items('wino_weights', rows=W.OVER_ROWS - 64, depth=W.OVER_DEPTH) <= W.CAP
    assert W.work_items('wino_weights', rows=W.OVER_ROWS, depth=W.OVER_DEPTH - 32) <= W.CAP
    assert W.OVER_ROWS % 64 == 0 and W.OVER_DEPTH % 32 == 0
    assert set(W.OVER_WGRAD_OUT) == {(t, st) for t in (4, 6) for st in (0, 1)}
    assert W.work_items('wino2_wgrad_out', cout=W.OVER_ROWS, cin=W.OVER_DEPTH) > W.CAP
    assert [row[4] for row in W.OVER_DY] == [4, 6]
    for n, oh, ow, cout, tile in W.OVER_DY:
        tiles = lambda h: n * ((h + tile - 1) // tile) * ((ow + tile - 1) // tile)
        assert W.work_items('wino2_dy', tiles=tiles(oh), c=cout) > W.CAP >= W.work_items('wino2_dy', tiles=tiles(oh - tile), c=cout)
    n, oh, ow, ch, pad, relu = W.BNBWD_OVER
    assert W.work_items('wino26_bnbwd', tiles=W.bnbwd_tiles(n, oh, ow, pad)[0], c=ch) > W.CAP
    assert W.work_items('wino26_bnbwd', tiles=W.bnbwd_tiles(n, oh - 6, ow, pad)[0], c=ch) <= W.CAP


def test_the_weight_gradient_and_bn_backward_tables_reach_their_edges():
    cases = W.WGRAD_CASES
    assert {(c.tile, c.pad, route) for c, route, _ in cases} == {(t, p, r) for t in (4, 6) for p in (0, 1) for r in ('fwd', 'own')}
    assert {alias for c, route, alias in cases if route == 'fwd'} == {True, False}
    assert any((c.cin, c.cout) == (64, 256) and route == 'own' for c, route, _ in cases)
    assert any(W.pad_class(c) == 'above' for c, _, _ in cases)
    # the swapped route (s transposed) is taken by exactly the cases wgrad_swapped names: ops.Wino2Wgrad's rule on the library's picker
    import ctypes
    from hnd_ghnd_object_detectors_amd import _lib, ops
    L = _lib.load()

    def variant(c, kc, kr):
        d = ops.WgradDesc()
        d.n, d.h, d.w_, d.cin, d.cin_real, d.oh, d.ow, d.cout, d.ldy = 1, 1, c.tiles, kc, kc, 1, c.tiles, kr, kr
        d.kh, d.kw, d.stride, d.pad, d.splitk, d.groups = 1, 1, 1, 0, 0, c.ncomp
        d.x_group_stride, d.dy_group_stride, d.dw_group_stride = c.tiles_pad * kc, c.tiles_pad * kr, kc * kr
        return int(L.hnd_conv2d_wgrad_variant(ctypes.byref(d)))
    for c, _, _ in cases:
        assert (variant(c, c.cin, c.cout) != 3 and variant(c, c.cout, c.cin) == 3) == W.wgrad_swapped(c), c
    assert {W.wgrad_swapped(c) for c, _, _ in cases} == {True, False}
    assert {(pad, relu) for _, _, _, _, pad, relu in W.BNBWD_CASES} == {(p, r) for p in (0, 1) for r in (True, False)}
    smaller = larger = 0
    for n, oh, ow, ch, pad, relu in W.BNBWD_CASES:
        walked, d, w = W.bnbwd_tiles(n, oh, ow, pad)
        assert walked == max(d, w) or walked > max(d, w)
        smaller += d < w
        larger += d > w
        assert pad == 1 or d <= w
    assert smaller and larger                 # the data gradient's grid the smaller of the two (pad 0), and the larger (pad 1)
    assert any(U.round_up(W.bnbwd_tiles(n, oh, ow, pad)[2], 128) > 128 for n, oh, ow, ch, pad, relu in W.BNBWD_CASES)


def test_no_relu_decision_of_the_bn_backward_cases_hangs_on_a_rounding():
    for row in W.BNBWD_CASES:
        t = W.bnbwd_inputs(*row)
        pre = t['x'].double() * t['scale'].double()[None, :, None, None] + t['shift'].double()[None, :, None, None]
        assert float(pre.abs().min()) >= 1e-3, row
    for c in W.ALL_CASES:
        if 'bwd' in U.epi_of(c.epi):
            t = W.inputs(c)
            pre = t['bx'].double() * t['bsc'].double()[None, :, None, None] + t['bsh'].double()[None, :, None, None]
            assert float(pre.abs().min()) >= 1e-3, c


# --------------------------------------------------------------------------------------------------------- host arithmetic

def test_host_arithmetic_of_the_wrappers_equals_the_restated_tiling(ops):
    from hnd_ghnd_object_detectors_amd import _lib
    L = _lib.load()
    for c in W.ALL_CASES + W.OVER_CASES:
        lo = W.lanes_out(c)
        if c.k == 3:
            assert ops.wino_tiles_pad(c.n, c.oh, c.ow, c.tile) == c.tiles_pad
            assert ops.WinoConv.scratch_elems(c.n, c.oh, c.ow, c.cin, c.cout, c.tile) == (c.ncomp * c.tiles_pad * c.cin, c.ncomp * c.tiles_pad * lo)
        else:
            assert int(L.hnd_wino2_tiles_pad(c.n, c.oh, c.ow, c.tile)) == c.tiles_pad
            assert ops.Wino2Conv.scratch_elems(c.n, c.oh, c.ow, c.cin, c.cout, c.tile) == (c.ncomp * c.tiles_pad * c.cin, c.ncomp * c.tiles_pad * lo)
            assert ops.Wino2Conv.stats_blocks(c.n, c.oh, c.ow, lo, c.tile) == W.stats_blocks(c)
            assert ops.Wino2InputTransform.scratch_elems(c.n, c.oh, c.ow, c.cin, c.tile) == c.ncomp * c.tiles_pad * c.cin
        d = W.patches(torch.zeros(c.n, 1, c.h, c.w), c.k, c.tile, c.pad) if c not in W.OVER_CASES else None
        assert d is None or (d.shape[0] * d.shape[2] * d.shape[3] == c.tiles and d.shape[4] ** 2 == c.ncomp)
    assert ops.wino_tiles_pad(1, 4, 4, 3) == -1 and int(L.hnd_wino2_tiles_pad(1, 4, 4, 2)) == -1
    assert ops.Wino2Conv.stats_blocks(1, 4, 4, 32, 5) == -1


# --------------------------------------------------------------------------------------------------------- the reference against itself

def test_direct64_is_torchs_fp64_convolution():
    for c in (W.TEETH_CASES[(3, 4)], W.TEETH_CASES[(2, 6)], W.TABLES[(2, 4, 'dgrad')][3]):
        t = W.inputs(c)
        a = t['x'].double()
        ref = F.conv2d(a, t['w'].double(), None, 1, c.pad)
        assert float((W.direct64(a, t['w'].double(), c.pad) - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
        if c.dgrad:                                         # the launch's correlation IS the data gradient of the parameter
            dx = torch.nn.grad.conv2d_input((c.n, c.cout, c.oh, c.ow), t['wp'].double(), a, stride=1, padding=c.k - 1 - c.pad)
            assert float((dx - ref).abs().max()) <= 1e-13 * float(ref.abs().max())


@pytest.mark.parametrize('key', KEYS, ids=str)
def test_the_bar_is_reachable_and_the_matrices_are_the_algorithm(key):
    """the fp32 restatement <= 0.5 of the bar and inside the relative-to-max bar on every case; the fp64 Winograd with the
    same matrices <= 1e-6 of the bar against the direct fp64 correlation"""
    k, tile, _ = key
    worst = (0.0, None)
    for c in W.TABLES[key]:
        t, y64, bw = W.conv_case(c)
        rel, ratio = W.bars(W.restate(c, t), y64, bw, c.cin, W.t_of(k, tile))
        assert ratio <= 0.5 and rel < W.rel_bar(tile), (c, rel, ratio)
        assert W.bars(W.restate(c, t, torch.float64), y64, bw, c.cin, W.t_of(k, tile))[1] <= 1e-6, c
        worst = max(worst, (ratio, W.case_id(c)))
    print('%s: T = %d, worst ratio of the fp32 restatement %.3f at %s' % (key, W.t_of(k, tile), worst[0], worst[1]))


def test_the_weight_gradient_bar_is_reachable():
    for tile in (4, 6):
        worst = (0.0, None)
        for c, _, _ in W.WGRAD_CASES:
            if c.tile != tile:
                continue
            t = W.wgrad_inputs(c)
            dw64, bw = W.wgrad_reference(c, t)
            rel, ratio = W.bars(W.wgrad_restate(c, t), dw64, bw, c.tiles, W.t_wgrad(tile))
            assert ratio <= 0.5 and rel < 2e-4, (c, rel, ratio)
            assert W.bars(W.wgrad_restate(c, t, torch.float64), dw64, bw, c.tiles, W.t_wgrad(tile))[1] <= 1e-6, c
            worst = max(worst, (ratio, W.case_id(c)))
        print('wgrad tile %d: T = %d, worst ratio of the fp32 restatement %.3f at %s' % (tile, W.t_wgrad(tile), worst[0], worst[1]))


def test_t_is_counted_from_the_matrices():
    assert {kt: W.t_of(*kt) for kt in W.KINDS} == {(3, 2): 30, (3, 4): 38, (3, 6): 46, (2, 4): 34, (2, 6): 42}
    assert (W.t_wgrad(4), W.t_wgrad(6), W.t_v(), W.t_z()) == (38, 50, 22, 22)
    for (k, tile), m in W.MATS.items():
        a = tile + k - 1
        assert m['BT'].shape == (a, a) and m['G'].shape == (a, k) and m['AT'].shape == (tile, a)
        assert k == 3 or (m['G2'].shape == (a, tile) and m['A2T'].shape == (2, a))


# --------------------------------------------------------------------------------------------------------- teeth

@pytest.mark.parametrize('kind', W.KINDS, ids=str)
def test_the_bar_has_teeth_where_the_relative_bar_has_none(kind):
    """Four bugs planted in the fp32 restatement on the quiet-image case of each tile (three images, the last scaled by
    1e-5; a partial last tile in both directions):
      edge: the last image reads the column one past its right edge as the next row's first pixel instead of zero;
      wrap: the out-of-image position right of row 0 of its last partial tile, epilogue shift applied, lands on row 1, column 0;
      sign: one coefficient of one row of A^T has the wrong sign;
      chan: the last input channel is dropped.
    Each must exceed the element-wise bar.  edge and wrap are confined to the quiet image, so the relative-to-max bar of
    tests/test_ops_gpu.py passes them: that is what the new bar adds.  sign and chan are wrong everywhere and cannot slip
    under any bar; they are here to show the bar sees the plain bugs too.  (The issue plants the wrong sign in tile 6's
    A^T; the same bug is planted for every tile.)"""
    c = W.TEETH_CASES[kind]
    assert c.quiet and c.n == 3 and c.tw * c.tile > c.ow and c.th * c.tile > c.oh and c.pad == 1 and 'eb' in c.epi
    t, y64, bw = W.conv_case(c)
    rel, ratio = W.bars(W.restate(c, t), y64, bw, c.cin, W.t_of(*kind))
    assert ratio <= 0.5 and rel < W.rel_bar(c.tile)
    for mutation in W.MUTATIONS:
        rel, ratio = W.bars(W.restate(c, t, mutate=mutation), y64, bw, c.cin, W.t_of(*kind))
        print('%s %s: relative to max %.2e, ratio to the element-wise bound %.1f' % (kind, mutation, rel, ratio))
        assert ratio > 1.0, (mutation, ratio)
        assert (rel < W.rel_bar(c.tile)) == (mutation in ('edge', 'wrap')), (mutation, rel)
