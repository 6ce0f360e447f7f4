"""CPU: the weight-gradient case tables of tests/wgrad_util.py, held before anyone has a GPU.

* the fp64 reference of tests/test_wgrad_gpu.py equals torch's fp64 autograd of the same expression;
* every case reaches the kernel its table claims, under the switches the table names (hnd_conv2d_wgrad_variant reads
  pointer VALUES only and answers without a device, as in tests/test_conv_picker_cpu.py);
* the ring cases cover every template build wring_plan can choose (csrc/conv_wgrad_ring.hip), by a restatement of its rule;
* the staged table keeps the geometries the suite never ran before: the conditions below keep it from quietly shrinking."""
import ctypes
import itertools
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_util as U

SWITCHES = ('HND_WGRAD_RING', 'HND_THIN_WGRAD', 'HND_STEM7', 'HND_DEBUG_PICKER')


@pytest.fixture(scope='module')
def variant_of():
    """variant_of(switches, fields) -> hnd_conv2d_wgrad_variant's code, with the switches set for that call only"""
    import __graft_entry__ as g
    g.build()
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    names = [n for n, _ in _lib.WgradDesc._fields_]
    ptr = dict((n, 0x100000 * (i + 1)) for i, n in enumerate(names))          # distinct 16-byte aligned pointer values
    saved = {s: os.environ.get(s) for s in SWITCHES}

    def ask(env, fields):
        d = _lib.WgradDesc()
        for n in names:
            if n in fields:
                setattr(d, n, int(fields[n]))
        d.x, d.dy, d.dw, d.slabs = ptr['x'], ptr['dy'], ptr['dw'], ptr['slabs']
        d.pro_scale = ptr['pro_scale'] if fields['has_scale'] else None
        d.pro_shift = ptr['pro_shift'] if fields['has_shift'] else None
        for s in SWITCHES:
            os.environ.pop(s, None)
        os.environ.update(env)
        return int(lib.hnd_conv2d_wgrad_variant(ctypes.byref(d)))

    try:
        yield ask
    finally:
        for s in SWITCHES:
            os.environ.pop(s, None)
        os.environ.update({s: v for s, v in saved.items() if v is not None})


@pytest.mark.parametrize('case', [(2, 32, 7, 9, 5, 3, 1, 1, 'relu'), (1, 64, 6, 5, 8, 2, 1, 0, 'none'),
                                  (2, 3, 11, 10, 6, 3, 2, 1, 'shift'), (1, 32, 5, 5, 4, 1, 1, 0, 'scale')])
def test_the_reference_is_torch_fp64_autograd_of_the_same_expression(case):
    n, cin, h, w, cout, k, stride, pad, pro = case
    x, dy, ps, pb, relu, dw64, s64, m = U.conv_inputs(*case)
    assert dw64.dtype == torch.float64 and s64.dtype == torch.float64 and dw64.shape == s64.shape == (cout, cin, k, k)
    assert m == n * dy.shape[2] * dy.shape[3]
    wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    a = x.double()
    if ps is not None:
        a = a * ps.double()[None, :, None, None]
    if pb is not None:
        a = a + pb.double()[None, :, None, None]
    if relu:
        a = F.relu(a)
    F.conv2d(a, wt, None, stride, pad).backward(dy.double())
    assert float((dw64 - wt.grad).abs().max() / wt.grad.abs().max()) < 1e-12
    # the magnitude sum: every term of dw taken by absolute value, so it bounds |dw| and is the plain sum without a prologue
    assert bool((s64 >= dw64.abs() * (1 - 1e-12)).all())
    if ps is None:
        wt.grad = None
        F.conv2d(x.double().abs(), wt, None, stride, pad).backward(dy.double().abs())
        assert float((s64 - wt.grad).abs().max() / wt.grad.abs().max()) < 1e-12


def test_the_grouped_reference_is_the_per_group_matrix_product():
    xs, dys, dw64, s64, m = U.grouped_inputs(2, 13, 8, 5)
    for g in range(2):
        assert float((dw64[g] - dys[g].double().t() @ xs[g].double()).abs().max()) < 1e-12
    assert m == 13 and bool((s64 >= dw64.abs()).all())


def test_every_case_reaches_the_kernel_its_table_names(variant_of):
    routes = U.routing()
    assert len(routes) > 100
    wrong = []
    for label, env, fields, expect in routes:
        code = variant_of(env, fields)
        if code != U.VARIANT_CODE[expect] or (code == 0 and expect != U.staged_name(fields['cout'])):
            wrong.append((label, env, expect, code))
    assert not wrong, wrong
    assert {e for _, _, _, e in routes} == set(U.KERNELS)


def test_the_ring_boundaries_sit_where_the_table_says(variant_of):
    """ow == 4 is the narrowest map of the tap form and ow == 3 falls to the staged kernel; without the debug picker
    the tap form is off altogether"""
    by_ow = {U.desc_fields(*c[:9])['ow']: c for c in U.RING_CASES if c[:3] == (2, 64, 9) and c[5] == 2}
    assert by_ow[4][10] == 'wgrad_ring' and by_ow[3][10] == 'wgrad_m128' and by_ow[4][:3] + by_ow[4][4:9] == by_ow[3][:3] + by_ow[3][4:9]
    for c in U.RING_CASES:
        if c[9]:
            assert variant_of(U.ring_env(False), U.desc_fields(*c[:9])) == 0, c
    small = [c for c in U.RING_CASES if c[10] == 'wgrad_ring' and U.desc_fields(*c[:9])['oh'] * U.desc_fields(*c[:9])['ow'] * c[0] < 32]
    assert {c[11][2] for c in small} == {True, False}                  # splits clamped by the block count, both forms


def test_the_ring_cases_state_their_build_and_cover_every_reachable_one():
    seen = set()
    for n, cin, h, w, cout, k, stride, pad, pro, picker, expect, build in U.RING_CASES:
        if expect != 'wgrad_ring':
            assert build is None
            continue
        assert U.ring_takes(cin, cout, k, stride, pad) and build == U.ring_build(cin, cout, k, stride, pad), (cin, cout, k, build)
        assert picker == build[2]                                       # the tap form needs the debug picker, the 1x1 form not
        seen.add(build)
    for groups, tiles, cin, cout, build in U.GROUPED_CASES:
        assert groups > 1 and tiles % 32 != 0 and U.ring_takes(cin, cout, 1, 1, 0) and build == U.ring_build(cin, cout, 1, 1, 0)
        seen.add(build)
    assert seen == U.REACHABLE_BUILDS, (seen ^ U.REACHABLE_BUILDS)
    # every non-tap ring case is a plain conv with no prologue; the tap cases run with and without one
    assert all(c[8] == 'none' for c in U.RING_CASES if c[11] and not c[11][2])
    assert {c[8] == 'none' for c in U.RING_CASES if c[11] and c[11][2]} == {True, False}
    assert {'scale', 'shift', 'relu', U.SCALE_RELU} <= {c[8] for c in U.RING_CASES if c[11] and c[11][2]}
    # what the rule can reach at all, over every channel pair and geometry the predicate admits
    reached = {U.ring_build(cin, cout, k, stride, pad)
               for cin, cout, k, stride, pad in itertools.product(range(64, 577, 64), range(128, 1025, 128), (1, 2, 3), (1, 2), (0, 1))
               if U.ring_takes(cin, cout, k, stride, pad)}
    assert reached == U.REACHABLE_BUILDS, (reached ^ U.REACHABLE_BUILDS)
    # AH == 1 means cout % 256 != 0, which is taps_small: a tap build <1, *> always runs as "taps x2"
    assert not [b for b in reached if b[2] and b[0] == 1 and not b[3]]
    assert all(b[:2] == (1, 1) for b in reached if b[3] or b[4])


def test_the_staged_table_keeps_what_the_suite_never_ran_before():
    cases = U.STAGED_CASES
    assert 24 <= len(cases) <= 36 and len(set(c[:9] for c in cases)) == len(cases)
    hand = [(2, 256, 9, 11, 64, 1, 1, 0), (2, 64, 9, 12, 128, 1, 2, 0), (2, 64, 16, 20, 64, 3, 1, 1), (2, 128, 17, 21, 128, 3, 2, 1),
            (2, 128, 16, 20, 128, 3, 2, 1), (1, 32, 11, 13, 64, 5, 1, 2), (2, 32, 19, 23, 64, 7, 2, 3), (2, 96, 10, 12, 192, 3, 1, 1),
            (2, 160, 9, 9, 100, 1, 1, 0), (2, 64, 8, 10, 5, 2, 1, 1), (2, 64, 8, 10, 6, 2, 1, 1), (2, 64, 8, 10, 7, 2, 1, 1),
            (1, 64, 4, 4, 64, 2, 1, 0), (1, 64, 5, 5, 64, 2, 1, 0), (1, 64, 5, 6, 64, 2, 1, 0)]
    assert set(hand) <= {c[:8] for c in cases}
    fields = [U.desc_fields(*c[:9]) for c in cases]
    assert all(f['oh'] > 0 and f['ow'] > 0 and f['pad'] <= f['kh'] // 2 + 1 for f in fields)
    assert {1, 2, 3, 4, 5, 7} <= {c[5] for c in cases}
    assert {(c[6], c[7] > 0) for c in cases} == {(1, False), (1, True), (2, False), (2, True)}
    assert {c[4] % 4 for c in cases} == {0, 1, 2, 3}
    assert [c for c in cases if 128 < c[4] < 256 and c[4] % 128]
    assert {(4, 3), (32, 32), (96, 96), (160, 160)} <= {(f['cin'], f['cin_real']) for f in fields}
    assert all(f['ldy'] == 8 for f in fields if f['cout'] in (5, 6, 7))
    m = [f['n'] * f['oh'] * f['ow'] for f in fields]
    assert min(m) < 16 and 16 in m and 20 in m
    assert [1 for c, mm in zip(cases, m) if max(c[9]) > math.ceil(mm / 16)]
    assert 1000 in [c for c in cases if c[:8] == (1, 64, 5, 6, 64, 2, 1, 0)][0][9]
    # the four prologue forms across the list, all four on at least two geometries, split-K 0 / 1 / 3 on a third
    assert {c[8] for c in cases} == set(U.ALL_FORMS)
    forms = {}
    for c in cases:
        forms.setdefault(c[:8], set()).add(c[8])
    assert sum(v >= set(U.PRO_FORMS) for v in forms.values()) >= 2
    assert [c for c in cases if max(c[9]) >= 32 and max(c[9]) <= math.ceil(c[0] * 16 * 20 / 16)]      # >= 32 slabs really summed
    assert all(c[9][0] == 0 for c in cases) and 3 * sum(c[9][:3] == (0, 1, 3) for c in cases) >= len(cases)


def test_the_thin_and_stem_tables_keep_their_edges():
    thin = [c for c in U.THIN_CASES if c[7] == 'thin_wgrad']
    conv3, conv4 = [c for c in thin if c[1] == 64], [c for c in thin if c[4] == 64]
    assert len(conv3) + len(conv4) == len(thin)
    assert {c[4] for c in conv3 if c[0] * c[2] * c[3] < 512} == {1, 2, 3, 4} and {c[1] for c in conv4} == {3, 4}
    for form in (conv3, conv4):
        assert {c[5] for c in form} == {0, 1}
        assert [c for c in form if U.out_extent(c[2], 2, 1, c[5]) == 1 and U.out_extent(c[3], 2, 1, c[5]) == 1]
        assert [c for c in form if c[0] * c[2] * c[3] > 1024]
    assert [c for c in U.THIN_CASES if c[7] == 'wgrad_m64' and c[1] == 64 and c[4] == 5]
    assert all(set(U.ALL_FORMS) <= {c[6] for c in form} for form in (conv3, conv4))
    th, tw = U.STEM_TILE
    ext = [(U.out_extent(h, 7, 2, 3), U.out_extent(w, 7, 2, 3), c) for n, c, h, w in U.STEM_CASES]
    assert [1 for oh, ow, c in ext if oh < th and ow < tw] and [1 for oh, ow, c in ext if oh == 1]
    assert [1 for oh, ow, c in ext if ow == tw + 1] and [1 for oh, ow, c in ext if oh == th + 1]
    assert {c for _, _, c in ext} == {3, 4}
