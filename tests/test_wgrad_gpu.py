"""GPU: every weight-gradient kernel and build of hnd_conv2d_wgrad against an fp64 reference, across geometries.

The cases are the tables of tests/wgrad_util.py (tests/test_wgrad_cases_cpu.py holds their routing and coverage without a
GPU).  Every case: launch on NaN-filled dw and slabs, compare with fp64 under BOTH bars of wgrad_util.bars -- relative to
the largest element < 1e-4 (the project's bar for fp32-MFMA convs) and, element by element,
|got - dw64| <= (M + 8) 2^-24 S64 + 1e-30, which holds for any summation order and catches an error confined to small
elements (a wrong tap at a border, a padded column leaking) -- then launch again and ask for the same bits: the fixed
summation order is a documented property of all four kernels.  Where a second kernel takes the same descriptor both run."""
import pytest
import torch

from tests import wgrad_util as U

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
SWITCHES = ('HND_WGRAD_RING', 'HND_THIN_WGRAD', 'HND_STEM7', 'HND_DEBUG_PICKER')
WORST = {k: [0.0, 0.0, 0] for k in U.KERNELS}       # kernel -> [relative to max, ratio to the element-wise bound, launches]


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
        record_achieved(lambda k=k: '[weight gradient vs fp64, %-11s %3d launches] worst relative to max %.2e (held to 1e-4), worst '
                        '|got - ref| / ((M + 8) 2^-24 S64) %.3f (held to 1)' % (k + ',', WORST[k][2], WORST[k][0], WORST[k][1]))
    yield


def switches(monkeypatch, env):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def hold(got, dw64, s64, m, kernel, what):
    """both bars, after the figures are on record"""
    assert bool(torch.isfinite(got).all()), (kernel, what)
    rel, ratio = U.bars(got, dw64, s64, m)
    w = WORST[kernel]
    w[0], w[1], w[2] = max(w[0], rel), max(w[1], ratio), w[2] + 1
    print('%s %s: relative to max %.3e, ratio to the element-wise bound %.4f' % (kernel, what, rel, ratio))
    assert rel < 1e-4, (kernel, what, rel)
    assert ratio <= 1.0, (kernel, what, ratio)


def operands(x, dy, ps, pb, fields, lane_value=0.0):
    """NHWC device tensors with the channel lanes the descriptor names (padding lanes hold lane_value)"""
    xd = U.pad_channels(x.permute(0, 2, 3, 1), fields['cin'], lane_value).contiguous().to(DEV)
    dyd = U.pad_channels(dy.permute(0, 2, 3, 1), fields['ldy'], lane_value).contiguous().to(DEV)
    psd = None if ps is None else U.pad_channels(ps, fields['cin']).to(DEV)
    pbd = None if pb is None else U.pad_channels(pb, fields['cin']).to(DEV)
    return xd, dyd, psd, pbd


def launch(ops, opnds, fields, relu, expect, slabs=None):
    """one launch on NaN-filled dw and slabs -> dw on the host; the descriptor is the one the CPU file routed"""
    xd, dyd, psd, pbd = opnds
    k = fields['kh']
    dw = torch.full((fields['cout'], fields['cin_real'], k, k), NAN, device=DEV)
    l = ops.conv_wgrad(xd, dyd, dw, k, fields['stride'], fields['pad'], pro_scale=psd, pro_shift=pbd, pro_relu=relu,
                       splitk=fields['splitk'], slabs=slabs)
    got = {n: getattr(l.desc, n) for n in fields if not n.startswith('has_')}
    assert got == {n: v for n, v in fields.items() if not n.startswith('has_')}, got
    assert l.variant == expect, (l.variant, expect)
    assert slabs is None or l.desc.slabs == slabs.data_ptr()
    l.keep[3].fill_(NAN)
    l.run()
    ops.sync_check()
    return dw.cpu()


def run_case(ops, monkeypatch, env, case, expect, splitk=0, what=''):
    """the whole procedure for one direct-conv case on one kernel: NaN buffers, both bars, the same bits twice"""
    switches(monkeypatch, env)
    x, dy, ps, pb, relu, dw64, s64, m = U.conv_inputs(*case)
    fields = U.desc_fields(*case, splitk=splitk)
    opnds = operands(x, dy, ps, pb, fields)
    first = launch(ops, opnds, fields, relu, expect)
    hold(first, dw64, s64, m, expect, '%r %s' % (case, what))
    assert torch.equal(first, launch(ops, opnds, fields, relu, expect)), (expect, case, what)
    return first


@pytest.mark.parametrize('case', U.STAGED_CASES, ids=lambda c: '-'.join(str(v) for v in c[:9]))
def test_staged_kernel_geometry_matrix(ops, case, monkeypatch):
    """csrc/conv_wgrad.hip wgrad_kernel<64 | 128>: kernel sizes 1 .. 7, both strides with and without padding, channel
    tails of both loaders, ragged column and row tiles, reductions around one k-step, the four prologue forms, split-K
    chosen / 1 / 3 / far more than there are k-steps"""
    for splitk in case[9]:
        run_case(ops, monkeypatch, U.STAGED_ENV, case[:9], U.staged_name(case[4]), splitk, 'splitk %d' % splitk)


@pytest.mark.parametrize('case', U.RING_CASES, ids=lambda c: '-'.join(str(v) for v in c[:9]))
def test_ring_builds_and_the_staged_kernel_on_the_same_descriptor(ops, case, monkeypatch):
    """csrc/conv_wgrad_ring.hip: one case per template build (the 1x1 form ungrouped, the tap form at 3x3, stride 2 and
    1x1 stride 2), the ow == 4 / ow == 3 boundary of wgrad_ring_applies and fewer pixels than one ring block"""
    run_case(ops, monkeypatch, U.ring_env(case[9]), case[:9], case[10], what='build %r' % (case[11],))
    run_case(ops, monkeypatch, U.ring_env(case[9], False), case[:9], U.staged_name(case[4]), what='ring off')


@pytest.mark.parametrize('case', U.GROUPED_CASES, ids=lambda c: '-'.join(str(v) for v in c[:4]))
def test_grouped_ring_form_with_ragged_tiles(ops, case, monkeypatch):
    """the Winograd-domain reductions: `groups` 1x1 problems over `tiles` pixels, 77 = 2 ring blocks + 13"""
    groups, tiles, cin, cout, build = case
    xs, dys, dw64, s64, m = U.grouped_inputs(groups, tiles, cin, cout)
    xd, dyd = xs.to(DEV).contiguous(), dys.to(DEV).contiguous()
    fields = U.grouped_fields(groups, tiles, cin, cout)
    for ring_on, expect in ((True, 'wgrad_ring'), (False, U.staged_name(cout))):
        switches(monkeypatch, U.ring_env(False, ring_on))
        outs = []
        for _ in range(2):
            dw = torch.full((groups, cout, cin), NAN, device=DEV)
            d = ops.WgradDesc()
            for n, v in fields.items():
                if not n.startswith('has_'):
                    setattr(d, n, v)
            d.x, d.dy, d.dw = xd.data_ptr(), dyd.data_ptr(), dw.data_ptr()
            slabs = torch.full(((ops.wgrad_workspace_of(d) + 3) // 4,), NAN, device=DEV)
            d.slabs = slabs.data_ptr()
            l = ops.WgradLaunch(d, (xd, dyd, dw, slabs), 2 * groups * tiles * cout * cin)
            assert l.variant == expect, (l.variant, expect)
            l.run()
            ops.sync_check()
            outs.append(dw.cpu())
        hold(outs[0], dw64, s64, m, expect, 'grouped %r build %r' % (case[:4], build))
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('case', U.THIN_CASES, ids=lambda c: '-'.join(str(v) for v in c[:7]))
def test_thin_kernel_small_maps_and_channel_counts(ops, case, monkeypatch):
    """csrc/conv_wgrad.hip thin_wgrad_kernel: one block, a ragged last block, 1 .. 4 thin channels, a single output
    pixel, both forms and both pads; cout 5 must fall to the staged kernel.  Each also on the staged kernel."""
    n, cin, h, w, cout, pad, pro, expect = case
    conv = (n, cin, h, w, cout, 2, 1, pad, pro)
    run_case(ops, monkeypatch, {'HND_THIN_WGRAD': '1'}, conv, expect)
    run_case(ops, monkeypatch, {'HND_THIN_WGRAD': '0'}, conv, U.staged_name(cout), what='thin off')


@pytest.mark.parametrize('case', U.STEM_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_stem_kernel_below_and_across_one_tile(ops, case, monkeypatch):
    """csrc/conv_stem.hip stem7_wgrad_kernel: maps smaller than its 8 x 16 output tile, a single output row, a single
    column or row beyond a tile, three and four real input channels.  Each also on the staged kernel."""
    n, cin, h, w = case
    conv = (n, cin, h, w, 64, 7, 2, 3, 'none')
    run_case(ops, monkeypatch, {'HND_STEM7': '1'}, conv, 'stem7_wgrad')
    run_case(ops, monkeypatch, {'HND_STEM7': '0'}, conv, 'wgrad_m64', what='stem off')


def test_three_layers_share_one_dirty_oversized_workspace(ops, monkeypatch):
    """the engine hands every layer the same slabs, sized for the largest: whatever another layer left there (NaN here,
    before each launch) must not reach dw, and the bits are those of a private workspace"""
    switches(monkeypatch, {})
    layers, need = [], 0
    for case in U.SHARED_CASES:
        x, dy, ps, pb, relu, dw64, s64, m = U.conv_inputs(*case[:9])
        fields = U.desc_fields(*case[:9])
        opnds = operands(x, dy, ps, pb, fields)
        private = launch(ops, opnds, fields, relu, case[9])
        probe = ops.conv_wgrad(opnds[0], opnds[1], torch.empty_like(private, device=DEV), fields['kh'], fields['stride'],
                               fields['pad'], pro_scale=opnds[2], pro_shift=opnds[3], pro_relu=relu)
        need = max(need, ops.wgrad_workspace_of(probe.desc))
        layers.append((case, opnds, fields, relu, private, dw64, s64, m))
    assert len({c[9] for c in U.SHARED_CASES}) == 3 and need > 0
    shared = torch.empty((need + 3) // 4 + 1024, device=DEV)
    for case, opnds, fields, relu, private, dw64, s64, m in layers:
        got = launch(ops, opnds, fields, relu, case[9], slabs=shared)        # (launch fills the slabs it is given with NaN)
        hold(got, dw64, s64, m, case[9], '%r shared workspace' % (case[:9],))
        assert torch.equal(got, private), case


@pytest.mark.parametrize('case', U.PAD_LANE_CASES, ids=lambda c: '-'.join(str(v) for v in c[:10]))
def test_padding_lanes_of_x_and_dy_never_reach_dw(ops, case, monkeypatch):
    """include/hnd_hip.h stores 3 channels in 4 lanes (x) and cout in ldy lanes (dy) and does not ask callers to zero the
    rest: dw is the same bit for bit when those lanes hold 3e4"""
    switches(monkeypatch, case[10])
    x, dy, ps, pb, relu, dw64, s64, m = U.conv_inputs(*case[:9])
    fields = U.desc_fields(*case[:9])
    assert fields['cin'] > fields['cin_real'] or fields['ldy'] > fields['cout']
    clean = launch(ops, operands(x, dy, ps, pb, fields), fields, relu, case[9])
    hold(clean, dw64, s64, m, case[9], '%r zero padding lanes' % (case[:9],))
    dirty = launch(ops, operands(x, dy, ps, pb, fields, U.PAD_LANE_VALUE), fields, relu, case[9])
    assert torch.equal(clean, dirty), case
