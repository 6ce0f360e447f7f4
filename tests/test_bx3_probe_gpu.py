"""The exact plane-product probes of tests/bx3_probe_util.py on the kernels: every launch here has ONE right answer in fp32,
the fp64 matmul of its operands, and every element must have exactly those bits -- in the emulated family (csrc/conv_bx3.hip,
conv_bx3_tiled.hip, conv_bxs.hip: a lost, doubled or crossed plane product in any build, k pass, tail chunk or column slice is
a wrong bit) and in the native fp32 kernels on the same operands.  tests/test_bx3_probe_cpu.py shows, with the reference
alone, that the operands are exact in any summation order and that every single fault of the six-pair product changes a bit
in every k block of every shape used here.

A probe SET is four launches: the cross layout at three phases and the mm launch (A and B both hi + mid).  Outputs are
pre-filled with NaN.  A failure names the first wrong (row, column): row class / chunk / tail, k block / 256-k pass, B class.
The statistical companion at the end holds full 24-bit non-negative operands to the native kernel's own error."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import bx3_probe_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NAN = float('nan')

# as tests/test_guard_bands_gpu.py selects them
BX3_BUILDS = [('persistent', 'bx3_tiled=0'), ('tiled', 'bx3_tiled=1,bx3_tiled_mi=1'), ('tiled', 'bx3_tiled=1,bx3_tiled_mi=2')]
BUILD_IDS = ['persistent', 'tiled_mi1', 'tiled_mi2']
PICKER_ENV = ('HND_DEBUG_PICKER', 'HND_BRES', 'HND_BRES2', 'HND_BSTREAM', 'HND_THIN_N')
NO_PERSISTENT = dict(HND_BRES='0', HND_BSTREAM='0')


@pytest.fixture(scope='module')
def ops():
    from hnd_ghnd_object_detectors_amd import ops as O
    return O


@pytest.fixture(scope='module')
def lib():
    from hnd_ghnd_object_detectors_amd import _lib
    return _lib.load()


def set_env(monkeypatch, **env):
    """the pickers' switches: everything not named is unset"""
    for k in PICKER_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=8)
def gemm_set(m, kdim, cout, stride=1):
    return U.gemm_probe_set(U.GEMM_MS[m] if isinstance(m, int) else m, kdim, cout, stride)


@functools.lru_cache(maxsize=4)
def tap_set(i):
    return U.conv_probe_set(*U.TAP_CASES[i][1:])


def variant_of(l):
    return l.variant if l.build is None else '%s/%s' % (l.variant, l.build)


def forward(ops, p, mode, expect, relay=None, **kw):
    """the probe's convolution under ops.emulation(mode) -> (y on the host, launch).  relay: 'own' = a zero-filled workspace
    of exactly the queried size, as the guard-band relay tests give it"""
    x, pk = p.x.to(DEV), ops.pack_weights(p.w.to(DEV).contiguous())
    y = torch.full(p.oshape, NAN, device=DEV)
    with ops.emulation(mode):
        l = ops.conv_forward(x, pk, y, p.k, p.stride, p.pad, **kw)
    assert variant_of(l) == expect, (variant_of(l), expect)
    assert (l.relay is not None) == (relay is not None), (l.relay is None, relay)
    if relay == 'own':
        from hnd_ghnd_object_detectors_amd import _lib
        need = int(_lib.load().hnd_conv2d_igemm_workspace(l.ref))
        assert need > 0
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        l.relay, l.desc.relay_ws = ws, ws.data_ptr()
        assert int(_lib.load().hnd_conv2d_igemm_workspace(l.ref)) == need
    l.run()
    ops.sync_check()
    return y.cpu(), l


def check_set(ops, probes, mode, expect, where, **kw):
    wrong = []
    for p in probes:
        y, _ = forward(ops, p, mode, expect, **kw)
        msg = p.first_wrong(y)
        if msg:
            wrong.append('[%s, %s] %s' % (where, expect, msg))
    return wrong


# -------------------------------------------------------------------------------------------- the emulated 1x1 family
@pytest.mark.parametrize('cout', U.GEMM_COUTS)
@pytest.mark.parametrize('kdim', U.GEMM_KS)
@pytest.mark.parametrize('build', BX3_BUILDS, ids=BUILD_IDS)
def test_emulated_1x1_gemm_is_exact_in_every_build_pass_and_tail(ops, monkeypatch, build, kdim, cout):
    """K = 128 / 256 / 512 / 1024: one, one, two and four 256-k passes; M = 64 (one chunk), 128, 240 and 364 (tails)"""
    set_env(monkeypatch, HND_DEBUG_PICKER=build[1])
    wrong = []
    for m in U.GEMM_MS:
        wrong += check_set(ops, gemm_set(m, kdim, cout), 'force', 'bx3_64/' + build[0], 'M %d K %d cout %d' % (m, kdim, cout))
    assert not wrong, '\n'.join(wrong[:8])


@pytest.mark.parametrize('build', BX3_BUILDS, ids=BUILD_IDS)
def test_emulated_stride2_1x1_gemm_is_exact(ops, monkeypatch, build):
    """(the input pixels a stride-2 1x1 conv never reads hold NaN)"""
    set_env(monkeypatch, HND_DEBUG_PICKER=build[1])
    kdim, cout, m = U.STRIDE2_CASE
    wrong = check_set(ops, gemm_set(m, kdim, cout, 2), 'force', 'bx3_64/' + build[0], 'stride 2, M %d K %d' % (m, kdim))
    assert not wrong, '\n'.join(wrong[:8])


@pytest.mark.parametrize('build', BX3_BUILDS, ids=BUILD_IDS)
def test_emulated_data_gradient_is_exact(ops, monkeypatch, build):
    """dx = dy W: the transposed operand (hnd_pack_weights transposed = 1) of a 1x1 conv's data gradient"""
    set_env(monkeypatch, HND_DEBUG_PICKER=build[1])
    kdim, cout, m = U.DGRAD_CASE
    wrong = []
    for p in gemm_set(m, kdim, cout):
        dy = p.x.to(DEV)
        w = p.B.contiguous().view(kdim, cout, 1, 1).to(DEV)            # the forward conv's OIHW weight: cout -> cin = K -> N
        dx = torch.full(p.oshape, NAN, device=DEV)
        with ops.emulation('force'):
            ls, _ = ops.conv_dgrad(dy, w, dx, 1, 1, 0)
        assert [variant_of(l) for l in ls] == ['bx3_64/' + build[0]]
        ls[0].run()
        ops.sync_check()
        msg = p.first_wrong(dx.cpu())
        if msg:
            wrong.append('[data gradient, %s] %s' % (build[0], msg))
    assert not wrong, '\n'.join(wrong[:8])


def _nibbles(y):
    v = y.view(*y.shape[:3], y.shape[3] // 4, 4) > 0
    return (v[..., 0].to(torch.uint8) | (v[..., 1].to(torch.uint8) << 1) | (v[..., 2].to(torch.uint8) << 2)
            | (v[..., 3].to(torch.uint8) << 3))


def _exact_sum(*terms):
    s = sum(t.double() for t in terms)
    assert torch.equal(s.float().double(), s), 'the riders leave the fp32 grid'
    return s.float()


@pytest.mark.parametrize('build', BX3_BUILDS, ids=BUILD_IDS)
def test_emulated_gemm_with_residual_relu_and_mask_nibbles_is_exact(ops, monkeypatch, build):
    """the residual is small integers, so the sum stays exact; K = 512: the ReLU and the nibbles belong to the last pass"""
    set_env(monkeypatch, HND_DEBUG_PICKER=build[1])
    kdim, cout, m = U.RIDER_CASE
    g = torch.Generator().manual_seed(3)
    wrong = []
    for p in gemm_set(m, kdim, cout):
        res = torch.randint(-3, 4, p.oshape, generator=g).float()
        want = F.relu(_exact_sum(p.want.view(p.oshape), res))
        mo = torch.full(p.oshape[:3] + (cout // 4,), 255, dtype=torch.uint8, device=DEV)
        y, _ = forward(ops, p, 'force', 'bx3_64/' + build[0], res1=res.to(DEV), relu=True, mask_out=mo)
        p.want, keep = want.view(p.M, p.N), p.want
        msg = p.first_wrong(y)
        p.want = keep
        if msg:
            wrong.append('[residual + ReLU + mask_out, %s] %s' % (build[0], msg))
        assert torch.equal(mo.cpu(), _nibbles(y)), 'mask nibbles differ from the stored values'
    assert not wrong, '\n'.join(wrong[:8])


@pytest.mark.parametrize('build', BX3_BUILDS, ids=BUILD_IDS)
def test_emulated_gemm_with_the_upsampled_residual_is_exact(ops, monkeypatch, build):
    set_env(monkeypatch, HND_DEBUG_PICKER=build[1])
    kdim, cout, m = U.RES_UP_CASE
    g = torch.Generator().manual_seed(4)
    wrong = []
    for p in gemm_set(m, kdim, cout):
        n, oh, ow, _ = p.oshape
        top = torch.randint(-3, 4, (n, oh // 2, ow // 2, cout), generator=g).float()
        up = top.repeat_interleave(2, 1).repeat_interleave(2, 2)
        want = _exact_sum(p.want.view(p.oshape), up)
        y, _ = forward(ops, p, 'force', 'bx3_64/' + build[0], res1=top.to(DEV), res1_up=True)
        p.want, keep = want.view(p.M, p.N), p.want
        msg = p.first_wrong(y)
        p.want = keep
        if msg:
            wrong.append('[res1_up, %s] %s' % (build[0], msg))
    assert not wrong, '\n'.join(wrong[:8])


# ------------------------------------------------------------------------------------- the B-streamed emulation kernel
@pytest.mark.parametrize('wn1', [False, True], ids=['default_tile', 'bxs_wn1'])
@pytest.mark.parametrize('case', range(len(U.TAP_CASES)), ids=[c[0] + '_%d' % c[2] for c in U.TAP_CASES])
def test_bxs_over_taps_and_long_k_is_exact(ops, monkeypatch, case, wn1):
    """every tap has its own k blocks; the padding is the convolution's own zeros, so border rows stay exact"""
    cout = U.TAP_CASES[case][2]
    set_env(monkeypatch, HND_DEBUG_PICKER='bxs_wn1' if wn1 else '')
    expect = 'bxs_128' if cout % 128 == 0 and not wn1 else 'bxs_64'
    wrong = check_set(ops, tap_set(case), 'bxs', expect, U.TAP_CASES[case][0])
    assert not wrong, '\n'.join(wrong[:8])


def test_bxs_with_the_relay_is_exact(ops, lib, monkeypatch):
    """tiles split between neighbouring workgroups and their partial sums parked in the relay workspace: still one answer"""
    set_env(monkeypatch, HND_DEBUG_PICKER='bstream_all', HND_BRES='0')
    _, n, cin, h, w, cout = U.RELAY_CASE
    lib.hnd_relay_timeouts(1)
    wrong = check_set(ops, gemm_set((n, h, w), cin, cout), 'bxs', 'bxs_128', 'relay', relay='own')
    assert lib.hnd_relay_timeouts(0) == 0
    assert not wrong, '\n'.join(wrong[:8])


# -------------------------------------------------------------------------------- the native family on the same operands
@pytest.mark.parametrize('tile', [0, 1, 2, 3])
@pytest.mark.parametrize('kdim', U.NATIVE_KS)
def test_native_tiled_kernel_is_exact_on_every_block_tile(ops, monkeypatch, kdim, tile):
    set_env(monkeypatch, HND_DEBUG_PICKER='igemm_tile=%d' % tile, HND_THIN_N='0', **NO_PERSISTENT)
    wrong = check_set(ops, gemm_set(U.NATIVE_M, kdim, U.NATIVE_COUT), 'off', ops.TILE_NAMES[tile], 'native K %d' % kdim)
    wrong += check_set(ops, tap_set(U.NATIVE_TAP_CASE), 'off', ops.TILE_NAMES[tile], 'native 3x3 stride 2')
    assert not wrong, '\n'.join(wrong[:8])


def test_native_b_streamed_kernel_is_exact(ops, monkeypatch):
    set_env(monkeypatch, HND_DEBUG_PICKER='bstream_all', HND_BRES='0')
    wrong = check_set(ops, gemm_set(U.NATIVE_M, 1024, U.NATIVE_COUT), 'off', 'bstream_128', 'native K 1024')
    wrong += check_set(ops, tap_set(U.NATIVE_TAP_CASE), 'off', 'bstream_128', 'native 3x3 stride 2')
    assert not wrong, '\n'.join(wrong[:8])


@pytest.mark.parametrize('case', U.BRES_CASES, ids=[c[0] for c in U.BRES_CASES])
def test_native_b_resident_kernels_are_exact(ops, monkeypatch, case):
    expect, kdim, cout, m_shape, bres2 = case
    set_env(monkeypatch, HND_DEBUG_PICKER='bres_all', HND_BRES='512', HND_BSTREAM='0', HND_BRES2=bres2)
    wrong = check_set(ops, gemm_set(m_shape, kdim, cout), 'off', expect, 'native B-resident')
    assert not wrong, '\n'.join(wrong[:8])


# ------------------------------------------------------------------------------------------- the statistical companion
def _rowsum_abs(x, wt):
    """sum over k of |x_k| |w_k| per output element: the scale every summation error is proportional to"""
    return x.double().abs() @ wt.double().abs()


@pytest.mark.parametrize('kdim', [256, 1024])
@pytest.mark.parametrize('build', BX3_BUILDS, ids=BUILD_IDS)
def test_full_width_non_negative_operands_stay_within_the_native_kernels_error(ops, monkeypatch, build, kdim):
    """What the probes cannot carry: full 24-bit operands.  Non-negative A (as after a ReLU) with a range of exp2(3 randn)
    per row and per k block, non-negative B, no epilogue.  q = max |y - fp64| / sum_k |a||b| over 240 x 128 = 30 720
    elements; the bar is q_emulated <= 1.5 q_native + 2^-24 on the same operands (the margin of the project's emulation
    tests, one output rounding).  With operands of one sign a lost hi.lo product does not average away: it costs about
    2^-17, more than ten times the native figure."""
    n, oh, ow = U.GEMM_MS[U.TAIL_M]
    m, cout, nb = n * oh * ow, 128, kdim // U.KSTEP
    g = torch.Generator().manual_seed(11 + kdim)
    scale = torch.exp2(3 * torch.randn(m, nb, generator=g)).repeat_interleave(U.KSTEP, 1)
    A = (torch.randn(m, kdim, generator=g).abs() * scale).float()
    B = torch.randn(kdim, cout, generator=g).abs() / kdim ** 0.5
    ref, den = A.double() @ B.double(), _rowsum_abs(A, B)
    assert m * cout >= 10 ** 4
    x = A.view(n, oh, ow, kdim).contiguous().to(DEV)
    pk = ops.pack_weights(B.t().contiguous().view(cout, kdim, 1, 1).to(DEV))
    q = {}
    for mode, picker in (('off', ''), ('force', build[1])):
        set_env(monkeypatch, HND_DEBUG_PICKER=picker)
        y = torch.full((n, oh, ow, cout), NAN, device=DEV)
        with ops.emulation(mode):
            l = ops.conv_forward(x, pk, y, 1, 1, 0)
        assert (variant_of(l) == 'bx3_64/' + build[0]) if mode == 'force' else not l.variant.startswith('bx'), variant_of(l)
        l.run()
        ops.sync_check()
        assert not bool(torch.isnan(y).any())
        q[mode] = float(((y.cpu().double().view(m, cout) - ref).abs() / den).max())
    from tests.conftest import record_achieved
    record_achieved('[bf16x3 probes, %s K %d, non-negative full-width operands] q_emulated %.3e, q_native %.3e '
                    '(max |y - fp64| / sum |a||b|)' % (BUILD_IDS[BX3_BUILDS.index(build)], kdim, q['force'], q['off']))
    print('q_emulated %.4e q_native %.4e' % (q['force'], q['off']))
    assert q['force'] <= 1.5 * q['off'] + 2.0 ** -24, (q['force'], q['off'])
