"""GPU: every kernel stays inside the buffers its ABI sizes (include/hnd_hip.h: caller-owned buffers of stated sizes).

Each case puts every device buffer its launch touches into ONE tests/guard_util.Arena -- inputs, outputs, residuals,
masks, nibbles, statistics, scratch, workspaces, packed operands and their bf16 images, each exactly as large as the
header or the size query says -- runs the launch once, then ops.sync_check(), then arena.check() (no guard byte
changed), then compares the result (finite, since every view and guard starts as 0xFF = NaN) with a torch CPU reference
at the bar the existing test of that kernel states:
  native fp32 convs / weight gradients: 1e-4 relative-to-max (tests/test_ops_gpu.py, module docstring and every conv test);
  emulated convs: rel-L2 against fp64 < 1e-6 and <= 1.5 x the native kernel's on the same operands + 1e-8
  (tests/test_bx3_gpu.py::test_bx3_1x1_conv_against_fp64_beside_the_native_kernel, tests/test_bxs_gpu.py);
  index work and re-layouts: exact.
The GEMM, conv and weight-gradient families are deterministic and placement-independent (asserted all over the suite),
so their guarded output must also be torch.equal to the same launch on ordinary buffers.

Every case declares the exports it covers (@covers) and records the kernel variant that ran; the last test of the file
holds the union of variants to the names of the header's enums (ops.TILE_NAMES, ops.WGRAD_NAMES), tests/test_guard_ledger_cpu.py holds the
union of exports, with NO_DEVICE_OUTPUT, to the header.  Importing this module does not touch the GPU.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import guard_util as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# ---------------------------------------------------------------------------------------------------------- the ledger
LEDGER = {}          # test function name -> exports of include/hnd_hip.h whose device writes it guards


def covers(*exports):
    def deco(fn):
        LEDGER.setdefault(fn.__name__, set()).update(exports)
        return fn
    return deco


# exports that write no device memory a caller owns: nothing to guard
NO_DEVICE_OUTPUT = {
    'hnd_last_error_string': 'error string (host)',
    'hnd_abi_version': 'constant',
    'hnd_sync_check': 'stream synchronisation, no buffer',
    'hnd_relay_timeouts': 'reads / clears a host-visible error word the library owns',
    'hnd_device_arch': 'device name (host)',
    'hnd_conv2d_igemm_workspace': 'size query',
    'hnd_conv2d_igemm_tile': 'variant query',
    'hnd_conv2d_igemm_build': 'variant query',
    'hnd_bf16x3_recommended': 'policy query',
    'hnd_bf16x3s_recommended': 'policy query',
    'hnd_pack_bf16x3_elems': 'size query',
    'hnd_pack_bf16x3s_elems': 'size query',
    'hnd_conv2d_wgrad_workspace': 'size query',
    'hnd_conv2d_wgrad_variant': 'variant query',
    'hnd_wino_tiles_pad': 'size query',
    'hnd_wino2_tiles_pad': 'size query',
    'hnd_wino2_stats_blocks': 'size query',
    'hnd_bn_bwd_ntiles': 'size query',
    'hnd_mse_scratch_elems': 'size query',
    'hnd_minmax_scratch_elems': 'size query',
    'hnd_channel_sum_scratch_elems': 'size query',
    'hnd_nms_workspace': 'size query',
    'hnd_argsort_desc_workspace': 'size query',
    'hnd_workspace_size': 'size query',
    'hnd_comm_unique_id': 'RCCL (host buffer): tests/test_ops_gpu.py world-of-one test',
    'hnd_comm_init': 'RCCL: tests/test_ops_gpu.py world-of-one test',
    'hnd_comm_destroy': 'RCCL: tests/test_ops_gpu.py world-of-one test',
    'hnd_allreduce_avg_flat': 'RCCL writes the buffer: tests/test_ops_gpu.py world-of-one test',
}

# kernel variants (ops.ConvLaunch.variant [+ '/' + build], ops.WgradLaunch.variant) that ran under guards in this process
RAN = set()


# ------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


@pytest.fixture(scope='module')
def lib():
    from hnd_ghnd_object_detectors_amd import _lib
    return _lib.load()


PICKER_ENV = ('HND_DEBUG_PICKER', 'HND_BRES', 'HND_BRES2', 'HND_BSTREAM', 'HND_STEM7', 'HND_THIN_N', 'HND_WGRAD_RING',
              'HND_THIN_WGRAD')


def set_env(monkeypatch, **env):
    """the pickers' switches (the ones the bit-identity tests use): everything not named is unset"""
    for k in PICKER_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


class Plain(object):
    """ordinary buffers with the interface of guard_util.Arena: the same launch is built on these first (its output is what
    the guarded one must equal bit for bit), and what it asked for sizes the arena"""

    def __init__(self):
        self.specs = []

    def take(self, name, shape, dtype=torch.float32, fill=None, guard_rows=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.specs.append((shape, dtype))
        t = torch.full((G.view_bytes(shape, dtype),), G.FILL, dtype=torch.uint8, device=DEV).view(dtype).view(shape)
        if fill is not None:
            t.fill_(fill)
        return t

    def load(self, name, tensor, guard_rows=None):
        v = self.take(name, tuple(tensor.shape), tensor.dtype)
        v.copy_(tensor)
        return v

    def check(self):
        pass


def guarded(ops, build):
    """build(alloc) makes its buffers with alloc.take / alloc.load, launches once and returns its outputs.  Runs it on
    ordinary buffers, then inside an Arena sized from what it asked for: launch, sync_check, arena.check -- in that order."""
    plain = Plain()
    out_p = build(plain)
    ops.sync_check()
    arena = G.Arena(DEV, G.arena_bytes(plain.specs))
    out_g = build(arena)
    ops.sync_check()
    arena.check()
    return out_p, out_g


def only_guarded(ops, build):
    return guarded(ops, build)[1]


def nhwc(t, cpad=None):
    """NCHW cpu tensor -> NHWC cpu tensor (channels zero-padded to cpad)"""
    t = t.permute(0, 2, 3, 1).contiguous()
    if cpad is not None and cpad != t.shape[-1]:
        t = F.pad(t, (0, cpad - t.shape[-1]))
    return t.contiguous()


def relmax(a, b):
    """relative-to-max error (tests/test_ops_gpu.py relerr)"""
    return float((a.double().cpu() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def rel_l2(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm())


def finite(t):
    return bool(torch.isfinite(t).all())


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rehome(ops, alloc, pk0, name, emu='off'):
    """the packed operand pk0 (made by the library into a buffer of its own) copied into a view of exactly rows_pad * kdim
    floats per group, and its bf16 images made by hnd_pack_bf16x3(s) into views of exactly *_elems uint16 elements"""
    from hnd_ghnd_object_detectors_amd import _lib
    L = _lib.load()
    assert pk0.buf.numel() == max(pk0.groups, 1) * pk0.rows_pad * pk0.kdim
    buf = alloc.load(name, pk0.buf)
    pk = ops.PackedWeight(buf, pk0.rows, pk0.kdim, pk0.chan_pad, pk0.chan_real, groups=pk0.groups,
                          group_stride=pk0.group_stride, taps=pk0.taps)
    if emu in ('bx3', 'force') and pk.can_bx3():
        img = alloc.take(name + '_bx3', int(L.hnd_pack_bf16x3_elems(pk.rows_pad, pk.kdim, pk.groups)), torch.int16)
        pk.bx3 = ops.bx3_image(buf, pk.rows_pad, pk.kdim, pk.groups, pk.group_stride, out=img)
    if emu in ('bxs', 'force') and pk.can_bxs():
        img = alloc.take(name + '_bxs', int(L.hnd_pack_bf16x3s_elems(pk.rows_pad, pk.kdim, pk.groups)), torch.int16)
        pk.bxs = ops.bxs_image(buf, pk.rows_pad, pk.kdim, pk.groups, pk.group_stride, out=img)
    return pk


def own_relay(ops, alloc, l, ws=None):
    """the launch's relay workspace replaced by a zero-filled view of exactly hnd_conv2d_igemm_workspace bytes"""
    from hnd_ghnd_object_detectors_amd import _lib
    need = int(_lib.load().hnd_conv2d_igemm_workspace(l.ref))
    assert need > 0 and l.relay is not None
    if ws is None:
        ws = alloc.take('relay', need, torch.uint8, fill=0)
    assert ws.numel() == need
    l.relay, l.desc.relay_ws = ws, ws.data_ptr()
    assert int(_lib.load().hnd_conv2d_igemm_workspace(l.ref)) == need
    return ws


def variant_of(l):
    return l.variant if l.build is None else '%s/%s' % (l.variant, l.build)


def conv_build(ops, c):
    """c: dict of a conv case (cpu tensors: x NHWC, wt OIHW, optional pro / epi vectors, res1 / res2 / mask NHWC,
    mask_bits uint8; flags relu, pro_relu, res1_up, stats, mask_out; k, s, p; emu; expect = variant that must run).
    Returns build(alloc) for guarded()."""
    wdev = c['wt'].to(DEV).contiguous()
    cin_pad = c['x'].shape[3]
    pk0 = ops.pack_weights(wdev, chan_pad=cin_pad)
    n, h, w, _ = c['x'].shape
    k, s, p = c['k'], c.get('s', 1), c.get('p', 0)
    oh, ow = ops.conv_out_size(h, k, s, p), ops.conv_out_size(w, k, s, p)
    ldc = ops.chan_pad_of(c['wt'].shape[0])
    emu = c.get('emu', 'off')

    def build(alloc):
        x = alloc.load('x', c['x'])
        pk = rehome(ops, alloc, pk0, 'w', emu)
        y = alloc.take('y', (n, oh, ow, ldc))
        kw = {}
        for name in ('pro_scale', 'pro_shift', 'epi_scale', 'epi_shift', 'res1', 'res2', 'mask', 'mask_bits'):
            if c.get(name) is not None:
                kw[name] = alloc.load(name, c[name])
        if c.get('mask_out'):
            kw['mask_out'] = alloc.take('mask_out', (n, oh, ow, ldc // 4), torch.uint8)
            assert kw['mask_out'].shape == ops.mask_nibbles_like(y).shape
        if c.get('stats'):
            kw['stats'] = alloc.take('stats', (ops.stats_tiles(n * oh * ow), 2, ldc))
        with ops.emulation(emu):
            l = ops.conv_forward(x, pk, y, k, s, p, relu=c.get('relu', False), pro_relu=c.get('pro_relu', False),
                                 res1_up=c.get('res1_up', False), **kw)
        assert variant_of(l) == c['expect'], (variant_of(l), c['expect'])
        assert (l.relay is not None) == bool(c.get('relay')), (l.relay is None, c.get('relay'))
        outs = {}
        if l.relay is not None:
            ws = own_relay(ops, alloc, l)
            l.run()                                     # the second epoch on the same workspace must stay inside it too
            ops.sync_check()
            outs['y_first'] = y.clone()
        l.run()
        ops.sync_check()
        if isinstance(alloc, G.Arena):
            RAN.add(variant_of(l))
        outs.update(y=y, launch=l, **{q: kw[q] for q in ('mask_out', 'stats') if q in kw})
        return outs
    return build


def conv_ref(c):
    """fp64 torch CPU reference of conv_build's launch, NHWC [n, oh, ow, cout]"""
    x = c['x'].double().permute(0, 3, 1, 2)[:, :c['wt'].shape[1]]
    if c.get('pro_scale') is not None:
        cr = c['wt'].shape[1]
        x = x * c['pro_scale'][:cr].double()[None, :, None, None] + c['pro_shift'][:cr].double()[None, :, None, None]
        if c.get('pro_relu'):
            x = F.relu(x)
    r = F.conv2d(x, c['wt'].double(), None, c.get('s', 1), c.get('p', 0))
    co = r.shape[1]
    if c.get('epi_scale') is not None:
        r = r * c['epi_scale'][:co].double()[None, :, None, None]
    if c.get('epi_shift') is not None:
        r = r + c['epi_shift'][:co].double()[None, :, None, None]
    r = r.permute(0, 2, 3, 1)
    if c.get('res1') is not None:
        r1 = c['res1'].double()[..., :co]
        if c.get('res1_up'):
            r1 = F.interpolate(r1.permute(0, 3, 1, 2), size=r.shape[1:3], mode='nearest').permute(0, 2, 3, 1)
        r = r + r1
    if c.get('res2') is not None:
        r = r + c['res2'].double()[..., :co]
    if c.get('mask') is not None:
        r = torch.where(c['mask'][..., :co] > 0, r, torch.zeros_like(r))
    if c.get('mask_bits') is not None:
        bits = c['mask_bits']
        on = torch.stack([(bits >> q) & 1 for q in range(4)], -1).reshape(r.shape[0], r.shape[1], r.shape[2], -1)[..., :co]
        r = torch.where(on > 0, r, torch.zeros_like(r))
    if c.get('relu'):
        r = F.relu(r)
    return r.contiguous()


def nibbles_of(y):
    b = (y > 0).view(tuple(y.shape[:-1]) + (y.shape[-1] // 4, 4)).to(torch.uint8)
    return b[..., 0] | (b[..., 1] << 1) | (b[..., 2] << 2) | (b[..., 3] << 3)


def check_native_conv(ops, c):
    """guarded == plain bit for bit; finite; 1e-4 relative-to-max against fp64 (the bar of tests/test_ops_gpu.py)"""
    out_p, out_g = guarded(ops, conv_build(ops, c))
    ref = conv_ref(c)
    co = ref.shape[-1]
    y = out_g['y'].cpu()
    assert finite(y), 'NaN / Inf in the guarded output: a load outside an input reached a result'
    assert torch.equal(out_g['y'], out_p['y'])
    if 'y_first' in out_g:
        assert torch.equal(out_g['y_first'], out_g['y'])
    assert relmax(y[..., :co], ref) < 1e-4, relmax(y[..., :co], ref)
    if y.shape[-1] != co:
        assert float(y[..., co:].abs().max()) == 0.0
    if 'mask_out' in out_g:
        assert torch.equal(out_g['mask_out'].cpu(), nibbles_of(y)) and torch.equal(out_g['mask_out'], out_p['mask_out'])
    if 'stats' in out_g:
        st = out_g['stats'].cpu().double()
        assert finite(st) and torch.equal(out_g['stats'], out_p['stats'])
        assert relmax(st.sum(0)[0, :co], ref.sum((0, 1, 2))) < 1e-4
        assert relmax(st.sum(0)[1, :co], (ref ** 2).sum((0, 1, 2))) < 1e-4
    return out_g


def check_emulated_conv(ops, c):
    """the bar of tests/test_bx3_gpu.py / test_bxs_gpu.py: rel-L2 against fp64 < 1e-6 and at most 1.5 x the native
    kernel's error on the same operands (+ 1e-8); guarded == plain bit for bit"""
    out_p, out_g = guarded(ops, conv_build(ops, c))
    native = dict(c, emu='off', expect=None)
    ref = conv_ref(c)
    y = out_g['y'].cpu()
    assert finite(y), 'NaN / Inf in the guarded output: a load outside an input reached a result'
    assert torch.equal(out_g['y'], out_p['y'])
    if 'y_first' in out_g:
        assert torch.equal(out_g['y_first'], out_g['y'])
    # the native kernel beside it, on ordinary buffers
    y0 = torch.empty_like(out_p['y'])
    kw = {q: native[q].to(DEV) for q in ('pro_scale', 'pro_shift', 'epi_scale', 'epi_shift', 'res1', 'res2', 'mask',
                                         'mask_bits') if native.get(q) is not None}
    if c.get('stats'):
        kw['stats'] = torch.empty_like(out_p['stats'])
    with ops.emulation('off'):
        l0 = ops.conv_forward(c['x'].to(DEV), ops.pack_weights(c['wt'].to(DEV).contiguous(), chan_pad=c['x'].shape[3]), y0,
                              c['k'], c.get('s', 1), c.get('p', 0), relu=c.get('relu', False),
                              pro_relu=c.get('pro_relu', False), res1_up=c.get('res1_up', False), **kw)
    assert not l0.variant.startswith('bx'), l0.variant
    l0.run()
    ops.sync_check()
    e0, e1 = rel_l2(y0, ref), rel_l2(y, ref)
    print('%s: rel-L2 vs fp64 %.3e (native %s %.3e)' % (c['expect'], e1, l0.variant, e0))
    assert e1 < 1e-6 and e1 <= 1.5 * e0 + 1e-8, (e1, e0)
    if 'mask_out' in out_g:
        assert torch.equal(out_g['mask_out'].cpu(), nibbles_of(y)) and torch.equal(out_g['mask_out'], out_p['mask_out'])
    if 'stats' in out_g:
        st = out_g['stats'].cpu().double()
        assert finite(st) and torch.equal(out_g['stats'], out_p['stats'])
        assert relmax(st.sum(0)[0], ref.sum((0, 1, 2))) < 1e-4 and relmax(st.sum(0)[1], (ref ** 2).sum((0, 1, 2))) < 1e-4
    return out_g


def conv_case(seed, n, cin, h, w, cout, k, s=1, p=0, **extra):
    g = gen(seed)
    c = dict(x=nhwc(torch.randn(n, cin, h, w, generator=g), 4 if cin <= 4 else (cin + 31) // 32 * 32),
             wt=torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k), k=k, s=s, p=p)
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    ldc = 4 if cout <= 4 else (cout + 31) // 32 * 32
    for name in extra.pop('with_', ()):
        if name in ('pro_scale', 'epi_scale'):
            c[name] = torch.rand(c['x'].shape[3] if name[0] == 'p' else ldc, generator=g) + 0.5
        elif name in ('pro_shift', 'epi_shift'):
            c[name] = torch.randn(c['x'].shape[3] if name[0] == 'p' else ldc, generator=g) * 0.5
        elif name in ('res1', 'res2', 'mask'):
            c[name] = torch.randn(n, oh, ow, ldc, generator=g)
        elif name == 'mask_bits':
            c[name] = torch.randint(0, 16, (n, oh, ow, ldc // 4), generator=g).to(torch.uint8)
        elif name == 'res1_up':
            c['res1'], c['res1_up'] = torch.randn(n, (oh + 1) // 2, (ow + 1) // 2, ldc, generator=g), True
    c.update(extra)
    return c


# ------------------------------------------------------------------------------------------- native fp32 GEMMs: tiled
NO_PERSISTENT = dict(HND_BRES='0', HND_BSTREAM='0')


def _tile_name(tile, cout, stats=False, mask_out=False):
    """what csrc/conv_igemm.hip pick_tile makes of a forced igemm_tile (128-column tiles need cout % 128 == 0,
    statistics 128-row tiles, mask nibbles 128-column tiles)"""
    if tile in (0, 2) and cout % 128 != 0:
        tile += 1
    if stats and tile in (2, 3):
        tile -= 2
    if mask_out and tile in (1, 3):
        tile -= 1
    from hnd_ghnd_object_detectors_amd._lib import CONV_TILES
    return {code: name for name, code in CONV_TILES.items()}[tile]             # enum hnd_conv_tile


@covers('hnd_conv2d_igemm')
@pytest.mark.parametrize('tile', [0, 1, 2, 3])
@pytest.mark.parametrize('shape', [
    (3, 64, 33, 41, 64, 1, 1, 0),        # M = 4059: 91 mod 128, 27 mod 64
    (2, 64, 10, 12, 3, 2, 1, 1),         # cout 3 stored as 4, the vector-ALU kernel switched off: 60 / 124 dead columns
    (2, 128, 17, 21, 128, 3, 2, 1),      # stride-2 3x3 at odd extents: the last strided row / column, M = 99
])
def test_tiled_kernel_on_every_block_tile(ops, monkeypatch, shape, tile):
    """every igemm_tile the picker lets a shape run on (cout % 128 != 0 maps the 128-column tiles 0 / 2 onto 1 / 3: those
    shapes run each 64-column tile twice).  The issue's fourth shape, the cin-4 build, has ONE tile: pick_conv sends cin == 4
    to igemm_c4_128x64 before pick_tile is asked (test_thin_output_and_four_channel_input_builds)."""
    n, cin, h, w, cout, k, s, p = shape
    set_env(monkeypatch, HND_DEBUG_PICKER='igemm_tile=%d' % tile, HND_THIN_N='0', **NO_PERSISTENT)
    check_native_conv(ops, conv_case(sum(shape) + tile, n, cin, h, w, cout, k, s, p,
                                     expect=_tile_name(tile, 4 if cout == 3 else cout)))


@covers('hnd_conv2d_igemm')
def test_thin_output_and_four_channel_input_builds(ops, monkeypatch):
    set_env(monkeypatch, **NO_PERSISTENT)
    # cout 3 stored as 4: the vector-ALU kernel (switched off, the tiled kernel takes it: the sweep above)
    check_native_conv(ops, conv_case(1, 2, 64, 10, 12, 3, 2, 1, 1, expect='thin_n4'))
    # cin 3 stored as 4: the cin-4 build, whatever tile is asked for
    set_env(monkeypatch, HND_DEBUG_PICKER='igemm_tile=3', **NO_PERSISTENT)
    check_native_conv(ops, conv_case(2, 2, 3, 12, 14, 64, 2, 1, 0, expect='igemm_c4_128x64'))


@covers('hnd_conv2d_igemm')
@pytest.mark.parametrize('tile,stats,mask_out', [(0, True, True), (1, True, False), (2, False, True), (3, False, False)])
def test_tiled_kernel_with_the_whole_epilogue(ops, monkeypatch, tile, stats, mask_out):
    """prologue, scale / shift, res1, res2, ReLU, mask_out nibbles of mask_nibbles_like size, stats of exactly
    stats_tiles(M) * 2 * cout floats; (2, 64, 15, 19) under a 2x2 conv: M = 2 * 14 * 18 = 504 = 120 mod 128.  Statistics
    are per 128-row tile and a lane must own whole nibbles, so only the 128 x 128 tile takes the WHOLE epilogue; every
    other tile runs it with the parts it can take (stats on 128-row tiles, mask_out on 128-column tiles)."""
    set_env(monkeypatch, HND_DEBUG_PICKER='igemm_tile=%d' % tile, **NO_PERSISTENT)
    c = conv_case(7 + tile, 2, 64, 15, 19, 128, 2, 1, 0, relu=True, pro_relu=True, stats=stats, mask_out=mask_out,
                  with_=('pro_scale', 'pro_shift', 'epi_scale', 'epi_shift', 'res1', 'res2'),
                  expect=_tile_name(tile, 128, stats=stats, mask_out=mask_out))
    assert c['expect'] == ('igemm_128x128', 'igemm_128x64', 'igemm_64x128', 'igemm_64x64')[tile]
    check_native_conv(ops, c)


@covers('hnd_conv2d_igemm')
@pytest.mark.parametrize('tile', [0, 1, 2, 3])
def test_tiled_kernel_reading_mask_bits_and_the_upsampled_residual(ops, monkeypatch, tile):
    set_env(monkeypatch, HND_DEBUG_PICKER='igemm_tile=%d' % tile, **NO_PERSISTENT)
    check_native_conv(ops, conv_case(11, 3, 64, 9, 13, 128, 1, with_=('mask_bits', 'res1'), expect=_tile_name(tile, 128)))
    # FPN lateral: 512 -> 256 at 10 x 14 on a 5 x 7 coarse map (res1_mode 1)
    check_native_conv(ops, conv_case(12, 2, 512, 10, 14, 256, 1, with_=('epi_shift', 'res1_up'),
                                     expect=_tile_name(tile, 256)))


# ------------------------------------------------------------------------------------------------------ data gradient
class ArenaWeights(object):
    """what ops.conv_dgrad takes for its weight cache: the transposed tap-subset operands, each re-homed into the arena"""

    def __init__(self, ops, alloc, weight):
        self.ops, self.alloc, self.weight, self.count = ops, alloc, weight, 0

    def get(self, transposed, chan_pad, taps, kscale=None):
        pk0 = self.ops.pack_weights(self.weight, transposed=transposed, chan_pad=chan_pad, taps=taps, kscale=kscale)
        self.count += 1
        return rehome(self.ops, self.alloc, pk0, 'wt%d' % self.count)


@covers('hnd_conv2d_igemm')
@pytest.mark.parametrize('tile', [0, 3])
def test_stride2_parity_data_gradient_keeps_its_rows_inside_dx(ops, monkeypatch, tile):
    """the four parity launches (y_sh = y_sw = 2) of (2, 128, 17, 21 -> 128, 3x3 s2 p1): with odd extents the last strided
    row and column are the edge.  dx starts as a known base; together the launches write every pixel, each exactly once
    (no accumulation), and nothing else."""
    set_env(monkeypatch, HND_DEBUG_PICKER='igemm_tile=%d' % tile, **NO_PERSISTENT)
    n, cin, h, w, cout, k, s, p = 2, 128, 17, 21, 128, 3, 2, 1
    g = gen(150 + tile)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    out = F.conv2d(x, wt.double(), None, s, p)
    dy = torch.randn(out.shape, generator=g)
    out.backward(dy.double())
    wdev = wt.to(DEV).contiguous()

    def build(alloc):
        dyd = alloc.load('dy', nhwc(dy))
        dx = alloc.take('dx', (n, h, w, cin))
        launches, _ = ops.conv_dgrad(dyd, ArenaWeights(ops, alloc, wdev), dx, k, s, p)
        assert len(launches) == 4 and all(l.variant == _tile_name(tile, cin) for l in launches), [l.variant for l in launches]
        seen = []
        for l in launches:
            before = dx.clone()
            l.run()
            ops.sync_check()
            ph, pw_ = l.desc.y_oh, l.desc.y_ow
            touched = torch.zeros(h, w, dtype=torch.bool, device=DEV)
            touched[ph::2, pw_::2] = True
            same = (dx.view(torch.int32) == before.view(torch.int32)).all(-1).all(0)
            assert bool(same[~touched].all()), 'parity (%d, %d) wrote a pixel of another parity' % (ph, pw_)
            seen.append((ph, pw_))
        assert sorted(seen) == [(0, 0), (0, 1), (1, 0), (1, 1)]
        if isinstance(alloc, G.Arena):
            RAN.update(l.variant for l in launches)
        return dx
    dx_p, dx_g = guarded(ops, build)
    assert finite(dx_g) and torch.equal(dx_p, dx_g)
    assert relmax(dx_g.cpu().permute(0, 3, 1, 2), x.grad) < 1e-4


@covers('hnd_conv2d_igemm')
def test_accumulating_stride2_1x1_data_gradient_leaves_unreached_pixels_alone(ops, monkeypatch):
    """(2, 256, 9, 12 -> 512) 1x1 stride 2 with a mask, adding into dx: pixels no launch reaches keep the base bit for bit"""
    set_env(monkeypatch, HND_DEBUG_PICKER='igemm_tile=2', **NO_PERSISTENT)
    n, cin, h, w, cout = 2, 256, 9, 12, 512
    g = gen(5)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(cout, cin, 1, 1, generator=g) / math.sqrt(cin)
    sc = torch.rand(cout, generator=g) + 0.5
    out = F.conv2d(x, wt.double(), None, 2, 0)
    dy = torch.randn(out.shape, generator=g)
    out.backward(dy.double() * sc.double()[None, :, None, None])
    base, mk = torch.randn(n, h, w, cin, generator=g), torch.randn(n, h, w, cin, generator=g)
    ref = torch.where(mk > 0, base.double() + x.grad.permute(0, 2, 3, 1), torch.zeros(n, h, w, cin, dtype=torch.float64))
    wdev = wt.to(DEV).contiguous()

    def build(alloc):
        dyd, dx, mkd, scd = alloc.load('dy', nhwc(dy)), alloc.load('dx', base), alloc.load('mask', mk), alloc.load('sc', sc)
        launches, _ = ops.conv_dgrad(dyd, ArenaWeights(ops, alloc, wdev), dx, 1, 2, 0, accumulate=True, pro_scale=scd,
                                     mask=mkd)
        assert len(launches) == 1 and launches[0].variant == 'igemm_64x128', [l.variant for l in launches]
        launches[0].run()
        ops.sync_check()
        if isinstance(alloc, G.Arena):
            RAN.add(launches[0].variant)
        return dx
    dx_p, dx_g = guarded(ops, build)
    got = dx_g.cpu()
    assert finite(got) and torch.equal(dx_p, dx_g)
    assert relmax(got[:, ::2, ::2], ref[:, ::2, ::2]) < 1e-4
    assert torch.equal(got[:, 1::2], base[:, 1::2]) and torch.equal(got[:, :, 1::2], base[:, :, 1::2])


# -------------------------------------------------------------------------------------------------------------- stem
@covers('hnd_conv2d_igemm', 'hnd_conv2d_wgrad')
def test_stem_conv_and_its_weight_gradient_from_the_lds_patch(ops, monkeypatch):
    """(1, 3 -> 64, 75 x 133) 7x7 s2 p3: 38 x 67 outputs, partial edge patches on both axes"""
    set_env(monkeypatch, HND_STEM7='1')
    c = conv_case(21, 1, 3, 75, 133, 64, 7, 2, 3, relu=True, with_=('epi_scale', 'epi_shift'), expect='stem7_lds')
    check_native_conv(ops, c)
    g = gen(31)
    x = torch.randn(1, 3, 75, 133, generator=g)
    wt = torch.randn(64, 3, 7, 7, generator=g, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(x.double(), wt, stride=2, padding=3)
    dy = torch.randn(out.shape, generator=g)
    out.backward(dy.double())
    dw_p, dw_g = guarded(ops, wgrad_build(ops, nhwc(x, 4), nhwc(dy), (64, 3, 7, 7), 7, 2, 3, expect='stem7_wgrad'))
    assert finite(dw_g) and torch.equal(dw_p, dw_g)
    assert relmax(dw_g, wt.grad) < 1e-4


# ---------------------------------------------------------------------------------------- B-resident persistent GEMMs
@covers('hnd_conv2d_igemm')
@pytest.mark.parametrize('case', [
    # expect, cin, cout, n, h, w, extra operands, env.  A B-resident kernel gives every 64- / 128-column slice to one workgroup
    # of a team (csrc/common.h team_count: 8 * 32 / slices teams on 256 CUs) and wants 2 chunks of 64 rows per wave row:
    # these are the smallest shapes that reach each build, all with a ragged last chunk.
    ('bres_128', 64, 1024, 1, 129, 131, (), dict(HND_BRES2='0')),              # M = 16 899 = 3 mod 128; 32 teams x 8 chunks
    ('bres_64', 512, 2048, 1, 91, 93, ('res1',), dict(HND_BRES2='0')),          # M = 8 463 = 15 mod 128; 8 teams x 16 chunks
    ('bres2_128', 128, 1024, 1, 91, 93, (), dict(HND_BRES2='1')),               # one wave per SIMD, 128-column slice
    ('bres2_64', 512, 2048, 1, 61, 69, (), dict(HND_BRES2='1')),                # M = 4 209 = 113 mod 128, 64-column slice
    ('bres_128', 128, 1024, 1, 129, 131, ('mask_bits', 'res1', 'pro_scale', 'pro_shift'), dict(HND_BRES2='1')),
])
def test_b_resident_kernels_at_a_ragged_last_chunk(ops, monkeypatch, case):
    expect, cin, cout, n, h, w, with_, env = case
    set_env(monkeypatch, HND_DEBUG_PICKER='bres_all', HND_BRES='512', HND_BSTREAM='0', **env)
    check_native_conv(ops, conv_case(len(expect) + cin, n, cin, h, w, cout, 1, relu='mask_bits' not in with_,
                                     with_=with_ + ('epi_scale', 'epi_shift'), expect=expect))


# ----------------------------------------------------------------------------------------- B-streamed persistent GEMMs
def relay_shape(wn, n, h, w, cout, kdim):
    """T tiles x nit iterations of 128 k against the persistent grid (csrc/stream_k_relay.h relay_grid / relay_split)"""
    bm, bn = 64 * (4 // wn), 64 * wn
    grid = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8
    return -(-(n * h * w) // bm) * (cout // bn), kdim // 128, grid


@covers('hnd_conv2d_igemm')
@pytest.mark.parametrize('case', [
    ('bstream_128', 2, 128, 17, 21, 128, 3, 2, 1),      # taps, K = 1152, 99 rows: one ragged tile
    ('bstream_64', 1, 128, 13, 17, 64, 3, 1, 1),        # the 256 x 64 tile with 221 rows
    ('bstream_128', 1, 1024, 7, 9, 128, 1, 1, 0),       # tap-free long K
])
def test_b_streamed_kernel_without_the_relay(ops, monkeypatch, case):
    expect, n, cin, h, w, cout, k, s, p = case
    set_env(monkeypatch, HND_DEBUG_PICKER='bstream_all', HND_BRES='0')
    check_native_conv(ops, conv_case(60 + cout, n, cin, h, w, cout, k, s, p, relu=True, with_=('epi_scale', 'epi_shift'),
                                     expect=expect))


RELAY_CASES = [
    # wn, n, cin, h, w, cout: a 1x1 conv with K = 256 (nit = 2) whose T = 258 tiles do not divide over 256 workgroups
    (2, 2, 256, 82, 100, 256),          # M = 16 400: 129 row tiles of 128 (a 16-row tail) x 2 column tiles
    (1, 1, 256, 150, 146, 192),         # M = 21 900: 86 row tiles of 256 (a 140-row tail) x 3 column tiles
]


def _relay_case(wn, n, cin, h, w, cout, family, emu):
    tiles, nit, grid = relay_shape(wn, n, h, w, cout, cin)
    # the relay exists only with a tile per workgroup, and splits tiles between neighbours only when T * nit is no
    # multiple of the grid
    assert tiles >= grid and (tiles * nit) % grid != 0, (tiles, nit, grid)
    return conv_case(70 + cout, n, cin, h, w, cout, 1, relu=True, with_=('epi_scale', 'epi_shift'), relay=True, emu=emu,
                     expect='%s_%d' % (family, 128 if wn == 2 else 64))


@covers('hnd_conv2d_igemm')
@pytest.mark.parametrize('case', RELAY_CASES)
def test_b_streamed_kernel_with_the_relay_stays_inside_its_workspace(ops, lib, monkeypatch, case):
    """the workspace is exactly hnd_conv2d_igemm_workspace bytes, zero-filled once; two launches (two epochs) on it"""
    set_env(monkeypatch, HND_DEBUG_PICKER='bstream_all', HND_BRES='0')
    lib.hnd_relay_timeouts(1)
    check_native_conv(ops, _relay_case(*case, family='bstream', emu='off'))
    assert lib.hnd_relay_timeouts(0) == 0


@covers('hnd_conv2d_igemm', 'hnd_pack_bf16x3s')
@pytest.mark.parametrize('case', RELAY_CASES)
def test_emulated_b_streamed_kernel_with_the_relay(ops, lib, monkeypatch, case):
    set_env(monkeypatch, HND_DEBUG_PICKER='bstream_all' + ('' if case[0] == 2 else ',bxs_wn1'), HND_BRES='0')
    lib.hnd_relay_timeouts(1)
    check_emulated_conv(ops, _relay_case(*case, family='bxs', emu='bxs'))
    assert lib.hnd_relay_timeouts(0) == 0


@covers('hnd_conv2d_igemm')
@pytest.mark.parametrize('order', ['native_first', 'emulated_first'])
def test_native_and_emulated_b_streamed_launches_share_one_relay_workspace(ops, lib, monkeypatch, order):
    """one zero-filled workspace of exactly the queried size serves a bstream and a bxs launch, in both orders: each
    launch's bits equal those it gives on a workspace of its own"""
    set_env(monkeypatch, HND_DEBUG_PICKER='bstream_all', HND_BRES='0')
    lib.hnd_relay_timeouts(1)
    wn, n, cin, h, w, cout = RELAY_CASES[0]
    c = _relay_case(wn, n, cin, h, w, cout, 'bstream', 'off')
    pk0 = ops.pack_weights(c['wt'].to(DEV).contiguous())

    def build(alloc):
        x = alloc.load('x', c['x'])
        es, eb = alloc.load('es', c['epi_scale']), alloc.load('eb', c['epi_shift'])
        pk = rehome(ops, alloc, pk0, 'w', 'bxs')
        ys, ls = {}, {}
        for emu in ('off', 'bxs'):
            ys[emu] = alloc.take('y_' + emu, (n, h, w, cout))
            with ops.emulation(emu):
                ls[emu] = ops.conv_forward(x, pk, ys[emu], 1, 1, 0, epi_scale=es, epi_shift=eb, relu=True)
        assert ls['off'].variant == 'bstream_128' and ls['bxs'].variant == 'bxs_128'
        ws = own_relay(ops, alloc, ls['off'])
        own_relay(ops, alloc, ls['bxs'], ws)                # the same bytes: both queries give one size
        for emu in (('off', 'bxs') if order == 'native_first' else ('bxs', 'off')) * 2:
            ls[emu].run()
            ops.sync_check()
        return ys
    ys_p, ys_g = guarded(ops, build)
    assert lib.hnd_relay_timeouts(0) == 0
    ref = conv_ref(c)
    for emu in ('off', 'bxs'):
        assert finite(ys_g[emu]) and torch.equal(ys_g[emu], ys_p[emu])
    assert relmax(ys_g['off'], ref) < 1e-4
    e0, e1 = rel_l2(ys_g['off'], ref), rel_l2(ys_g['bxs'], ref)
    assert e1 < 1e-6 and e1 <= 1.5 * e0 + 1e-8, (e1, e0)


# ------------------------------------------------------------------------------------------------------ emulated GEMMs
BX3_BUILDS = [('persistent', 'bx3_tiled=0'), ('tiled', 'bx3_tiled=1,bx3_tiled_mi=1'), ('tiled', 'bx3_tiled=1,bx3_tiled_mi=2')]


@covers('hnd_conv2d_igemm', 'hnd_pack_bf16x3')
@pytest.mark.parametrize('build', BX3_BUILDS, ids=['persistent', 'tiled_mi1', 'tiled_mi2'])
@pytest.mark.parametrize('cout', [64, 256])
@pytest.mark.parametrize('kdim', [128, 256, 512])
def test_bx3_kernel_in_every_build(ops, monkeypatch, kdim, cout, build):
    """1x1, M = 3 * 33 * 41 = 4059 (27 mod 64: a ragged last chunk); K = 512 runs two k passes; the image is made by
    hnd_pack_bf16x3 into exactly hnd_pack_bf16x3_elems uint16 (rows_pad 64 / 256, kdim 128 / 256 / 512)"""
    set_env(monkeypatch, HND_DEBUG_PICKER=build[1])
    check_emulated_conv(ops, conv_case(kdim + cout, 3, kdim, 33, 41, cout, 1, relu=True, emu='bx3',
                                       with_=('epi_scale', 'epi_shift'), expect='bx3_64/' + build[0]))


@covers('hnd_conv2d_igemm', 'hnd_pack_bf16x3')
@pytest.mark.parametrize('build', BX3_BUILDS, ids=['persistent', 'tiled_mi1', 'tiled_mi2'])
def test_bx3_kernel_with_mask_nibbles_and_the_upsampled_residual(ops, monkeypatch, build):
    set_env(monkeypatch, HND_DEBUG_PICKER=build[1])
    # reads mask_bits (with the same-geometry residual its build rides on); writes mask_out
    check_emulated_conv(ops, conv_case(81, 3, 128, 9, 13, 128, 1, emu='bx3', with_=('mask_bits', 'res1'),
                                       expect='bx3_64/' + build[0]))
    check_emulated_conv(ops, conv_case(82, 3, 256, 9, 13, 128, 1, relu=True, mask_out=True, emu='bx3', with_=('res1',),
                                       expect='bx3_64/' + build[0]))
    # FPN lateral with the exactly 2x coarser top-down map.  The kernel takes M >= 64 and ow % 4 == 0 (bx3_applies), so the
    # smallest map is 8 x 8 on 4 x 4 (M = 64, one chunk): the row clamp of the residual gather (mrows - 4) is the last group
    check_emulated_conv(ops, conv_case(83, 1, 256, 8, 8, 256, 1, emu='bx3', with_=('epi_shift', 'res1_up'),
                                       expect='bx3_64/' + build[0]))


@covers('hnd_conv2d_igemm', 'hnd_pack_bf16x3s')
@pytest.mark.parametrize('case', [
    ('bxs_128', '', 2, 128, 17, 21, 128, 3, 2, 1, False),          # 3x3 stride 2 pad 1 at odd extents
    ('bxs_64', 'bxs_wn1', 2, 128, 17, 21, 128, 3, 2, 1, False),    # ... on the 256 x 64 tile
    ('bxs_64', '', 2, 64, 13, 17, 64, 2, 1, 1, True),              # 2x2 pad 1 with statistics (14 x 18 outputs, 3.9 stat tiles)
    ('bxs_128', '', 2, 64, 13, 17, 128, 2, 1, 1, True),
    ('bxs_128', '', 1, 1024, 7, 9, 128, 1, 1, 0, False),           # tap-free long K
])
def test_bxs_kernel_over_taps_with_statistics_and_long_k(ops, monkeypatch, case):
    expect, picker, n, cin, h, w, cout, k, s, p, stats = case
    set_env(monkeypatch, HND_DEBUG_PICKER=picker)
    with_ = ('pro_scale', 'pro_shift') if stats else ('epi_scale', 'epi_shift')
    check_emulated_conv(ops, conv_case(90 + cout + k, n, cin, h, w, cout, k, s, p, relu=not stats, pro_relu=stats,
                                       stats=stats, emu='bxs', with_=with_, expect=expect))


@covers('hnd_pack_bf16x3', 'hnd_pack_bf16x3s')
@pytest.mark.parametrize('rows_pad,kdim,groups', [(64, 128, 1), (192, 512, 1), (64, 512, 16), (192, 128, 16)])
def test_weight_images_fill_exactly_their_elems(ops, lib, rows_pad, kdim, groups):
    """both images into views of exactly *_elems uint16: every element equals the image the library makes into a buffer of
    its own (the layout itself is held by tests/test_bx3_gpu.py), none keeps the 0xFFFF (a bf16 NaN) it started with, and
    nothing outside the view is touched"""
    g = gen(rows_pad + kdim + groups)
    wp = torch.randn(groups, rows_pad, kdim, generator=g)

    def build(alloc):
        buf = alloc.load('w', wp.view(-1))
        a = alloc.take('bx3', int(lib.hnd_pack_bf16x3_elems(rows_pad, kdim, groups)), torch.int16)
        b = alloc.take('bxs', int(lib.hnd_pack_bf16x3s_elems(rows_pad, kdim, groups)), torch.int16)
        ops.bx3_image(buf, rows_pad, kdim, groups, rows_pad * kdim, out=a)
        ops.bxs_image(buf, rows_pad, kdim, groups, rows_pad * kdim, out=b)
        ops.sync_check()
        return a, b
    a_g, b_g = only_guarded(ops, build)
    wd = wp.view(-1).to(DEV)
    assert torch.equal(a_g, ops.bx3_image(wd, rows_pad, kdim, groups, rows_pad * kdim))
    assert torch.equal(b_g, ops.bxs_image(wd, rows_pad, kdim, groups, rows_pad * kdim))
    assert a_g.numel() == b_g.numel() == 3 * groups * rows_pad * kdim
    for img in (a_g, b_g):
        vals = (img.cpu().to(torch.int32) << 16).view(torch.float32).double()       # bf16 -> fp32 is a 16-bit shift
        assert finite(vals)
        assert float(vals.sum()) == pytest.approx(float(wp.double().sum()), rel=1e-12, abs=1e-9)    # hi + mid + lo == x


# -------------------------------------------------------------------------------------------------- weight gradients
def wgrad_build(ops, x, dy, dw_shape, k, s, p, expect, splitk=0, pro=None):
    from hnd_ghnd_object_detectors_amd import _lib

    def build(alloc):
        xd, dyd = alloc.load('x', x), alloc.load('dy', dy)
        dw = alloc.take('dw', dw_shape)
        kw = {}
        if pro is not None:
            kw = dict(pro_scale=alloc.load('ps', pro[0]), pro_shift=alloc.load('pb', pro[1]), pro_relu=True)
        probe = ops.conv_wgrad(xd, dyd, dw, k, s, p, splitk=splitk, **kw)       # (its own slabs: only asked for the size)
        need = int(_lib.load().hnd_conv2d_wgrad_workspace(probe.ref))
        slabs = alloc.take('slabs', max(need, 4), torch.uint8) if need else None
        l = ops.conv_wgrad(xd, dyd, dw, k, s, p, splitk=splitk, slabs=slabs.view(torch.float32) if need else None, **kw)
        assert need == 0 or l.desc.slabs == slabs.data_ptr()
        assert l.variant == expect, (l.variant, expect)
        l.run()
        ops.sync_check()
        if isinstance(alloc, G.Arena):
            RAN.add(l.variant)
        return dw
    return build


def wgrad_case(ops, seed, n, cin, h, w, cout, k, s, p):
    g = gen(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    ps, pb = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    wt = (torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / math.sqrt(cin * k * k)).requires_grad_(True)
    a = F.relu(x.double() * ps.double()[None, :, None, None] + pb.double()[None, :, None, None])
    out = F.conv2d(a, wt, None, s, p)
    dy = torch.randn(out.shape, generator=g)
    out.backward(dy.double())
    cp = ops.chan_pad_of(cin)
    return nhwc(x, cp), nhwc(dy, ops.chan_pad_of(cout)), (F.pad(ps, (0, cp - cin)), F.pad(pb, (0, cp - cin))), wt.grad


@covers('hnd_conv2d_wgrad')
@pytest.mark.parametrize('splitk', [0, 1, 3])
@pytest.mark.parametrize('case', [('wgrad_m64', 2, 64, 13, 17, 64, 2, 1, 1), ('wgrad_m128', 2, 64, 14, 18, 256, 2, 1, 1),
                                  ('wgrad_m64', 3, 64, 31, 31, 32, 3, 2, 0)])
def test_split_k_weight_gradient_uses_exactly_its_slabs(ops, monkeypatch, case, splitk):
    """slabs: exactly hnd_conv2d_wgrad_workspace bytes; dw: exactly [cout, cin, k, k]"""
    expect, n, cin, h, w, cout, k, s, p = case
    set_env(monkeypatch, HND_WGRAD_RING='0')
    x, dy, pro, ref = wgrad_case(ops, 2000 + sum(case[1:]), n, cin, h, w, cout, k, s, p)
    dw_p, dw_g = guarded(ops, wgrad_build(ops, x, dy, (cout, cin, k, k), k, s, p, expect, splitk, pro))
    assert finite(dw_g) and torch.equal(dw_p, dw_g)
    assert relmax(dw_g, ref) < 1e-4


@covers('hnd_conv2d_wgrad')
def test_ring_and_thin_weight_gradients(ops, monkeypatch):
    set_env(monkeypatch, HND_WGRAD_RING='1', HND_DEBUG_PICKER='wgrad_ring_taps')
    x, dy, pro, ref = wgrad_case(ops, 500, 2, 64, 9, 9, 128, 2, 1, 1)               # fewer pixels than workgroups
    dw_p, dw_g = guarded(ops, wgrad_build(ops, x, dy, (128, 64, 2, 2), 2, 1, 1, 'wgrad_ring', 0, pro))
    assert finite(dw_g) and torch.equal(dw_p, dw_g) and relmax(dw_g, ref) < 1e-4
    x, dy, pro, ref = wgrad_case(ops, 501, 2, 64, 37, 53, 256, 2, 1, 1)             # 256 x 256 tile, odd extents
    dw_p, dw_g = guarded(ops, wgrad_build(ops, x, dy, (256, 64, 2, 2), 2, 1, 1, 'wgrad_ring', 0, pro))
    assert finite(dw_g) and torch.equal(dw_p, dw_g) and relmax(dw_g, ref) < 1e-4
    set_env(monkeypatch, HND_THIN_WGRAD='1')
    x, dy, pro, ref = wgrad_case(ops, 77, 2, 64, 57, 83, 3, 2, 1, 1)                # (64, 3, pad 1, 2, 57, 83)
    dw_p, dw_g = guarded(ops, wgrad_build(ops, x, dy, (3, 64, 2, 2), 2, 1, 1, 'thin_wgrad', 0, pro))
    assert finite(dw_g) and torch.equal(dw_p, dw_g) and relmax(dw_g, ref) < 1e-4


# ----------------------------------------------------------------------------------------------------------- Winograd
@covers('hnd_wino_weights', 'hnd_wino_input', 'hnd_wino_output', 'hnd_conv2d_igemm')
@pytest.mark.parametrize('tile', [2, 4, 6])
@pytest.mark.parametrize('dgrad', [False, True])
def test_winograd_3x3_conv_inside_exact_scratch(ops, lib, monkeypatch, tile, dgrad):
    """(2, 64, 13, 17 -> 64): v and m hold exactly WinoConv.scratch_elems elements, U exactly ncomp * rows_pad * depth;
    forward with mask_out (tile 4 / 6), and the data gradient (flipped, transposed weights).  Bar: the Winograd tests of
    tests/test_ops_gpu.py (tile 2: 1e-4, tile 4 / 6: 2e-4 relative-to-max against the direct convolution)."""
    set_env(monkeypatch, HND_DEBUG_PICKER='igemm_tile=1', **NO_PERSISTENT)
    n, cin, h, w, cout = 2, 64, 13, 17, 64
    g = gen(40 + tile)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    if dgrad:
        ref = F.conv_transpose2d(x.double(), wt.double(), None, 1, 1).permute(0, 2, 3, 1)      # cout == cin here
    else:
        ref = F.relu(F.conv2d(x.double(), wt.double(), None, 1, 1)).permute(0, 2, 3, 1)
    wdev = wt.to(DEV).contiguous()
    with ops.emulation('off'):
        ww0 = ops.WinoWeights(wdev, dgrad=dgrad, tile=tile)
    with_mask = not dgrad and tile in (4, 6)

    def build(alloc):
        xd = alloc.load('x', nhwc(x))
        wsrc = alloc.load('w_oihw', wt)
        u = alloc.take('u', ww0.buf.numel())
        ww = ops.PackedWeight(u, ww0.rows, ww0.kdim, ww0.chan_pad, groups=ww0.groups, group_stride=ww0.group_stride)
        ww.tile, ww.ncomp, ww.depth, ww.K, ww.dgrad = tile, ww0.ncomp, ww0.depth, 3, dgrad
        assert lib.hnd_wino_weights(wsrc.data_ptr(), u.data_ptr(), cout, cin, int(dgrad), tile, ops.stream_ptr()) == 0
        y = alloc.take('y', (n, h, w, cout))
        nv, nm = ops.WinoConv.scratch_elems(n, h, w, cin, cout, tile)
        v, m = alloc.take('v', nv), alloc.take('m', nm)
        bits = alloc.take('mask_out', (n, h, w, cout // 4), torch.uint8) if with_mask else None
        with ops.emulation('off'):
            conv = ops.WinoConv(xd, ww, y, v, m, relu=not dgrad, mask_out=bits)
        assert conv.gemm.variant == 'igemm_128x64' and conv.gemm.desc.w_group_rows > 0, conv.gemm.variant
        conv.run()
        ops.sync_check()
        if isinstance(alloc, G.Arena):
            RAN.add(conv.gemm.variant)
        return y, bits, u
    (y_p, b_p, u_p), (y_g, b_g, u_g) = guarded(ops, build)
    assert finite(y_g) and finite(u_g) and torch.equal(y_p, y_g) and torch.equal(u_g, ww0.buf)
    assert relmax(y_g, ref) < (1e-4 if tile == 2 else 2e-4), relmax(y_g, ref)
    if with_mask:
        assert torch.equal(b_g.cpu(), nibbles_of(y_g.cpu())) and torch.equal(b_p, b_g)


# --------------------------------------------------------------------------------------------------- everything else
@covers('hnd_pack_weights', 'hnd_pack_weights_batched', 'hnd_scale_packed_k', 'hnd_fbn_fold')
def test_weight_repacks_and_folds_fill_exactly_their_operands(ops, lib):
    """dst holds exactly round_up(rows, 64) * kdim floats (kdim = taps * chan_pad rounded up to 32), zero padding included;
    single and batched launches give the same bytes; layout as tests/test_ops_gpu.py::test_pack_weights_layouts"""
    from hnd_ghnd_object_detectors_amd._lib import PackDesc
    g = gen(9)
    cout, cin, k = 70, 3, 2                                   # rows 70 -> 128, K = 4 taps x 4 channels = 16 -> 32
    wt = torch.randn(cout, cin, k, k, generator=g)
    scale = torch.rand(cin, generator=g) + 0.5
    bn = [torch.randn(5, generator=g) for _ in range(3)] + [torch.rand(5, generator=g) + 0.5]

    def build(alloc):
        src = alloc.load('src', wt)
        a, b, t = alloc.take('fwd', 128 * 32), alloc.take('fwd_batched', 128 * 32), alloc.take('transposed', 64 * 384)
        args = (cout, cin, k, k, 0, 4, 0, 1, k, 0, 1, k)
        assert lib.hnd_pack_weights(src.data_ptr(), a.data_ptr(), *args, ops.stream_ptr()) == 0
        arr = (PackDesc * 2)()
        arr[0].src, arr[0].dst = src.data_ptr(), b.data_ptr()
        (arr[0].cout, arr[0].cin, arr[0].kh, arr[0].kw, arr[0].transposed, arr[0].chan_pad, arr[0].i0, arr[0].istep,
         arr[0].ni, arr[0].j0, arr[0].jstep, arr[0].nj) = args
        arr[1].src, arr[1].dst = src.data_ptr(), t.data_ptr()          # transposed: rows = cin 3 -> 64, K = 4 x 96 = 384
        (arr[1].cout, arr[1].cin, arr[1].kh, arr[1].kw, arr[1].transposed, arr[1].chan_pad, arr[1].i0, arr[1].istep,
         arr[1].ni, arr[1].j0, arr[1].jstep, arr[1].nj) = (cout, cin, k, k, 1, 96, 0, 1, k, 0, 1, k)
        assert lib.hnd_pack_weights_batched(arr, 2, ops.stream_ptr()) == 0
        s = alloc.load('scale', scale)
        scaled = alloc.load('scaled', torch.ones(128 * 32))
        assert lib.hnd_scale_packed_k(scaled.data_ptr(), 128, 32, 4, 4, s.data_ptr(), 3, ops.stream_ptr()) == 0
        wgt, bias, mean, var = [alloc.load('bn%d' % i, q) for i, q in enumerate(bn)]
        fs, fb = alloc.take('fold_scale', 8), alloc.take('fold_shift', 8)
        ops.fbn_fold(wgt, bias, mean, var, eps=1e-5, cs=8, out=(fs, fb))
        ops.sync_check()
        return a, b, t, scaled, fs, fb
    a, b, t, scaled, fs, fb = [q.cpu() for q in only_guarded(ops, build)]
    want = torch.zeros(128, 4, 4)
    want[:cout, :, :cin] = wt.permute(0, 2, 3, 1).reshape(cout, 4, cin)
    # packed row r holds channel (r & ~63) | ((r & 15) << 2) | ((r >> 4) & 3) (hnd::chan_of_row, see test_pack_weights_layouts)
    chan = torch.tensor([(r & ~63) | ((r & 15) << 2) | ((r >> 4) & 3) for r in range(128)])
    want = F.pad(want.view(128, 16), (0, 16))[chan]
    assert torch.equal(a, want.reshape(-1)) and torch.equal(b, a)
    want_t = torch.zeros(64, 4, 96)
    want_t[:cin, :, :cout] = wt.permute(1, 2, 3, 0).reshape(cin, 4, cout)
    assert torch.equal(t, want_t.view(64, 384)[chan[:64]].reshape(-1))
    ws = torch.ones(128, 32)
    ws.view(128, 8, 4)[:, :4, :3] *= scale
    assert torch.equal(scaled, ws.view(-1))
    sc = bn[0].double() / torch.sqrt(bn[3].double() + 1e-5)
    assert torch.allclose(fs[:5].double(), sc, rtol=1e-6, atol=0) and float(fs[5:].abs().max()) == 0.0
    assert torch.allclose(fb[:5].double(), bn[1].double() - bn[2].double() * sc, rtol=1e-5, atol=1e-6)
    assert float(fb[5:].abs().max()) == 0.0


@covers('hnd_maxpool3x3s2_fwd', 'hnd_maxpool3x3s2_bwd_relu_scale')
@pytest.mark.parametrize('n,c,h,w', [(1, 8, 1, 2), (3, 64, 7, 9)])
def test_max_pool_forward_and_backward(ops, n, c, h, w):
    g = gen(n + c)
    act = torch.randn(n, c, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    out = F.max_pool2d(act, 3, 2, 1)
    dy = torch.randn(out.shape, generator=g)
    out.backward(dy.double())
    sc = torch.rand(c, generator=g) + 0.5
    ref_dx = act.grad * (act.detach() > 0) * sc.double()[None, :, None, None]
    oh, ow = out.shape[2], out.shape[3]

    def build(alloc):
        x = alloc.load('x', nhwc(act.detach().float()))
        y, idx = alloc.take('y', (n, oh, ow, c)), alloc.take('idx', (n, oh, ow, c), torch.uint8)
        ops.maxpool_fwd(x, y, idx)
        dyd, scd, dx = alloc.load('dy', nhwc(dy)), alloc.load('sc', sc), alloc.take('dx', (n, h, w, c))
        ops.maxpool_bwd_relu_scale(dyd, idx, x, scd, dx)
        ops.sync_check()
        return y, idx, dx
    y, idx, dx = [q.cpu() for q in only_guarded(ops, build)]
    assert torch.equal(y, nhwc(out.detach().float())) and int(idx.max()) <= 8
    assert finite(dx) and relmax(dx, nhwc(ref_dx)) < 1e-6            # (tests/test_ops_gpu.py test_maxpool_fwd_bwd)


@covers('hnd_affine_relu', 'hnd_relu_mask_nibbles')
def test_affine_relu_and_the_one_byte_nibble_mask(ops):
    g = gen(4)
    x = torch.randn(3, 5, 7, 36, generator=g)
    sc, sh = torch.rand(36, generator=g) + 0.5, torch.randn(36, generator=g)
    one = torch.tensor([0.5, -1.0, 0.0, 2.0])                 # one pixel of four channels: a ONE-byte mask

    def build(alloc):
        xd, scd, shd = alloc.load('x', x), alloc.load('sc', sc), alloc.load('sh', sh)
        y, bits = alloc.take('y', x.shape), alloc.take('bits', (3, 5, 7, 9), torch.uint8)
        ops.affine_relu(xd, scd, shd, y, True, mask_out=bits)
        px, b1 = alloc.load('pixel', one), alloc.take('one_byte', 1, torch.uint8)
        ops.relu_mask_nibbles(px, b1)
        whole = alloc.take('bits_of_x', (3, 5, 7, 9), torch.uint8)
        ops.relu_mask_nibbles(xd, whole)
        ops.sync_check()
        return y, bits, b1, whole
    y, bits, b1, whole = [q.cpu() for q in only_guarded(ops, build)]
    assert torch.allclose(y, torch.relu(x * sc + sh), rtol=1e-6, atol=1e-6)      # (tests/test_ops_gpu.py: one fma)
    assert torch.equal(bits, nibbles_of(y)) and torch.equal(whole, nibbles_of(x))
    assert b1.tolist() == [0b1001]


@covers('hnd_adam_step_flat', 'hnd_sgd_step_flat', 'hnd_scale_by_device_scalar', 'hnd_fill', 'hnd_add_inplace',
        'hnd_roundtrip_f16')
@pytest.mark.parametrize('numel', [1, 63, 10007])
def test_flat_optimizer_steps_and_flat_elementwise_ops(ops, numel):
    """reference and bar: tests/test_ops_gpu.py test_adam_matches_torch / test_sgd_matches_torch (torch's fp32 optimizer,
    largest absolute difference < 1e-6)"""
    g = gen(numel)
    p0, gr = torch.randn(numel, generator=g), torch.randn(numel, generator=g)
    n4 = (numel + 3) // 4 * 4                                 # hnd_add_inplace takes whole float4s

    def build(alloc):
        p, gd = alloc.load('p', p0), alloc.load('g', gr)
        m, v = alloc.load('m', torch.zeros(numel)), alloc.load('v', torch.zeros(numel))
        for step in (1, 2):
            ops.adam_step_flat(p, gd, m, v, 1e-3, 0.9, 0.999, 1e-8, step, grad_scale=0.5)
        q, buf = alloc.load('q', p0), alloc.take('buf', numel)
        for step in (1, 2):
            ops.sgd_step_flat(q, gd, buf, 1e-2, 0.9, 0.0, 1e-4, False, step == 1)
        s, two = alloc.load('s', p0), alloc.load('two', torch.tensor([2.0]))
        ops.scale_by_device_scalar(s, two)
        f = alloc.take('f', numel)
        ops.fill(f, 3.25)
        a, b = alloc.load('a', F.pad(p0, (0, n4 - numel))), alloc.load('b', F.pad(gr, (0, n4 - numel)))
        ops.add_inplace(a, b)
        h = alloc.load('h', p0)
        ops.roundtrip_f16(h)
        ops.sync_check()
        return p, m, v, q, buf, s, f, a, h
    p, m, v, q, buf, s, f, a, h = [t.cpu() for t in only_guarded(ops, build)]
    rp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([rp], lr=1e-3)
    rq = torch.nn.Parameter(p0.clone())
    sgd = torch.optim.SGD([rq], lr=1e-2, momentum=0.9, weight_decay=1e-4)
    for _ in range(2):
        rp.grad = gr * 0.5
        opt.step()
        rq.grad = gr.clone()
        sgd.step()
    assert float((p - rp.detach()).abs().max()) < 1e-6 and finite(m) and finite(v)
    assert float((q - rq.detach()).abs().max()) < 1e-6 and finite(buf)
    assert torch.equal(s, p0 * 2) and torch.equal(f, torch.full((numel,), 3.25))
    assert torch.equal(a[:numel], p0 + gr) and torch.equal(h, p0.half().float())


@covers('hnd_subsample2', 'hnd_upsample_nearest_bwd')
def test_subsample_and_nearest_upsample_backward_at_odd_extents(ops):
    g = gen(6)
    n, h, w, c = 2, 7, 9, 36
    x = torch.randn(n, h, w, c, generator=g)
    fine = torch.randn(n, 13, 17, c, generator=g)
    coarse = torch.zeros(n, c, 7, 9, dtype=torch.float64, requires_grad=True)
    F.interpolate(coarse, size=(13, 17), mode='nearest').backward(fine.double().permute(0, 3, 1, 2))
    base = torch.randn(n, 7, 9, c, generator=g)

    def build(alloc):
        xd, y = alloc.load('x', x), alloc.take('y', (n, 4, 5, c))
        ops.subsample2(xd, y)
        gf, gc, ga = alloc.load('g_fine', fine), alloc.take('g_coarse', (n, 7, 9, c)), alloc.load('g_acc', base)
        ops.upsample_nearest_bwd(gf, gc, False)
        ops.upsample_nearest_bwd(gf, ga, True)
        ops.sync_check()
        return y, gc, ga
    y, gc, ga = [t.cpu() for t in only_guarded(ops, build)]
    want = coarse.grad.permute(0, 2, 3, 1)
    assert torch.equal(y, x[:, ::2, ::2])
    assert finite(gc) and torch.allclose(gc.double(), want, rtol=1e-6, atol=1e-6)
    assert torch.allclose(ga.double(), base.double() + want, rtol=1e-6, atol=1e-6)


@covers('hnd_nms', 'hnd_argsort_desc_f32')
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
def test_nms_inside_exactly_its_workspace(ops, lib, n):
    """workspace: exactly hnd_nms_workspace(n) bytes; order from hnd_argsort_desc_f32 into exactly n int64 with exactly
    hnd_argsort_desc_workspace(n) bytes.  Kept set: exact, against a plain greedy NMS in the operator's own fp32 terms."""
    g = gen(n)
    xy = torch.rand(n, 2, generator=g) * 100
    boxes = torch.cat([xy, xy + torch.rand(n, 2, generator=g) * 40 + 1], 1)
    scores = torch.rand(n, generator=g)

    def build(alloc):
        b, s = alloc.load('boxes', boxes), alloc.load('scores', scores)
        order = alloc.take('order', n, torch.int64)
        sw = alloc.take('sort_ws', int(lib.hnd_argsort_desc_workspace(n)), torch.uint8)
        assert lib.hnd_argsort_desc_f32(s.data_ptr(), n, order.data_ptr(), sw.data_ptr(), ops.stream_ptr()) == 0
        ws = alloc.take('nms_ws', int(lib.hnd_nms_workspace(n)), torch.uint8)
        keep = alloc.take('keep', n, torch.uint8)
        assert lib.hnd_nms(b.data_ptr(), order.data_ptr(), n, 0.5, ws.data_ptr(), keep.data_ptr(), ops.stream_ptr()) == 0
        ops.sync_check()
        return order, keep
    order, keep = [t.cpu() for t in only_guarded(ops, build)]
    want_order = torch.sort(scores, descending=True, stable=True)[1]
    assert torch.equal(order, want_order)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    alive, want = torch.ones(n, dtype=torch.bool), torch.zeros(n, dtype=torch.uint8)
    for i in want_order.tolist():
        if not alive[i]:
            continue
        want[i] = 1
        lt, rb = torch.maximum(boxes[i, :2], boxes[:, :2]), torch.minimum(boxes[i, 2:], boxes[:, 2:])
        wh = (rb - lt).clamp(min=0)
        inter = wh[:, 0] * wh[:, 1]
        alive &= ~(inter / (area[i] + area - inter) > 0.5)
    assert torch.equal(keep, want)


@covers('hnd_argsort_desc_f32')
@pytest.mark.parametrize('n', [5, 4096, 4097, 10000])
def test_argsort_inside_exactly_its_workspace(ops, lib, n):
    g = gen(n)
    keys = torch.randn(n, generator=g).round(decimals=2)          # ties: ascending index order

    def build(alloc):
        k, order = alloc.load('keys', keys), alloc.take('order', n, torch.int64)
        ws = alloc.take('ws', int(lib.hnd_argsort_desc_workspace(n)), torch.uint8)
        assert lib.hnd_argsort_desc_f32(k.data_ptr(), n, order.data_ptr(), ws.data_ptr(), ops.stream_ptr()) == 0
        ops.sync_check()
        return order
    assert torch.equal(only_guarded(ops, build).cpu(), torch.sort(keys, descending=True, stable=True)[1])


@covers('hnd_nonzero_u8', 'hnd_nonzero_gt_f32', 'hnd_nonzero_eq_i64', 'hnd_nonzero_min_size')
@pytest.mark.parametrize('n', [1, 257, 5000])
def test_nonzero_family_writes_count_entries_of_an_n_entry_buffer(ops, lib, n):
    """out has room for n entries (the header's size); entries past *count keep the pattern"""
    g = gen(n)
    flags = (torch.rand(n, generator=g) > 0.4).to(torch.uint8)
    xs = torch.randn(n, generator=g)
    lv = torch.randint(0, 4, (n,), generator=g)
    xy = torch.rand(n, 2, generator=g) * 50
    boxes = torch.cat([xy, xy + torch.rand(n, 2, generator=g) * 4], 1)
    want = [torch.nonzero(flags).flatten(), torch.nonzero(xs > 0.25).flatten(), torch.nonzero(lv == 2).flatten(),
            torch.nonzero(((boxes[:, 2] - boxes[:, 0]) >= 2.0) & ((boxes[:, 3] - boxes[:, 1]) >= 2.0)).flatten()]

    def build(alloc):
        f, x, l, b = alloc.load('flags', flags), alloc.load('x', xs), alloc.load('levels', lv), alloc.load('boxes', boxes)
        outs = [alloc.take('out%d' % i, n, torch.int64) for i in range(4)]
        cnts = [alloc.take('count%d' % i, 1, torch.int64) for i in range(4)]
        s = ops.stream_ptr()
        assert lib.hnd_nonzero_u8(f.data_ptr(), n, outs[0].data_ptr(), cnts[0].data_ptr(), s) == 0
        assert lib.hnd_nonzero_gt_f32(x.data_ptr(), n, 0.25, outs[1].data_ptr(), cnts[1].data_ptr(), s) == 0
        assert lib.hnd_nonzero_eq_i64(l.data_ptr(), n, 2, outs[2].data_ptr(), cnts[2].data_ptr(), s) == 0
        assert lib.hnd_nonzero_min_size(b.data_ptr(), n, 2.0, outs[3].data_ptr(), cnts[3].data_ptr(), s) == 0
        ops.sync_check()
        return outs, cnts
    outs, cnts = only_guarded(ops, build)
    for o, c, wnt in zip(outs, cnts, want):
        k = int(c.cpu())
        assert k == wnt.numel() and torch.equal(o.cpu()[:k], wnt)
        assert bool((o.cpu()[k:] == -1).all())


@covers('hnd_mask_run_boundaries')
def test_mask_run_boundaries_drops_what_does_not_fit(ops, lib):
    """capacity smaller than the number of boundaries: nothing is written past `capacity`, *count is still the true number"""
    g = gen(17)
    n, h, w = 3, 11, 13
    probs = torch.rand(n, h, w, generator=g)
    bit = (probs > 0.5).permute(0, 2, 1).reshape(n, -1)                 # column-major positions p = x * h + y
    keys = torch.nonzero(bit[:, 1:] != bit[:, :-1])
    keys = (keys[:, 0] * h * w + keys[:, 1] + 1).sort()[0]
    total = keys.numel()
    assert total > 40

    def build(alloc):
        p = alloc.load('probs', probs)
        res = []
        for tag, cap in (('all', total), ('short', 40)):
            out, cnt = alloc.take('out_' + tag, cap, torch.int64), alloc.take('count_' + tag, 1, torch.int64, fill=0)
            first = alloc.take('first_' + tag, n, torch.uint8)
            assert lib.hnd_mask_run_boundaries(p.data_ptr(), n, h, w, 0.5, out.data_ptr(), cap, cnt.data_ptr(),
                                               first.data_ptr(), ops.stream_ptr()) == 0
            res.append((out, cnt, first))
        ops.sync_check()
        return res
    (out, cnt, first), (out_s, cnt_s, first_s) = only_guarded(ops, build)
    assert int(cnt.cpu()) == total and torch.equal(out.cpu().sort()[0], keys)
    assert int(cnt_s.cpu()) == total and set(out_s.cpu().tolist()) <= set(keys.tolist()) and out_s.cpu().unique().numel() == 40
    assert torch.equal(first.cpu(), bit[:, 0].to(torch.uint8)) and torch.equal(first_s, first)


# ------------------------------------------------------------------------------------------- Winograd F(t x t, 2x2)
def wino_weights_in(ops, lib, alloc, name, wt, dgrad, tile, k, emu='off'):
    """hnd_wino_weights / hnd_wino2_weights into a view of exactly ncomp * rows_pad * depth floats (+ the bf16x3 image of the
    grouped operand in exactly hnd_pack_bf16x3_elems(rows_pad, depth, ncomp) uint16)"""
    cout, cin = wt.shape[0], wt.shape[1]
    rows, depth = (cin, cout) if dgrad else (cout, cin)
    ncomp, rows_pad = (tile + k - 1) ** 2, (rows + 63) // 64 * 64
    src = alloc.load(name + '_oihw', wt)
    u = alloc.take(name, ncomp * rows_pad * depth)
    fn = lib.hnd_wino_weights if k == 3 else lib.hnd_wino2_weights
    assert fn(src.data_ptr(), u.data_ptr(), cout, cin, int(dgrad), tile, ops.stream_ptr()) == 0
    ww = ops.PackedWeight(u, rows, depth, depth, groups=ncomp, group_stride=rows_pad * depth)
    ww.tile, ww.ncomp, ww.depth, ww.K, ww.dgrad = tile, ncomp, depth, k, dgrad
    if emu == 'bx3':
        img = alloc.take(name + '_bx3', int(lib.hnd_pack_bf16x3_elems(rows_pad, depth, ncomp)), torch.int16)
        ww.bx3 = ops.bx3_image(u, rows_pad, depth, ncomp, rows_pad * depth, out=img)
    return ww


@covers('hnd_conv2d_igemm', 'hnd_pack_bf16x3', 'hnd_wino_weights', 'hnd_wino_input', 'hnd_wino_output')
@pytest.mark.parametrize('build', BX3_BUILDS, ids=['persistent', 'tiled_mi1', 'tiled_mi2'])
def test_winograd_component_gemms_on_the_emulation_kernel(ops, lib, monkeypatch, build):
    """one grouped launch (w_group_rows = tiles_pad > 0) on bx3_64: F(4x4,3x3) of (2, 128, 13, 17 -> 128), the 36 component
    images in one exact hnd_pack_bf16x3_elems view.  Bar: tests/test_bx3_gpu.py
    test_bx3_winograd_component_gemms_match_the_native_path (rel-L2 vs the direct fp64 conv < 2e-5 and <= 1.5 x native)"""
    set_env(monkeypatch, HND_DEBUG_PICKER=build[1])
    n, c, h, w, tile = 2, 128, 13, 17, 4
    g = gen(77)
    x = torch.randn(n, c, h, w, generator=g).relu()
    wt = torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5
    ref = F.conv2d(x.double(), wt.double(), None, 1, 1).permute(0, 2, 3, 1)

    def build_(alloc, emu='bx3'):
        xd = alloc.load('x', nhwc(x))
        ww = wino_weights_in(ops, lib, alloc, 'u', wt, False, tile, 3, emu)
        y = alloc.take('y', (n, h, w, c))
        nv, nm = ops.WinoConv.scratch_elems(n, h, w, c, c, tile)
        v, m = alloc.take('v', nv), alloc.take('m', nm)
        with ops.emulation(emu):
            conv = ops.WinoConv(xd, ww, y, v, m)
        if emu == 'bx3':
            assert variant_of(conv.gemm) == 'bx3_64/' + build[0] and conv.gemm.desc.w_group_rows > 0, variant_of(conv.gemm)
        else:
            assert not conv.gemm.variant.startswith('bx')
        conv.run()
        ops.sync_check()
        if isinstance(alloc, G.Arena):
            RAN.add(variant_of(conv.gemm))
        return y
    y_p, y_g = guarded(ops, build_)
    y0 = build_(Plain(), 'off')
    assert finite(y_g) and torch.equal(y_p, y_g)
    e0, e1 = rel_l2(y0, ref), rel_l2(y_g, ref)
    assert e1 < 2e-5 and e1 <= 1.5 * e0, (e1, e0)


@covers('hnd_wino2_weights', 'hnd_wino2_input', 'hnd_wino2_output', 'hnd_wino2_dy', 'hnd_wino2_wgrad_output_t',
        'hnd_wino2_wgrad_output', 'hnd_conv2d_igemm', 'hnd_conv2d_wgrad', 'hnd_wino26_bnbwd_transforms',
        'hnd_wino26_output_bnbwd_stats', 'hnd_bn_bwd_apply')
@pytest.mark.parametrize('pad', [0, 1])
@pytest.mark.parametrize('tile', [4, 6])
def test_winograd_2x2_conv_input_transform_and_weight_gradient_inside_exact_scratch(ops, lib, monkeypatch, tile, pad):
    """(2, 64, 13, 17 -> 64): Wino2Conv forward (BN + ReLU on load, statistics of exactly stats_blocks * 2 * cout floats),
    Wino2InputTransform, Wino2Wgrad (z, s and slabs of exactly the stated / queried size), the data gradient -- at tile 6
    also with the BatchNorm-backward sums (partials of exactly stats_blocks) -- and wino26_bnbwd_step writing the v / z of
    those two launches.  Bars: 2e-4 relative-to-max (tests/test_ops_gpu.py Winograd 2x2 tests), 2e-6 for the fused sums and
    transforms against the unfused kernels (test_bn_backward_* there).  hnd_wino2_wgrad_output is hnd_wino2_wgrad_output_t
    with s_transposed = 0, the call Wino2Wgrad makes."""
    set_env(monkeypatch, HND_DEBUG_PICKER='igemm_tile=1', HND_WGRAD_RING='0', **NO_PERSISTENT)
    n, cin, h, w, cout = 2, 64, 13, 17, 64
    g = gen(60 + tile + pad)
    x = torch.randn(n, cin, h, w, generator=g)
    ps, pb = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    wt = (torch.randn(cout, cin, 2, 2, generator=g, dtype=torch.float64) / math.sqrt(cin * 4)).requires_grad_(True)
    a = F.relu(x.double() * ps.double()[None, :, None, None] + pb.double()[None, :, None, None]).requires_grad_(True)
    out = F.conv2d(a, wt, None, 1, pad)
    dy = torch.randn(out.shape, generator=g)
    out.backward(dy.double())
    oh, ow = out.shape[2], out.shape[3]
    wf = wt.detach().float()
    bn = [torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.5, torch.randn(cin, generator=g) * 0.2,
          torch.rand(cin, generator=g) + 0.5]                       # scale, shift, mean, rstd of the BN before the conv
    k123 = torch.randn(3, cout, generator=g) * 0.5
    gq, xq = torch.randn(n, oh, ow, cout, generator=g), torch.randn(n, oh, ow, cout, generator=g)

    def build(alloc):
        r = {}
        xd, psd, pbd = alloc.load('x', nhwc(x)), alloc.load('ps', ps), alloc.load('pb', pb)
        ww = wino_weights_in(ops, lib, alloc, 'u', wf, False, tile, 2)
        y = alloc.take('y', (n, oh, ow, cout))
        nv, nm = ops.Wino2Conv.scratch_elems(n, oh, ow, cin, cout, tile)
        v, m = alloc.take('v', nv), alloc.take('m', nm)
        st = alloc.take('stats', (ops.Wino2Conv.stats_blocks(n, oh, ow, cout, tile), 2, cout))
        with ops.emulation('off'):
            fwd = ops.Wino2Conv(xd, ww, y, v, m, pad, pro_scale=psd, pro_shift=pbd, pro_relu=True, stats=st)
        assert fwd.variant == 'igemm_128x64', fwd.variant
        fwd.run()
        v2 = alloc.take('v_alone', ops.Wino2InputTransform.scratch_elems(n, oh, ow, cin, tile))
        it = ops.Wino2InputTransform(xd, v2, pad, cout, tile, pro_scale=psd, pro_shift=pbd, pro_relu=True)
        it._run_input()
        # weight gradient
        dyd, dw = alloc.load('dy', nhwc(dy)), alloc.take('dw', (cout, cin, 2, 2))
        nc = (tile + 1) ** 2
        z, s = alloc.take('z', nc * fwd.tiles_pad * cout), alloc.take('s', nc * cout * cin)
        probe = ops.Wino2Wgrad(fwd, dyd, dw, z, s)
        need = int(lib.hnd_conv2d_wgrad_workspace(probe.gemm.ref))
        slabs = alloc.take('slabs', need, torch.uint8).view(torch.float32) if need else None
        wg = ops.Wino2Wgrad(fwd, dyd, dw, z, s, slabs=slabs)
        assert wg.variant == 'wgrad_m64' and not wg.swapped and (not need or wg.gemm.desc.slabs == slabs.data_ptr())
        wg.run()
        # data gradient (the same correlation with flipped, transposed weights and padding 1 - pad)
        wd = wino_weights_in(ops, lib, alloc, 'u_dgrad', wf, True, tile, 2)
        dx = alloc.take('dx', (n, h, w, cin))
        nv2, nm2 = ops.Wino2Conv.scratch_elems(n, h, w, cout, cin, tile)
        vd, md = alloc.take('v_dgrad', nv2), alloc.take('m_dgrad', nm2)
        with ops.emulation('off'):
            dg = ops.Wino2Conv(dyd, wd, dx, vd, md, 1 - pad)
        assert dg.variant == 'igemm_128x64', dg.variant
        dg.run()
        ops.sync_check()
        r.update(y=y, st=st, v=v.clone(), v2=v2, dw=dw, dx=dx)
        if tile == 6:
            # ... again with the BatchNorm-backward sums of the gradient it writes
            xr = alloc.load('bn_x', nhwc(x))
            bsc, bsh, bmu, brs = [alloc.load('bn%d' % i, q) for i, q in enumerate(bn)]
            part = alloc.take('bn_partials', (ops.Wino2Conv.stats_blocks(n, h, w, cin, 6), 2, cin))
            dx2 = alloc.take('dx_with_sums', (n, h, w, cin))
            with ops.emulation('off'):
                ops.Wino2Conv(dyd, wd, dx2, vd, md, 1 - pad, bwd_stats=(xr, bsc, bsh, bmu, brs, True, part)).run()
            ref_part = torch.empty(ops.bn_bwd_ntiles(n * h * w), 2, cin, device=DEV)
            ops.bn_bwd_reduce(dx2, xr, bsc, bsh, bmu, brs, True, ref_part)
            ops.sync_check()
            r.update(dx2=dx2, part=part, ref_part=ref_part)
            # wino26_bnbwd_step: v of the data gradient and z of the weight gradient from (g, x_raw), dy never written
            gd, xo = alloc.load('g', gq), alloc.load('x_raw', xq)
            sc2, sh2, kk = alloc.load('sc2', bn[0]), alloc.load('sh2', bn[1]), alloc.load('k123', k123)
            vd.view(torch.uint8).fill_(G.FILL)
            z.view(torch.uint8).fill_(G.FILL)
            ops.wino26_bnbwd_step(gd, xo, sc2, sh2, kk, True, dg, wg).run()
            dym = alloc.take('dy_materialised', (n, oh, ow, cout))
            ops.bn_bwd_apply(gd, xo, sc2, sh2, kk, True, dym)
            v_ref, z_ref = torch.empty_like(vd), torch.empty_like(z)
            sp = ops.stream_ptr()
            assert lib.hnd_wino2_input(dym.data_ptr(), v_ref.data_ptr(), n, oh, ow, cout, 1 - pad, None, None, 0, 6, sp) == 0
            assert lib.hnd_wino2_dy(dym.data_ptr(), z_ref.data_ptr(), n, oh, ow, cout, cout, 6, sp) == 0
            ops.sync_check()
            td, tw = n * ((h + 5) // 6) * ((w + 5) // 6), n * ((oh + 5) // 6) * ((ow + 5) // 6)
            r.update(fused=[(vd.view(49, -1, cout)[:, :td], v_ref.view(49, -1, cout)[:, :td]),
                            (z.view(49, -1, cout)[:, :tw], z_ref.view(49, -1, cout)[:, :tw])], dym=dym)
        if isinstance(alloc, G.Arena):
            RAN.update((fwd.variant, wg.variant, dg.variant))
        return r
    rp, rg = guarded(ops, build)
    ref = out.detach().permute(0, 2, 3, 1)
    assert finite(rg['y']) and torch.equal(rp['y'], rg['y']) and relmax(rg['y'], ref) < 2e-4
    tot = rg['st'].double().sum(0).cpu()
    assert finite(tot) and relmax(tot[0], ref.sum((0, 1, 2))) < 2e-4 and relmax(tot[1], (ref * ref).sum((0, 1, 2))) < 2e-4
    assert torch.equal(rg['v'].view(torch.int32), rg['v2'].view(torch.int32))          # the transform alone: the same bits
    assert finite(rg['dw']) and torch.equal(rp['dw'], rg['dw']) and relmax(rg['dw'], wt.grad) < 2e-4
    assert finite(rg['dx']) and torch.equal(rp['dx'], rg['dx']) and relmax(rg['dx'], a.grad.permute(0, 2, 3, 1)) < 2e-4
    if tile == 6:
        assert torch.equal(rg['dx2'], rg['dx'])
        pa, pr = rg['part'].double().sum(0).cpu(), rg['ref_part'].double().sum(0).cpu()
        assert finite(pa) and float((pa - pr).abs().max() / pr.abs().max()) < 2e-6
        assert finite(rg['dym'])
        for got, want in rg['fused']:
            assert finite(got) and finite(want) and relmax(got, want.cpu()) < 2e-6


# --------------------------------------------------------------------------------------------- train-mode BatchNorm
@covers('hnd_bn_finalize', 'hnd_bn_bwd_reduce', 'hnd_bn_bwd_finalize', 'hnd_bn_bwd_apply', 'hnd_affine_relu')
@pytest.mark.parametrize('c,relu', [(3, True), (64, False)])
def test_train_mode_batchnorm_forward_and_backward(ops, c, relu):
    """as tests/test_ops_gpu.py::test_train_bn_forward_backward (bars 1e-5 forward, 2e-5 backward), 2 x 13 x 17 = 442 pixels:
    partials of exactly stats_tiles / hnd_bn_bwd_ntiles tiles, per-channel vectors of exactly cs (c for gamma, beta,
    running statistics, dgamma, dbeta), k123 of exactly 3 * cs"""
    g = gen(11 + c)
    n, h, w = 2, 13, 17
    cs, npix = ops.chan_pad_of(c), n * h * w
    x = (torch.randn(n, c, h, w, generator=g) * 1.7 + 0.4).requires_grad_(True)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).requires_grad_(True), torch.randn(c, generator=g).requires_grad_(True)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    rm_ref, rv_ref = rm.clone(), rv.clone()
    out = F.batch_norm(x, rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5)
    out = F.relu(out) if relu else out
    gout = torch.randn(out.shape, generator=g)
    out.backward(gout)
    xh = nhwc(x.detach(), cs)
    nt = ops.stats_tiles(npix)
    blocks = F.pad(xh.view(npix, cs), (0, 0, 0, nt * 128 - npix)).view(nt, 128, cs)
    part_h = torch.stack([blocks.sum(1), (blocks * blocks).sum(1)], 1)

    def build(alloc):
        xd, part = alloc.load('x', xh), alloc.load('partials', part_h)
        gam, bet = alloc.load('gamma', gamma.detach()), alloc.load('beta', beta.detach())
        rmd, rvd = alloc.load('running_mean', rm), alloc.load('running_var', rv)
        nbt = alloc.load('nbt', torch.zeros(1, dtype=torch.int64))
        scale, shift, mean, rstd = [alloc.take(q, cs) for q in ('scale', 'shift', 'mean', 'rstd')]
        ops.bn_finalize(part, nt, c, cs, npix, gam, bet, rmd, rvd, nbt, 0.1, 1e-5, scale, shift, mean, rstd)
        y = alloc.take('y', xh.shape)
        ops.affine_relu(xd, scale, shift, y, relu)
        gd = alloc.load('g', nhwc(gout, cs))
        ntb = ops.bn_bwd_ntiles(npix)
        bpart = alloc.take('bwd_partials', (ntb, 2, cs))
        ops.bn_bwd_reduce(gd, xd, scale, shift, mean, rstd, relu, bpart)
        dgamma, dbeta, k123 = alloc.take('dgamma', c), alloc.take('dbeta', c), alloc.take('k123', (3, cs))
        ops.bn_bwd_finalize(bpart, ntb, c, cs, npix, gam, mean, rstd, dgamma, dbeta, k123)
        dx = alloc.take('dx', xh.shape)
        ops.bn_bwd_apply(gd, xd, scale, shift, k123, relu, dx)
        ops.sync_check()
        return y, rmd, rvd, nbt, scale, dgamma, dbeta, dx, bpart
    y, rmd, rvd, nbt, scale, dgamma, dbeta, dx, bpart = [t.cpu() for t in only_guarded(ops, build)]
    assert all(finite(t) for t in (y, rmd, rvd, scale, dgamma, dbeta, dx, bpart))
    assert relmax(y[..., :c], nhwc(out.detach())) < 1e-5
    assert relmax(rmd, rm_ref) < 1e-5 and relmax(rvd, rv_ref) < 1e-5 and int(nbt) == 1
    if cs != c:
        assert float(scale[c:].abs().max()) == 0 and float(y[..., c:].abs().max()) == 0
    assert relmax(dgamma, gamma.grad) < 2e-5 and relmax(dbeta, beta.grad) < 2e-5
    assert relmax(dx[..., :c], nhwc(x.grad)) < 2e-5


# ------------------------------------------------------------------------------------------------------------- losses
@covers('hnd_mse_sum_fwd_bwd', 'hnd_mimic_loss_fwd_bwd')
def test_loss_launches_with_exact_out_and_scratch(ops, lib):
    """numel 4, 12 and 4100 (the ABI takes positive multiples of 4 only: the smallest, a second one-block size and one past
    4096); MseLaunch / MimicLaunch with `out` (zero-filled once, double[1 + npairs]) and `scratch`
    (double[hnd_mse_scratch_elems()]) replaced by exact-size views.  Bars: 1e-6 relative on terms and gradients
    (tests/test_ops_gpu.py::test_mse_fused_loss_and_grad, tests/test_mimic_loss_gpu.py)."""
    g = gen(12)
    numels, factors = (4, 12, 4100), (1.0, 0.5, 2.0)
    ts = [torch.randn(k, generator=g) for k in numels]
    ss = [F.relu(torch.randn(k, generator=g)) for k in numels]

    def build(alloc):
        res = {}
        for kind in ('mse_launch', 'mse', 'l1', 'smooth_l1', 'huber'):
            pairs = []
            for i, (t, s, f) in enumerate(zip(ts, ss, factors)):
                grad = alloc.take('grad_%s_%d' % (kind, i), t.numel())
                base = (alloc.load('t_%s_%d' % (kind, i), t), alloc.load('s_%s_%d' % (kind, i), s), grad, f, 1)
                pairs.append(base if kind == 'mse_launch' else base + (kind, 0.7, t.numel() if kind == 'l1' else 0))
            ml = ops.MseLaunch(pairs, DEV) if kind == 'mse_launch' else ops.MimicLaunch(pairs, DEV)
            ml.out = alloc.take('out_' + kind, 1 + len(pairs), torch.float64, fill=0)
            ml.scratch = alloc.take('scratch_' + kind, int(lib.hnd_mse_scratch_elems()), torch.float64)
            ml.run()
            res[kind] = (ml.out, [p[2] for p in pairs])
        ops.sync_check()
        return res
    res = only_guarded(ops, build)
    for kind, (out, grads) in res.items():
        out, total = out.cpu(), 0.0
        for i, (t, s, f) in enumerate(zip(ts, ss, factors)):
            d = s.double() - t.double()
            w = f / t.numel() if kind == 'l1' else f
            if kind in ('mse_launch', 'mse'):
                val, gr = (d * d).sum(), 2 * w * d
            elif kind == 'l1':
                val, gr = d.abs().sum(), w * d.sign()
            elif kind == 'smooth_l1':
                val = torch.where(d.abs() < 0.7, 0.5 * d * d / 0.7, d.abs() - 0.35).sum()
                gr = w * torch.where(d.abs() < 0.7, d / 0.7, d.sign())
            else:
                val = torch.where(d.abs() <= 0.7, 0.5 * d * d, 0.7 * (d.abs() - 0.35)).sum()
                gr = w * torch.where(d.abs() <= 0.7, d, 0.7 * d.sign())
            gr = gr * (s > 0)
            term = float(val) * w
            total += term
            assert abs(float(out[1 + i]) - term) <= 1e-6 * term, (kind, i)
            assert finite(grads[i]) and rel_l2(grads[i], gr) < 1e-6, (kind, i)
        assert abs(float(out[0]) - total) <= 1e-6 * total, kind
    assert torch.equal(res['mse_launch'][0], res['mse'][0])            # kind = MSE with count = 0: the bits of hnd_mse_sum_fwd_bwd


# -------------------------------------------------------------------------------------------- input pipeline, codec
@covers('hnd_transform_image', 'hnd_transform_image_u8', 'hnd_transform_images', 'hnd_scale_boxes')
def test_image_transforms_and_box_rescale(ops, lib):
    """per-image and batched transforms into exactly [n][hp][wp][4]; bars: 2e-5 absolute against the oracle
    (test_transform_matches_oracle), batched == per-image bit for bit (test_batched_transform_...), boxes exact"""
    from oracle import hnd_oracle as O
    from hnd_ghnd_object_detectors_amd._lib import BoxesDesc
    g = gen(9)
    img = torch.rand(3, 37, 61, generator=g)
    u8 = torch.randint(0, 256, (33, 47, 3), generator=g, dtype=torch.uint8)
    scale = 1.37
    sizes = [(ops.interp_out_size(37, scale), ops.interp_out_size(61, scale)),
             (ops.interp_out_size(33, scale), ops.interp_out_size(47, scale))]
    hp, wp = 51, 85                                         # one row / column more than the larger resized image
    boxes = [torch.rand(5, 4, generator=g) * 400, torch.rand(1, 4, generator=g) * 400]

    def build(alloc):
        a, b = alloc.take('per_image', (2, hp, wp, 4)), alloc.take('batched', (2, hp, wp, 4))
        s0, s1 = alloc.load('img', img), alloc.load('u8', u8)
        ops.transform_image(s0, a, 0, sizes[0][0], sizes[0][1], 1 / scale, 1 / scale, O.IMAGE_MEAN, O.IMAGE_STD)
        ops.transform_image_u8(s1, a, 1, sizes[1][0], sizes[1][1], 1 / scale, 1 / scale, O.IMAGE_MEAN, O.IMAGE_STD, True, True)
        ops.transform_images([(s0, False, False, False) + sizes[0] + (1 / scale, 1 / scale),
                              (s1, True, True, True) + sizes[1] + (1 / scale, 1 / scale)], b, O.IMAGE_MEAN, O.IMAGE_STD)
        arr, outs = (BoxesDesc * 2)(), []
        for d, (i, bx) in zip(arr, enumerate(boxes)):
            src, dst = alloc.load('boxes%d' % i, bx), alloc.take('scaled%d' % i, tuple(bx.shape))
            d.src, d.dst, d.k, d.scale_w, d.scale_h = src.data_ptr(), dst.data_ptr(), bx.shape[0], 1.25, 0.75
            outs.append(dst)
        assert lib.hnd_scale_boxes(arr, 2, ops.stream_ptr()) == 0
        ops.sync_check()
        return a, b, outs
    a, b, outs = only_guarded(ops, build)
    assert finite(a) and torch.equal(a, b)
    a = a.cpu()
    for i, src in enumerate((img, O.to_tensor_u8(u8).flip(-1))):
        oh, ow = sizes[i]
        t = (src - torch.tensor(O.IMAGE_MEAN)[:, None, None]) / torch.tensor(O.IMAGE_STD)[:, None, None]
        ref = F.interpolate(t[None], scale_factor=scale, mode='bilinear', align_corners=False)[0]
        assert tuple(ref.shape[1:]) == (oh, ow)
        assert float((a[i, :oh, :ow, :3].permute(2, 0, 1) - ref).abs().max()) < 2e-5
        assert float(a[i, oh:].abs().max()) == 0 and float(a[i, :, ow:].abs().max()) == 0 and float(a[i, ..., 3].abs().max()) == 0
    for o, bx in zip(outs, boxes):
        assert torch.equal(o.cpu(), torch.stack((bx[:, 0] * 1.25, bx[:, 1] * 0.75, bx[:, 2] * 1.25, bx[:, 3] * 0.75), 1))


@covers('hnd_quantize_u8', 'hnd_dequantize_u8')
@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 13, 17)])
def test_bottleneck_codec_with_exact_scratch(ops, shape):
    """bit-exact against oracle/myutils_r.py (tests/test_ops_gpu.py::test_bottleneck_codec_matches_myutils_semantics);
    scratch: exactly hnd_minmax_scratch_elems floats, qparams exactly 4"""
    from oracle.myutils_r import quantize_tensor, dequantize_tensor
    n, h, w = shape
    c, cs = 3, 4
    z = torch.randn(n, c, h, w, generator=gen(18)) * 3 + 0.3
    if z.numel() == c:
        z[0, 1:] += 2.0
    ref_q = quantize_tensor(z.clone(), num_bits=8)
    ref = dequantize_tensor(ref_q)

    def build(alloc):
        buf = alloc.load('z', nhwc(z, cs))
        q, qp = alloc.take('q', buf.shape, torch.uint8), alloc.take('qparams', 4)
        scratch = alloc.take('scratch', int(ops.minmax_scratch_elems()))
        ops.quantize_u8(buf, c, q, qp, scratch)
        out = alloc.take('out', buf.shape)
        ops.dequantize_u8(q, qp, out, c)
        ops.sync_check()
        return q, qp, out
    q, qp, out = [t.cpu() for t in only_guarded(ops, build)]
    lo, hi, scale, zp = [float(v) for v in qp]
    assert (lo, hi, scale, zp) == (float(z.min()), float(z.max()), float(ref_q.scale), float(ref_q.zero_point))
    assert torch.equal(q[..., :c].permute(0, 3, 1, 2), ref_q.tensor) and torch.equal(out[..., :c].permute(0, 3, 1, 2), ref)
    assert float(out[..., c:].abs().max()) == 0.0 and int(q[..., c:].max()) == 0


# ---------------------------------------------------------------------------------------------------------- filter.hip
@covers('hnd_adaptive_avgpool_fwd', 'hnd_adaptive_avgpool_bwd', 'hnd_linear_fwd', 'hnd_linear_bwd', 'hnd_softmax_rows',
        'hnd_softmax_ce_rows_fwd_bwd', 'hnd_channel_sum')
def test_neural_filter_ops(ops):
    """references and bars (1e-6; channel sum 1e-5) of the filter tests in tests/test_ops_gpu.py, at their smallest shapes;
    channel-sum scratch: exactly hnd_channel_sum_scratch_elems(c)"""
    g = gen(31)
    x = torch.randn(3, 32, 14, 14, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.adaptive_avg_pool2d(x, (8, 8))
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy.double())
    n, c, h, w, nout = 5, 16, 8, 8, 2
    lx = torch.randn(n, c, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    wt = (torch.randn(nout, c * h * w, generator=g, dtype=torch.float64) / 32).requires_grad_(True)
    b = torch.randn(nout, generator=g, dtype=torch.float64).requires_grad_(True)
    lo = F.linear(lx.flatten(1), wt, b)
    do = torch.randn(lo.shape, generator=g)
    lo.backward(do.double())
    sx = torch.randn(7, 2, generator=g) * 5
    cx = (torch.randn(300, 2, generator=g) * 6).double().requires_grad_(True)
    labels = torch.randint(0, 2, (300,), generator=g)
    labels[1] = -100
    ce = F.cross_entropy(cx, labels)
    ce.backward()
    t = torch.randn(3, 16, 14, 14, generator=g)

    def build(alloc):
        xd, yd = alloc.load('x', nhwc(x.detach().float())), alloc.take('y', (3, 8, 8, 32))
        ops.adaptive_avgpool_fwd(xd, yd)
        dyd, dx = alloc.load('dy', nhwc(dy)), alloc.take('dx', (3, 14, 14, 32))
        ops.adaptive_avgpool_bwd(dyd, dx)
        lxd = alloc.load('lx', nhwc(lx.detach().float(), 32))
        wd, bd = alloc.load('lw', wt.detach().float()), alloc.load('lb', b.detach().float())
        od = alloc.take('lout', (n, nout))
        ops.linear_fwd(lxd, c, wd, bd, od)
        dod = alloc.load('ldout', do)
        dw, db, ldx = alloc.take('ldw', (nout, c * h * w)), alloc.take('ldb', nout), alloc.take('ldx', (n, h, w, 32))
        ops.linear_bwd(lxd, c, wd, dod, dw, db, ldx)
        sxd, sy = alloc.load('sx', sx), alloc.take('sy', (7, 2))
        ops.softmax_rows(sxd, sy)
        cxd, lab = alloc.load('logits', cx.detach().float()), alloc.load('labels', labels)
        loss, dlog = alloc.take('loss', 1), alloc.take('dlogits', (300, 2))
        ops.softmax_ce_rows(cxd, lab, loss, dlog)
        td, cs_out = alloc.load('t', nhwc(t, 32)), alloc.take('channel_sum', 16)
        scratch = alloc.take('cs_scratch', int(ops.channel_sum_scratch_elems(16)))
        ops.channel_sum(td, 16, cs_out, scratch)
        ops.sync_check()
        return yd, dx, od, dw, db, ldx, sy, loss, dlog, cs_out
    yd, dx, od, dw, db, ldx, sy, loss, dlog, cs_out = [q.cpu() for q in only_guarded(ops, build)]
    assert finite(yd) and relmax(yd, nhwc(y.detach())) < 1e-6 and finite(dx) and relmax(dx, nhwc(x.grad)) < 1e-6
    assert relmax(od, lo.detach()) < 1e-6 and relmax(dw, wt.grad) < 1e-6 and relmax(db, b.grad) < 1e-6
    assert finite(ldx) and relmax(ldx[..., :c], nhwc(lx.grad)) < 1e-6 and float(ldx[..., c:].abs().max()) == 0.0
    assert float((sy.double() - sx.double().softmax(1)).abs().max()) < 1e-6
    assert abs(float(loss) - float(ce.detach())) <= 1e-6 * abs(float(ce.detach())) + 1e-7
    assert finite(dlog) and relmax(dlog, cx.grad) < 1e-6 and float(dlog[1].abs().max()) == 0.0
    assert relmax(cs_out, t.double().sum((0, 2, 3))) < 1e-5


# ---------------------------------------------------------------------------------------------- detect.hip, detect_heads.hip
@covers('hnd_rpn_decode', 'hnd_clip_boxes', 'hnd_box_decode_clip', 'hnd_roi_align')
def test_box_branch_operators(ops, lib):
    """references and bars of tests/test_detect_gpu.py (oracle/tv042_det.py).  hnd_rpn_decode writes one level's window
    [off, off + h * w * A) of [n][total]; hnd_roi_align writes the rows idx selects: everything else keeps 0xFF"""
    import ctypes as C
    from oracle import tv042_det as TV
    from hnd_ghnd_object_detectors_amd import detection as D
    g = gen(31)
    n, a, (h, w), img_hw = 2, 3, (5, 7), (40, 56)
    before, after = 11 * a, 6 * a                                   # anchors of the levels before / after this one
    total = before + h * w * a + after
    obj, reg = torch.randn(n, a, h, w, generator=g), torch.randn(n, a * 4, h, w, generator=g) * 0.5
    reg[0, 2, 0, 0] = 9.0                                           # dw beyond the clip
    base = D.AnchorGenerator(((32,),), ((0.5, 1.0, 2.0),)).cell_anchors()[0]
    sy, sx = img_hw[0] / h, img_hw[1] / w
    shifts = torch.stack(torch.meshgrid(torch.arange(h) * sy, torch.arange(w) * sx, indexing='ij'), -1)   # (y, x)
    anchors = (torch.stack([shifts[..., 1], shifts[..., 0], shifts[..., 1], shifts[..., 0]], -1)[:, :, None] + base).reshape(-1, 4)
    o_flat, r_flat = TV.concat_box_prediction_layers([obj], [reg])
    ref_prop = TV.BoxCoder((1.0, 1.0, 1.0, 1.0)).decode(r_flat, [anchors] * n).view(n, -1, 4)
    head = F.pad(torch.cat([obj, reg], 1).permute(0, 2, 3, 1), (0, 1)).contiguous()            # ldc 16
    boxes = torch.randn(65, 4, generator=g) * 60 + 30
    k, ncls = 37, 5
    props = torch.rand(k, 2, generator=g) * 100
    props = torch.cat([props, props + torch.rand(k, 2, generator=g) * 40 + 2], 1)
    deltas = torch.randn(k, ncls * 4, generator=g)
    img_of = (torch.arange(k) >= 20).float()
    shapes = [(120, 180), (112, 200)]
    ref_dec = TV.BoxCoder((10., 10., 5., 5.)).decode(deltas, [props[:20], props[20:]])
    ref_dec = torch.cat([TV.clip_boxes_to_image(q, s) for q, s in zip(ref_dec.split([20, k - 20], 0), shapes)], 0)
    feat = torch.randn(2, 8, 9, 11, generator=g)
    rois = torch.cat([torch.randint(0, 2, (21, 1), generator=g).float(), torch.rand(21, 2, generator=g) * 30], 1)
    rois = torch.cat([rois, rois[:, 1:] + torch.rand(21, 2, generator=g) * 20 + 1], 1)
    rois[0, 1:] = torch.tensor([-30.0, -20.0, -5.0, -2.0])
    rois[2, 1:] = torch.tensor([30.0, 20.0, 400.0, 300.0])
    ref_roi = TV.roi_align(feat, rois, (7, 7), 0.25, 2)

    def build(alloc):
        hd = alloc.load('head', head)
        objectness, proposals = alloc.take('objectness', (n, total)), alloc.take('proposals', (n, total, 4))
        flat = (C.c_float * 12)(*[float(v) for v in base.reshape(-1)])
        assert lib.hnd_rpn_decode(hd.data_ptr(), n, h, w, 16, a, flat, sy, sx, before, total, D.XFORM_CLIP,
                                  objectness.data_ptr(), proposals.data_ptr(), ops.stream_ptr()) == 0
        bx = alloc.load('boxes', boxes)
        D.clip_boxes_(bx, (50, 70))
        dd = alloc.load('deltas', deltas)
        rd = alloc.load('rois5', torch.cat([img_of[:, None], props], 1))
        hw = alloc.load('image_hw', torch.tensor([[float(p), float(q)] for p, q in shapes]))
        dec = alloc.take('decoded', (k, ncls, 4))
        assert lib.hnd_box_decode_clip(dd.data_ptr(), ncls * 4, rd.data_ptr(), hw.data_ptr(), k, ncls, 10., 10., 5., 5.,
                                       D.XFORM_CLIP, dec.data_ptr(), ops.stream_ptr()) == 0
        f, rr = alloc.load('feat', feat.permute(0, 2, 3, 1).contiguous()), alloc.load('rois', rois)
        sel = alloc.load('idx', torch.arange(0, 21, 2))
        pooled = alloc.take('pooled', (21, 7, 7, 8))
        assert lib.hnd_roi_align(f.data_ptr(), 2, 9, 11, 8, rr.data_ptr(), sel.data_ptr(), sel.numel(), 0.25, 7, 7, 2,
                                 pooled.data_ptr(), ops.stream_ptr()) == 0
        ops.sync_check()
        return objectness, proposals, bx, dec, pooled
    objectness, proposals, bx, dec, pooled = [q.cpu() for q in only_guarded(ops, build)]
    win = slice(before, before + h * w * a)
    assert torch.equal(objectness[:, win], o_flat.reshape(n, -1))
    assert float((proposals[:, win] - ref_prop).abs().max() / ref_prop.abs().max()) < 2e-6
    for t in (objectness, proposals):                                # outside the window: the pattern, bit for bit
        rest = torch.cat([t[:, :before], t[:, before + h * w * a:]], 1)
        assert bool((rest.contiguous().view(torch.int32) == -1).all())
    want = torch.stack([boxes[:, 0].clamp(0, 70), boxes[:, 1].clamp(0, 50), boxes[:, 2].clamp(0, 70), boxes[:, 3].clamp(0, 50)], 1)
    assert torch.equal(bx, want)
    assert finite(dec) and float((dec.view(k, -1) - ref_dec.view(k, -1)).abs().max()) < 2e-4
    got = pooled.permute(0, 3, 1, 2)
    assert bool((pooled[1::2].contiguous().view(torch.int32) == -1).all())          # rows of other levels stay 0xFF
    assert finite(got[0::2]) and float((got[0::2] - ref_roi[0::2]).abs().max()) <= 1e-6 * float(ref_roi.abs().max())


@covers('hnd_mask_probs', 'hnd_paste_masks', 'hnd_resize_mask_nearest_u8', 'hnd_upsample_bilinear_nhwc',
        'hnd_heatmaps_to_keypoints')
def test_mask_and_keypoint_branch_operators(ops, lib):
    """references and bars of tests/test_detect_gpu.py (paste 2e-6, bilinear 1e-6, keypoint scores 1e-4 relative and
    >= 98 % equal maxima) and test_gt_mask_nearest_resize_equals_torch_bytes (bytes)"""
    from oracle import tv042_det as TV
    g = gen(61)
    k, m, ldc = 5, 14, 8
    logits = torch.randn(k, m, m, ldc, generator=g)
    labels = torch.randint(0, 7, (k,), generator=g)
    im_h, im_w = 37, 53
    boxes = torch.tensor([[10.3, 12.9, 40.2, 30.7], [-15.5, -8.2, 30.0, 20.0], [40.0, 30.0, 70.5, 50.25],
                          [20.0, 20.0, 20.4, 20.3], [-20.0, -30.0, 80.0, 60.0]])
    masks = torch.rand(k, 1, m, m, generator=g)
    ref_paste = TV.paste_masks_in_image(masks, boxes, (im_h, im_w))
    sc = float(m + 2) / m
    wh, hh = (boxes[:, 2] - boxes[:, 0]) * .5 * sc, (boxes[:, 3] - boxes[:, 1]) * .5 * sc
    xc, yc = (boxes[:, 2] + boxes[:, 0]) * .5, (boxes[:, 3] + boxes[:, 1]) * .5
    exp = torch.stack([xc - wh, yc - hh, xc + wh, yc + hh], 1).to(torch.int64).contiguous()   # (detection.paste_masks_in_image)
    gt = (torch.rand(3, 37, 53, generator=g) < 0.4).to(torch.uint8) * 200
    scale = 1.7027027027027026
    oh, ow = ops.interp_out_size(37, scale), ops.interp_out_size(53, scale)
    ref_gt = F.interpolate(gt[None].float(), scale_factor=scale)[0].byte()
    ux = torch.randn(2, 5, 7, 9, generator=g)
    ref_up = F.interpolate(ux, scale_factor=2, mode='bilinear', align_corners=False)
    nkp, hm = 5, 14
    maps = torch.randn(3, nkp, hm, hm, generator=g)
    rois = torch.tensor([[3.2, 4.1, 80.7, 120.3], [10.0, 10.0, 10.4, 10.2], [50.5, 20.25, 64.5, 34.25]])
    ref_xy, ref_sc = TV.heatmaps_to_keypoints(maps, rois)

    def build(alloc):
        s = ops.stream_ptr()
        lg, lb, probs = alloc.load('logits', logits), alloc.load('labels', labels), alloc.take('probs', (k, m, m))
        assert lib.hnd_mask_probs(lg.data_ptr(), lb.data_ptr(), k, m, ldc, probs.data_ptr(), s) == 0
        mk, ex, pasted = alloc.load('masks', masks), alloc.load('boxes', exp), alloc.take('pasted', (k, im_h, im_w))
        assert lib.hnd_paste_masks(mk.data_ptr(), ex.data_ptr(), k, m, im_h, im_w, pasted.data_ptr(), s) == 0
        gi, go = alloc.load('gt', gt), alloc.take('gt_out', (3, oh, ow), torch.uint8)
        assert lib.hnd_resize_mask_nearest_u8(gi.data_ptr(), 3, 37, 53, oh, ow, scale, go.data_ptr(), s) == 0
        ui, uo = alloc.load('up_in', ux.permute(0, 2, 3, 1).contiguous()), alloc.take('up_out', (2, 14, 18, 5))
        assert lib.hnd_upsample_bilinear_nhwc(ui.data_ptr(), 2, 7, 9, 5, 2, uo.data_ptr(), s) == 0
        mp, rr = alloc.load('maps', maps.permute(0, 2, 3, 1).contiguous()), alloc.load('rois', rois)
        xy, ksc = alloc.take('xy', (3, nkp, 3)), alloc.take('scores', (3, nkp))
        assert lib.hnd_heatmaps_to_keypoints(mp.data_ptr(), 3, hm, hm, nkp, nkp, rr.data_ptr(), xy.data_ptr(),
                                             ksc.data_ptr(), s) == 0
        ops.sync_check()
        return probs, pasted, go, uo, xy, ksc
    probs, pasted, go, uo, xy, ksc = [q.cpu() for q in only_guarded(ops, build)]
    want = torch.sigmoid(logits[torch.arange(k), :, :, labels].double())
    assert finite(probs) and float((probs.double() - want).abs().max()) < 1e-6
    assert finite(pasted) and torch.equal(pasted == 0, ref_paste[:, 0] == 0)
    assert float((pasted - ref_paste[:, 0]).abs().max()) < 2e-6
    assert torch.equal(go, ref_gt)
    assert finite(uo) and float((uo.permute(0, 3, 1, 2) - ref_up).abs().max()) < 1e-6
    assert finite(xy) and float((xy == ref_xy).all(2).float().mean()) >= 0.98 and bool((xy[..., 2] == 1).all())
    assert float((ksc - ref_sc).abs().max()) < 1e-4 * float(ref_sc.abs().max())


# ------------------------------------------------------------------------------------------------- variant coverage
def test_every_kernel_variant_ran_under_guards(ops):
    """LAST in the file: the union of variants that ran inside an arena equals every name ConvLaunch.refresh_variant can
    give (enum hnd_conv_tile minus 'unused', and the 4-lane tile) plus the weight-gradient kernels plus both builds of the emulation kernel -- a kernel added
    later without a guard case turns this red.  RAN is filled by the cases above IN THIS PROCESS: the test needs the whole
    file in one run and fails under -k, --lf, a node id of its own or pytest-xdist."""
    names = (set(ops.TILE_NAMES.values()) - {'unused'}) | {'igemm_c4_128x64'}      # enum hnd_conv_tile and the 4-lane special case
    assert len(names) >= 16, sorted(names)
    expect = (names - {'bx3_64'}) | {'bx3_64/persistent', 'bx3_64/tiled'}
    expect |= (set(ops.WGRAD_NAMES.values()) - {'staged'}) | {'wgrad_m64', 'wgrad_m128'}      # enum hnd_wgrad_variant
    assert expect >= {'wgrad_m64', 'wgrad_m128', 'stem7_wgrad', 'thin_wgrad', 'wgrad_ring'}
    assert RAN == expect, (sorted(expect - RAN), sorted(RAN - expect))
