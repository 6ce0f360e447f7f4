"""The forward / data-gradient wall: the case tables, the fp64 reference and the bars shared by tests/test_conv_cases_cpu.py
(routing, coverage conditions, the reference against itself: no GPU) and tests/test_conv_gpu.py (the launches).  Nothing
here loads the library or touches a device; both files read the SAME tuples, so a geometry the CPU file routed is the one
the GPU runs.

hnd_conv2d_igemm dispatches to eight native kernels (csrc/conv_igemm.hip: pick_conv): the tiled kernel in four block tiles,
the 4-lane tile, thin_n4, stem7_lds, the 8-wave and one-wave B-resident builds and the B-streamed builds.  A logical channel
count c is stored as chan_pad_of(c): 3 / 4 as 4 lanes, anything else as a multiple of 32.  Every launch is the native fp32
family (ops.emulation('off')); the emulated bf16x3 kernels and the Winograd path have walls of their own."""
import collections
import functools
import math
import random

import torch
import torch.nn.functional as F

from hnd_ghnd_object_detectors_amd._lib import CONV_TILES         # enum hnd_conv_tile of include/hnd_hip.h (no library is loaded)
from tests.wgrad_util import ALL_FORMS, PRO_FORMS, SCALE_RELU

U = 2.0 ** -24                                      # unit roundoff of fp32
PAD_LANE_VALUE = 3.0e4
SWITCHES = ('HND_BRES', 'HND_BRES2', 'HND_BSTREAM', 'HND_THIN_N', 'HND_STEM7', 'HND_DEBUG_PICKER')
TILE_NAMES = tuple(sorted((n for n in CONV_TILES if n.startswith('igemm_')), key=CONV_TILES.get))      # the four block tiles, codes 0..3
# ConvLaunch.variant -> hnd_conv2d_igemm_tile's code: the 4-lane kernel answers with its 128x64 tile
TILE_CODE = dict(CONV_TILES, igemm_c4_128x64=CONV_TILES['igemm_128x64'])
KERNELS = ('tiled', 'igemm_c4_128x64', 'stem7_lds', 'thin_n4', 'bres', 'bres2', 'bstream')
EPI_OPERANDS = ('es', 'eb', 'r1', 'r2', 'up', 'mask', 'relu', 'stats', 'mout')
COMPUTE_UNITS = 256                                 # what the pickers assume without a device, and what an MI355X has


def kernel_of(variant):
    """the kernel (one achieved line each) behind a ConvLaunch.variant"""
    return 'tiled' if variant in TILE_NAMES else variant.split('_')[0] if variant.startswith(('bres', 'bstream')) else variant


def lanes(c):
    return 4 if c <= 4 else (c + 31) // 32 * 32


def round_up(x, m):
    return (x + m - 1) // m * m


def out_extent(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


# A forward case.  kh, kw: the kernel; pro: a prologue form of wgrad_util.ALL_FORMS; epi: '+'-joined epilogue operands of
# EPI_OPERANDS ('up': res1 is nearest-upsampled from ((oh + 1) // 2, (ow + 1) // 2); 'mout': mask_out); ldc: None = the
# launch's cout is the whole channel stride chan_pad_of(cout) (lanes beyond cout have zero weight rows and must come back
# as exact zeros), an int = cout is passed explicitly with that stride (lanes beyond it are not written at all).
Case = collections.namedtuple('Case', 'n cin h w cout kh kw stride pad pro epi ldc')


def fwd(n, cin, h, w, cout, k, stride=1, pad=0, pro='none', epi='', ldc=None):
    kh, kw = (k, k) if isinstance(k, int) else k
    assert pro in ALL_FORMS and set(epi_of(epi)) <= set(EPI_OPERANDS)
    return Case(n, cin, h, w, cout, kh, kw, stride, pad, pro, epi, ldc)


def epi_of(epi):
    return frozenset(e for e in epi.split('+') if e)


def case_id(c):
    return '-'.join(str(v) for v in c if v not in ('', None))


def rows_of(c):
    return c.n * out_extent(c.h, c.kh, c.stride, c.pad) * out_extent(c.w, c.kw, c.stride, c.pad)


def fwd_fields(c):
    """the integer fields of the hnd_conv_desc ops.conv_forward builds for a case, and `ptrs`: its optional operands"""
    oh, ow = out_extent(c.h, c.kh, c.stride, c.pad), out_extent(c.w, c.kw, c.stride, c.pad)
    e, cl, ldc = epi_of(c.epi), lanes(c.cin), c.ldc or lanes(c.cout)
    up = 'up' in e
    ptrs = {'pro_scale', 'pro_shift'} if c.pro != 'none' else set()
    ptrs |= {{'es': 'epi_scale', 'eb': 'epi_shift', 'r1': 'res1', 'r2': 'res2', 'mask': 'mask', 'stats': 'stats',
              'mout': 'mask_out'}[k] for k in e if k not in ('up', 'relu')}
    return dict(n=c.n, h=c.h, w_=c.w, cin=cl, oh=oh, ow=ow, yh=oh, yw=ow, cout=c.cout if c.ldc else ldc, ldc=ldc, y_sh=1, y_oh=0,
                y_sw=1, y_ow=0, kh=c.kh, kw=c.kw, sh=c.stride, dh=1, bh=-c.pad, sw=c.stride, dw=1, bw=-c.pad,
                kdim=round_up(c.kh * c.kw * cl, 32), pro_relu=int(c.pro in ('relu', SCALE_RELU)), relu=int('relu' in e),
                res1_mode=int(up), res1_h=(oh + 1) // 2 if up else 0, res1_w=(ow + 1) // 2 if up else 0, w_group_rows=0,
                w_group_stride=0, ptrs=frozenset(ptrs))


# --------------------------------------------------------------------------------------------------------- reference

def conv64(a, w, stride, pad):
    """fp64 convolution of NCHW a with OIHW w; an unpadded 1x1 as a plain matrix product (any device: no conv library)"""
    if w.shape[2] == 1 and w.shape[3] == 1 and pad == 0:
        rows = a[:, :, ::stride, ::stride].permute(0, 2, 3, 1)
        return (rows @ w[:, :, 0, 0].t()).permute(0, 3, 1, 2)
    return F.conv2d(a, w, None, stride, pad)


def prologue64(x, ps, pb, relu):
    """(a, magnitudes): a = relu?(x ps + pb) in fp64, |x ps| + |pb| beside it"""
    a = x.double()
    mag = a.abs()
    if ps is not None:
        a = a * ps.double()[None, :, None, None]
        mag = a.abs()
        if pb is not None:
            a = a + pb.double()[None, :, None, None]
            mag = mag + pb.double().abs()[None, :, None, None]
    return (a.clamp_min(0.0) if relu else a), mag


def fwd_reference(c, t):
    """(y64, B64) of one forward launch, NCHW, every operation in fp64 on the fp32 operands t (fwd_inputs' dict, on any
    device): a = relu?(x ps + pb), zero-padded AFTER the prologue; conv; * es + eb + r1 + r2; the mask by its operand
    (> 0); ReLU.  B64 = |es| S64 + |eb| + |r1| + |r2| with S64 the same convolution of |x ps| + |pb| with |w|."""
    e = epi_of(c.epi)
    a, mag = prologue64(t['x'], t.get('ps'), t.get('pb'), c.pro in ('relu', SCALE_RELU))
    w64 = t['w'].double()
    y, b = conv64(a, w64, c.stride, c.pad), conv64(mag, w64.abs(), c.stride, c.pad)
    if 'es' in e:
        y, b = y * t['es'].double()[None, :, None, None], b * t['es'].double().abs()[None, :, None, None]
    if 'eb' in e:
        y, b = y + t['eb'].double()[None, :, None, None], b + t['eb'].double().abs()[None, :, None, None]
    if 'r1' in e:
        r1 = t['r1'].double()
        if 'up' in e:
            r1 = F.interpolate(r1, size=y.shape[2:], mode='nearest')
        y, b = y + r1, b + r1.abs()
    if 'r2' in e:
        y, b = y + t['r2'].double(), b + t['r2'].double().abs()
    if 'mask' in e:
        y = torch.where(t['mask'] > 0, y, torch.zeros_like(y))
    if 'relu' in e:
        y = y.clamp_min(0.0)
    return y, b


def fwd_fp32(c, t):
    """torch's own fp32 CPU evaluation of the same launch (the room the bound leaves a correct fp32 result)"""
    e = epi_of(c.epi)
    a = t['x']
    if 'ps' in t:
        a = a * t['ps'][None, :, None, None]
    if 'pb' in t:
        a = a + t['pb'][None, :, None, None]
    if c.pro in ('relu', SCALE_RELU):
        a = F.relu(a)
    y = F.conv2d(a, t['w'], None, c.stride, c.pad)
    if 'es' in e:
        y = y * t['es'][None, :, None, None]
    if 'eb' in e:
        y = y + t['eb'][None, :, None, None]
    if 'r1' in e:
        y = y + (F.interpolate(t['r1'], size=y.shape[2:], mode='nearest') if 'up' in e else t['r1'])
    if 'r2' in e:
        y = y + t['r2']
    if 'mask' in e:
        y = torch.where(t['mask'] > 0, y, torch.zeros_like(y))
    return F.relu(y) if 'relu' in e else y


def bars(got, y64, b64, k):
    """(relative-to-max error, worst ratio of |got - y64| to the element-wise bound (K + 8) 2^-24 B64 + 1e-30).
    The first is the project's bar for fp32-MFMA convs (< 1e-4).  The second holds for ANY summation order: K is the number
    of real products behind the element (a number, or a map for a strided data gradient whose parity classes differ),
    gamma_K covers the dot product, and the + 8 absorbs the two prologue roundings, the one rounding of a folded scale, the
    four epilogue operations and second-order terms; mask and ReLU are exact and 1-Lipschitz.  It must be <= 1."""
    err = (got.double() - y64).abs()
    return float(err.max() / (y64.abs().max() + 1e-30)), float((err / ((k + 8) * U * b64 + 1e-30)).max())


def stats_bars(sums, y64, b64, k, m):
    """worst ratios of the per-channel (sum, sum of squares) `sums` [2, cout] (the per-tile partials added in fp64) to
    |S - S y64| <= sum_rows bound(y) + (M + 8) 2^-24 sum |y64| and
    |S2 - S y64^2| <= sum_rows 2 |y64| bound(y) + (M + 8) 2^-24 sum y64^2"""
    bound = (k + 8) * U * b64 + 1e-30
    s1, s2 = y64.sum((0, 2, 3)), (y64 * y64).sum((0, 2, 3))
    lim1 = bound.sum((0, 2, 3)) + (m + 8) * U * y64.abs().sum((0, 2, 3)) + 1e-30
    lim2 = (2 * y64.abs() * bound).sum((0, 2, 3)) + (m + 8) * U * s2 + 1e-30
    return float(((sums[0].double() - s1).abs() / lim1).max()), float(((sums[1].double() - s2).abs() / lim2).max())


def nibbles(t_nhwc):
    """[t > 0] of an NHWC tensor with lanes % 4 == 0 as hnd_conv_desc.mask_bits / mask_out stores it: uint8 [n, h, w, lanes / 4]"""
    bits = (t_nhwc > 0).reshape(t_nhwc.shape[:3] + (t_nhwc.shape[3] // 4, 4)).to(torch.uint8)
    return bits[..., 0] | (bits[..., 1] << 1) | (bits[..., 2] << 2) | (bits[..., 3] << 3)


def _seed(c):
    return 31000 + sum((i + 1) * v for i, v in enumerate(c[:9])) + 97 * ALL_FORMS.index(c.pro) + (hash_epi(c.epi) if c.epi else 0)


def hash_epi(epi):
    return sum(3 ** EPI_OPERANDS.index(e) for e in epi_of(epi))


def _nchw_rand(g, n, c, h, w):
    """a seeded NCHW tensor whose MEMORY is NHWC (the layout the launches take: no copy on the way to the device)"""
    return torch.randn(n, h, w, c, generator=g).permute(0, 3, 1, 2)


def _prologue(g, cin, pro):
    sign = torch.where(torch.rand(cin, generator=g) < 0.25, -1.0, 1.0)
    ps = (torch.rand(cin, generator=g) + 0.5) * sign if pro != 'none' else None
    pb = torch.randn(cin, generator=g) * 0.3 if pro in ('shift', 'relu') else None
    return ps, pb


@functools.lru_cache(maxsize=4)
def fwd_inputs(c):
    """seeded fp32 operands of a forward case (NCHW; x and the output-shaped operands in NHWC memory).  ps and es carry
    both signs; eb[1] is a SMALL shift (1e-3): the channel where a dropped epi_shift hides from a relative-to-max bar."""
    g = torch.Generator().manual_seed(_seed(c))
    e = epi_of(c.epi)
    oh, ow = out_extent(c.h, c.kh, c.stride, c.pad), out_extent(c.w, c.kw, c.stride, c.pad)
    t = {'x': _nchw_rand(g, c.n, c.cin, c.h, c.w),
         'w': torch.randn(c.cout, c.cin, c.kh, c.kw, generator=g) / math.sqrt(c.cin * c.kh * c.kw)}
    ps, pb = _prologue(g, c.cin, c.pro)
    if ps is not None:
        t['ps'] = ps
    if pb is not None:
        t['pb'] = pb
    if 'es' in e:
        t['es'] = (torch.rand(c.cout, generator=g) + 0.5) * torch.where(torch.rand(c.cout, generator=g) < 0.25, -1.0, 1.0)
    if 'eb' in e:
        t['eb'] = torch.randn(c.cout, generator=g) * 0.3
        t['eb'][1 % c.cout] = 1e-3
    if 'r1' in e:
        t['r1'] = _nchw_rand(g, c.n, c.cout, (oh + 1) // 2, (ow + 1) // 2) if 'up' in e else _nchw_rand(g, c.n, c.cout, oh, ow)
    if 'r2' in e:
        t['r2'] = _nchw_rand(g, c.n, c.cout, oh, ow)
    if 'mask' in e:
        t['mask'] = _nchw_rand(g, c.n, c.cout, oh, ow)
    return t


@functools.lru_cache(maxsize=2)
def fwd_case(c):
    """(operands, y64, B64, K, M) of a forward case with the reference on the CPU, computed once and shared"""
    t = fwd_inputs(c)
    y64, b64 = fwd_reference(c, t)
    return t, y64, b64, c.kh * c.kw * c.cin, rows_of(c)


# --------------------------------------------------------------------------------------------------------- A. tiled
# Every geometry runs on all four block tiles through HND_DEBUG_PICKER=igemm_tile=0..3; the variant is what the override's
# own fall-backs give (csrc/conv_igemm.hip: pick_tile).
TILED_ENV = {'HND_BRES': '0', 'HND_BSTREAM': '0', 'HND_THIN_N': '0', 'HND_STEM7': '0'}


def tiled_env(tile):
    return dict(TILED_ENV, HND_DEBUG_PICKER='igemm_tile=%d' % tile)


def tiled_name(tile, cout, stats=False, mask_out=False):
    """pick_tile's override restated: cout % 128 != 0 turns tiles 0 and 2 into 1 and 3, stats needs 128 rows, mask_out
    128 columns (cout: the launch's, i.e. the channel stride unless the case passes its own)"""
    if tile in (0, 2) and cout % 128 != 0:
        return TILE_NAMES[tile + 1]
    if stats and tile in (2, 3):
        return TILE_NAMES[tile - 2]
    if mask_out and tile in (1, 3):
        return TILE_NAMES[tile - 1]
    return TILE_NAMES[tile]


def tiled_variant(c, tile):
    f = fwd_fields(c)
    return tiled_name(tile, f['cout'], 'stats' in f['ptrs'], 'mask_out' in f['ptrs'])


RAGGED = (2, 64, 5, 7)                  # M = 70 rows of a 3x3 pad 1 conv: one ragged tile of every build
COUTS = (3, 5, 60, 64, 68, 100, 124, 128, 132, 192)
_TILED_HAND = (
    # a single output pixel, a map smaller than its kernel, pad = k - 1
    [fwd(1, 32, k, k, 64, k) for k in (1, 3, 7)] +
    [fwd(1, 32, 1, 1, 64, 3, 1, 1), fwd(1, 32, 2, 1, 64, 5, 1, 2), fwd(1, 32, 4, 5, 64, 2, 1, 1), fwd(1, 32, 4, 5, 64, 3, 1, 2)] +
    # n oh ow = 63 / 64 / 65 / 127 / 128 / 129 around the 64- and 128-row tiles
    [fwd(1, 32, 7, 9, 64, 3, 1, 1), fwd(1, 32, 8, 8, 64, 1), fwd(1, 32, 5, 13, 64, 3, 1, 1), fwd(1, 32, 1, 127, 64, 1),
     fwd(2, 32, 8, 8, 64, 3, 1, 1), fwd(3, 32, 1, 43, 64, 3, 1, 1)] +
    # channel tails: the lanes beyond cout are exact zeros; once with cout < ldc passed explicitly (they keep their NaN)
    [fwd(2, 32, 5, 7, cout, 3, 1, 1) for cout in COUTS] + [fwd(2, 32, 5, 7, 60, 3, 1, 1, ldc=64)] +
    [fwd(2, cin, 5, 7, 64, 3, 1, 1) for cin in (96, 160)] +
    # k = 1 .. 7 at both strides; the unpadded stride-2 rows leave input rows / columns no output pixel touches
    [fwd(2, 32, 9, 11, 64, 1, 2, 0), fwd(2, 32, 8, 10, 64, 1, 2, 0), fwd(2, 32, 6, 7, 64, 2, 1, 0), fwd(2, 32, 8, 9, 64, 2, 2, 0),
     fwd(2, 32, 8, 11, 64, 3, 2, 0), fwd(2, 32, 9, 11, 64, 3, 2, 1), fwd(2, 32, 8, 10, 64, 3, 2, 1), fwd(2, 32, 9, 12, 64, 4, 2, 0),
     fwd(2, 32, 9, 10, 64, 4, 2, 1), fwd(2, 32, 6, 7, 64, 4, 1, 1), fwd(1, 32, 9, 11, 64, 5, 1, 2), fwd(1, 32, 10, 11, 64, 5, 2, 0), fwd(1, 32, 9, 9, 64, 7, 1, 3),
     fwd(1, 32, 11, 14, 64, 7, 2, 3), fwd(2, 32, 5, 7, 64, (1, 3), 1, 1), fwd(2, 32, 5, 7, 64, (3, 1), 1, 0)] +
    # the fused forms, one ragged geometry each
    [fwd(*RAGGED, 64, 3, 1, 1, pro=p) for p in ALL_FORMS] +
    [fwd(*RAGGED, 64, 3, 1, 1, epi=e) for e in ('es', 'eb', 'r1', 'r1+r2', 'mask', 'mask+relu')] +
    [fwd(1, 32, 9, 13, 64, 3, 1, 1, epi='r1+up'),                                   # 9 x 13 from 5 x 7
     fwd(3, 32, 1, 43, 128, 3, 1, 1, epi='stats'),                                  # M = 129: the second tile nearly empty
     fwd(3, 32, 1, 43, 128, 3, 1, 1, pro='relu', epi='es+eb+stats'),
     fwd(*RAGGED, 128, 3, 1, 1, epi='relu+mout'), fwd(*RAGGED, 128, 3, 1, 1, epi='es+eb+mout'),
     fwd(*RAGGED, 128, 3, 1, 1, pro='relu', epi='es+eb+r1+r2+mask+relu')])


def _tiled_drawn(count=6, seed=20261020):
    rng, out = random.Random(seed), []
    while len(out) < count:
        k, stride = rng.choice((1, 2, 3, 5)), rng.choice((1, 2))
        pad = rng.randint(0, k // 2)
        n, cin, cout = rng.choice((1, 2, 3)), rng.choice((32, 64, 96, 160)), rng.randint(5, 200)
        h, w = rng.randint(k, 14), rng.randint(k, 14)
        out.append(fwd(n, cin, h, w, cout, k, stride, pad, rng.choice(PRO_FORMS), rng.choice(('', 'es+eb', 'r1+relu', 'mask'))))
    return out


TILED_CASES = _TILED_HAND + _tiled_drawn()

# --------------------------------------------------------------------------------------------------------- B. 4 lanes
# (case, switches, variant).  igemm_c4_128x64: cin 3 and a genuine cin 4, k = 2 and a k = 7 that HND_STEM7=0 keeps off the
# stem kernel; kdim (32 / 224) lies above kh kw 4 (16 / 196).  stem7_lds walks output tiles of 8 x 32 pixels (csrc/conv_stem.hip).
STEM_TILE = (8, 32)
C4_CASES = [
    (fwd(2, 3, 6, 7, 64, 2), {}, 'igemm_c4_128x64'),
    (fwd(2, 4, 6, 7, 64, 2, 1, 1, pro='relu'), {}, 'igemm_c4_128x64'),
    (fwd(2, 3, 6, 7, 100, 2, 1, 1, pro=SCALE_RELU, epi='eb+relu'), {}, 'igemm_c4_128x64'),
    (fwd(1, 3, 9, 13, 64, 7, 2, 3), {'HND_STEM7': '0'}, 'igemm_c4_128x64'),
    (fwd(2, 4, 12, 10, 64, 7, 2, 3, epi='es+eb+relu'), {'HND_STEM7': '0'}, 'igemm_c4_128x64'),
    (fwd(1, 4, 9, 13, 64, 7, 2, 3, pro='shift'), {}, 'igemm_c4_128x64'),            # a prologue keeps it off the stem kernel
]
# (n, cin_real, h, w, epilogue): each on stem7_lds and, with HND_STEM7=0, on igemm_c4_128x64 (the same bits: hnd_hip.h)
STEM_CASES = [
    (1, 3, 9, 13, ''),                  # 5 x 7 outputs: below one tile in both directions
    (2, 4, 12, 10, 'es+eb+relu'),       # 6 x 5, the stem's own epilogue (FrozenBatchNorm + ReLU)
    (1, 3, 2, 70, ''),                  # one output row, two column tiles and three columns
    (1, 4, 15, 66, 'eb'),               # 8 x 33: one full tile and a single column of the next
    (2, 3, 17, 65, ''),                 # 9 x 33: a single row and a single column beyond
    (1, 4, 18, 64, 'relu'),             # 9 x 32: a single row beyond, even extents
]


def stem_case(row):
    n, cin, h, w, epi = row
    return fwd(n, cin, h, w, 64, 7, 2, 3, epi=epi)


# --------------------------------------------------------------------------------------------------------- C. thin_n4
# (case, taken): thin_n4 under the default switches where `taken`, each also with HND_THIN_N=0 on the tiled kernel: the
# SAME bits (include/hnd_hip.h: "bit-identical to the MFMA tiles").  M = 1 / 127 / 128 / 129 around its 128-pixel block.
THIN_CASES = [
    (fwd(1, 64, 1, 1, 1, 1), True),                                   # M = 1
    (fwd(1, 64, 2, 2, 2, 2, pro='relu'), True),                       # M = 1, k = 2
    (fwd(1, 64, 1, 127, 3, 1, pro='scale'), True),                    # M = 127
    (fwd(2, 128, 8, 8, 4, 1, pro='shift'), True),                     # M = 128
    (fwd(3, 64, 1, 43, 3, 1, epi='stats'), True),                     # M = 129, statistics of a nearly empty block
    (fwd(3, 128, 2, 42, 3, 2, 1, 1, pro='relu', epi='es+eb+stats'), True),   # 3 x 43 outputs = 387: pad 1, three blocks
    (fwd(2, 64, 9, 12, 2, 1, 2, 0), True),                            # 1x1 stride 2
    (fwd(2, 64, 5, 6, 2, 1, 1, 1, pro='relu'), True),                 # 1x1 pad 1: a border of pixels with no in-bounds tap at
    (fwd(2, 128, 5, 6, 3, 1, 2, 1, pro='shift'), True),               # all -- exactly the epilogue of 0, whatever the shift
    (fwd(2, 64, 6, 5, 4, 1, 2, 1, epi='eb+relu'), True),
    (fwd(2, 128, 9, 12, 1, 2, 2, 0, pro=SCALE_RELU), True),           # 2x2 stride 2 unpadded, a leftover row
    (fwd(2, 64, 9, 11, 4, 2, 2, 1, epi='r1'), True),                  # 2x2 stride 2 pad 1, residual
    (fwd(2, 64, 6, 7, 3, 2, 1, 1, pro='relu', epi='r1+r2+mask+relu'), True),
    (fwd(1, 1024, 3, 3, 3, 2, pro='relu'), True),                     # kdim = 4096: the limit, taken
    (fwd(1, 1088, 3, 3, 3, 2, pro='relu'), False),                    # kdim = 4352: refused
    (fwd(2, 64, 6, 7, 5, 2, 1, 1), False),                            # cout 5 (32 lanes): not thin
]

# --------------------------------------------------------------------------------------------------------- D. B-resident
# (case, switches, variant, build).  bres_all takes every eligible launch, HND_BRES2=0 keeps the one-wave kernel away.
# build = (waves, WN, KQ): the template build (csrc/conv_bres.hip: launch_bres); WN = 64-column slices per workgroup, KQ =
# K / 64.  With 256 compute units a slice width bn gives 8 * (32 / (cout / bn)) teams; the 8-wave kernel wants 2 * (8 / WN)
# chunks of 64 rows per team, the one-wave kernel (bres_all) 2 * (4 / WN): every case sits in the LAST 64 rows below that
# count (bres_min_rows), so its last chunk is ragged and 64 rows fewer fall to the tiled kernel.
BRES8_ENV = {'HND_DEBUG_PICKER': 'bres_all', 'HND_BSTREAM': '0', 'HND_BRES2': '0'}
BRES1_ENV = {'HND_DEBUG_PICKER': 'bres_all', 'HND_BSTREAM': '0'}
BRES_OFF_ENV = {'HND_BRES': '0', 'HND_BSTREAM': '0'}
BRES_CASES = [
    (fwd(2, 64, 141, 230, 1024, 1, 2, 0), BRES8_ENV, 'bres_128', (8, 2, 1)),        # stride 2, odd h: 71 x 115 outputs
    (fwd(2, 128, 71, 115, 1024, 1), BRES8_ENV, 'bres_128', (8, 2, 2)),
    (fwd(2, 128, 71, 115, 1024, 1, epi='eb+r1+mout'), BRES8_ENV, 'bres_128', (8, 2, 2)),
    (fwd(2, 128, 71, 115, 1024, 1, epi='r1+up+relu'), BRES8_ENV, 'bres_128', (8, 2, 2)),
    (fwd(2, 128, 71, 115, 1024, 1, pro='relu', epi='es+eb+mask'), BRES8_ENV, 'bres_128', (8, 2, 2)),
    (fwd(2, 256, 71, 115, 1024, 1), BRES8_ENV, 'bres_128', (8, 2, 4)),
    (fwd(7, 256, 513, 73, 64, 1), BRES8_ENV, 'bres_64', (8, 1, 4)),
    (fwd(2, 512, 63, 65, 2048, 1, pro='shift'), BRES8_ENV, 'bres_64', (8, 1, 8)),
    (fwd(2, 128, 63, 65, 1024, 1), BRES1_ENV, 'bres2_128', (1, 2, 2)),
    (fwd(2, 128, 63, 65, 1024, 1, epi='r1'), BRES1_ENV, 'bres2_128', (1, 2, 2)),    # its residual build
    (fwd(2, 128, 63, 65, 1024, 1, pro='relu'), BRES1_ENV, 'bres2_128', (1, 2, 2)),  # its prologue build
    (fwd(2, 256, 63, 65, 1024, 1, epi='es+eb+relu+mout'), BRES1_ENV, 'bres2_128', (1, 2, 4)),
    (fwd(2, 256, 255, 257, 64, 1), BRES1_ENV, 'bres2_64', (1, 1, 4)),
    (fwd(1, 512, 63, 65, 2048, 1), BRES1_ENV, 'bres2_64', (1, 1, 8)),
]
BRES_BUILDS = {(8, 2, 1), (8, 2, 2), (8, 2, 4), (8, 1, 4), (8, 1, 8), (1, 2, 2), (1, 2, 4), (1, 1, 4), (1, 1, 8)}


def bres_min_rows(cout, wn, waves):
    """bres_variant's rule restated for 256 compute units: the fewest rows whose 64-row chunks give every team its count"""
    nsl = cout // (64 * wn)
    teams = 8 * (COMPUTE_UNITS // 8 // nsl)
    return (2 * ((8 if waves == 8 else 4) // wn) * teams - 1) * 64 + 1


# --------------------------------------------------------------------------------------------------------- E. B-streamed
# (case, variant, relay).  bstream_all, HND_BRES=0.  bstream_64: the 256 x 64 block tile (one wave column, cout % 128 != 0),
# bstream_128: 128 x 128.  Each wave-column build in its four forms -- taps or not, prologue or not -- at K = 256 (the
# minimum), 384 and 1152 (cin 128 over 3x3 taps, stride 1 and 2, on 5x7 and 8x9 maps: the padding is a zero AFTER the
# prologue).  relay: the launch has at least one tile per workgroup and reports a workspace.  The first relay row is the
# smallest such launch (256 tiles of 128 rows; 64 rows fewer report none); at that size every workgroup owns exactly one
# tile and nothing is parked, so the second has 257 tiles of K = 384: 771 units over 256 workgroups split tiles.
BSTREAM_ENV = {'HND_DEBUG_PICKER': 'bstream_all', 'HND_BRES': '0'}
BSTREAM_OFF_ENV = {'HND_BRES': '0', 'HND_BSTREAM': '0'}
BSTREAM_CASES = [
    (fwd(2, 256, 5, 7, 64, 1), 'bstream_64', False),
    (fwd(2, 256, 8, 9, 128, 1), 'bstream_128', False),
    (fwd(2, 256, 8, 9, 64, 1, pro='relu'), 'bstream_64', False),
    (fwd(2, 256, 5, 7, 128, 1, pro='shift', epi='es+eb+r1+mask+relu'), 'bstream_128', False),
    (fwd(2, 384, 5, 7, 128, 1), 'bstream_128', False),
    (fwd(2, 384, 8, 9, 64, 1, pro='scale', epi='r1+up'), 'bstream_64', False),
    (fwd(2, 128, 5, 7, 64, 3, 1, 1), 'bstream_64', False),
    (fwd(2, 128, 5, 7, 128, 3, 2, 1, epi='eb+r1+r2'), 'bstream_128', False),
    (fwd(2, 128, 8, 9, 64, 3, 2, 1, pro='relu'), 'bstream_64', False),
    (fwd(2, 128, 8, 9, 128, 3, 1, 1, pro='relu'), 'bstream_128', False),
    (fwd(2, 128, 8, 9, 64, 3, 1, 1, pro=SCALE_RELU, epi='es+relu'), 'bstream_64', False),
    (fwd(3, 256, 100, 109, 128, 1), 'bstream_128', True),             # 32700 rows: 256 tiles
    (fwd(3, 384, 95, 115, 128, 1, pro='relu', epi='eb'), 'bstream_128', True),      # 32775 rows: 257 tiles, split tiles
]


def bstream_tiles(c):
    f = fwd_fields(c)
    wn = 2 if f['cout'] % 128 == 0 else 1
    return -(-rows_of(c) // (64 * (4 // wn))) * (f['cout'] // (64 * wn))


# cases whose fp64 CPU convolution takes longer than about a second get their reference from torch in fp64 on the device
# (a plain matrix product: all of them are 1x1) and are left out of the CPU file's fp32 check
def heavy(c):
    return rows_of(c) * c.kh * c.kw * c.cin * c.cout > 1.2e9


# --------------------------------------------------------------------------------------------------------- F. data gradient
# ops.conv_dgrad of nn.Conv2d(cin -> cout, k, stride, pad) on an h x w input: dy [n, oh, ow, lanes(cout)] -> dx [n, h, w,
# lanes(cin)]; stride 2 is one launch per output parity.  opts: 'acc' accumulate on a seeded base (required where a parity
# has no tap), 'pro' / 'fold' the per-channel scale of dy as a prologue / folded into the packed weights, 'mask' / 'bits' the
# mask as floats / nibbles.  Launch i runs on block tile (index + i) % 4 unless its shape takes thin_n4 or the 4-lane tile.
Dgrad = collections.namedtuple('Dgrad', 'n cin h w cout k stride pad opts')
DGRAD_ENV = {'HND_BRES': '0', 'HND_BSTREAM': '0'}


def dg(n, cin, h, w, cout, k, stride=1, pad=0, opts=''):
    assert set(opts_of(opts)) <= {'acc', 'pro', 'fold', 'mask', 'bits'}
    return Dgrad(n, cin, h, w, cout, k, stride, pad, opts)


def opts_of(opts):
    return frozenset(o for o in opts.split('+') if o)


_STRIDED = [(1, 2, 0), (2, 2, 0), (3, 2, 0), (3, 2, 1), (4, 2, 0), (4, 2, 1), (5, 2, 0), (7, 2, 3)]        # table A's (k, stride, pad)
DGRAD_CASES = (
    [dg(2, 32, h, w, 64, k, s, p, 'acc' if k == 1 else '') for k, s, p in _STRIDED for h, w in ((9, 12), (10, 11))] +
    [dg(1, 32, 8, 8, 64, 3, 2, 0), dg(1, 32, 9, 9, 64, 4, 2, 0),                   # leftover rows and columns: exact zeros
     dg(2, 32, 9, 12, 64, 1, 2, 0, 'acc+mask'),                                     # tap-less parities keep the base's bits
     dg(2, 32, 1, 9, 64, 3, 2, 1), dg(2, 32, 8, 1, 64, 3, 2, 1),                    # an empty parity class
     dg(1, 32, 11, 14, 64, 7, 2, 3),                                                # (k = 7 stride 2 pad 3, cin 32: the k loop above too)
     dg(2, 3, 9, 11, 64, 2, 1, 0), dg(2, 3, 9, 11, 128, 2, 1, 1, 'pro'),            # dx in 4 lanes: thin_n4
     dg(2, 3, 9, 11, 16, 2, 1, 1), dg(2, 4, 8, 10, 3, 2, 1, 1),                     # ... the tiled kernel, the 4-lane tile
     dg(2, 32, 6, 7, 64, 2, 1, 1), dg(2, 96, 6, 7, 100, 3, 1, 1),
     dg(2, 128, 9, 10, 64, 3, 2, 1), dg(1, 128, 8, 9, 64, 3, 2, 0),                 # strided outputs on the 128-column tiles
     dg(1, 32, 8, 8, 64, 3, 2, 0, 'acc'), dg(1, 32, 9, 8, 64, 4, 2, 0, 'acc+mask'), # unread pixels inside a written parity
     dg(2, 32, 9, 10, 64, 3, 2, 1, 'fold'), dg(2, 32, 9, 10, 64, 3, 2, 1, 'pro'),   # the folded scale against the prologue form
     dg(2, 32, 8, 9, 64, 3, 1, 1, 'mask'), dg(2, 32, 8, 9, 64, 3, 1, 1, 'bits'),
     dg(2, 32, 9, 10, 64, 3, 2, 1, 'acc+fold+bits')])


def tap_classes(k, stride, pad):
    """per output parity: (i0, istep, ni, bh) of the taps that reach it (ops.dgrad_tap_classes restated)"""
    out = []
    for ph in range(stride):
        i0 = (ph + pad) % stride
        out.append((i0, stride, len(range(i0, k, stride)), (ph + pad - i0) // stride))
    return out


def dgrad_launches(c):
    """[(ph, pw, fields)] of the launches ops.conv_dgrad builds for a case, in its order"""
    o, out = opts_of(c.opts), []
    oh, ow = out_extent(c.h, c.k, c.stride, c.pad), out_extent(c.w, c.k, c.stride, c.pad)
    cl, ldc = lanes(c.cout), lanes(c.cin)
    ptrs = ({'pro_scale', 'pro_shift'} if 'pro' in o else set()) | ({'res1'} if 'acc' in o else set())
    ptrs |= ({'mask'} if 'mask' in o else set()) | ({'mask_bits'} if 'bits' in o else set())
    classes = tap_classes(c.k, c.stride, c.pad)
    for ph, (i0, _, ni, bh) in enumerate(classes):
        for pw, (j0, _, nj, bw) in enumerate(classes):
            ohv, owv = len(range(ph, c.h, c.stride)), len(range(pw, c.w, c.stride))
            if ni == 0 or nj == 0 or ohv == 0 or owv == 0:
                assert ni and nj or 'acc' in o
                continue
            out.append((ph, pw, dict(n=c.n, h=oh, w_=ow, cin=cl, oh=ohv, ow=owv, yh=c.h, yw=c.w, cout=ldc, ldc=ldc, y_sh=c.stride,
                                     y_oh=ph, y_sw=c.stride, y_ow=pw, kh=ni, kw=nj, sh=1, dh=-1, bh=bh, sw=1, dw=-1, bw=bw,
                                     kdim=round_up(ni * nj * cl, 32), pro_relu=0, relu=0, res1_mode=0, res1_h=0, res1_w=0,
                                     w_group_rows=0, w_group_stride=0, ptrs=frozenset(ptrs))))
    return out


def dgrad_variant(f, tile):
    """which kernel a data-gradient launch takes under DGRAD_ENV and igemm_tile=tile (pick_conv's order restated)"""
    if f['cin'] == 4:
        return 'igemm_c4_128x64'
    if f['cin'] % 64 == 0 and f['cout'] <= 4 and not f['ptrs'] & {'mask_bits', 'mask_out'} and f['kdim'] <= 4096:
        return 'thin_n4'
    return tiled_name(tile, f['cout'])


def dgrad_plan(c, index):
    """[(ph, pw, fields, switches, variant)]"""
    return [(ph, pw, f, dict(DGRAD_ENV, HND_DEBUG_PICKER='igemm_tile=%d' % ((index + i) % 4)), dgrad_variant(f, (index + i) % 4))
            for i, (ph, pw, f) in enumerate(dgrad_launches(c))]


@functools.lru_cache(maxsize=None)
def dgrad_case(c):
    """(operands, dx64, B64, K map) of a data-gradient case: dx64 = conv2d_input in fp64 of dy (times the scale s where the
    case has one: as a prologue on dy or folded into w, the same in exact arithmetic), + base with 'acc', masked where a launch writes; B64 the
    same on magnitudes; K = ni nj cout of the parity class that writes the element."""
    o = opts_of(c.opts)
    g = torch.Generator().manual_seed(47000 + sum((i + 1) * v for i, v in enumerate(c[:8])) + sum(ord(ch) for ch in c.opts))
    oh, ow = out_extent(c.h, c.k, c.stride, c.pad), out_extent(c.w, c.k, c.stride, c.pad)
    t = {'dy': _nchw_rand(g, c.n, c.cout, oh, ow), 'w': torch.randn(c.cout, c.cin, c.k, c.k, generator=g) / math.sqrt(c.cout * c.k * c.k)}
    w64 = t['w'].double()
    if o & {'pro', 'fold'}:
        t['s'] = (torch.rand(c.cout, generator=g) + 0.5) * torch.where(torch.rand(c.cout, generator=g) < 0.25, -1.0, 1.0)
        w64 = w64 * t['s'].double()[:, None, None, None]
    size = (c.n, c.cin, c.h, c.w)
    dx = torch.nn.grad.conv2d_input(size, w64, t['dy'].double(), stride=c.stride, padding=c.pad)
    b = torch.nn.grad.conv2d_input(size, w64.abs(), t['dy'].double().abs(), stride=c.stride, padding=c.pad)
    if 'acc' in o:
        t['base'] = _nchw_rand(g, *size)
        dx, b = dx + t['base'].double(), b + t['base'].double().abs()
    if o & {'mask', 'bits'}:
        t['mask'] = _nchw_rand(g, *size)
        dx = torch.where((t['mask'] > 0) | ~written_map(c), dx, torch.zeros_like(dx))
    kmap = torch.zeros(c.h, c.w, dtype=torch.float64)
    classes = tap_classes(c.k, c.stride, c.pad)
    for ph, (_, _, ni, _) in enumerate(classes):
        for pw, (_, _, nj, _) in enumerate(classes):
            kmap[ph::c.stride, pw::c.stride] = ni * nj * c.cout
    return t, dx, b, kmap[None, None]


def dgrad_fp32(c, t):
    """torch's own fp32 CPU evaluation of the same data gradient"""
    o, dy, w = opts_of(c.opts), t['dy'], t['w']
    if 'pro' in o:
        dy = dy * t['s'][None, :, None, None]
    if 'fold' in o:
        w = w * t['s'][:, None, None, None]
    dx = torch.nn.grad.conv2d_input((c.n, c.cin, c.h, c.w), w, dy.contiguous(), stride=c.stride, padding=c.pad)
    if 'acc' in o:
        dx = dx + t['base']
    return torch.where((t['mask'] > 0) | ~written_map(c), dx, torch.zeros_like(dx)) if 'mask' in t else dx


def written_map(c):
    """bool [h, w]: the pixels some launch of the case writes (a parity class without a tap has none: its pixels keep the
    base, mask or no mask)"""
    hit = torch.zeros(c.h, c.w, dtype=torch.bool)
    for ph, pw, _ in dgrad_launches(c):
        hit[ph::c.stride, pw::c.stride] = True
    return hit


def untouched(c):
    """bool [h, w]: input pixels no output pixel of the conv reads (their data gradient is an exact 0, or the base)"""
    oh, ow = out_extent(c.h, c.k, c.stride, c.pad), out_extent(c.w, c.k, c.stride, c.pad)
    rows = torch.ones(c.h, dtype=torch.bool)
    cols = torch.ones(c.w, dtype=torch.bool)
    for i in range(c.k):
        for o_, ext, hit in ((oh, c.h, rows), (ow, c.w, cols)):
            for p in range(o_):
                q = p * c.stride + i - c.pad
                if 0 <= q < ext:
                    hit[q] = False
    return rows[:, None] | cols[None, :]


# --------------------------------------------------------------------------------------------------------- G. padding lanes
# x lanes beyond cin_real (3 in 4, 12 in 32, 100 in 128) and dy lanes beyond cout hold 3e4 instead of 0: the packed operand
# has zero rows there, so the output is the same bits.  include/hnd_hip.h asks no caller to zero the padding lanes of x, dy
# or any other operand of hnd_conv_desc, so every case stands.  (case, switches, variant)
PAD_LANE_FWD = [
    (fwd(2, 3, 6, 7, 64, 2, 1, 1, pro='relu'), {}, 'igemm_c4_128x64'),
    (fwd(1, 3, 9, 13, 64, 7, 2, 3), {}, 'stem7_lds'),
    (fwd(2, 12, 5, 7, 64, 3, 1, 1), tiled_env(3), 'igemm_64x64'),
    (fwd(2, 100, 5, 7, 128, 3, 1, 1, pro='relu'), tiled_env(0), 'igemm_128x128'),
    (fwd(2, 100, 5, 7, 3, 1), {}, 'thin_n4'),
]
PAD_LANE_DGRAD = [dg(2, 32, 6, 7, 3, 2, 1, 1), dg(2, 32, 6, 7, 12, 3, 1, 1), dg(2, 3, 6, 7, 100, 3, 1, 1), dg(2, 32, 9, 10, 100, 3, 2, 1)]


# --------------------------------------------------------------------------------------------------------- routing

def routing():
    """every (label, switches, descriptor fields, variant, relay) the GPU file launches; relay: the launch must report a
    workspace (every other one must report none)"""
    out = []
    for c in TILED_CASES:
        for tile in range(4):
            out.append(('tiled %s tile %d' % (case_id(c), tile), tiled_env(tile), fwd_fields(c), tiled_variant(c, tile), False))
    for c, env, variant in C4_CASES + PAD_LANE_FWD:
        out.append(('c4 / pad lanes %s' % case_id(c), env, fwd_fields(c), variant, False))
    for row in STEM_CASES:
        c = stem_case(row)
        out.append(('stem %s' % case_id(c), {}, fwd_fields(c), 'stem7_lds', False))
        out.append(('stem %s, stem off' % case_id(c), {'HND_STEM7': '0'}, fwd_fields(c), 'igemm_c4_128x64', False))
    for c, taken in THIN_CASES:
        out.append(('thin %s' % case_id(c), {}, fwd_fields(c), 'thin_n4' if taken else None, False))
        out.append(('thin %s, thin off' % case_id(c), {'HND_THIN_N': '0'}, fwd_fields(c), None, False))
    for c, env, variant, _ in BRES_CASES:
        out.append(('bres %s' % case_id(c), env, fwd_fields(c), variant, False))
        out.append(('bres %s, bres off' % case_id(c), BRES_OFF_ENV, fwd_fields(c), None, False))
    for c, variant, relay in BSTREAM_CASES:
        out.append(('bstream %s' % case_id(c), BSTREAM_ENV, fwd_fields(c), variant, relay))
        out.append(('bstream %s, bstream off' % case_id(c), BSTREAM_OFF_ENV, fwd_fields(c), None, False))
    for i, c in enumerate(DGRAD_CASES + PAD_LANE_DGRAD):
        for ph, pw, f, env, variant in dgrad_plan(c, i):
            out.append(('dgrad %s parity %d %d' % (case_id(c), ph, pw), env, f, variant, False))
    return out
