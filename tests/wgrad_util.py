"""The weight-gradient wall: the case tables, the fp64 reference and the two bars shared by tests/test_wgrad_cases_cpu.py
(routing, ring builds, coverage conditions: no GPU) and tests/test_wgrad_gpu.py (the launches).  Nothing here imports the
library or touches a device; both files read the SAME tuples, so a geometry the CPU file routed is the one the GPU runs.

hnd_conv2d_wgrad dispatches to four partial-sum kernels (csrc/conv_wgrad.hip: pick_wgrad) and the ring kernel to one of
eight template builds (csrc/conv_wgrad_ring.hip: wring_plan).  A logical channel count c is stored as in the product:
cin 3 / 4 as 4 lanes, anything else as a multiple of 32; dy with a channel stride of cout rounded up to 4."""
import functools
import random

import torch
import torch.nn.functional as F

PRO_FORMS = ('none', 'scale', 'shift', 'relu')      # no prologue / scale only / scale + shift / scale + shift + ReLU
SCALE_RELU = 'srelu'                                # and scale + ReLU with no shift: the ReLU must not hang on the shift
ALL_FORMS = PRO_FORMS + (SCALE_RELU,)
VARIANT_CODE = {'wgrad_m64': 0, 'wgrad_m128': 0, 'stem7_wgrad': 1, 'thin_wgrad': 2, 'wgrad_ring': 3}
KERNELS = ('wgrad_m64', 'wgrad_m128', 'wgrad_ring', 'thin_wgrad', 'stem7_wgrad')
PICKER_TAPS = 'wgrad_ring_taps'                     # HND_DEBUG_PICKER key: the ring kernel also takes the tap form
U = 2.0 ** -24                                      # unit roundoff of fp32


def staged_name(cout):
    return 'wgrad_m128' if cout >= 128 else 'wgrad_m64'


def cin_lanes(cin):
    return 4 if cin <= 4 else (cin + 31) // 32 * 32


def dy_lanes(cout):
    return (cout + 3) // 4 * 4


def out_extent(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


# --------------------------------------------------------------------------------------------------------- reference

def reference(x, dy, k, stride, pad, ps=None, pb=None, relu=False):
    """(dw64, S64) for fp32 NCHW x [n, cin, h, w] and dy [n, cout, oh, ow]: dw64 the fp64 weight gradient of
    conv2d(a, W), a = relu?(x * ps + pb), every operation in fp64 on the fp32 inputs; S64 the same contraction on
    magnitudes, sum_m |dy| (|x ps| + |pb|) (sum |dy| |x| without a prologue), in the shape of dw."""
    x64, dy64 = x.double(), dy.double()
    a, mag = x64, x64.abs()
    if ps is not None:
        a = x64 * ps.double()[None, :, None, None]
        mag = a.abs()
        if pb is not None:
            a = a + pb.double()[None, :, None, None]
            mag = mag + pb.double().abs()[None, :, None, None]
    if relu:
        a = a.clamp_min(0.0)
    shape = (dy.shape[1], x.shape[1], k, k)
    dw64 = torch.nn.grad.conv2d_weight(a, shape, dy64, stride=stride, padding=pad)
    s64 = torch.nn.grad.conv2d_weight(mag, shape, dy64.abs(), stride=stride, padding=pad)
    return dw64, s64


def grouped_reference(xs, dys):
    """the grouped 1x1 form (the Winograd-domain reductions): xs [g, tiles, cin], dys [g, tiles, cout] fp32 ->
    (dw64, S64) [g, cout, cin]"""
    return (torch.einsum('gtc,gtd->gdc', xs.double(), dys.double()),
            torch.einsum('gtc,gtd->gdc', xs.double().abs(), dys.double().abs()))


def bars(got, dw64, s64, m):
    """(relative-to-max error, worst ratio of |got - dw64| to the element-wise bound (m + 8) 2^-24 S64 + 1e-30).
    The first is the project's bar for fp32-MFMA convs (< 1e-4).  The second holds for ANY summation order: each fp32
    prologue value is within 2u (|x ps| + |pb|) of the fp64 one, ReLU is 1-Lipschitz, a length-m fp32 dot product is
    within gamma_m sum |terms|, and the + 8 absorbs the prologue and second-order terms; it must be <= 1."""
    err = (got.double() - dw64).abs()
    return float(err.max() / (dw64.abs().max() + 1e-30)), float((err / ((m + 8) * U * s64 + 1e-30)).max())


@functools.lru_cache(maxsize=None)
def conv_inputs(n, cin, h, w, cout, k, stride, pad, pro):
    """seeded fp32 inputs of one case and their reference, computed once per geometry and prologue form and shared:
    (x, dy, ps, pb, relu, dw64, S64, M).  ps carries both signs (a BatchNorm weight may be negative)."""
    g = torch.Generator().manual_seed(9000 + 7 * sum((n, cin, h, w, cout, k, stride, pad)) + ALL_FORMS.index(pro))
    oh, ow = out_extent(h, k, stride, pad), out_extent(w, k, stride, pad)
    x, dy = torch.randn(n, cin, h, w, generator=g), torch.randn(n, cout, oh, ow, generator=g)
    sign = torch.where(torch.rand(cin, generator=g) < 0.25, -1.0, 1.0)
    ps = (torch.rand(cin, generator=g) + 0.5) * sign if pro != 'none' else None
    pb = torch.randn(cin, generator=g) * 0.3 if pro in ('shift', 'relu') else None
    relu = pro in ('relu', SCALE_RELU)
    dw64, s64 = reference(x, dy, k, stride, pad, ps, pb, relu)
    return x, dy, ps, pb, relu, dw64, s64, n * oh * ow


@functools.lru_cache(maxsize=None)
def grouped_inputs(groups, tiles, cin, cout):
    g = torch.Generator().manual_seed(9500 + groups + tiles + cin + cout)
    xs, dys = torch.randn(groups, tiles, cin, generator=g), torch.randn(groups, tiles, cout, generator=g)
    return (xs, dys) + grouped_reference(xs, dys) + (tiles,)


def desc_fields(n, cin, h, w, cout, k, stride, pad, pro='none', splitk=0):
    """the integer fields of the hnd_wgrad_desc of a direct conv case, and which prologue pointers it carries"""
    return dict(n=n, h=h, w_=w, cin=cin_lanes(cin), cin_real=cin, oh=out_extent(h, k, stride, pad),
                ow=out_extent(w, k, stride, pad), cout=cout, ldy=dy_lanes(cout), kh=k, kw=k, stride=stride, pad=pad,
                pro_relu=int(pro in ('relu', SCALE_RELU)), splitk=splitk, groups=0, x_group_stride=0, dy_group_stride=0, dw_group_stride=0,
                has_scale=pro != 'none', has_shift=pro in ('shift', 'relu'))


def grouped_fields(groups, tiles, cin, cout):
    return dict(n=1, h=1, w_=tiles, cin=cin, cin_real=cin, oh=1, ow=tiles, cout=cout, ldy=cout, kh=1, kw=1, stride=1, pad=0,
                pro_relu=0, splitk=0, groups=groups, x_group_stride=tiles * cin, dy_group_stride=tiles * cout,
                dw_group_stride=cout * cin, has_scale=False, has_shift=False)


# --------------------------------------------------------------------------------------------------------- A. staged
# (n, cin, h, w, cout, k, stride, pad, prologue form, splitk values).  The first fifteen geometries are the ones the
# suite never ran on this kernel: k = 1, 3x3 pad 1, 5x5, a 7x7 that is not the stem, ragged columns above one tile
# (cin 96 / 160), a row-tile tail on the 128-row build (cout 192 -> two tiles, co_pad 256), the three partial cases of the
# scalar channel-tail loader (cout % 4 = 1, 2, 3), and a reduction of fewer / exactly / barely more pixels than one k-step.
STAGED_ENV = {'HND_WGRAD_RING': '0', 'HND_THIN_WGRAD': '0', 'HND_STEM7': '0'}
_STAGED_HAND = [
    (2, 256, 9, 11, 64, 1, 1, 0, 'none', (0, 1, 3)),          # k = 1
    (2, 64, 9, 12, 128, 1, 2, 0, 'scale', (0,)),              # 1x1 stride 2, even and odd extent
    (2, 64, 16, 20, 64, 3, 1, 1, 'none', (0, 1, 3, 40)),      # 3x3 stride 1 pad 1, all prologue forms; 40 slabs: the reduce
    (2, 64, 16, 20, 64, 3, 1, 1, SCALE_RELU, (0,)),           # kernel's unrolled loop (one k-step per split)
    (2, 64, 16, 20, 64, 3, 1, 1, 'scale', (0,)),
    (2, 64, 16, 20, 64, 3, 1, 1, 'shift', (0,)),
    (2, 64, 16, 20, 64, 3, 1, 1, 'relu', (0,)),
    (2, 128, 17, 21, 128, 3, 2, 1, 'shift', (0, 1, 3)),       # 3x3 stride 2 pad 1, odd extents
    (2, 128, 16, 20, 128, 3, 2, 1, 'relu', (0,)),             # ... even extents
    (1, 32, 11, 13, 64, 5, 1, 2, 'none', (0, 1, 3)),          # 5x5
    (2, 32, 19, 23, 64, 7, 2, 3, 'scale', (0, 1, 3)),         # 7x7 that is not the stem
    (2, 96, 10, 12, 192, 3, 1, 1, 'none', (0, 1, 3)),         # ragged ncols; row-tile tail on m128; all four forms
    (2, 96, 10, 12, 192, 3, 1, 1, 'scale', (0,)),
    (2, 96, 10, 12, 192, 3, 1, 1, 'shift', (0,)),
    (2, 96, 10, 12, 192, 3, 1, 1, 'relu', (0,)),
    (2, 160, 9, 9, 100, 1, 1, 0, 'shift', (0,)),              # cin 160
    (2, 64, 8, 10, 5, 2, 1, 1, 'relu', (0, 1, 3)),            # cout % 4 == 1, ldy 8
    (2, 64, 8, 10, 6, 2, 1, 1, 'none', (0,)),                 # cout % 4 == 2, ldy 8
    (2, 64, 8, 10, 7, 2, 1, 1, 'scale', (0,)),                # cout % 4 == 3, ldy 8
    (1, 64, 4, 4, 64, 2, 1, 0, 'shift', (0, 1, 3)),           # M = 9: one partial k-step
    (1, 64, 5, 5, 64, 2, 1, 0, 'relu', (0,)),                 # M = 16: exactly one k-step
    (1, 64, 5, 6, 64, 2, 1, 0, 'none', (0, 1000)),            # M = 20; splitk 1000 > 2 steps: empty splits dropped
    (2, 3, 12, 14, 64, 2, 1, 0, 'relu', (0,)),                # cin 3 stored as 4
    (2, 3, 21, 25, 64, 7, 2, 3, 'none', (0, 1, 3)),           # the stem's geometry on this kernel, below one tile
    (2, 64, 14, 18, 64, 4, 2, 0, 'scale', (0,)),              # 4x4 stride 2 (neural filter)
    (1, 32, 13, 15, 16, 4, 2, 1, 'shift', (0,)),              # 4x4 stride 2 pad 1, cout 16
]


def _staged_drawn(count=6, seed=20261019):
    rng, out = random.Random(seed), []
    while len(out) < count:
        k, stride = rng.choice((1, 2, 3, 5)), rng.choice((1, 2))
        pad = rng.randint(0, k // 2)
        n, cin, cout = rng.choice((1, 2, 3)), rng.choice((32, 64, 96, 160)), rng.randint(1, 200)
        h, w = rng.randint(k, 14), rng.randint(k, 14)
        out.append((n, cin, h, w, cout, k, stride, pad, rng.choice(PRO_FORMS), (0, 1, 3) if len(out) % 3 == 0 else (0,)))
    return out


STAGED_CASES = _STAGED_HAND + _staged_drawn()

# --------------------------------------------------------------------------------------------------------- B. ring
# build = (ah, bh, taps, x2, narrow): the template build wring_plan chooses (csrc/conv_wgrad_ring.hip); None where the
# geometry must fall to the staged kernel.  picker: HND_DEBUG_PICKER=wgrad_ring_taps is set (the tap form is off by default).
# (n, cin, h, w, cout, k, stride, pad, prologue form, picker, expected kernel, build)
RING_CASES = [
    (2, 128, 9, 11, 128, 1, 1, 0, 'none', False, 'wgrad_ring', (1, 1, False, False, False)),
    (2, 256, 9, 11, 128, 1, 1, 0, 'none', False, 'wgrad_ring', (1, 2, False, False, False)),
    (2, 128, 9, 11, 256, 1, 1, 0, 'none', False, 'wgrad_ring', (2, 1, False, False, False)),
    (2, 256, 9, 11, 256, 1, 1, 0, 'none', False, 'wgrad_ring', (2, 2, False, False, False)),
    (2, 64, 9, 11, 256, 1, 1, 0, 'none', False, 'wgrad_ring', (1, 1, False, False, True)),       # narrow
    (2, 128, 9, 11, 256, 3, 1, 1, 'relu', True, 'wgrad_ring', (2, 1, True, False, False)),       # tap <2,1>, prologue
    (2, 128, 17, 21, 128, 3, 2, 1, 'none', True, 'wgrad_ring', (1, 1, True, True, False)),       # stride 2: taps x2
    (2, 64, 9, 9, 256, 2, 1, 1, 'shift', True, 'wgrad_ring', (2, 2, True, False, False)),        # tap <2,2>
    (2, 128, 9, 12, 128, 1, 2, 0, 'scale', True, 'wgrad_ring', (1, 1, True, True, False)),       # 1x1 stride 2 is a tap form
    (2, 64, 9, 9, 128, 2, 1, 0, SCALE_RELU, True, 'wgrad_ring', (1, 1, True, True, False)),      # ReLU without a shift
    (2, 64, 9, 3, 256, 2, 1, 1, 'relu', True, 'wgrad_ring', (2, 2, True, False, False)),         # ow == 4: a wrap every k-step
    (2, 64, 9, 2, 256, 2, 1, 1, 'relu', True, 'wgrad_m128', None),                               # ow == 3: not the ring
    (1, 64, 4, 6, 128, 2, 1, 0, 'none', True, 'wgrad_ring', (1, 1, True, True, False)),          # M = 15 < 32: splits clamped
    (1, 128, 3, 5, 256, 1, 1, 0, 'none', False, 'wgrad_ring', (2, 1, False, False, False)),      # ... on the 1x1 form
]
# (groups, tiles, cin, cout, build): the grouped Winograd-domain form, tiles ragged against the 32-pixel ring block
GROUPED_CASES = [
    (3, 77, 128, 256, (2, 1, False, False, False)),
    (3, 77, 64, 256, (1, 1, False, False, True)),
]
REACHABLE_BUILDS = {(1, 1, False, False, False), (1, 2, False, False, False), (2, 1, False, False, False),
                    (2, 2, False, False, False), (1, 1, False, False, True), (2, 1, True, False, False),
                    (2, 2, True, False, False), (1, 1, True, True, False)}


def ring_build(cin, cout, k, stride, pad):
    """wring_plan's rule restated: (ah, bh, taps, x2, narrow)"""
    taps = k * k > 1 or pad != 0 or stride != 1
    narrow = (not taps) and cin == 64 and cout % 256 == 0
    small = (taps and cout % 256 != 0) or narrow
    ah = 2 if cout % 256 == 0 and not small else 1
    bh = 2 if (k * k * cin) % 256 == 0 and not small else 1
    return ah, bh, taps, taps and ah == 1 and bh == 1 and cout % 256 != 0, narrow


def ring_takes(cin, cout, k, stride, pad):
    """the channel part of wgrad_ring_applies for a dense conv with no channel padding"""
    if cout % 128 or cin % 64:
        return False
    return (k * k * cin) % 128 == 0 or ring_build(cin, cout, k, stride, pad)[4]


# --------------------------------------------------------------------------------------------------------- C. thin
# 2x2 stride 1: (n, cin, h, w, cout, pad, prologue form, expected kernel under HND_THIN_WGRAD=1)
THIN_CASES = [
    (1, 64, 6, 7, 1, 1, 'relu', 'thin_wgrad'),        # conv3 form, 42 thick pixels: one block; cout 1 .. 4 in ldy 4
    (1, 64, 6, 7, 2, 0, 'none', 'thin_wgrad'),
    (1, 64, 6, 7, 3, 1, 'scale', 'thin_wgrad'),
    (1, 64, 6, 7, 4, 0, 'shift', 'thin_wgrad'),
    (1, 64, 6, 7, 3, 0, SCALE_RELU, 'thin_wgrad'),
    (2, 64, 23, 29, 3, 1, 'relu', 'thin_wgrad'),      # 1334 thick pixels: three blocks, the last one ragged
    (2, 64, 23, 29, 4, 0, 'none', 'thin_wgrad'),
    (1, 64, 2, 2, 3, 0, 'shift', 'thin_wgrad'),       # oh = ow = 1
    (1, 3, 6, 7, 64, 0, 'none', 'thin_wgrad'),        # conv4 form, cin_real 3 and 4
    (1, 4, 6, 7, 64, 1, 'relu', 'thin_wgrad'),
    (1, 3, 6, 7, 64, 1, SCALE_RELU, 'thin_wgrad'),
    (2, 3, 23, 29, 64, 1, 'scale', 'thin_wgrad'),
    (2, 4, 23, 29, 64, 0, 'shift', 'thin_wgrad'),
    (1, 3, 2, 2, 64, 0, 'relu', 'thin_wgrad'),        # oh = ow = 1
    (1, 64, 6, 7, 5, 1, 'relu', 'wgrad_m64'),         # cout 5 in ldy 8: just outside thin_wgrad_applies
]

# --------------------------------------------------------------------------------------------------------- D. stem7
# 7x7 stride 2 pad 3 -> 64: (n, cin_real, h, w).  csrc/conv_stem.hip walks output tiles of WTH x WTW = 8 x 16 pixels.
STEM_TILE = (8, 16)
STEM_CASES = [
    (1, 3, 9, 13),        # 5 x 7 outputs: below one tile in both directions
    (2, 4, 11, 9),        # 6 x 5
    (1, 3, 2, 40),        # oh == 1, two column tiles
    (2, 4, 1, 30),        # oh == 1 from a single input row
    (1, 3, 15, 33),       # 8 x 17: one full tile and a single column of the next
    (2, 4, 17, 33),       # 9 x 17: a single row and a single column beyond
]

# --------------------------------------------------------------------------------------------------------- E, F
# E: three layers of one engine sharing one workspace, default switches (n, cin, h, w, cout, k, stride, pad, form)
SHARED_CASES = [
    (2, 64, 16, 20, 64, 3, 1, 1, 'relu', 'wgrad_m64'),
    (2, 128, 9, 11, 256, 1, 1, 0, 'none', 'wgrad_ring'),
    (2, 64, 23, 29, 3, 2, 1, 1, 'relu', 'thin_wgrad'),
]
# F: padding lanes that are not zero.  (n, cin, h, w, cout, k, stride, pad, form, kernel, switches)
PAD_LANE_VALUE = 3.0e4
PAD_LANE_CASES = [
    (2, 3, 8, 9, 3, 2, 1, 1, 'none', 'wgrad_m64', STAGED_ENV),                          # cin 3 in 4 AND cout 3 in ldy 4
    (2, 64, 8, 9, 3, 2, 1, 1, 'relu', 'thin_wgrad', {'HND_THIN_WGRAD': '1'}),           # dy lanes on the conv3 form
    (2, 3, 8, 9, 64, 2, 1, 1, 'relu', 'thin_wgrad', {'HND_THIN_WGRAD': '1'}),           # x lanes on the conv4 form
    (2, 3, 8, 9, 64, 2, 1, 1, 'relu', 'wgrad_m64', STAGED_ENV),
]


def ring_env(picker, ring_on=True):
    env = {'HND_WGRAD_RING': '1' if ring_on else '0'}
    if picker:
        env['HND_DEBUG_PICKER'] = PICKER_TAPS
    return env


def routing():
    """every (label, switches, descriptor fields, expected kernel) the GPU file launches"""
    out = []
    for c in STAGED_CASES:
        for sk in c[9]:
            out.append(('staged %r splitk %d' % (c[:9], sk), STAGED_ENV, desc_fields(*c[:9], splitk=sk), staged_name(c[4])))
    for c in RING_CASES:
        f = desc_fields(*c[:9])
        out.append(('ring %r' % (c[:9],), ring_env(c[9]), f, c[10]))
        out.append(('ring %r, ring off' % (c[:9],), ring_env(c[9], False), f, staged_name(c[4])))
    for groups, tiles, cin, cout, _ in GROUPED_CASES:
        f = grouped_fields(groups, tiles, cin, cout)
        out.append(('grouped %r' % ((groups, tiles, cin, cout),), ring_env(False), f, 'wgrad_ring'))
        out.append(('grouped %r, ring off' % ((groups, tiles, cin, cout),), ring_env(False, False), f, staged_name(cout)))
    for n, cin, h, w, cout, pad, pro, expect in THIN_CASES:
        f = desc_fields(n, cin, h, w, cout, 2, 1, pad, pro)
        out.append(('thin %r' % ((n, cin, h, w, cout, pad, pro),), {'HND_THIN_WGRAD': '1'}, f, expect))
        out.append(('thin %r, thin off' % ((n, cin, h, w, cout, pad, pro),), {'HND_THIN_WGRAD': '0'}, f, staged_name(cout)))
    for n, cin, h, w in STEM_CASES:
        f = desc_fields(n, cin, h, w, 64, 7, 2, 3)
        out.append(('stem %r' % ((n, cin, h, w),), {'HND_STEM7': '1'}, f, 'stem7_wgrad'))
        out.append(('stem %r, stem off' % ((n, cin, h, w),), {'HND_STEM7': '0'}, f, 'wgrad_m64'))
    for c in SHARED_CASES:
        out.append(('shared %r' % (c[:9],), {}, desc_fields(*c[:9]), c[9]))
    for c in PAD_LANE_CASES:
        out.append(('pad lanes %r' % (c[:9],), c[10], desc_fields(*c[:9]), c[9]))
    return out


def pad_channels(t_nhwc, lanes, value=0.0):
    return t_nhwc if t_nhwc.shape[-1] == lanes else F.pad(t_nhwc, (0, lanes - t_nhwc.shape[-1]), value=value)
