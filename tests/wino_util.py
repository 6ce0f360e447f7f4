"""The Winograd wall: the case tables, the fp64 reference, the fp32 restatement and the bars shared by
tests/test_wino_cases_cpu.py (coverage conditions, host arithmetic, the reference against itself, teeth: no GPU) and
tests/test_wino_gpu.py (the launches of csrc/winograd.hip through ops.WinoConv / Wino2Conv / Wino2Wgrad and the fused
BN-backward transforms).  Nothing here loads the library or touches a device; both files read the SAME tuples.

A case describes the LAUNCH: a stride-1 correlation of an [n, cin, h, w] tensor with a k x k kernel and padding `pad` into
[n, cout, oh, ow], oh = h + 2 pad - k + 1.  For a data gradient (dgrad) the kernel is the flipped, transposed parameter
and cin / cout are the launch's own GEMM depth / output channels (the conv's cout / cin).

Reference: plain fp64 direct correlation of the fp32 operands (direct64), prologue before the zero padding, epilogue scale,
shift, res1, mask by its operand (> 0), ReLU -- the order of conv_util.fwd_reference.

Bar.  Winograd is not a reordering of the direct sum, so the direct B64 is no bound.  With the transform matrices restated
below, Bw = |A^T| [ sum_cin (|G| |g| |G|^T) . (|B^T| |d| |B|) ] |A|, then |es| Bw + |eb| + |r1|, and
    |got - y64| <= (K + T) 2^-24 Bw + 1e-30,        K = real input channels (the length of every component dot product).
T counts the sequential roundings outside the GEMM.  A 1-D stage out = M in evaluates each row as a sum of nnz(row)
terms: one rounding per product and nnz - 1 additions, and one more for a coefficient that is itself rounded (1/6, 2/9,
1/90 ... are not fp32 numbers), i.e. at most r(M) = max_row nnz(M) + 1 however the row is factorised, as long as every
intermediate is a partial sum of the row's own terms (true of every macro of winograd.hip: HND_WINO6_BT's e26_ / o15_,
HND_WINO4_AT's p12 / q34, mat_apply).  Each of the three transforms is applied twice (columns, rows), and the 8 of
conv_util.bars covers the prologue, the epilogue and second-order terms:
    T = 2 (r(B^T) + r(G) + r(A^T)) + 8.
The weight gradient dW = A'^T [ sum_tiles (G' dy G'^T) . (B^T d B) ] A' is held the same way with the roles swapped: the
reduction runs over the tiles, K = n th tw, T = 2 (r(B^T) + r(G') + r(A'^T)) + 8.  The fused BN-backward transforms are
held per element of V and Z: T_V = 2 r(B^T) + 8, T_Z = 2 r(G') + 8 (the 8: k1 d + k2 x + k3 is four roundings).

T, and the worst ratio |got - y64| / bar of the fp32 restatement (CPU, whole table) and of the kernels (MI355X), with the
case that gave it (tests/test_wino_cases_cpu.py asserts restatement <= 0.5, tests/test_wino_gpu.py asserts kernel <= 1):

    k  tile  direction   T  restatement  case                                           kernel  case
    3     2  fwd        30        0.016  3-2-0-3-32-3-5-32-1-none-es+eb-1                0.016  3-2-0-3-32-3-5-32-1-none-es+eb-1
    3     2  dgrad      30        0.006  3-2-1-2-32-3-5-256-1-scale-r1+mask-0            0.006  3-2-1-3-32-5-1-32-1-scale-0
    3     4  fwd        38        0.013  3-4-0-3-32-5-9-32-1-none-es+eb-1                0.013  3-4-0-3-32-5-9-32-1-none-es+eb-1
    3     4  dgrad      38        0.004  3-4-1-2-32-9-5-32-1-none-0                      0.003  3-4-1-2-32-5-9-256-1-scale-r1+mask-0
    3     6  fwd        46        0.012  3-6-0-3-32-7-13-32-1-none-es+eb-1               0.012  3-6-0-3-32-7-13-32-1-none-es+eb-1
    3     6  dgrad      46        0.004  3-6-1-3-32-7-13-32-1-scale-1                    0.005  3-6-1-3-32-7-13-32-1-scale-1
    2     4  fwd        34        0.025  2-4-0-3-32-5-9-32-1-scale-es+eb+stats-1         0.036  2-4-0-3-32-5-9-32-1-scale-es+eb+stats-1
    2     4  dgrad      34        0.037  2-4-1-2-32-5-9-96-1-none-0                      0.033  2-4-1-3-32-5-9-32-1-none-1
    2     4  wgrad      38        0.010  2-4-0-1-32-3-4-64-1-relu-0                      0.010  2-4-0-2-256-5-9-64-0-none-0
    2     6  fwd        42        0.037  2-6-0-2-32-7-13-32-1-scale-es+eb+relu-0         0.024  2-6-0-2-32-7-13-32-1-none-0
    2     6  dgrad      42        0.028  2-6-1-2-32-7-13-32-1-none-bwd+lin-0               0.034  2-6-1-2-64-7-13-256-1-none-bwd-0
    2     6  wgrad      50        0.003  2-6-0-1-32-5-6-64-1-relu-0                      0.003  2-6-0-1-32-5-6-64-1-relu-0
The over-cap cases (both transforms on their second trip; hnd_wino26_output_bnbwd_stats past its 2048 blocks) reach
0.001 - 0.003 on the kernels; the fused BN-backward transforms 0.138 of T_V = 22 (V) and 0.199 of T_Z = 22 (Z), both at
their over-cap case 1-1541-1536-64-0-1.  A case reads k-tile-dgrad-n-cin-oh-ow-cout-pad-pro-epi-quiet.  No kernel came
near its bar: nothing to explain, no bug found.

The transforms that no GEMM follows are also launched alone on their second trip (the weight transforms and
hnd_wino2_wgrad_output at 1600 x 1312 channels, hnd_wino2_dy at 65792 tiles) and held per element of U, dW and Z under
(2 r(G) + 8), (2 r(A'^T) + 8) and (2 r(G') + 8) roundings: worst ratios 0.292 (U), 0.146 (dW), 0.248 (Z).
"""
import collections
import functools
import math
from fractions import Fraction

import torch
import torch.nn.functional as F

from tests import conv_util as U
from tests.wgrad_util import ALL_FORMS, PRO_FORMS, SCALE_RELU

U24 = 2.0 ** -24
K_MAX_BLOCKS = 256 * 32                 # winograd.hip: kMaxBlocks
THREADS = 256
CAP = K_MAX_BLOCKS * THREADS            # work items one trip of a grid-stride loop covers (grid_for)
CAP_WINO2_OUTPUT = 2048 * THREADS       # hnd_wino2_stats_blocks caps the 2x2 output transforms at 2048 blocks
QUIET = 1e-5                            # amplitude of the quiet image of a teeth case


def _mat(rows):
    """exact rationals -> fp64 (the nearest double of each)"""
    return torch.tensor([[float(Fraction(v)) for v in r.split()] for r in rows], dtype=torch.float64)


# The matrices of csrc/winograd.hip, read off: F(2,3) lines 51-54 (G), 128-131 (B^T), 183-184 (A^T); F(4,3) lines 235, 262,
# 331; F(6,3) lines 425-430; F(4,2) lines 632-634 and, weight gradient, 834-836; F(6,2) lines 923-946 (W6_*).
MATS = {
    (3, 2): dict(BT=_mat(['1 0 -1 0', '0 1 1 0', '0 -1 1 0', '0 1 0 -1']),
                 G=_mat(['1 0 0', '1/2 1/2 1/2', '1/2 -1/2 1/2', '0 0 1']),
                 AT=_mat(['1 1 1 0', '0 1 -1 -1'])),
    (3, 4): dict(BT=_mat(['4 0 -5 0 1 0', '0 -4 -4 1 1 0', '0 4 -4 -1 1 0', '0 -2 -1 2 1 0', '0 2 -1 -2 1 0', '0 4 0 -5 0 1']),
                 G=_mat(['1/4 0 0', '-1/6 -1/6 -1/6', '-1/6 1/6 -1/6', '1/24 1/12 1/6', '1/24 -1/12 1/6', '0 0 1']),
                 AT=_mat(['1 1 1 1 1 0', '0 1 -1 2 -2 0', '0 1 1 4 4 0', '0 1 -1 8 -8 1'])),
    (3, 6): dict(BT=_mat(['1 0 -21/4 0 21/4 0 -1 0', '0 1 1 -17/4 -17/4 1 1 0', '0 -1 1 17/4 -17/4 -1 1 0',
                          '0 1/2 1/4 -5/2 -5/4 2 1 0', '0 -1/2 1/4 5/2 -5/4 -2 1 0', '0 2 4 -5/2 -5 1/2 1 0',
                          '0 -2 4 5/2 -5 -1/2 1 0', '0 -1 0 21/4 0 -21/4 0 1']),
                 G=_mat(['1 0 0', '-2/9 -2/9 -2/9', '-2/9 2/9 -2/9', '1/90 1/45 2/45', '1/90 -1/45 2/45', '32/45 16/45 8/45',
                         '32/45 -16/45 8/45', '0 0 1']),
                 AT=_mat(['1 1 1 1 1 1 1 0', '0 1 -1 2 -2 1/2 -1/2 0', '0 1 1 4 4 1/4 1/4 0', '0 1 -1 8 -8 1/8 -1/8 0',
                          '0 1 1 16 16 1/16 1/16 0', '0 1 -1 32 -32 1/32 -1/32 1'])),
    (2, 4): dict(BT=_mat(['2 -1 -2 1 0', '0 -2 -1 1 0', '0 2 -3 1 0', '0 -1 0 1 0', '0 2 -1 -2 1']),
                 G=_mat(['1/2 0', '-1/2 -1/2', '-1/6 1/6', '1/6 1/3', '0 1']),
                 AT=_mat(['1 1 1 1 0', '0 1 -1 2 0', '0 1 1 4 0', '0 1 -1 8 1']),
                 G2=_mat(['1/2 0 0 0', '-1/2 -1/2 -1/2 -1/2', '-1/6 1/6 -1/6 1/6', '1/6 1/3 2/3 4/3', '0 0 0 1']),
                 A2T=_mat(['1 1 1 1 0', '0 1 -1 2 1'])),
    (2, 6): dict(BT=_mat(['-2 4 5/2 -5 -1/2 1 0', '0 2 -2 -9/2 1/2 1 0', '0 -2 6 -7/2 -3/2 1 0', '0 1 -3/2 -2 3/2 1 0',
                          '0 -1 5/2 0 -5/2 1 0', '0 4 0 -5 0 1 0', '0 -2 4 5/2 -5 -1/2 1']),
                 G=_mat(['-1/2 0', '-1/3 -1/3', '1/9 -1/9', '1/36 1/18', '-1/60 1/30', '32/45 16/45', '0 1']),
                 AT=_mat(['1 1 1 1 1 1 0', '0 1 -1 2 -2 1/2 0', '0 1 1 4 4 1/4 0', '0 1 -1 8 -8 1/8 0', '0 1 1 16 16 1/16 0',
                          '0 1 -1 32 -32 1/32 1']),
                 G2=_mat(['-1/2 0 0 0 0 0', '-1/3 -1/3 -1/3 -1/3 -1/3 -1/3', '1/9 -1/9 1/9 -1/9 1/9 -1/9',
                          '1/36 1/18 1/9 2/9 4/9 8/9', '-1/60 1/30 -1/15 2/15 -4/15 8/15', '32/45 16/45 8/45 4/45 2/45 1/45',
                          '0 0 0 0 0 1']),
                 A2T=_mat(['1 1 1 1 1 1 0', '0 1 -1 2 -2 1/2 1'])),
}
KINDS = tuple(sorted(MATS))             # (kernel size, tile)


def roundings(m):
    """r(M) of the module docstring"""
    return int((m != 0).sum(1).max()) + 1


def t_of(k, tile):
    m = MATS[(k, tile)]
    return 2 * (roundings(m['BT']) + roundings(m['G']) + roundings(m['AT'])) + 8


def t_wgrad(tile):
    m = MATS[(2, tile)]
    return 2 * (roundings(m['BT']) + roundings(m['G2']) + roundings(m['A2T'])) + 8


def t_v(tile=6):
    return 2 * roundings(MATS[(2, tile)]['BT']) + 8


def t_z(tile=6):
    return 2 * roundings(MATS[(2, tile)]['G2']) + 8


# --------------------------------------------------------------------------------------------------------- cases
# pro: a prologue form of wgrad_util.ALL_FORMS; epi: '+'-joined operands of EPI ('mout': mask_out nibbles, 'stats': the
# per-block (sum, sum^2) partials of a Wino2Conv, 'bwd': the BN-backward partials of hnd_wino26_output_bnbwd_stats, with 'lin' for a BatchNorm without ReLU: relu_of_bn = 0);
# quiet: the last image of the batch is scaled by 1e-5 (the elements a relative-to-max bar cannot see).
EPI = ('es', 'eb', 'r1', 'mask', 'relu', 'mout', 'stats', 'bwd', 'lin')
_Case = collections.namedtuple('Case', 'k tile dgrad n cin oh ow cout pad pro epi quiet')


class Case(_Case):
    __slots__ = ()
    stride = 1

    @property
    def h(self):
        return self.oh - 2 * self.pad + self.k - 1

    @property
    def w(self):
        return self.ow - 2 * self.pad + self.k - 1

    @property
    def th(self):
        return (self.oh + self.tile - 1) // self.tile

    @property
    def tw(self):
        return (self.ow + self.tile - 1) // self.tile

    @property
    def tiles(self):
        return self.n * self.th * self.tw

    @property
    def tiles_pad(self):
        return U.round_up(self.tiles, 128)

    @property
    def ncomp(self):
        return (self.tile + self.k - 1) ** 2


def case(k, tile, dgrad, n, cin, oh, ow, cout, pad=None, pro='none', epi='', quiet=False):
    pad = 1 if pad is None else pad
    assert (k, tile) in MATS and pro in ALL_FORMS and U.epi_of(epi) <= set(EPI) and (k == 2 or pad == 1)
    c = Case(k, tile, bool(dgrad), n, cin, oh, ow, cout, pad, pro, epi, bool(quiet))
    assert c.h > 0 and c.w > 0, c
    return c


def case_id(c):
    return '-'.join(str(int(v) if isinstance(v, bool) else v) for v in c if v not in ('', None))


def lanes_out(c):
    """channel lanes the launch itself writes: cout rounded up to 4 (3x3) / 2 (2x2)"""
    return U.round_up(c.cout, 4 if c.k == 3 else 2)


def ldc_of(c):
    """the output's channel stride in the GPU file: a whole 32-lane group, so a cout that is no multiple of 32 leaves
    lanes in [lanes_out, ldc) that the launch must not touch (mask_out wants cout == ldc and gets such a cout)"""
    return U.round_up(c.cout, 32)


def extent_classes(e, t):
    """the raggedness classes an extent belongs to (tile 2: 1 is both 'one' and 'below')"""
    return {name for name, v in (('one', 1), ('below', t - 1), ('exact', t), ('above', t + 1), ('two_above', 2 * t + 1)) if v == e}


EXTENT_CLASSES = ('one', 'below', 'exact', 'above', 'two_above')


def pad_class(c):
    """where n th tw lies against the 128-row group of tiles_pad"""
    r = c.tiles % 128
    return 'on' if r == 0 else 'above' if r == 1 and c.tiles > 128 else 'below' if r == 127 else 'other'


def extents(t, least=1):
    """(oh, ow) in {1, t-1, t, t+1, 2t+1}, both orders, 1 x (t+1) among them; least: the smallest extent the launch can
    have (a 2x2 correlation with padding 1 has at least 2 outputs per direction)"""
    out = [(1, 1), (1, t + 1), (t + 1, 1), (t - 1, t), (t, t - 1), (t, t + 1), (t + 1, t), (2 * t + 1, t - 1), (t - 1, 2 * t + 1),
           (2 * t + 1, 2 * t + 1), (t, t)]
    seen = []
    for p in out:
        if min(p) >= least and p not in seen:
            seen.append(p)
    return seen


def pad_group(k, tile, dgrad, pad, **kw):
    """n th tw = 127, 128, 129: two output rows (one row of tiles), the last tile of each row partial"""
    return [case(k, tile, dgrad, 1, 32, 2, 127 * tile - 1, 32, pad, **kw), case(k, tile, dgrad, 2, 32, 2, 64 * tile - 1, 32, pad, **kw),
            case(k, tile, dgrad, 3, 32, 2, 43 * tile - 1, 32, pad, **kw)]


CHANNELS = ((64, 96), (96, 64), (256, 256), (32, 256), (256, 32), (32, 40))     # + the smallest cout below 32, per kernel size
REFUSED_DEPTH = 16                      # a GEMM depth below 32: ops refuses it ('... multiple of 32')
EPI3 = ('', 'es+eb', 'es+eb+r1+relu', 'r1', 'mout+relu')


def _epi3(tile, e):
    return e.replace('mout+', '') if tile == 2 else e        # F(2x2,3x3) has no mask_out (hnd_wino_output refuses it)


def _fwd3(tile):
    g = (2, 32, tile + 1, 2 * tile + 1, 32)
    out = [case(3, tile, False, (1, 3)[i % 2], 32, oh, ow, 32) for i, (oh, ow) in enumerate(extents(tile))]
    out += pad_group(3, tile, False, 1)
    out += [case(3, tile, False, 2, ci, tile + 1, 2 * tile + 1, co) for ci, co in CHANNELS + ((32, 1),)]
    out += [case(3, tile, False, *g, pro=p, epi=_epi3(tile, e)) for p in PRO_FORMS for e in EPI3]
    out += [case(3, tile, False, *g, pro=SCALE_RELU, epi='es+eb')]
    out += [case(3, tile, False, 3, 32, tile + 1, 2 * tile + 1, 32, epi='es+eb', quiet=True)]
    return out


DGRAD3_FORMS = (('none', ''), ('scale', ''), ('none', 'r1+mask'))


def _dgrad3(tile):
    out = [case(3, tile, True, (1, 3)[i % 2], 32, oh, ow, 32, pro=DGRAD3_FORMS[i % 3][0], epi=DGRAD3_FORMS[i % 3][1])
           for i, (oh, ow) in enumerate(extents(tile))]
    out += [case(3, tile, True, 2, 32, 2 * tile + 1, tile + 1, 32, pro=p, epi=e) for p, e in DGRAD3_FORMS]
    out += pad_group(3, tile, True, 1, pro='scale', epi='r1+mask')
    out += [case(3, tile, True, 2, ci, tile + 1, 2 * tile + 1, co, pro='scale', epi='r1+mask') for ci, co in ((64, 96), (96, 64), (256, 32), (32, 256), (32, 1))]
    out += [case(3, tile, True, 3, 32, tile + 1, 2 * tile + 1, 32, pro='scale', quiet=True)]
    return out


def _fwd2(tile, pad):
    e = extents(tile, 1 + pad)
    out = [case(2, tile, False, (1, 3)[i % 2], 32, oh, ow, 32, pad, pro='relu', epi=('stats', '')[i % 2]) for i, (oh, ow) in enumerate(e)]
    out += pad_group(2, tile, False, pad, pro='relu', epi='stats')
    out += [case(2, tile, False, 2, ci, tile + 1, 2 * tile + 1, co, pad, pro='relu', epi='' if 512 % U.round_up(co, 2) else 'stats')
            for ci, co in CHANNELS + ((32, 1),)]
    out += [case(2, tile, False, 2, 32, tile + 1, 2 * tile + 1, 32, pad, pro=p, epi=ep)
            for p, ep in (('none', ''), ('scale', 'es+eb+relu'), ('shift', 'es+eb+stats'), (SCALE_RELU, 'eb'))]
    out += [case(2, tile, False, 3, 32, tile + 1, 2 * tile + 1, 32, pad, pro='scale', epi='es+eb+stats', quiet=True)]
    return out


def _dgrad2(tile, pad):
    """pad: the launch's own padding, 1 - the conv's"""
    bwd = 'bwd' if tile == 6 else ''
    e = extents(tile, 1 + pad)
    out = [case(2, tile, True, (1, 3)[i % 2], 32, oh, ow, 32, pad, epi=(bwd, '')[i % 2]) for i, (oh, ow) in enumerate(e)]
    out += pad_group(2, tile, True, pad, epi=bwd)
    lin = bwd and 'bwd+lin'
    out += [case(2, tile, True, 2, ci, tile + 1, 2 * tile + 1, co, pad, epi=e)
            for ci, co, e in ((64, 256, bwd), (256, 64, lin), (96, 32, bwd), (32, 96, ''), (32, 32, lin), (32, 1, ''))]
    out += [case(2, tile, True, 3, 32, tile + 1, 2 * tile + 1, 32, pad, quiet=True)]
    return out


# one over-cap case per (kernel size, tile): cin = cout = 64, so the input AND the output transform (and the statistics of
# the 2x2 output transform) walk their grid-stride loop a second time; the smallest such extent with a partial last tile
def _over(k, tile):
    per = 4 if (k, tile) == (3, 2) else 2                   # channels per work item
    need = CAP // (64 // per) + 1                           # tiles
    tw = int(math.isqrt(need))
    th = -(-need // tw)
    return case(k, tile, False, 1, 64, th * tile - 1, tw * tile - 1, 64, 1 if k == 3 else 0, pro='relu', epi='es+eb' if k == 3 else 'stats')


# ... and one for hnd_wino26_output_bnbwd_stats, whose grid stops at the 2048 blocks of hnd_wino2_stats_blocks
OVER_BWD = case(2, 6, True, 1, 64, 129 * 6 - 1, 128 * 6 - 1, 64, 0, epi='bwd')
OVER_CASES = [_over(k, t) for k, t in KINDS] + [OVER_BWD]

# the transforms without a GEMM are launched alone (rows x depth of the weight, cout x cin of S): 64 a x 32 b > 2^21 needs
# a b >= 1025 = 25 x 41.  (k, tile, dgrad) / (tile, s_transposed)
OVER_ROWS, OVER_DEPTH = 25 * 64, 41 * 32
OVER_WEIGHTS = [(k, t, bool(i % 2)) for i, (k, t) in enumerate(KINDS)]
OVER_WGRAD_OUT = [(t, st) for t in (4, 6) for st in (0, 1)]
# hnd_wino2_dy: the dy of the 2x2 over-cap forward cases, (n, oh, ow, cout, tile)
OVER_DY = [(c.n, c.oh, c.ow, c.cout, c.tile) for c in OVER_CASES[:2]]


def t_u(k, tile):
    """U = G g G^T alone"""
    return 2 * roundings(MATS[(k, tile)]['G']) + 8


def t_dw(tile):
    """dW = A'^T S A' alone"""
    return 2 * roundings(MATS[(2, tile)]['A2T']) + 8


def chan_of_row(r):
    """csrc/common.h: the output channel a packed GEMM-operand row holds"""
    return (r & ~63) | ((r & 15) << 2) | ((r >> 4) & 3)


def weights_reference(w, k, tile, dgrad):
    """(U64, |G| |g| |G|^T) as [ncomp, rows, depth] by CHANNEL (not packed row) of an OIHW parameter w (any device)"""
    g = w.double()
    if dgrad:
        g = g.flip(2, 3).transpose(0, 1)
    G = MATS[(k, tile)]['G'].to(w.device)
    a = tile + k - 1
    return (torch.einsum('ia,ocab,jb->ijoc', G, g, G).reshape(a * a, g.shape[0], g.shape[1]),
            torch.einsum('ia,ocab,jb->ijoc', G.abs(), g.abs(), G.abs()).reshape(a * a, g.shape[0], g.shape[1]))


def wgrad_out_reference(s, tile):
    """(dW64, |A'^T| |S| |A'|) [cout, cin, 2, 2] of S [ncomp, cout, cin]"""
    a, A2T = tile + 1, MATS[(2, tile)]['A2T'].to(s.device)
    s = s.double().reshape(a, a, s.shape[1], s.shape[2])
    return torch.einsum('pi,ijoc,qj->ocpq', A2T, s, A2T), torch.einsum('pi,ijoc,qj->ocpq', A2T.abs(), s.abs(), A2T.abs())


def dy_reference(dy, tile):
    """(Z64, |G'| |dy| |G'|^T) [ncomp, tiles, cout] of NCHW dy (any device)"""
    G2 = MATS[(2, tile)]['G2'].to(dy.device)
    t = dy_tiles(dy.double(), tile)
    z = torch.einsum('ia,ncyxab,jb->ijnyxc', G2, t, G2)
    m = torch.einsum('ia,ncyxab,jb->ijnyxc', G2.abs(), t.abs(), G2.abs())
    return z.reshape((tile + 1) ** 2, -1, z.shape[-1]), m.reshape((tile + 1) ** 2, -1, m.shape[-1])


def wgrad_swapped(c):
    """Wino2Wgrad runs a 256 -> 64 conv with its operands swapped (s comes out transposed): ops.py, round 5"""
    return (c.cin, c.cout) == (256, 64)

TABLES = collections.OrderedDict()
for _t in (2, 4, 6):
    TABLES[(3, _t, 'fwd')] = _fwd3(_t)
    TABLES[(3, _t, 'dgrad')] = _dgrad3(_t)
for _t in (4, 6):
    TABLES[(2, _t, 'fwd')] = _fwd2(_t, 0) + _fwd2(_t, 1)
    TABLES[(2, _t, 'dgrad')] = _dgrad2(_t, 0) + _dgrad2(_t, 1)
ALL_CASES = [c for cases in TABLES.values() for c in cases]
# the teeth of the CPU file bite here: a quiet image, padding 1 (so the column past the edge is read), a partial last tile
TEETH_CASES = {(k, t): [c for c in TABLES[(k, t, 'fwd')] if c.quiet and c.pad == 1][0] for k, t in KINDS}

# weight gradient: (case of the forward conv, route, z aliases the forward's m).  'fwd': from a Wino2Conv forward, 'own':
# from a Wino2InputTransform (the 64 -> 256 route).  The prologue is the forward's (baked into V).
WGRAD_CASES = [(case(2, t, False, n, ci, oh, ow, co, pad, pro=pro), route, alias)
               for t in (4, 6) for pad in (0, 1)
               for n, ci, oh, ow, co, pro, route, alias in (
                   (3, 32, t + 1, 2 * t + 1, 32, 'relu', 'fwd', True), (1, 32, t - 1, t, 64, 'relu', 'fwd', False),
                   (2, 64, 2 * t + 1, t + 1, 256, 'shift', 'own', False), (3, 32, 2, 43 * t - 1, 32, 'none', 'own', False),
                   (2, 256, t + 1, 2 * t + 1, 64, 'none', 'own', False))]

# fused BN backward (F(6x6,2x2)): (n, oh, ow, c, pad of the data gradient, relu); oh x ow the extent of g / x / dy
BNBWD_CASES = [(n, oh, ow, c, pad, relu) for pad in (0, 1) for relu in (True, False)
               for n, oh, ow, c in ((3, 7, 13, 32), (1, 6, 7, 32), (2, 5, 6, 64), (1, 13, 2, 32), (3, 2, 43 * 6 - 1, 32))]
BNBWD_OVER = (1, 6 * 257 - 1, 6 * 256, 64, 0, True)         # 257 x 256 tiles x 32 channel pairs: one tile row above CAP


def work_items(kernel, **g):
    """work items of a transform launch, as the extern "C" wrappers of winograd.hip compute them (grid_for's argument)"""
    if kernel in ('wino_weights', 'wino2_weights'):
        return U.round_up(g['rows'], 64) * g['depth']
    if kernel in ('wino_input', 'wino_output'):
        return g['tiles'] * (g['c'] // (4 if g['tile'] == 2 else 2))
    if kernel in ('wino2_input', 'wino2_output', 'wino2_dy', 'wino26_bnbwd'):
        return g['tiles'] * (g['c'] // 2)
    if kernel == 'wino2_wgrad_out':
        return g['cout'] * g['cin']
    raise KeyError(kernel)


def conv_work(c):
    """{transform kernel: (work items, cap)} of a forward / data-gradient case"""
    name = 'wino' if c.k == 3 else 'wino2'
    return {name + '_input': (work_items(name + '_input', tiles=c.tiles, c=c.cin, tile=c.tile), CAP),
            name + '_output': (work_items(name + '_output', tiles=c.tiles, c=lanes_out(c), tile=c.tile),
                               CAP if c.k == 3 else CAP_WINO2_OUTPUT)}


def bnbwd_tiles(n, oh, ow, pad):
    """(tiles walked, tiles of V, tiles of Z) of hnd_wino26_bnbwd_transforms"""
    ih, iw = oh + 2 * pad - 1, ow + 2 * pad - 1
    thd, twd, thw, tww = (ih + 5) // 6, (iw + 5) // 6, (oh + 5) // 6, (ow + 5) // 6
    return n * max(thd, thw) * max(twd, tww), n * thd * twd, n * thw * tww


def stats_blocks(c):
    """hnd_wino2_stats_blocks restated"""
    return max(1, min(2048, (c.tiles * (lanes_out(c) // 2) + 255) // 256))


# --------------------------------------------------------------------------------------------------------- the algorithm

def direct64(a, w, pad):
    """plain fp64 stride-1 correlation of NCHW a with OIHW w: one matrix product per tap (any device, no conv library)"""
    k = w.shape[2]
    oh, ow = a.shape[2] + 2 * pad - k + 1, a.shape[3] + 2 * pad - k + 1
    ap = F.pad(a, (pad, pad, pad, pad))
    y = torch.zeros(a.shape[0], w.shape[0], oh, ow, dtype=a.dtype, device=a.device)
    for i in range(k):
        for j in range(k):
            y += torch.einsum('nchw,oc->nohw', ap[:, :, i:i + oh, j:j + ow], w[:, :, i, j])
    return y


def patches(a, k, tile, pad, edge=False):
    """[n, c, th, tw, A, A]: the (tile + k - 1)^2 input patch of every output tile, zero outside the image.
    edge (teeth 1): the last image reads the column one past its right edge as the neighbouring row's first pixel"""
    n, c, h, w = a.shape
    oh, ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    th, tw, A = (oh + tile - 1) // tile, (ow + tile - 1) // tile, tile + k - 1
    ap = F.pad(a, (pad, tw * tile + k - 1 - pad - w, pad, th * tile + k - 1 - pad - h))
    if edge:
        ap = ap.clone()
        ap[n - 1, :, pad:pad + h - 1, pad + w] = ap[n - 1, :, pad + 1:pad + h, pad]
    return ap.unfold(2, A, tile).unfold(3, A, tile)


def winograd(a, g, k, tile, pad, BT, G, AT, edge=False, full=False):
    """A^T [ sum_c (G g G^T) . (B^T d B) ] A in the dtype of the operands: transform, per-component matrix product over
    the channels, inverse transform.  full: the whole tiles, before the crop to oh x ow."""
    d = patches(a, k, tile, pad, edge)
    v = torch.einsum('ia,ncyxab,jb->ncyxij', BT, d, BT)
    u = torch.einsum('ia,ocab,jb->ocij', G, g, G)
    m = torch.einsum('ncyxij,ocij->noyxij', v, u)
    y = torch.einsum('pi,noyxij,qj->noypxq', AT, m, AT)
    n, o, th, _, tw, _ = y.shape
    y = y.reshape(n, o, th * tile, tw * tile)
    oh, ow = a.shape[2] + 2 * pad - k + 1, a.shape[3] + 2 * pad - k + 1
    return y if full else y[:, :, :oh, :ow]


def mats(k, tile, dtype=torch.float64, device='cpu', absolute=False):
    m = MATS[(k, tile)]
    return [(m[name].abs() if absolute else m[name]).to(device=device, dtype=dtype) for name in ('BT', 'G', 'AT')]


def _chan(v):
    return v[None, :, None, None]


def reference(c, t):
    """(y64, Bw) of a forward / data-gradient case on the device of the operands t (inputs' dict)"""
    e = U.epi_of(c.epi)
    a, mag = U.prologue64(t['x'], t.get('ps'), t.get('pb'), c.pro in ('relu', SCALE_RELU))
    w64 = t['w'].double()
    y = direct64(a, w64, c.pad)
    b = winograd(mag, w64.abs(), c.k, c.tile, c.pad, *mats(c.k, c.tile, device=a.device, absolute=True))
    if 'es' in e:
        y, b = y * _chan(t['es'].double()), b * _chan(t['es'].double().abs())
    if 'eb' in e:
        y, b = y + _chan(t['eb'].double()), b + _chan(t['eb'].double().abs())
    if 'r1' in e:
        y, b = y + t['r1'].double(), b + t['r1'].double().abs()
    if 'mask' in e:
        y = torch.where(t['mask'] > 0, y, torch.zeros_like(y))
    if 'relu' in e:
        y = y.clamp_min(0.0)
    return y, b


MUTATIONS = ('edge', 'wrap', 'sign', 'chan')


def restate(c, t, dtype=torch.float32, mutate=None):
    """the launch restated in plain torch in `dtype` (fp32: what a correct kernel computes up to the order of its sums;
    fp64: the algorithm itself).  mutate: one of MUTATIONS, the bugs of tests/test_wino_cases_cpu.py's teeth."""
    e = U.epi_of(c.epi)
    a, w = t['x'].to(dtype), t['w'].to(dtype)
    if 'ps' in t:
        a = a * _chan(t['ps'].to(dtype))
    if 'pb' in t:
        a = a + _chan(t['pb'].to(dtype))
    if c.pro in ('relu', SCALE_RELU):
        a = F.relu(a)
    if mutate == 'chan':                                    # teeth 4: the last input channel is dropped
        a, w = a[:, :-1], w[:, :-1]
    BT, G, AT = mats(c.k, c.tile, dtype)
    if mutate == 'sign':                                    # teeth 3: one coefficient of one row of A^T
        AT = AT.clone()
        AT[1, 2] = -AT[1, 2]
    y = winograd(a, w, c.k, c.tile, c.pad, BT, G, AT, edge=mutate == 'edge', full=True)
    if 'es' in e:
        y = y * _chan(t['es'].to(dtype))
    if 'eb' in e:
        y = y + _chan(t['eb'].to(dtype))
    whole, y = y, y[:, :, :c.oh, :c.ow]
    if mutate == 'wrap':                                    # teeth 2: the out-of-image position right of row 0 of the last
        assert whole.shape[3] > c.ow and c.oh > 1           # image's partial tile is stored: it lands on row 1, column 0
        y = y.clone()
        y[c.n - 1, :, 1, 0] = whole[c.n - 1, :, 0, c.ow]
    if 'r1' in e:
        y = y + t['r1'].to(dtype)
    if 'mask' in e:
        y = torch.where(t['mask'] > 0, y, torch.zeros_like(y))
    return F.relu(y) if 'relu' in e else y


def bars(got, y64, bw, k, t):
    """(relative-to-max error: the bar of tests/test_ops_gpu.py, < 1e-4 for tile 2 and < 2e-4 for tiles 4 / 6; worst ratio
    of |got - y64| to (K + T) 2^-24 Bw + 1e-30: <= 1)"""
    err = (got.double() - y64).abs()
    return float(err.max() / (y64.abs().max() + 1e-30)), float((err / ((k + t) * U24 * bw + 1e-30)).max())


def rel_bar(tile):
    return 1e-4 if tile == 2 else 2e-4


def _seed(c):
    return 53000 + sum((i + 1) * int(v) for i, v in enumerate(c[:9])) + 97 * ALL_FORMS.index(c.pro) + (U.hash_epi(
        '+'.join(x for x in U.epi_of(c.epi) if x in U.EPI_OPERANDS)) if c.epi else 0) + 7 * len(c.epi) + int(c.quiet)


def make_inputs(c, device='cpu'):
    """seeded fp32 operands (NCHW; x and the output-shaped operands in NHWC memory): x, w (the correlation the launch
    computes, OIHW of the launch), wp (the conv parameter ops takes: w itself, or for a data gradient the parameter whose
    flipped transpose w is), ps / pb, es / eb (eb[1] is a small shift, 1e-3), r1, mask"""
    g = torch.Generator().manual_seed(_seed(c))
    e = U.epi_of(c.epi)
    x = U._nchw_rand(g, c.n, c.cin, c.h, c.w)
    if c.quiet:
        x[c.n - 1] *= QUIET
    t = {'x': x, 'w': torch.randn(c.cout, c.cin, c.k, c.k, generator=g) / math.sqrt(c.cin * c.k * c.k)}
    t['wp'] = t['w'].flip(2, 3).transpose(0, 1).contiguous() if c.dgrad else t['w']
    ps, pb = U._prologue(g, c.cin, c.pro)
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
        t['r1'] = U._nchw_rand(g, c.n, c.cout, c.oh, c.ow)
    if 'mask' in e:
        t['mask'] = U._nchw_rand(g, c.n, c.cout, c.oh, c.ow)
    if 'bwd' in e:                                          # the BatchNorm whose backward statistics the launch also makes
        t['bsc'], t['bsh'] = torch.rand(c.cout, generator=g) + 0.5, torch.randn(c.cout, generator=g) * 0.5
        t['bmu'], t['brs'] = torch.randn(c.cout, generator=g) * 0.2, torch.rand(c.cout, generator=g) + 0.5
        t['bx'] = decided(g, U._nchw_rand(g, c.n, c.cout, c.oh, c.ow), t['bsc'], t['bsh'])
    return {k: v.to(device) for k, v in t.items()}


def decided(g, x, scale, shift, margin=1e-3):
    """x (NCHW) with every element whose |scale x + shift| < margin resampled (on the CPU, a few times over): no ReLU
    decision then depends on a rounding"""
    for _ in range(64):
        bad = (x.double() * _chan(scale.double()) + _chan(shift.double())).abs() < margin
        if not bool(bad.any()):
            return x
        x = torch.where(bad, torch.randn(x.shape, generator=g), x)
    raise AssertionError('could not draw a decided x')


def over_inputs(c, device):
    """make_inputs for the over-cap cases, drawn on `device` (150 M elements: too slow to draw on the CPU)"""
    g = torch.Generator(device=device).manual_seed(_seed(c))
    t = {'x': torch.randn(c.n, c.h, c.w, c.cin, generator=g, device=device).permute(0, 3, 1, 2),
         'w': torch.randn(c.cout, c.cin, c.k, c.k, generator=g, device=device) / math.sqrt(c.cin * c.k * c.k)}
    t['wp'] = t['w'].flip(2, 3).transpose(0, 1).contiguous() if c.dgrad else t['w']
    small = make_inputs(c._replace(oh=1 + c.pad, ow=1 + c.pad))
    t.update({k: v.to(device) for k, v in small.items() if k in ('ps', 'pb', 'es', 'eb', 'bsc', 'bsh', 'bmu', 'brs')})
    if 'bwd' in U.epi_of(c.epi):
        bx = torch.randn(c.n, c.oh, c.ow, c.cout, generator=g, device=device).permute(0, 3, 1, 2)
        pre = bx.double() * _chan(t['bsc'].double()) + _chan(t['bsh'].double())
        t['bx'] = torch.where(pre.abs() < 1e-3, bx + 0.5, bx)             # (bsc >= 0.5: the moved elements are decided)
    return t


@functools.lru_cache(maxsize=4)
def inputs(c):
    return make_inputs(c)


@functools.lru_cache(maxsize=2)
def conv_case(c):
    """(operands, y64, Bw) of a case with the reference on the CPU, computed once and shared"""
    t = inputs(c)
    return (t,) + reference(c, t)


def bwd_stats_reference(c, t, y64, bw):
    """fp64 BN-backward sums of the reference's own gradient y64: d = [bsc x + bsh > 0] y64, (sum d, sum d xhat) [2, cout]
    and the bounds of both: the element-wise bar of d carried through the sums plus (M + 8 + 3) 2^-24 sum |terms| for the
    summation itself and the three roundings of d xhat."""
    x = t['bx'].double()
    on = (x * _chan(t['bsc'].double()) + _chan(t['bsh'].double())) > 0
    if 'lin' in U.epi_of(c.epi):
        on = torch.ones_like(on)
    d = torch.where(on, y64, torch.zeros_like(y64))
    xhat = (x - _chan(t['bmu'].double())) * _chan(t['brs'].double())
    bound = torch.where(on, (c.cin + t_of(c.k, c.tile)) * U24 * bw + 1e-30, torch.zeros_like(bw))
    m = c.n * c.oh * c.ow
    s = torch.stack([d.sum((0, 2, 3)), (d * xhat).sum((0, 2, 3))])
    lim = torch.stack([bound.sum((0, 2, 3)) + (m + 8) * U24 * d.abs().sum((0, 2, 3)) + 1e-30,
                       (bound * xhat.abs()).sum((0, 2, 3)) + (m + 11) * U24 * (d * xhat).abs().sum((0, 2, 3)) + 1e-30])
    return s, lim


# --------------------------------------------------------------------------------------------------------- weight gradient

def wgrad_inputs(c):
    """the forward case's operands and a seeded dy [n, cout, oh, ow]"""
    t = dict(make_inputs(c))
    g = torch.Generator().manual_seed(_seed(c) + 1)
    t['dy'] = U._nchw_rand(g, c.n, c.cout, c.oh, c.ow)
    return t


def wgrad_reference(c, t):
    """(dw64 [cout, cin, 2, 2], Bw) : the fp64 weight gradient of the 2x2 conv over the prologued input, and
    |A'^T| [ sum_tiles (|G'| |dy| |G'|^T) . (|B^T| |d| |B|) ] |A'|"""
    a, mag = U.prologue64(t['x'], t.get('ps'), t.get('pb'), c.pro in ('relu', SCALE_RELU))
    dy = t['dy'].double()
    dw = torch.nn.grad.conv2d_weight(a, (c.cout, c.cin, 2, 2), dy, stride=1, padding=c.pad)
    return dw, wgrad_winograd(mag, dy.abs(), c, torch.float64, absolute=True)


def dy_tiles(dy, tile):
    """[n, c, th, tw, tile, tile]: the output tiles of dy, zero beyond its extent"""
    n, c, oh, ow = dy.shape
    th, tw = (oh + tile - 1) // tile, (ow + tile - 1) // tile
    return F.pad(dy, (0, tw * tile - ow, 0, th * tile - oh)).unfold(2, tile, tile).unfold(3, tile, tile)


def wgrad_winograd(a, dy, c, dtype, absolute=False):
    """dW = A'^T [ sum_tiles (G' dy G'^T) . (B^T d B) ] A' in dtype"""
    m = MATS[(2, c.tile)]
    BT, G2, A2T = [(m[k].abs() if absolute else m[k]).to(dtype) for k in ('BT', 'G2', 'A2T')]
    v = torch.einsum('ia,ncyxab,jb->ncyxij', BT, patches(a.to(dtype), 2, c.tile, c.pad), BT)
    z = torch.einsum('ia,noyxab,jb->noyxij', G2, dy_tiles(dy.to(dtype), c.tile), G2)
    s = torch.einsum('noyxij,ncyxij->ocij', z, v)
    return torch.einsum('pi,ocij,qj->ocpq', A2T, s, A2T)


def wgrad_restate(c, t, dtype=torch.float32):
    a = t['x'].to(dtype)
    if 'ps' in t:
        a = a * _chan(t['ps'].to(dtype))
    if 'pb' in t:
        a = a + _chan(t['pb'].to(dtype))
    if c.pro in ('relu', SCALE_RELU):
        a = F.relu(a)
    return wgrad_winograd(a, t['dy'], c, dtype)


# --------------------------------------------------------------------------------------------------------- fused BN backward

def bnbwd_inputs(n, oh, ow, c, pad, relu):
    """g, x (NCHW, NHWC memory), scale, shift, k123 [3, c]; |scale x + shift| >= 1e-3 everywhere"""
    gen = torch.Generator().manual_seed(61000 + 13 * n + 7 * oh + 3 * ow + c + 2 * pad + int(relu))
    g = U._nchw_rand(gen, n, c, oh, ow)
    sc, sh = torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen) * 0.5
    x = decided(gen, U._nchw_rand(gen, n, c, oh, ow), sc, sh)
    return dict(g=g, x=x, scale=sc, shift=sh, k123=torch.randn(3, c, generator=gen) * 0.5)


def bnbwd_reference(t, pad, relu):
    """(V64, |V| bound map, Z64, |Z| bound map) as [49, tiles, c]: dy = k1 [scale x + shift > 0] g + k2 x + k3 in fp64,
    |dy|_mag = |k1| |g| + |k2| |x| + |k3|, V = B^T dy B over the data gradient's patches (padding pad), Z = G' dy G'^T over
    dy's own tiles; the maps are |B^T| |dy|_mag |B| and |G'| |dy|_mag |G'|^T"""
    g, x = t['g'].double(), t['x'].double()
    k1, k2, k3 = [_chan(t['k123'][i].double()) for i in range(3)]
    d = torch.where(x * _chan(t['scale'].double()) + _chan(t['shift'].double()) > 0, g, torch.zeros_like(g)) if relu else g
    dy, mag = k1 * d + k2 * x + k3, k1.abs() * g.abs() + k2.abs() * x.abs() + k3.abs()
    m = {k: v.to(dy.device) for k, v in MATS[(2, 6)].items()}

    def comp(tiles, mat):
        out = torch.einsum('ia,ncyxab,jb->ijnyxc', mat, tiles, mat)
        return out.reshape(49, -1, out.shape[-1])
    return (comp(patches(dy, 2, 6, pad), m['BT']), comp(patches(mag, 2, 6, pad), m['BT'].abs()),
            comp(dy_tiles(dy, 6), m['G2']), comp(dy_tiles(mag, 6), m['G2'].abs()))
