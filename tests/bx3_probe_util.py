"""Exact plane-product probes for the emulated GEMM family (csrc/conv_bx3.hip, conv_bx3_tiled.hip, conv_bxs.hip on the split
of csrc/bf16x3.h).  Plain functions on CPU tensors, no fixtures.

The emulation takes a b as six bf16 plane products (hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid) and drops three
(mid.lo, lo.mid, lo.lo).  The operands made here are chosen so that
  * every kept product, and every partial sum of them in ANY order, is an exact fp32 number: all products of one output
    element are multiples of one unit u, and the sum of their MAGNITUDES stays below 2^24 u (bit_budget);
  * the dropped products are exactly zero.
The fp64 matmul cast to fp32 is then the only right answer of the emulated kernels and of the native fp32 ones, bit for bit,
and a plane pair that is lost, doubled or crossed is a wrong bit at a known (row, column).

Layout of one probe (an [M, K] x [K, N] GEMM; KSTEP = 32 is the k step of all three kernels: one v_mfma_f32_16x16x32_bf16 per
plane pair, `KS = K / 32` in conv_bx3.hip, "per 32-k step" in conv_bx3_tiled.hip, "every 32-deep k step" in conv_bxs.hip):
  * column j looks at ONE k block: B[k, j] != 0 only for k in block j % nblocks, at four of its 32 positions -- one in each
    8-k group a lane group of the MFMA holds, two on even and two on odd k;
  * (j // nblocks + phase) % 3 is the column's B class: planes hi / hi + mid / hi + mid + lo;
  * (r + phase) % 3 is the row's A class, the same three (ROW_PERIOD = 3 does not divide 64: body chunks, tail chunks, every
    wave and every lane group see every class);
  * layout 'cross': on even k the A value carries its row's planes and B only hi, on odd k A carries only hi and B its
    column's planes.  Every (A class, B class) cell of one launch is then free of dropped products, and the cells are the
    six classes' hh (hi, hi), hm (hi, hi + mid), mh, hl, lh and their unions; mid.mid never occurs;
  * layout 'mm': A and B both hi + mid on every k -- the sixth class, a launch of its own.
A probe SET (probe_set) is the cross layout at phases 0, 1, 2 and the mm layout: over a set every row residue mod 3 and every
(64-column slice, k block) has carried every class.  Magnitudes: A planes 1 or 2, B planes 1 or 3 (asymmetric, so a crossed
pairing changes the sum) times 1 / 2^-9 / 2^-18 for hi / mid / lo, signs mixed; the builders check through split3 that the
planes land where they were meant to and never assume bit positions."""
import torch
import torch.nn.functional as F

KSTEP = 32
HI, MID, LO = 0, 1, 2
PLANE_NAMES = ('hi', 'mid', 'lo')
KEPT = ((HI, HI), (HI, MID), (MID, HI), (HI, LO), (LO, HI), (MID, MID))
DROPPED = ((MID, LO), (LO, MID), (LO, LO))
ROW_PERIOD = 3
CLASS_NAMES = ('hi', 'hi+mid', 'hi+mid+lo')          # planes a value of class 0 / 1 / 2 occupies
# the six probe classes: (A class, B class) -> name of the highest kept pair it exercises
PAIR_CLASSES = {'hh': (0, 0), 'hm': (0, 1), 'mh': (1, 0), 'hl': (0, 2), 'lh': (2, 0), 'mm': (1, 1)}
PLANE_SCALE = (1.0, 2.0 ** -9, 2.0 ** -18)
A_MULT, B_MULT = (1.0, 2.0), (1.0, 3.0)
PHASES = (0, 1, 2)

# ---- the shapes of tests/test_bx3_probe_gpu.py; tests/test_bx3_probe_cpu.py validates every one of them
GEMM_KS = (128, 256, 512, 1024)                       # one, one, two and four 256-k passes of the persistent build
GEMM_COUTS = (64, 128, 256)
# M -> (n, oh, ow), ow % 4 == 0.  64: one chunk; 128: two chunks and fewer rows than the 256 teams a 64-column launch has;
# 240 = 64 * 3 + 48 and 364 = 64 * 5 + 44: tails
GEMM_MS = {64: (1, 4, 16), 128: (1, 4, 32), 240: (1, 6, 40), 364: (1, 7, 52)}
TAIL_M = 240
# (K, cout, M) of the once-per-build cases: stride 2, the data gradient, residual + ReLU + mask_out, the upsampled residual
STRIDE2_CASE, DGRAD_CASE, RIDER_CASE, RES_UP_CASE = (512, 128, 240), (1024, 256, 364), (512, 128, 364), (256, 256, 240)
NATIVE_KS, NATIVE_M, NATIVE_COUT, NATIVE_TAP_CASE = (256, 1024), 364, 128, 2       # the native tiled / B-streamed kernels
# (name, cin, cout, n, h, w, k, stride, pad): the B-streamed emulation kernel over taps / long K
TAP_CASES = (('2x2_pad1', 64, 64, 1, 9, 11, 2, 1, 1), ('2x2_pad1', 64, 128, 1, 9, 11, 2, 1, 1),
             ('3x3_s2_pad1', 128, 128, 2, 17, 21, 3, 2, 1), ('tap_free_k1024', 1024, 128, 1, 7, 36, 1, 1, 0))
# wn, n, cin, h, w, cout: the relay shape of tests/test_guard_bands_gpu.py (258 tiles of two 128-k iterations on 256 CUs)
RELAY_CASE = (2, 2, 256, 82, 100, 256)
# native B-resident kernels want runs of 64-row chunks per team: (variant, K, cout, (n, oh, ow), HND_BRES2)
BRES_CASES = (('bres2_128', 256, 1024, (1, 103, 80), '1'), ('bres_128', 256, 1024, (2, 103, 80), '0'))


def split3(x):
    """hnd::split_pair (csrc/bf16x3.h) for every element of an fp32 tensor: hi = top 16 bits of x, mid = top 16 bits of
    x - hi, lo = x - hi - mid"""
    assert x.dtype == torch.float32
    top = lambda t: (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    hi = top(x)
    r = x - hi
    mid = top(r)
    return hi, mid, r - mid


def _matmul64(a, b):
    """a @ b in fp64 for finite a, skipping the (k block, column) parts of b that are exactly zero"""
    out = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float64)
    for k0 in range(0, b.shape[0], KSTEP):
        cols = (b[k0:k0 + KSTEP] != 0).any(0).nonzero().flatten()
        if cols.numel():
            out[:, cols] += a[:, k0:k0 + KSTEP] @ b[k0:k0 + KSTEP][:, cols]
    return out


def plane_products(A, B):
    """{(a plane, b plane): fp64 [M, N]} for all nine pairs"""
    pa, pb = [p.double() for p in split3(A)], [p.double() for p in split3(B)]
    return {(a, b): _matmul64(pa[a], pb[b]) for a in range(3) for b in range(3)}


def model_gemm(A, B, pairs=KEPT, products=None):
    """fp64 sum over `pairs` of (A plane) x (B plane) products.  A pair may be left out, listed twice, or given another
    plane on either side: the single faults tests/test_bx3_probe_cpu.py plants."""
    prod = plane_products(A, B) if products is None else products
    out = torch.zeros_like(prod[(HI, HI)])
    for p in pairs:
        out = out + prod[tuple(p)]
    return out


def mutations():
    """[(name, pairs)]: every single fault of the six-pair product -- one pair dropped, taken twice, or taken with the wrong
    B plane or the wrong A plane"""
    out = []
    for i, (a, b) in enumerate(KEPT):
        rest = KEPT[:i] + KEPT[i + 1:]
        tag = '%s.%s' % (PLANE_NAMES[a], PLANE_NAMES[b])
        out.append(('drop ' + tag, rest))
        out.append(('twice ' + tag, KEPT + ((a, b),)))
        for o in range(3):
            if o != b:
                out.append(('%s with B %s' % (tag, PLANE_NAMES[o]), rest + ((a, o),)))
            if o != a:
                out.append(('%s with A %s' % (tag, PLANE_NAMES[o]), rest + ((o, b),)))
    return out


def expected(A, B):
    """the plain fp64 matmul, cast to fp32 (exact by construction: bit_budget)"""
    return (A.double() @ B.double()).float()


# ------------------------------------------------------------------------------------------------------------ builders
def _mix(*terms):
    """a cheap integer hash of broadcastable int64 index tensors"""
    h = torch.zeros((), dtype=torch.int64)
    for i, t in enumerate(terms):
        h = (h * 1103515245 + t * (2654435761 + 40503 * i) + 12345) % 4294967296
        h = h ^ (h >> 13)
    return (h * 1664525 % 4294967296) >> 11


def _values(h, mult, occ):
    """fp32 values sign * sum over occupied planes of mult[bit] * PLANE_SCALE; h: hash tensor, occ: int tensor 0 / 1 / 2
    (class of the value: how many planes it occupies beyond hi)"""
    m = torch.tensor(mult, dtype=torch.float64)
    v = m[(h >> 1) & 1] * PLANE_SCALE[HI]
    v = v + torch.where(occ >= 1, m[(h >> 2) & 1] * PLANE_SCALE[MID], torch.zeros((), dtype=torch.float64))
    v = v + torch.where(occ >= 2, m[(h >> 3) & 1] * PLANE_SCALE[LO], torch.zeros((), dtype=torch.float64))
    v = torch.where((h & 1) > 0, -v, v)
    x = v.float()
    assert torch.equal(x.double(), v)
    return x


def _check_occupancy(x, occ, nonzero):
    """the planes split3 finds are the ones the class claims: the builders never assume bit positions"""
    hi, mid, lo = split3(x)
    assert torch.equal((hi != 0), nonzero) and torch.equal((mid != 0), nonzero & (occ >= 1)) \
        and torch.equal((lo != 0), nonzero & (occ >= 2)), 'a probe value renormalised into other planes'


def row_class(r, phase):
    return (r + phase) % ROW_PERIOD


def col_block(j, nblocks):
    return j % nblocks


def col_class(j, nblocks, phase, layout='cross'):
    return 1 if layout == 'mm' else (j // nblocks + phase) % 3


def a_operand(rows, kdim, phase, layout):
    """[rows, kdim]: every element non-zero; row r of class (r + phase) % 3"""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    k = torch.arange(kdim, dtype=torch.int64)[None, :]
    if layout == 'mm':
        occ = torch.ones(rows, kdim, dtype=torch.int64)
    else:
        occ = torch.where(k % 2 == 0, row_class(r, phase), torch.zeros((), dtype=torch.int64)).expand(rows, kdim)
    x = _values(_mix(r, k, torch.tensor(7 + phase)), A_MULT, occ)
    _check_occupancy(x, occ, torch.ones(rows, kdim, dtype=torch.bool))
    return x


def b_operand(kdim, cout, phase, layout):
    """[kdim, cout]: column j non-zero at four positions of k block j % nblocks"""
    nb = kdim // KSTEP
    k = torch.arange(kdim, dtype=torch.int64)[:, None]
    j = torch.arange(cout, dtype=torch.int64)[None, :]
    q, t = j // nb, k % KSTEP
    g = t // 8
    want = 8 * g + 2 * ((q + 3 * g + phase) % 4) + ((g + q + phase) & 1)
    nonzero = (k // KSTEP == col_block(j, nb)) & (t == want)
    if layout == 'mm':
        occ = torch.ones(kdim, cout, dtype=torch.int64)
    else:
        occ = torch.where(k % 2 == 1, col_class(j, nb, phase), torch.zeros((), dtype=torch.int64)).expand(kdim, cout)
    x = _values(_mix(j, k, torch.tensor(101 + phase)), B_MULT, occ)
    x = torch.where(nonzero, x, torch.zeros((), dtype=torch.float32))
    _check_occupancy(x, occ, nonzero)
    return x


def im2col(x, k, stride, pad):
    """x NHWC -> [n * oh * ow, k * k * cin], K ordered (tap row, tap column, channel); zero padding"""
    n, h, w, c = x.shape
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    cols = [xp[:, i:i + (oh - 1) * stride + 1:stride, j:j + (ow - 1) * stride + 1:stride, :] for i in range(k) for j in range(k)]
    return torch.cat(cols, 3).reshape(n * oh * ow, k * k * c)


class Probe(object):
    """one launch's operands.  A [M, K] / B [K, N]: the GEMM (A = im2col of x); x NHWC / w OIHW: the convolution;
    want: fp32 [M, N], the one right answer"""

    def __init__(self, layout, phase, x, w, k, stride, pad):
        self.layout, self.phase, self.x, self.w, self.k, self.stride, self.pad = layout, phase, x, w, k, stride, pad
        self.A = im2col(x, k, stride, pad)
        self.B = w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous()
        self.M, self.K = self.A.shape
        self.N = self.B.shape[1]
        self.nblocks = self.K // KSTEP
        self.want = expected(self.A, self.B)
        n, h, w_ = x.shape[:3]
        self.oshape = (n, (h + 2 * pad - k) // stride + 1, (w_ + 2 * pad - k) // stride + 1, self.N)

    def name(self):
        return '%s/phase %d' % (self.layout, self.phase)

    def describe(self, r, j):
        """what a wrong element at (row r, column j) says about the kernel"""
        b = col_block(j, self.nblocks)
        tap, cin = divmod(b * KSTEP, self.x.shape[3])
        rc = 'rows read pixels of every class' if self.k > 1 else 'A class %s' % (
            'hi+mid' if self.layout == 'mm' else CLASS_NAMES[row_class(r, self.phase)])
        return ('row %d (%s, chunk %d%s) column %d (k block %d = k %d..%d, 256-k pass %d%s, B class %s, 64-column slice %d)'
                % (r, rc, r // 64, ', in the tail' if r // 64 == self.M // 64 and self.M % 64 else '', j, b, b * KSTEP,
                   b * KSTEP + KSTEP - 1, b * KSTEP // 256, ', tap %d' % tap if self.k > 1 else '',
                   CLASS_NAMES[col_class(j, self.nblocks, self.phase, self.layout)], j // 64))

    def first_wrong(self, y):
        """None, or a message naming the first wrong element of y [M, N] (a CPU fp32 tensor)"""
        y = y.reshape(self.M, self.N)
        bad = ~((y == self.want) | (torch.isnan(y) & torch.isnan(self.want)))
        bad |= torch.isnan(y)
        if not bool(bad.any()):
            return None
        r, j = [int(v) for v in bad.nonzero()[0]]
        return ('%s: %d of %d elements wrong; first at %s: got %r, want %r' %
                (self.name(), int(bad.sum()), bad.numel(), self.describe(r, j), float(y[r, j]), float(self.want[r, j])))


def gemm_probe(m_shape, kdim, cout, layout, phase, stride=1):
    """a 1x1 convolution on an (n, oh, ow) output: GEMM row r = output pixel r.  stride 2: the pixels in between are never
    read and hold NaN"""
    n, oh, ow = m_shape
    A = a_operand(n * oh * ow, kdim, phase, layout).view(n, oh, ow, kdim)
    if stride == 1:
        x = A
    else:
        x = torch.full((n, (oh - 1) * stride + 1, (ow - 1) * stride + 1, kdim), float('nan'))
        x[:, ::stride, ::stride] = A
    w = b_operand(kdim, cout, phase, layout).t().contiguous().view(cout, kdim, 1, 1)
    return Probe(layout, phase, x.contiguous(), w, 1, stride, 0)


def conv_probe(cin, cout, n, h, w, k, stride, pad, layout, phase):
    """a k x k convolution: the class belongs to the INPUT pixel (pixel p of class (p + phase) % 3), every tap has its own
    k blocks (block = tap * cin / 32 + channel / 32), and the padding is the convolution's own zeros"""
    x = a_operand(n * h * w, cin, phase, layout).view(n, h, w, cin)
    B = b_operand(k * k * cin, cout, phase, layout)                     # K ordered (tap row, tap column, channel)
    wt = B.view(k, k, cin, cout).permute(3, 2, 0, 1).contiguous()
    return Probe(layout, phase, x, wt, k, stride, pad)


def probe_set(make):
    """make(layout, phase) -> Probe: the cross layout at every phase, then the mm layout"""
    return [make('cross', ph) for ph in PHASES] + [make('mm', 0)]


def gemm_probe_set(m_shape, kdim, cout, stride=1):
    return probe_set(lambda layout, phase: gemm_probe(m_shape, kdim, cout, layout, phase, stride))


def conv_probe_set(cin, cout, n, h, w, k, stride, pad):
    return probe_set(lambda layout, phase: conv_probe(cin, cout, n, h, w, k, stride, pad, layout, phase))


# ------------------------------------------------------------------------------------------------- what the CPU file asks
def _lsb_unit(t):
    """the smallest power of two that every non-zero element of t is a multiple of (inf for an all-zero tensor)"""
    t = t[t != 0].double()
    if t.numel() == 0:
        return float('inf')
    m, e = torch.frexp(t)
    mant = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mant & -mant).double()
    return float((low * torch.exp2(e.double() - 53)).min())


def significant_bits(t):
    """the widest mantissa (leading one to last one) among the elements of t"""
    t = t[t != 0].double()
    if t.numel() == 0:
        return 0
    m, _ = torch.frexp(t)
    mant = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (mant & -mant).double()
    return int((54 - torch.log2(low)).max().item()) - 1


def bit_budget(A, B, pairs=KEPT):
    """(u, s): every plane product of `pairs` is a multiple of u, and no output element's products have magnitudes that sum
    to more than s.  s < 2^24 u: every partial sum, in any order and through any adder that keeps 24 bits below its largest
    operand, is exact."""
    pa, pb = split3(A), split3(B)
    u = min(_lsb_unit(pa[a]) * _lsb_unit(pb[b]) for a, b in pairs)
    s = sum(_matmul64(pa[a].double().abs(), pb[b].double().abs()) for a, b in pairs)
    return u, float(s.max())


def cells_pinned(probes):
    """(row class x k block x B class) cells that carry a non-zero expected value somewhere in the set"""
    cells = set()
    for p in probes:
        if p.k > 1:
            continue
        nz = p.want != 0
        for r0 in range(ROW_PERIOD):
            cols = nz[r0::ROW_PERIOD].any(0).nonzero().flatten().tolist()
            rc = 1 if p.layout == 'mm' else row_class(r0, p.phase)
            cells.update((p.layout == 'mm', rc, col_block(j, p.nblocks), col_class(j, p.nblocks, p.phase, p.layout))
                         for j in cols)
    return len(cells)
