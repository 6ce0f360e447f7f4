"""The kernels between the convs of a training step (csrc/elementwise.hip: training BatchNorm, the 3x3 stride-2 max pool,
the FPN helpers): the case tables, the fp64 references, the a-priori bars and plain fp32 stand-ins shared by
tests/test_elementwise_cases_cpu.py (references, attainability, injected faults, branch coverage: no GPU) and
tests/test_elementwise_gpu.py (the launches).  Nothing here imports the library or touches a device.

Idiom of tests/conv_util.py and tests/wgrad_util.py: a reference is fp64 arithmetic on the SAME fp32 inputs, a bar is an
element-wise rounding bound with u = 2^-24 derived before any device output was seen (each `*_bars` docstring carries the
derivation), and the assertion is "worst |got - ref| / (bound + 1e-30) <= 1".  Every kernel is held alone: the inputs of
its reference are what the previous stage stored on the device, so a miss names one kernel and upstream rounding never
widens a bound.

Sizes.  The streaming kernels (affine_relu, relu_mask_nibbles, bn_bwd_apply) walk chunks of 1024 float4 vectors on a grid
that grid_for_chunks caps at 16384 workgroups, i.e. 2^24 vectors or 268 MB per tensor; no case here comes near it (the
largest tensors are the two grid-stride cases of the pool and of add_inplace, whose grid_for caps at 4096 workgroups of
256 threads).  The loop above that cap is safe by construction and needs no case: a lane's channel group is read once,
outside the loop, only when `fixed` holds (cs / 4 divides 256), and the loop's stride gridDim * 1024 is then a multiple of
cs / 4, so the lane's vector index keeps its residue modulo cs / 4 on every pass."""
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24                  # unit roundoff of fp32
TINY = 1e-30                    # added to every bound
EPS, MOMENTUM = 1e-5, 0.1
STAT_TILE = 128                 # pixels per (sum, sum^2) partial of the conv epilogues
BWD_TILE = 1024                 # kBnTilePix
CHUNK = 1024                    # 256 * kEwU vectors per workgroup and pass
CHUNK_CAP = 16384               # grid_for_chunks
GRID_CAP = 4096                 # grid_for (workgroups of 256 threads)
POOL_STRIP = 8                  # kPoolStrip


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(v):
    """the fp32 value nearest to the Python float v, as a Python float"""
    return float(torch.tensor(v, dtype=torch.float32))


def worst(got, ref, bound):
    """worst |got - ref| / (bound + 1e-30); NaN (which fails `<= 1`) where got holds a NaN the reference does not"""
    if ref.numel() == 0:
        return 0.0
    return float(((got.double() - ref.double()).abs() / (bound + TINY)).max())


# ===================================================================================================== BN: finalize
# (ntiles, pixels of the last tile, c, cs, running statistics given).  ntiles classes of bn_finalize_kernel (16 waves x 4
# tile sub-lanes stride over the tiles 64 at a time, 4x unrolled while t + 192 < ntiles): every class with a padded and an
# unpadded cs; (40, 64) and (80, 96) have a 16-channel block that straddles c.
FINALIZE_NTILES = (1, 63, 64, 65, 192, 193, 256, 257, 449, 1000)
FINALIZE_CASES = [
    (1, 128, 3, 4, True), (1, 77, 64, 64, False),
    (1, 1, 12, 32, True), (1, 1, 256, 256, False),            # count == 1: unbiased == biased
    (63, 128, 12, 32, False), (63, 5, 256, 256, True),
    (64, 128, 40, 64, True), (64, 127, 64, 64, False),
    (65, 1, 80, 96, False), (65, 128, 256, 256, True),
    (192, 128, 3, 4, False), (192, 100, 64, 64, True),
    (193, 17, 40, 64, False), (193, 128, 64, 64, True),       # the first lane enters the unrolled loop
    (256, 128, 12, 32, True), (256, 31, 256, 256, False),
    (257, 1, 80, 96, True), (257, 128, 64, 64, False),
    (449, 128, 40, 64, True), (449, 3, 64, 64, False),        # a remainder after one unrolled pass
    (1000, 99, 3, 4, True), (1000, 128, 64, 64, True),        # several unrolled passes
]
CONST_CH, FAR_CH, CLAMP_CH = 0, 1, 2          # the constant 0.5, mean = 10 std, and a constant whose fp64 variance is < 0


def finalize_lane_passes(ntiles, t0):
    """bn_finalize_kernel's tile loop restated for the lane that starts at tile t0 (0..63): (unrolled passes, remainder)"""
    t, passes, rem = t0, 0, 0
    while t + 3 * 64 < ntiles:
        t, passes = t + 4 * 64, passes + 1
    while t < ntiles:
        t, rem = t + 64, rem + 1
    return passes, rem


def _clamp_value(ntiles, last):
    """an fp32 constant v in [30, 100) whose rounded partials give s2 / count - mean^2 < -2 eps in fp64: a full tile holds
    exactly 128 v and fl32(128 v^2) = 128 fl32(v^2), so the raw variance is fl32(v^2) - v^2, up to 2^-24 v^2 below zero"""
    cand = torch.arange(1, 400, dtype=torch.float32) * 0.173 + 30.0
    n_t = torch.tensor([float(STAT_TILE)] * (ntiles - 1) + [float(last)], dtype=torch.float64)
    v = cand.double()
    s1 = (n_t[:, None] * v[None, :]).float().double().sum(0)
    s2 = (n_t[:, None] * (v * v)[None, :]).float().double().sum(0)
    mean = s1 / n_t.sum()
    raw = s2 / n_t.sum() - mean * mean
    i = int(raw.argmin())
    assert float(raw[i]) < -2 * EPS, (ntiles, last, float(raw[i]))
    return float(cand[i])


@functools.lru_cache(maxsize=None)
def finalize_inputs(ntiles, last, c, cs, running):
    """seeded inputs of one finalize case: fp32 x [count, c] and, from it, the partials [ntiles, 2, cs] as the conv
    epilogues store them -- per-128-pixel fp64 sums of x and x^2, rounded once to fp32, padded channels 0"""
    count = (ntiles - 1) * STAT_TILE + last
    g = gen(4100 + 7 * ntiles + 3 * last + c + cs)
    x = torch.randn(count, c, generator=g) * (torch.rand(c, generator=g) + 0.5) + torch.randn(c, generator=g)
    x[:, CONST_CH] = 0.5
    x[:, FAR_CH] = torch.randn(count, generator=g) * 0.3 + 3.0
    x[:, CLAMP_CH] = _clamp_value(ntiles, last)
    x64 = F.pad(x.double(), (0, 0, 0, ntiles * STAT_TILE - count)).view(ntiles, STAT_TILE, c)
    part = torch.zeros(ntiles, 2, cs)
    part[:, 0, :c], part[:, 1, :c] = x64.sum(1).float(), (x64 * x64).sum(1).float()
    sign = torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0)
    gamma, beta = (torch.rand(c, generator=g) + 0.5) * sign, torch.randn(c, generator=g)
    rm, rv = (torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5) if running else (None, None)
    return dict(x=x, part=part, count=count, gamma=gamma, beta=beta, rm=rm, rv=rv)


def finalize_reference(part, c, count, gamma, beta, rm=None, rv=None, momentum=MOMENTUM, eps=EPS):
    """bn_finalize in fp64 on the given partials (fp32 or fp64): the kernel's own formulas, biased variance
    E[x^2] - mean^2 clamped at 0, momentum and eps at their fp32 values"""
    p = part.double()
    s1, s2 = p[:, 0, :c].sum(0), p[:, 1, :c].sum(0)
    mean = s1 / count
    raw = s2 / count - mean * mean
    var = raw.clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    scale = gamma.double() * rstd
    out = dict(mean=mean, rstd=rstd, scale=scale, shift=beta.double() - mean * scale, raw_var=raw, var=var)
    if rm is not None:
        m = f32(momentum)
        unbiased = var * count / (count - 1.0) if count > 1 else var
        out['rm_terms'] = ((1.0 - m) * rm.double(), m * mean)
        out['rv_terms'] = ((1.0 - m) * rv.double(), m * unbiased)
        out['rm'], out['rv'] = sum(out['rm_terms']), sum(out['rv_terms'])
    return out


def finalize_bars(got, ref, beta, eps=EPS):
    """worst ratio per output of bn_finalize; got: dict of fp32 tensors [c] (mean, rstd, scale, shift and, with running
    statistics, rm, rv), ref: finalize_reference of the same partials.  The kernel sums the partials in fp64, so a sum
    carries ~1e-16 and only the fp32 roundings of the outputs count:
      mean   one rounding of the fp64 mean: u |ref|, held to 2u |ref|.
      rstd   one rounding, u |ref|; plus the fp64 cancellation of E[x^2] - mean^2 (2^-52 mean^2, whether or not the
             compiler contracts it), which reaches rstd as 2^-53 mean^2 / (var + eps) relative: held to
             (2u + 2^-52 mean^2 / (var + eps)) |ref|.  The clamp is 1-Lipschitz and does not widen this, and where the
             raw variance is below -2^-50 mean^2 both sides clamp to 0 and the term is dropped.  scale and shift are
             formed from rstd and carry the same term (below 1e-11 on these inputs).
      scale  gamma * fl(rstd): u from rstd, u from the product: 3u |ref|.
      shift  beta - fl(mean) * fl(scale): fl(mean) u, fl(scale) 2u, the product u (0 as an fma), all on |mean scale|,
             and the difference u (|beta| + |mean scale|): 6u (|beta| + |mean scale|).
      running  (1 - m) old + m fl(stat): fl(1 - m) u, each product u, fl(stat) u, the sum u on both terms:
             4u (|(1 - m) old| + |m stat|)."""
    r = {}
    r['mean'] = worst(got['mean'], ref['mean'], 2 * U * ref['mean'].abs())
    m2 = ref['mean'] ** 2
    cancel = torch.where(ref['raw_var'] < -2.0 ** -50 * m2, torch.zeros_like(m2), 2.0 ** -52 * m2 / (ref['var'] + f32(eps)))
    r['rstd'] = worst(got['rstd'], ref['rstd'], (2 * U + cancel) * ref['rstd'].abs())
    r['scale'] = worst(got['scale'], ref['scale'], (3 * U + cancel) * ref['scale'].abs())
    ms = (ref['mean'] * ref['scale']).abs()
    r['shift'] = worst(got['shift'], ref['shift'], 6 * U * (beta.double().abs() + ms) + cancel * ms)
    for k in ('rm', 'rv'):
        if k in ref:
            a, b = ref[k + '_terms']
            r[k] = worst(got[k], ref[k], 4 * U * (a.abs() + b.abs()))
    return r


def finalize_standin(part, c, count, gamma, beta, rm=None, rv=None, momentum=MOMENTUM, eps=EPS, drop_tile=None):
    """plain CPU stand-in of bn_finalize: the tile sums in fp64 (as the kernel; an fp32 sum of 1000 tiles could not meet a
    2u bar), every output and the scale / shift / running arithmetic in fp32.  drop_tile: the injected fault."""
    p = part.double()
    if drop_tile is not None:
        p = p.clone()
        p[drop_tile] = 0.0
    mean = p[:, 0, :c].sum(0) / count
    var = (p[:, 1, :c].sum(0) / count - mean * mean).clamp_min(0.0)
    rstd = (1.0 / torch.sqrt(var + f32(eps))).float()
    scale = gamma * rstd
    out = dict(mean=mean.float(), rstd=rstd, scale=scale, shift=beta - mean.float() * scale)
    if rm is not None:
        m = torch.tensor(momentum, dtype=torch.float32)
        unbiased = var * count / (count - 1.0) if count > 1 else var
        out['rm'] = (1.0 - m) * rm + m * mean.float()
        out['rv'] = (1.0 - m) * rv + m * unbiased.float()
    return out


# ===================================================================================================== BN: elementwise
# affine_relu and bn_bwd_apply: (cs, pixels).  n4 = pixels * cs / 4 vectors: below 256 (one partial row of loads), between
# 1024 and 2048 and no multiple of 256 (a second workgroup with a ragged tail), several chunks.  cs / 4 = 512 admits
# neither of the first two (n4 is a multiple of 512): one pixel, three and eleven there.  cs 96 and 2048 are the `!fixed`
# path (cs / 4 does not divide 256), 2048 with cs / 4 above the block.
STREAM_CASES = [(4, 255), (4, 1500), (4, 5000), (32, 31), (32, 191), (32, 625), (64, 15), (64, 95), (64, 313),
                (96, 10), (96, 50), (96, 200), (256, 3), (256, 23), (256, 79), (2048, 1), (2048, 3), (2048, 11)]
STREAM_CS = (4, 32, 64, 96, 256, 2048)
# bn_bwd_reduce: (pixels, cs); one 1024-pixel tile per workgroup, rows = 256 / (cs / 4) pixels per pass.  66 tiles at
# cs 4 only: bn_bwd_finalize's lane loop (64 lanes over the tiles) wraps.
REDUCE_CASES = [(1, 4), (1023, 4), (1024, 4), (1025, 4), (2 * 1024 + 37, 4), (65 * 1024 + 5, 4),
                (1, 32), (1023, 32), (1024, 32), (1025, 32), (2 * 1024 + 37, 32),
                (1, 64), (1023, 64), (1024, 64), (1025, 64), (2 * 1024 + 37, 64),
                (1025, 128), (1023, 256), (2 * 1024 + 37, 256), (1025, 512), (1, 1024), (1025, 1024)]
REDUCE_REFUSED_CS = (96, 2048)
# bn_bwd_finalize on the partials of a device reduce: (pixels, c, cs)
BWD_FINALIZE_CASES = [(65 * 1024 + 5, 3, 4), (2 * 1024 + 37, 12, 32), (1025, 40, 64), (1023, 64, 64), (1, 100, 128),
                      (2 * 1024 + 37, 256, 256), (1025, 1024, 1024)]
NEAR_FRACTION = 0.08            # of the real elements of a relu case (the issue asks for 5 % at least)


def reduce_accepts(cs):
    """hnd_bn_bwd_reduce's requirement restated"""
    return cs % 4 == 0 and cs <= 1024 and 256 % (cs // 4) == 0


def stream_fixed(cs):
    return 256 % (cs // 4) == 0


def bwd_ntiles(npix):
    return (npix + BWD_TILE - 1) // BWD_TILE


@functools.lru_cache(maxsize=None)
def bn_inputs(npix, cs, c, relu):
    """seeded fp32 inputs of the backward kernels and of affine_relu, [npix, cs] with channels c.. zero: x, the incoming
    gradient g, per-channel scale (both signs), shift, mean, rstd, gamma.  relu: NEAR_FRACTION of the real elements lie
    where x * scale + shift is within a few ulps of zero -- x is the fp32 nearest to -shift / scale moved by -4..+4 ulps,
    |g| >= 0.5 there -- so that a site whose gate disagrees with the stored forward misses its bar by a wide margin."""
    g = gen(4300 + 11 * npix + 5 * cs + c + (1 if relu else 0))
    x = torch.randn(npix, cs, generator=g) * 1.7 + 0.4
    gout = torch.randn(npix, cs, generator=g)
    sign = torch.where(torch.rand(cs, generator=g) < 0.25, -1.0, 1.0)
    scale, shift = (torch.rand(cs, generator=g) + 0.5) * sign, torch.randn(cs, generator=g) * 0.5
    mean, rstd = torch.randn(cs, generator=g) * 0.3 + 0.4, 1.0 / (torch.rand(cs, generator=g) + 1.2)
    gamma = (torch.rand(cs, generator=g) + 0.5) * sign
    near = torch.zeros(npix, cs, dtype=torch.bool)
    if relu:
        near = torch.rand(npix, cs, generator=g) < NEAR_FRACTION
        x0 = (-shift / scale).expand(npix, cs).contiguous()
        k = torch.randint(-4, 5, (npix, cs), generator=g, dtype=torch.int32)
        xn = (x0.view(torch.int32) + k).view(torch.float32)
        x = torch.where(near, xn, x)
        gout = torch.where(near, torch.copysign(0.5 + torch.rand(npix, cs, generator=g), gout), gout)
    for t in (x, gout, near):
        t[:, c:] = 0
    for t in (scale, shift, mean, rstd, gamma):
        t[c:] = 0
    return dict(x=x, g=gout, scale=scale, shift=shift, mean=mean, rstd=rstd, gamma=gamma, near=near)


def nibbles_of(y):
    """the ReLU-mask nibbles of fp32 y [..., cs]: uint8 [..., cs / 4], bit i = (value i > 0) under IEEE"""
    b = (y > 0).reshape(-1, 4).to(torch.int32)
    v = b[:, 0] + 2 * b[:, 1] + 4 * b[:, 2] + 8 * b[:, 3]
    return v.to(torch.uint8).view(tuple(y.shape[:-1]) + (y.shape[-1] // 4,))


def gate_of(mask):
    """bool [..., cs] of mask nibbles [..., cs / 4]"""
    m = mask.to(torch.int32).unsqueeze(-1)
    bits = (m >> torch.arange(4, dtype=torch.int32)) & 1
    return bits.bool().view(tuple(mask.shape[:-1]) + (mask.shape[-1] * 4,))


def affine_reference(x, scale, shift, relu):
    y = x.double() * scale.double() + shift.double()
    return y.clamp_min(0.0) if relu else y


def affine_bars(y, x, scale, shift, relu):
    """(worst ratio, every sign right) of affine_relu's y against fp64.  x s + b as one fma rounds once, u |x s + b|; as a
    product and a sum, u |x s| + u |fl(x s) + b|; both are within 2u (|x s| + |b|), and ReLU is 1-Lipschitz.  Where |ref|
    exceeds the bound the stored value must carry the reference's sign."""
    ref = affine_reference(x, scale, shift, relu)
    bound = 2 * U * ((x.double() * scale.double()).abs() + shift.double().abs()) + TINY
    sure = ref.abs() > bound
    signs = bool((torch.sign(y.double())[sure] == torch.sign(ref)[sure]).all())
    return worst(y, ref, bound), signs


def affine_standin(x, scale, shift, relu, wrong_group_at=None):
    """plain fp32: y = x * scale + shift (a product and a sum), ReLU.  wrong_group_at: flat vector index whose four
    channels take the scale / shift of the NEXT channel group (the injected fault of a `!fixed` lane)"""
    y = x * scale + shift
    if wrong_group_at is not None:
        cs4 = x.shape[-1] // 4
        p, c4 = divmod(wrong_group_at, cs4)
        o = ((c4 + 1) % cs4) * 4
        y[p, c4 * 4:c4 * 4 + 4] = x[p, c4 * 4:c4 * 4 + 4] * scale[o:o + 4] + shift[o:o + 4]
    return y.clamp_min(0.0) if relu else y


def tile_sums(v):
    """[npix, cs] fp64 -> per-1024-pixel-tile sums [ntiles, cs]"""
    npix, cs = v.shape
    nt = bwd_ntiles(npix)
    return F.pad(v, (0, 0, 0, nt * BWD_TILE - npix)).view(nt, BWD_TILE, cs).sum(1)


def tile_pixels(npix):
    nt = bwd_ntiles(npix)
    return torch.tensor([min(BWD_TILE, npix - t * BWD_TILE) for t in range(nt)], dtype=torch.float64)[:, None]


def reduce_reference(gout, x, mean, rstd, gate):
    """bn_bwd_reduce in fp64: per tile (sum d, sum d xhat, sum |d|, sum |d xhat|), d = g where gate (None: everywhere),
    xhat = (x - mean) rstd"""
    d = gout.double()
    if gate is not None:
        d = torch.where(gate, d, torch.zeros_like(d))
    t = d * ((x.double() - mean.double()) * rstd.double())
    return tile_sums(d), tile_sums(t), tile_sums(d.abs()), tile_sums(t.abs())


def reduce_bars(part, ref, npix):
    """worst ratios (sum d, sum d xhat) of the partials [ntiles, 2, cs].  A tile of P pixels is summed in some order in
    fp32: within (P - 1) u sum |terms| for any order; a term d xhat carries three more roundings (the difference, two
    products, fewer as fmas); held to (P + 8) u sum |d| and (P + 8) u sum |d xhat|."""
    s1, s2, a1, a2 = ref
    pix = tile_pixels(npix)
    return worst(part[:, 0], s1, (pix + 8) * U * a1), worst(part[:, 1], s2, (pix + 8) * U * a2)


def reduce_standin(gout, x, mean, rstd, gate, skip_pixel=None):
    """plain fp32 per-tile sums [ntiles, 2, cs].  skip_pixel: the injected fault"""
    d = gout if gate is None else torch.where(gate, gout, torch.zeros_like(gout))
    t = d * ((x - mean) * rstd)
    if skip_pixel is not None:
        d, t = d.clone(), t.clone()
        d[skip_pixel], t[skip_pixel] = 0.0, 0.0
    npix, cs = d.shape
    nt = bwd_ntiles(npix)
    pad = lambda v: F.pad(v, (0, 0, 0, nt * BWD_TILE - npix)).view(nt, BWD_TILE, cs).sum(1)
    return torch.stack((pad(d), pad(t)), 1)


def bwd_finalize_reference(part, c, count, gamma, mean, rstd):
    """bn_bwd_finalize in fp64 on the partials [ntiles, 2, cs]: dbeta, dgamma, k1 = gamma rstd, k2 = -k1 rstd s2 / count,
    k3 = k1 (mean rstd s2 - s1) / count, so that dx = k1 d + k2 x + k3"""
    p = part.double()
    s1, s2 = p[:, 0, :c].sum(0), p[:, 1, :c].sum(0)
    ga, mu, rs = gamma.double()[:c], mean.double()[:c], rstd.double()[:c]
    k1 = ga * rs
    return dict(dbeta=s1, dgamma=s2, k1=k1, k2=-k1 * rs * s2 / count, k3=k1 * (mu * rs * s2 - s1) / count,
                k3_terms=(mu * rs * s2).abs() + s1.abs())


def bwd_finalize_bars(got, ref, count):
    """worst ratio per output.  Everything is fp64 in the kernel and rounded once: u |ref|, held to 2u |ref|; k3 is a
    difference in fp64, whose cancellation adds 1e-12 (|mean rstd s2| + |s1|) |k1| / count."""
    r = {k: worst(got[k], ref[k], 2 * U * ref[k].abs()) for k in ('dbeta', 'dgamma', 'k1', 'k2')}
    r['k3'] = worst(got['k3'], ref['k3'], 2 * U * ref['k3'].abs() + 1e-12 * ref['k3_terms'] * ref['k1'].abs() / count)
    return r


def bwd_finalize_standin(part, c, count, gamma, mean, rstd, drop_tile=None):
    p = part.double()
    if drop_tile is not None:
        p = p.clone()
        p[drop_tile] = 0.0
    ref = bwd_finalize_reference(p, c, count, gamma, mean, rstd)
    return {k: ref[k].float() for k in ('dbeta', 'dgamma', 'k1', 'k2', 'k3')}


def apply_reference(gout, x, k123, gate):
    """bn_bwd_apply in fp64 on k123 [3, cs]: (dx, |k1 d| + |k2 x| + |k3|)"""
    d = gout.double()
    if gate is not None:
        d = torch.where(gate, d, torch.zeros_like(d))
    k = k123.double()
    a, b = k[0] * d, k[1] * x.double()
    return a + b + k[2], a.abs() + b.abs() + k[2].abs()


def apply_bars(dx, ref):
    """k1 d + k2 x + k3 in fp32: two products and two sums, or two fmas: at most four roundings, each on a partial
    result no larger than |k1 d| + |k2 x| + |k3| (to first order): 4u (|k1 d| + |k2 x| + |k3|)."""
    return worst(dx, ref[0], 4 * U * ref[1])


def apply_standin(gout, x, k123, gate, wrong_group_at=None):
    d = gout if gate is None else torch.where(gate, gout, torch.zeros_like(gout))
    dx = k123[0] * d + k123[1] * x + k123[2]
    if wrong_group_at is not None:
        cs4 = x.shape[-1] // 4
        p, c4 = divmod(wrong_group_at, cs4)
        o, s = ((c4 + 1) % cs4) * 4, slice(c4 * 4, c4 * 4 + 4)
        dx[p, s] = k123[0, o:o + 4] * d[p, s] + k123[1, o:o + 4] * x[p, s] + k123[2, o:o + 4]
    return dx


# relu_mask_nibbles: exact
MASK_N4 = (1, 255, 256, 1025)


@functools.lru_cache(maxsize=None)
def mask_inputs(n4):
    """fp32 [n4 * 4] with +0, -0, the smallest positive subnormal, +inf, -inf and NaN among the values; the expected bit
    is what `x > 0` gives under IEEE (0 for both zeros, -inf and NaN; 1 for the subnormal and +inf)"""
    x = torch.randn(n4 * 4, generator=gen(4500 + n4))
    special = torch.tensor([0.0, -0.0, 2.0 ** -149, float('inf'), float('-inf'), float('nan'), -2.0 ** -149])
    at = torch.randperm(n4 * 4, generator=gen(4600 + n4))[:min(n4 * 4, 4 * len(special))]
    x[at] = special[torch.arange(len(at)) % len(special)]
    return x


# ===================================================================================================== max pool
POOL_EXTENTS = (1, 2, 3, 15, 16, 17, 33)       # oh = 1, 1, 2, 8, 8, 9, 17: both sides of the strip boundary, three strips
POOL_CHANNELS = (4, 64, 68)                    # 68 / 4 = 17 is no power of two
POOL_BATCHES = (1, 3)


def pool_cases():
    """(n, c, h, w): every pair of extents; channels and batch cycle so that every (c, n) meets every h"""
    out = []
    for i, h in enumerate(POOL_EXTENTS):
        for j, w in enumerate(POOL_EXTENTS):
            k = i + j
            out.append((POOL_BATCHES[(k // 3) % 2], POOL_CHANNELS[k % 3], h, w))
    return out


# One thread per (image, strip of 8 output rows, output column, 4 channels); grid_for caps at 4096 * 256 threads.  One
# input row and three columns per image keep the tensor small: 8200 * 2 * 64 = 1 049 600 threads, 6.3 M input floats.
POOL_GRID_STRIDE_CASE = (8200, 256, 1, 3)


def pool_out(h):
    return (h + 2 - 3) // 2 + 1


def pool_threads(n, c, h, w):
    return n * ((pool_out(h) + POOL_STRIP - 1) // POOL_STRIP) * pool_out(w) * (c // 4)


@functools.lru_cache(maxsize=4)
def pool_inputs(n, c, h, w, special=True):
    """fp32 NCHW x, not post-ReLU: negative values and windows whose maximum is negative, exact ties (a third of the
    values on a grid of halves), and with `special` a corner block of -inf (windows that hold nothing else) and scattered
    NaNs (windows with one and with two)"""
    g = gen(4700 + 13 * n + 7 * c + 3 * h + w)
    x = torch.randn(n, c, h, w, generator=g) - 0.3
    coarse = torch.rand(n, c, h, w, generator=g) < 0.35
    x = torch.where(coarse, (x * 2).round() / 2, x)
    if special:
        x[:, ::2, :max(1, h // 3), :max(1, w // 3)] = float('-inf')
        x = torch.where(torch.rand(n, c, h, w, generator=g) < 0.04, torch.full_like(x, float('nan')), x)
    return x


def pool_expected(x):
    """(values, tap index uint8) of the 3x3 stride-2 pad-1 pool of NCHW x on the CPU: torch's scan takes the first element
    of a window, then a strictly greater value or any NaN (the last NaN wins).
    tap = (iy - (2 oy - 1)) * 3 + (ix - (2 ox - 1)) from return_indices."""
    w = x.shape[3]
    y, ind = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    oy = torch.arange(y.shape[2])[:, None]
    ox = torch.arange(y.shape[3])[None, :]
    tap = (ind // w - (2 * oy - 1)) * 3 + (ind % w - (2 * ox - 1))
    assert int(tap.min()) >= 0 and int(tap.max()) <= 8
    return y, tap.to(torch.uint8)


def same_bits(a, b):
    """torch.equal on the bit patterns: NaN equals NaN, +0 differs from -0"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def pool_scan(x):
    """the kernel's rule restated in plain torch (the stand-in): taps in row-major order, the first valid one is taken,
    then a strictly greater value or a NaN"""
    n, c, h, w = x.shape
    oh, ow = pool_out(h), pool_out(w)
    xp = F.pad(x, (1, 2, 1, 2), value=0.0)
    ok_map = F.pad(torch.ones(h, w, dtype=torch.bool), (1, 2, 1, 2), value=False)
    best = torch.full((n, c, oh, ow), float('-inf'))
    bi = torch.zeros(n, c, oh, ow, dtype=torch.uint8)
    seen = torch.zeros(oh, ow, dtype=torch.bool)
    for tap in range(9):
        dy, dx = divmod(tap, 3)
        v = xp[:, :, dy:dy + 2 * oh:2, dx:dx + 2 * ow:2]
        ok = ok_map[dy:dy + 2 * oh:2, dx:dx + 2 * ow:2]
        take = ok & (~seen | (v > best) | torch.isnan(v))
        best, bi = torch.where(take, v, best), torch.where(take, torch.full_like(bi, tap), bi)
        seen = seen | ok
    return best, bi


def pool_bwd_reference(dy, tap, act, scale):
    """backward of the pool fused with the ReLU gate and a per-channel scale, fp64, NCHW: (grad * (act > 0) * scale, the
    same on magnitudes).  A NaN or -inf in act closes the gate."""
    n, c, h, w = act.shape
    oh, ow = dy.shape[2], dy.shape[3]
    t = tap.long()
    iy = 2 * torch.arange(oh)[:, None] - 1 + t // 3
    ix = 2 * torch.arange(ow)[None, :] - 1 + t % 3
    flat = (iy * w + ix).view(n, c, -1)
    grad = torch.zeros(n, c, h * w, dtype=torch.float64).scatter_add_(2, flat, dy.double().view(n, c, -1))
    mag = torch.zeros(n, c, h * w, dtype=torch.float64).scatter_add_(2, flat, dy.double().abs().view(n, c, -1))
    s = scale.double()[None, :, None, None]
    gate = act > 0
    zero = torch.zeros(n, c, h, w, dtype=torch.float64)
    return torch.where(gate, grad.view(n, c, h, w) * s, zero), torch.where(gate, mag.view(n, c, h, w) * s.abs(), zero)


def pool_bwd_bars(dx, ref):
    """a pixel sums at most four window gradients (three roundings) and multiplies by the scale (one):
    4u scale sum |contributions|; a closed gate or an untouched pixel must be exactly 0."""
    return worst(dx, ref[0], 4 * U * ref[1])


def pool_bwd_standin(dy, tap, act, scale):
    n, c, h, w = act.shape
    t = tap.long()
    iy = 2 * torch.arange(dy.shape[2])[:, None] - 1 + t // 3
    ix = 2 * torch.arange(dy.shape[3])[None, :] - 1 + t % 3
    grad = torch.zeros(n, c, h * w).scatter_add_(2, (iy * w + ix).view(n, c, -1), dy.reshape(n, c, -1))
    return torch.where(act > 0, grad.view(n, c, h, w) * scale[None, :, None, None], torch.zeros(n, c, h, w))


# ===================================================================================================== FPN helpers
UPSAMPLE_GEOMS = [((7, 9), (14, 18)), ((7, 9), (13, 17)), ((7, 9), (7, 9)), ((1, 1), (2, 1)), ((25, 42), (50, 84)),
                  ((25, 42), (49, 83))]
UPSAMPLE_CHANNELS = (4, 36, 256)
UPSAMPLE_BATCHES = (1, 2)
SUBSAMPLE_CASES = [(2, 7, 9, 4), (2, 8, 10, 68), (1, 7, 10, 68), (3, 8, 9, 4), (2, 1, 1, 4)]     # n, h, w, c
ADD_N4 = (1, 255, 256, GRID_CAP * 256 + 3)     # the last: a grid-stride second pass
# where the kernel's exact integer rule and torch's float rule give the same source index for every fine pixel
INDEX_RULE_LIMIT = 1500
INDEX_RULE_COUNTEREXAMPLE = (820, 1122)        # (h, H)


def fpn_coarse_extents(H):
    """the coarse extents the FPN pairs with a fine extent H: the next level of a stride-2 conv or pool, or H itself"""
    return sorted({(H + 1) // 2, max(1, H // 2), H})


def nearest_src_exact(H, h):
    """upsample_nearest_bwd_kernel's rule: fine Y reads coarse floor(Y h / H), in integers"""
    return (torch.arange(H) * h) // H


def nearest_src_float(H, h):
    """torch's rule (nearest_neighbor_compute_source_index): min(floorf(Y * (float)h / (float)H), h - 1), all in fp32"""
    scale = torch.tensor(float(h), dtype=torch.float32) / torch.tensor(float(H), dtype=torch.float32)
    return (torch.arange(H, dtype=torch.float32) * scale).floor().clamp_max(h - 1).long()


def upsample_reference(g_fine, h, w):
    """fp64 autograd of F.interpolate(coarse [n, c, h, w], size=(H, W), mode='nearest') for the fine gradient g_fine"""
    n, c, H, W = g_fine.shape
    z = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
    F.interpolate(z, size=(H, W), mode='nearest').backward(g_fine.double())
    return z.grad


def upsample_bars(got, g_fine, base, h, w):
    """worst ratio of g_coarse.  A coarse pixel adds its P preimage values to the base (0 without accumulate) in fp32:
    P roundings, each on a partial sum no larger than sum |terms| + |base|: (P + 1) u (sum |terms| + |base|)."""
    ref, mag = upsample_reference(g_fine, h, w), upsample_reference(g_fine.abs(), h, w)
    pre = upsample_reference(torch.ones_like(g_fine), h, w)
    if base is not None:
        ref, mag = ref + base.double(), mag + base.double().abs()
    return worst(got, ref, (pre + 1) * U * mag)


def upsample_standin(g_fine, h, w, base=None, miss_row_of=None, dtype=torch.float32):
    """the kernel's integer rule in plain torch: coarse (y, x) sums rows [ceil(y H / h), ceil((y + 1) H / h)) x columns
    likewise, row-major.  miss_row_of: coarse pixel (y, x) that skips the last row of its preimage (the injected fault)"""
    n, c, H, W = g_fine.shape
    out = torch.zeros(n, c, h, w, dtype=dtype) if base is None else base.to(dtype).clone()
    g = g_fine.to(dtype)
    for y in range(h):
        y0, y1 = -((-y * H) // h), -((-(y + 1) * H) // h)
        for x in range(w):
            x0, x1 = -((-x * W) // w), -((-(x + 1) * W) // w)
            rows = range(y0, y1 - 1) if miss_row_of == (y, x) else range(y0, y1)
            for yy in rows:
                for xx in range(x0, x1):
                    out[:, :, y, x] += g[:, :, yy, xx]
    return out
