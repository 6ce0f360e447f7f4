"""Thin Python host over the C ABI: descriptor builders and launch helpers.

Tensors are torch-ROCm allocations used for STORAGE ONLY (NHWC fp32); every arithmetic op on
the hot path goes through libhnd_hip.so.  Launch objects are built once per geometry and
replayed each step (no per-step ctypes struct construction).
"""
import ctypes as C
import os
import math

import torch

from . import _lib
from ._lib import ConvDesc, WgradDesc, MsePair, MimicPair, MIMIC_KINDS, check

_L = _lib.load()
TILE_NAMES = {code: name for name, code in _lib.CONV_TILES.items()}          # enum hnd_conv_tile
WGRAD_NAMES = {code: name for name, code in _lib.WGRAD_VARIANTS.items()}     # enum hnd_wgrad_variant
# advanced by every fused optimizer step: packed-weight caches (engine.weight_version) key on it because the raw-pointer
# parameter update does not touch torch's tensor version counter
PARAM_EPOCH = [0]


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def round_up(x, m):
    return (x + m - 1) // m * m


def chan_pad_of(c):
    """channel stride used for a logical channel count: the kernels take cin == 4 or cin % 32 == 0, so the
    3-channel image / bottleneck is stored as 4 and other bottleneck widths (6, 9, 12, 15) as 32."""
    return 4 if c <= 4 else round_up(c, 32)


def sync_check():
    check(_L.hnd_sync_check(stream_ptr()), 'hnd_sync_check')


def device_arch():
    return (_L.hnd_device_arch() or b'').decode()


# --------------------------------------------------------------------------------------- weights
# fp32 EMULATED on the bf16 matrix pipe (csrc/conv_bx3.hip) is the DEFAULT for the launches it covers since round 6
# (VERDICT r5 item 1): a launch carries a three-plane bf16 image of its packed operand when hnd_bf16x3_recommended says so
# for its LAYER (rows one image contributes, depth, output channels -- never the batch).
# Covered launches compute with fp32-level accuracy (0.8x the native kernel's error against fp64) but NOT the fp32 kernels'
# bits.  HND_BF16X3=0: no image anywhere, native fp32 MFMA everywhere (the `value_native_fp32` leg of bench.py).
#   mode 'policy' (default) / 'off' / 'force' (tests: attach an image whenever the operand can have one, whatever the
#   policy says) / 'bx3' / 'bxs' (force that one family, attach no image of the other).  Read by conv_desc only.
BX3_MODE = ['policy' if os.environ.get('HND_BF16X3', '1') != '0' else 'off']


def bx3_on():
    return BX3_MODE[0] != 'off'


class emulation(object):
    """with ops.emulation('off' | 'policy' | 'force' | 'bx3' | 'bxs'): ... -- launches BUILT inside take that mode (tests
    hold the native and the emulated family side by side with it)."""

    def __init__(self, mode):
        assert mode in ('policy', 'off', 'force', 'bx3', 'bxs'), mode
        self.mode = mode

    def __enter__(self):
        self.saved, BX3_MODE[0] = BX3_MODE[0], self.mode
        return self

    def __exit__(self, *exc):
        BX3_MODE[0] = self.saved
        return False


def emulation_unless(allowed):
    """context: launches built inside stay on native fp32 MFMA unless `allowed`"""
    import contextlib
    return contextlib.nullcontext() if allowed else emulation('off')


def bxs_recommended(rows_per_image, kdim, cout, taps):
    """the B-streamed emulation kernel, by LAYER (never by batch): hnd_bf16x3s_recommended"""
    return bool(_L.hnd_bf16x3s_recommended(int(rows_per_image), int(kdim), int(cout), int(taps)))


def bx3_recommended(rows_per_image, kdim, cout):
    return bool(_L.hnd_bf16x3_recommended(int(rows_per_image), int(kdim), int(cout)))


# The two image builders take a packed fp32 buffer and (re)build its image into `out`, or into a new tensor.
def bx3_image(buf, rows_pad, kdim, groups=1, group_stride=0, out=None):
    """the bf16x3 image (hnd_pack_bf16x3: the B-resident emulation kernel, csrc/conv_bx3.hip)"""
    if out is None:
        out = torch.empty(int(_L.hnd_pack_bf16x3_elems(rows_pad, kdim, groups)), dtype=torch.int16, device=buf.device)
    check(_L.hnd_pack_bf16x3(buf.data_ptr(), out.data_ptr(), rows_pad, kdim, groups, int(group_stride), stream_ptr()),
          'hnd_pack_bf16x3')
    return out


def bxs_image(buf, rows_pad, kdim, groups=1, group_stride=0, out=None):
    """the STREAM image (hnd_pack_bf16x3s: the B-streamed emulation kernel, csrc/conv_bxs.hip)"""
    if out is None:
        out = torch.empty(int(_L.hnd_pack_bf16x3s_elems(rows_pad, kdim, groups)), dtype=torch.int16, device=buf.device)
    check(_L.hnd_pack_bf16x3s(buf.data_ptr(), out.data_ptr(), rows_pad, kdim, groups, int(group_stride), stream_ptr()),
          'hnd_pack_bf16x3s')
    return out


class PackedWeight(object):
    """A GEMM weight operand: `groups` fp32 matrices [rows_pad][kdim] (K contiguous), `group_stride` floats apart in `buf`;
    K holds `taps` taps of chan_pad channels (chan_real of them real).  The subclasses fill `buf` from a conv weight
    (pack_weights, WinoWeights, Wino2Weights); a PackedWeight itself wraps a buffer its caller filled.

    The pre-split bf16 images of the emulation kernels (bx3, bxs) are made when a launch descriptor first asks for one
    (attach) and from then on re-made in place by every repack(), for as long as the operand lives.  An image set from
    outside (bx3_image) is the one a launch gets, and re-packs refresh it too."""
    groups, group_stride, taps, bx3, bxs = 1, 0, 1, None, None          # an ungrouped, tap-free operand without images

    def __init__(self, buf, rows, kdim, chan_pad, chan_real=None, groups=1, group_stride=0, taps=1):
        self.buf, self.rows, self.rows_pad, self.kdim = buf, rows, round_up(rows, 64), kdim
        self.chan_pad, self.chan_real = chan_pad, chan_pad if chan_real is None else chan_real
        self.groups, self.group_stride, self.taps = groups, group_stride, taps
        self.bx3 = self.bxs = None

    def fill(self):
        """(re)compute buf from the source weight (nothing to do for a buffer the caller filled)"""

    def repack(self):
        self.fill()
        self.refresh_images()

    def refresh_images(self):
        if self.bx3 is not None:
            bx3_image(self.buf, self.rows_pad, self.kdim, self.groups, self.group_stride, out=self.bx3)
        if self.bxs is not None:
            bxs_image(self.buf, self.rows_pad, self.kdim, self.groups, self.group_stride, out=self.bxs)

    def can_bx3(self):
        return (self.taps == 1 and self.kdim == self.chan_pad and self.rows_pad % 64 == 0          # tap-free operands only
                and (self.kdim == 128 or (self.kdim % 256 == 0 and self.kdim <= 2048)))

    def can_bxs(self):
        return (self.groups == 1 and self.kdim % 128 == 0 and self.chan_pad % 64 == 0 and self.rows_pad % 64 == 0
                and self.kdim == self.taps * self.chan_pad)

    def attach(self, which):
        """the image ('bx3' / 'bxs') a launch descriptor is about to point at, made now if it is the first to ask;
        None when the kernel cannot use this operand"""
        if which == 'bx3':
            if self.bx3 is None and self.can_bx3():
                self.bx3 = bx3_image(self.buf, self.rows_pad, self.kdim, self.groups, self.group_stride)
            return self.bx3
        if self.bxs is None and self.can_bxs():
            self.bxs = bxs_image(self.buf, self.rows_pad, self.kdim, self.groups, self.group_stride)
        return self.bxs


class DirectWeights(PackedWeight):
    """One conv weight packed for the direct launches (hnd_pack_weights).  w: torch OIHW parameter (device, contiguous);
    taps = (i0, istep, ni, j0, jstep, nj) or None = all.  kscale: per-channel scale of the GEMM's K operand folded into
    the packed weights (hnd_scale_packed_k)."""
    def __init__(self, w, transposed=False, chan_pad=None, taps=None, kscale=None):
        cout, cin, kh, kw = w.shape
        assert w.is_contiguous() and w.dtype == torch.float32
        if taps is None:
            taps = (0, 1, kh, 0, 1, kw)
        i0, istep, ni, j0, jstep, nj = taps
        chans = cout if transposed else cin
        rows = cin if transposed else cout
        if chan_pad is None:
            chan_pad = chan_pad_of(chans)
        kdim = round_up(ni * nj * chan_pad, 32)
        PackedWeight.__init__(self, torch.empty(round_up(rows, 64) * kdim, dtype=torch.float32, device=w.device), rows,
                              kdim, chan_pad, chans, taps=ni * nj)
        self.src, self.kscale = w, kscale
        self.args = (cout, cin, kh, kw, int(transposed), chan_pad, i0, istep, ni, j0, jstep, nj)
        self.repack()

    def repack(self):
        if PACK_BATCH['open'] and self.kscale is None:
            PACK_BATCH['items'].append(self)        # flushed as ONE launch by pack_batch_end()
        else:
            PackedWeight.repack(self)

    def fill(self):
        check(_L.hnd_pack_weights(self.src.data_ptr(), self.buf.data_ptr(), *self.args, stream_ptr()), 'hnd_pack_weights')
        if self.kscale is not None:         # a per-channel scale of the K operand folded into the weights
            check(_L.hnd_scale_packed_k(self.buf.data_ptr(), self.rows_pad, self.kdim, self.taps, self.chan_pad,
                                        self.kscale.data_ptr(), min(self.kscale.numel(), self.chan_pad), stream_ptr()),
                  'hnd_scale_packed_k')


pack_weights = DirectWeights


# A caller that refreshes many small operands in a row (the trainable head after every optimizer step) brackets the loop
# with pack_batch_begin() / pack_batch_end(): the DirectWeights.repack() calls in between are collected into one batched
# launch.
PACK_BATCH = {'open': False, 'items': []}


def pack_batch_begin():
    PACK_BATCH['open'], PACK_BATCH['items'] = True, []


def pack_batch_end():
    from ._lib import PackDesc
    items, PACK_BATCH['open'], PACK_BATCH['items'] = PACK_BATCH['items'], False, []
    if not items:
        return
    arr = (PackDesc * len(items))()
    for d, pw in zip(arr, items):
        d.src, d.dst = pw.src.data_ptr(), pw.buf.data_ptr()
        (d.cout, d.cin, d.kh, d.kw, d.transposed, d.chan_pad, d.i0, d.istep, d.ni, d.j0, d.jstep, d.nj) = pw.args
    check(_L.hnd_pack_weights_batched(arr, len(items), stream_ptr()), 'hnd_pack_weights_batched')
    for pw in items:
        pw.refresh_images()


def fbn_fold(weight, bias, mean, var, eps=0.0, cs=None, out=None):
    c = weight.numel()
    cs = cs or c
    if out is not None:
        scale, shift = out
        assert scale.numel() == cs and shift.numel() == cs
    else:
        scale = torch.empty(cs, dtype=torch.float32, device=weight.device)
        shift = torch.empty(cs, dtype=torch.float32, device=weight.device)
    check(_L.hnd_fbn_fold(ptr(weight), ptr(bias), ptr(mean), ptr(var), ptr(scale), ptr(shift), c, cs, float(eps),
                          stream_ptr()), 'hnd_fbn_fold')
    return scale, shift


# --------------------------------------------------------------------------------------- conv launches
class ConvLaunch(object):
    """One prebuilt hnd_conv2d_igemm launch (descriptor + keep-alive references)."""
    __slots__ = ('desc', 'ref', 'keep', 'flops', 'alg_flops', 'variant', 'build', 'relay')

    def __init__(self, desc, keep, flops=0):
        self.desc, self.keep, self.flops = desc, keep, flops
        self.alg_flops = flops      # 2*MAC of the convolution this launch stands for (== flops unless Winograd)
        self.ref = C.byref(desc)
        self.relay = None
        # which kernel instantiation hnd_conv2d_igemm dispatches to (mirrors csrc/conv_igemm.hip)
        self.refresh_variant()

    def refresh_variant(self):
        """call again after editing the descriptor or the picker's environment: the dispatch may change"""
        need = int(_L.hnd_conv2d_igemm_workspace(self.ref))
        if need == 0:
            self.relay, self.desc.relay_ws = None, None
        elif self.relay is None or self.relay.numel() * 4 < need:
            # work-balancing workspace of the B-streamed kernel: zero-filled once, owned by this launch object
            self.relay = torch.zeros((need + 3) // 4, dtype=torch.float32, device=torch.device('cuda', torch.cuda.current_device()))
            self.desc.relay_ws = self.relay.data_ptr()
        tile = _L.hnd_conv2d_igemm_tile(self.ref)
        name = TILE_NAMES[tile]
        self.variant = name if self.desc.cin != 4 or name == 'stem7_lds' else 'igemm_c4_128x64'
        # which build of that kernel (the emulation kernel has two that give the same bits); None: no such distinction
        self.build = ('persistent', 'tiled')[int(_L.hnd_conv2d_igemm_build(self.ref))] if name == 'bx3_64' else None

    def run(self, stream=None):
        rc = _L.hnd_conv2d_igemm(self.ref, stream if stream is not None else stream_ptr())
        if rc:
            check(rc, 'hnd_conv2d_igemm')


def _nhwc(t):
    assert t.dim() == 4 and t.is_contiguous() and t.dtype == torch.float32, (t.shape, t.stride(), t.dtype)
    return t.shape


def conv_desc(x, pw, y, *, kh, kw, oh, ow, sh, dh, bh, sw, dw, bw, cout, y_sh=1, y_oh=0, y_sw=1, y_ow=0,
              pro_scale=None, pro_shift=None, pro_relu=False, epi_scale=None, epi_shift=None, res1=None,
              res1_up=False, res2=None, mask=None, relu=False, stats=None, mask_bits=None, mask_out=None,
              bwd_stats=None, rows_per_image=None, w_group_rows=0):
    """Generic descriptor (see include/hnd_hip.h).  x, y, res*, mask are NHWC tensors; mask_bits / mask_out are uint8
    ReLU-mask nibble tensors of y's geometry with a quarter of its channels (mask_nibbles_like).
    bwd_stats = (x_raw, scale, shift, mean, rstd, relu): `stats` receives the BatchNorm-backward partials of the stored
    y (hnd_conv_desc.bwd_x) instead of its sum / sum of squares.
    rows_per_image: GEMM rows ONE image contributes (default oh * ow; the Winograd launches fold the batch into ow and say
    components x tiles per image): what hnd_bf16x3_recommended prices the emulation kernel on -- never the batch.
    w_group_rows: GEMM rows that each of the pw.groups weight matrices of a grouped operand multiplies (the Winograd
    component GEMMs: tiles per component)."""
    n, h, w, cin = _nhwc(x)
    ny, yh, yw, ldc = _nhwc(y)
    assert ny == n and pw.kdim >= kh * kw * cin and pw.chan_pad == cin, (pw.kdim, kh, kw, cin, pw.chan_pad)
    assert (pw.groups > 1) == (w_group_rows > 0), (pw.groups, w_group_rows)
    if pro_scale is not None and pro_shift is None:
        pro_shift = _zeros(cin, x.device)
    d = ConvDesc()
    d.x, d.w, d.y = ptr(x), ptr(pw.buf), ptr(y)
    d.pro_scale, d.pro_shift = ptr(pro_scale), ptr(pro_shift)
    d.epi_scale, d.epi_shift = ptr(epi_scale), ptr(epi_shift)
    d.res1, d.res2, d.mask, d.stats = ptr(res1), ptr(res2), ptr(mask), ptr(stats)
    d.n, d.h, d.w_, d.cin = n, h, w, cin
    d.oh, d.ow, d.yh, d.yw, d.cout, d.ldc = oh, ow, yh, yw, cout, ldc
    d.y_sh, d.y_oh, d.y_sw, d.y_ow = y_sh, y_oh, y_sw, y_ow
    d.kh, d.kw = kh, kw
    d.sh, d.dh, d.bh, d.sw, d.dw, d.bw = sh, dh, bh, sw, dw, bw
    d.kdim = pw.kdim
    d.w_group_rows, d.w_group_stride = w_group_rows, pw.group_stride
    d.pro_relu, d.relu = int(pro_relu), int(relu)
    if res1 is not None and res1_up:
        d.res1_mode, d.res1_h, d.res1_w = 1, res1.shape[1], res1.shape[2]
        assert res1.shape[0] == n and res1.shape[3] == ldc
    elif res1 is not None:
        assert tuple(res1.shape) == tuple(y.shape)
    for t in (res2, mask):
        assert t is None or tuple(t.shape) == tuple(y.shape)
    for t in (mask_bits, mask_out):
        assert t is None or (t.dtype == torch.uint8 and t.is_contiguous() and ldc % 4 == 0
                             and tuple(t.shape) == (ny, yh, yw, ldc // 4)), (None if t is None else t.shape, y.shape)
    assert mask is None or mask_bits is None
    d.mask_bits, d.mask_out = ptr(mask_bits), ptr(mask_out)
    # fp32 emulated on the bf16 matrix pipe: by layer, never by batch
    rpi, mode = oh * ow if rows_per_image is None else rows_per_image, BX3_MODE[0]
    if mode in ('force', 'bx3') or (mode == 'policy' and bx3_recommended(rpi, pw.kdim, cout)):
        d.w_bf16x3 = ptr(pw.attach('bx3'))
    # ... and its B-streamed build for what the B-resident kernel does not take (taps, long K, strided outputs, statistics)
    if mode in ('force', 'bxs') or (mode == 'policy' and bxs_recommended(rpi, pw.kdim, cout, kh * kw)):
        d.w_bf16x3s = ptr(pw.attach('bxs'))
    if stats is not None:
        assert stats.numel() >= stats_tiles(n * oh * ow) * 2 * cout
    if bwd_stats is not None:
        bx, bsc, bsh, bmu, brs, brelu = bwd_stats
        assert stats is not None and tuple(bx.shape) == tuple(y.shape) and cout == ldc
        assert res1 is None and res2 is None and mask is None and mask_bits is None and not relu
        assert min(t.numel() for t in (bsc, bsh, bmu, brs)) >= ldc
        d.bwd_x, d.bwd_scale, d.bwd_shift, d.bwd_mean, d.bwd_rstd = ptr(bx), ptr(bsc), ptr(bsh), ptr(bmu), ptr(brs)
        d.bwd_relu = int(brelu)
    keep = (x, pw, y, pro_scale, pro_shift, epi_scale, epi_shift, res1, res2, mask, stats, mask_bits, mask_out,
            bwd_stats)                  # (pw holds its images: once made they live as long as it does)
    return ConvLaunch(d, keep, flops=2 * n * oh * ow * min(cout, pw.rows) * kh * kw * min(cin, pw.chan_real))


_ZEROS = {}


def _zeros(n, device):
    key = (n, str(device))
    if key not in _ZEROS:
        _ZEROS[key] = torch.zeros(n, dtype=torch.float32, device=device)
    return _ZEROS[key]


def stats_tiles(m):
    return (m + 127) // 128


def conv_out_size(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def conv_forward(x, pw, y, k, stride=1, pad=0, **kw_):
    """nn.Conv2d(k, stride, pad) forward: x [N,H,W,Cin] -> y [N,OH,OW,ldc]; cout defaults to pw.rows."""
    kh, kwid = (k, k) if isinstance(k, int) else k
    n, h, w, cin = x.shape
    oh, ow = conv_out_size(h, kh, stride, pad), conv_out_size(w, kwid, stride, pad)
    assert (y.shape[1], y.shape[2]) == (oh, ow), (y.shape, oh, ow)
    cout = kw_.pop('cout', y.shape[3])     # pad channels get zero weight rows -> written as exact zeros
    assert cout <= round_up(pw.rows, 64)
    return conv_desc(x, pw, y, kh=kh, kw=kwid, oh=oh, ow=ow, sh=stride, dh=1, bh=-pad, sw=stride, dw=1, bw=-pad,
                     cout=cout, **kw_)


def dgrad_tap_classes(k, stride, pad):
    """Per output parity ph: (i0, istep, ni, bh) of the taps that reach it (stride-s conv, kernel k, pad p)."""
    out = []
    for ph in range(stride):
        i0 = (ph + pad) % stride
        ni = len(range(i0, k, stride))
        bh = (ph + pad - i0) // stride
        out.append((i0, stride, ni, bh))
    return out


def conv_dgrad(dy, w_param, dx, k, stride=1, pad=0, accumulate=False, fold_scale=None, **kw_):
    """Data gradient of nn.Conv2d(k, stride, pad): dy [N,OH,OW,Cout] -> dx [N,H,W,Cin_pad].
    fold_scale: per-output-channel scale s of a frozen affine between the conv and dy (FrozenBatchNorm2d):
    W^T (dy * s) is computed as (W^T diag(s)) dy with s folded into the packed operand -- no prologue on the launch.
    w_param: the OIHW weight tensor, or an object with .weight and .get(transposed, chan_pad, taps) (engine
    WeightCache) so the transposed operands are cached and refreshed with the parameter.
    Returns (launches, packed_weights).  Stride 2 is decomposed into one dense launch per output parity.
    With accumulate=True each launch adds into dx (res1 = dx), which also lets tap-less parities be skipped."""
    n, h, w, ldc = dx.shape
    cache = None
    if not isinstance(w_param, torch.Tensor):
        cache, w_param = w_param, w_param.weight
    cout_w, cin_w, kh, kwid = w_param.shape
    assert kh == k and kwid == k and dy.shape[3] == chan_pad_of(cout_w)
    launches, packs = [], []
    classes = dgrad_tap_classes(k, stride, pad)
    for ph, (i0, istep, ni, bh) in enumerate(classes):
        for pw_, (j0, jstep, nj, bw) in enumerate(classes):
            if ni == 0 or nj == 0:
                assert accumulate, 'tap-less output parity: caller must accumulate into a defined dx'
                continue
            ohv, owv = len(range(ph, h, stride)), len(range(pw_, w, stride))
            if ohv == 0 or owv == 0:
                continue
            taps = (i0, istep, ni, j0, jstep, nj)
            if cache is not None:
                pk = cache.get(True, dy.shape[3], taps, kscale=fold_scale)
            else:
                pk = pack_weights(w_param, transposed=True, chan_pad=dy.shape[3], taps=taps, kscale=fold_scale)
            packs.append(pk)
            extra = dict(kw_)
            if accumulate:
                extra['res1'] = dx
            launches.append(conv_desc(dy, pk, dx, kh=ni, kw=nj, oh=ohv, ow=owv, sh=1, dh=-1, bh=bh, sw=1, dw=-1,
                                      bw=bw, cout=ldc, y_sh=stride, y_oh=ph, y_sw=stride,
                                      y_ow=pw_, **extra))
    return launches, packs


class WgradLaunch(object):
    __slots__ = ('desc', 'ref', 'keep', 'flops', 'alg_flops', 'variant')

    def __init__(self, desc, keep, flops):
        self.desc, self.keep, self.flops = desc, keep, flops
        self.alg_flops = flops
        self.ref = C.byref(desc)
        # which kernel hnd_conv2d_wgrad dispatches to (asked of the library: csrc/conv_wgrad.hip)
        name = WGRAD_NAMES[int(_L.hnd_conv2d_wgrad_variant(self.ref))]
        self.variant = name if name != 'staged' else 'wgrad_m128' if desc.cout >= 128 else 'wgrad_m64'

    def run(self, stream=None):
        rc = _L.hnd_conv2d_wgrad(self.ref, stream if stream is not None else stream_ptr())
        if rc:
            check(rc, 'hnd_conv2d_wgrad')


def conv_wgrad(x, dy, dw, k, stride=1, pad=0, pro_scale=None, pro_shift=None, pro_relu=False, splitk=0,
               slabs=None):
    """dW of nn.Conv2d(k, stride, pad): x [N,H,W,Cin_pad], dy [N,OH,OW,ldy] -> dw [Cout,Cin,k,k] (torch layout)."""
    n, h, w, cin = _nhwc(x)
    _, oh, ow, ldy = _nhwc(dy)
    cout, cin_real, kh, kwid = dw.shape
    assert dw.is_contiguous() and kh == k and kwid == k
    d = WgradDesc()
    d.x, d.dy, d.dw = ptr(x), ptr(dy), ptr(dw)
    d.pro_scale, d.pro_shift, d.pro_relu = ptr(pro_scale), ptr(pro_shift), int(pro_relu)
    d.n, d.h, d.w_, d.cin, d.cin_real = n, h, w, cin, cin_real
    d.oh, d.ow, d.cout, d.ldy = oh, ow, cout, ldy
    d.kh, d.kw, d.stride, d.pad, d.splitk = k, k, stride, pad, splitk
    need = _L.hnd_conv2d_wgrad_workspace(C.byref(d))
    if slabs is None or slabs.numel() * 4 < need:
        slabs = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
    d.slabs = ptr(slabs)
    return WgradLaunch(d, (x, dy, dw, slabs, pro_scale, pro_shift), 2 * n * oh * ow * cout * k * k * cin_real)


def wgrad_workspace_of(desc):
    """bytes of split-K workspace hnd_conv2d_wgrad needs for a filled-in WgradDesc"""
    return int(_L.hnd_conv2d_wgrad_workspace(C.byref(desc)))


def wgrad_workspace_bytes(n, h, w, cin, oh, ow, cout, k, stride, pad):
    d = WgradDesc()
    d.n, d.h, d.w_, d.cin, d.cin_real, d.oh, d.ow, d.cout, d.ldy = n, h, w, cin, cin, oh, ow, cout, chan_pad_of(cout)
    d.kh, d.kw, d.stride, d.pad = k, k, stride, pad
    return _L.hnd_conv2d_wgrad_workspace(C.byref(d))


# --------------------------------------------------------------------------------------- elementwise
def transform_image(src, dst, index, out_h, out_w, rscale_h, rscale_w, mean, std):
    """src CHW fp32 -> image `index` of dst [N,Hp,Wp,4] (normalise, bilinear resize, zero pad)."""
    c, h, w = src.shape
    assert c == 3 and src.is_contiguous() and dst.shape[3] == 4
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    _hbm('transform_image', 12 * h * w + 16 * dst.shape[1] * dst.shape[2], lambda: check(
        _L.hnd_transform_image(ptr(src), h, w, ptr(dst), index, out_h, out_w, dst.shape[1], dst.shape[2],
                               float(rscale_h), float(rscale_w), m, s, stream_ptr()), 'hnd_transform_image'))


def transform_image_u8(src, dst, index, out_h, out_w, rscale_h, rscale_w, mean, std, hwc, flip=False):
    """src uint8 [H,W,3] (hwc) or [3,H,W] -> image `index` of dst [N,Hp,Wp,4]: /255, optional horizontal flip,
    normalise, bilinear resize, zero pad -- one pass."""
    assert src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 3 and dst.shape[3] == 4
    h, w = (src.shape[0], src.shape[1]) if hwc else (src.shape[1], src.shape[2])
    assert src.shape[2 if hwc else 0] == 3
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    check(_L.hnd_transform_image_u8(ptr(src), h, w, int(bool(hwc)), int(bool(flip)), ptr(dst), index, out_h, out_w,
                                    dst.shape[1], dst.shape[2], float(rscale_h), float(rscale_w), m, s, stream_ptr()),
          'hnd_transform_image_u8')


def transform_images(items, dst, mean, std):
    """The whole batch in one launch.  items: per image (src, is_u8, hwc, flip, out_h, out_w, rscale_h, rscale_w) with
    src fp32 [3,H,W] or uint8 [H,W,3] / [3,H,W]; image i lands in dst[i] of dst [N,Hp,Wp,4]."""
    from ._lib import ImageDesc
    assert dst.shape[3] == 4 and dst.shape[0] == len(items)
    arr = (ImageDesc * len(items))()
    nbytes = 0
    for d, (src, is_u8, hwc, flip, out_h, out_w, rh, rw) in zip(arr, items):
        assert src.is_contiguous() and src.dim() == 3 and src.dtype == (torch.uint8 if is_u8 else torch.float32)
        h, w = (src.shape[0], src.shape[1]) if (is_u8 and hwc) else (src.shape[1], src.shape[2])
        assert src.shape[2 if (is_u8 and hwc) else 0] == 3
        d.src, d.h, d.w, d.out_h, d.out_w = ptr(src), h, w, out_h, out_w
        d.is_u8, d.hwc, d.flip, d.scale_h, d.scale_w = int(is_u8), int(bool(hwc)), int(bool(flip)), float(rh), float(rw)
        nbytes += (3 if is_u8 else 12) * h * w + 16 * dst.shape[1] * dst.shape[2]
    m = (C.c_float * 3)(*mean)
    s = (C.c_float * 3)(*std)
    _hbm('transform_image', nbytes, lambda: check(
        _L.hnd_transform_images(arr, len(items), ptr(dst), dst.shape[1], dst.shape[2], m, s, stream_ptr()),
        'hnd_transform_images'))


def scale_boxes(items):
    """items: per image (boxes [k,4] fp32 device tensor, scale_w, scale_h) -> list of rescaled [k,4] tensors, one launch
    for the whole list (hnd_scale_boxes)."""
    from ._lib import BoxesDesc
    arr = (BoxesDesc * len(items))()
    outs = []
    for d, (bx, rw, rh) in zip(arr, items):
        assert bx.dtype == torch.float32 and bx.dim() == 2 and bx.shape[1] == 4 and bx.is_cuda
        src = bx if bx.is_contiguous() else bx.contiguous()
        out = torch.empty_like(src)
        d.src, d.dst, d.k, d.scale_w, d.scale_h = ptr(src), ptr(out), src.shape[0], float(rw), float(rh)
        outs.append((src, out))
    if items:
        check(_L.hnd_scale_boxes(arr, len(items), stream_ptr()), 'hnd_scale_boxes')
    return [o for _, o in outs]


# bench.py's hbm_roofline: HIP events (torch's current stream == the launch stream) around the HBM-bound launches
# that do not go through an engine plan entry, with the bytes each of them must move
HBM_PROFILE = {'enabled': False, 'records': []}


def _hbm(kernel, nbytes, call):
    if HBM_PROFILE['enabled']:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        HBM_PROFILE['records'].append((kernel, int(nbytes), e0, e1))
    else:
        call()


def maxpool_fwd(x, y, idx):
    n, h, w, c = x.shape
    _hbm('maxpool_fwd', x.numel() * 4 + y.numel() * 4 + idx.numel() * idx.element_size(), lambda: check(
        _L.hnd_maxpool3x3s2_fwd(ptr(x), ptr(y), ptr(idx), n, h, w, c, y.shape[1], y.shape[2], stream_ptr()),
        'hnd_maxpool3x3s2_fwd'))


def maxpool_bwd_relu_scale(dy, idx, act, scale, dx):
    n, h, w, c = act.shape
    nbytes = dy.numel() * 4 + idx.numel() * idx.element_size() + act.numel() * 4 + dx.numel() * 4
    _hbm('maxpool_bwd', nbytes, lambda: check(
        _L.hnd_maxpool3x3s2_bwd_relu_scale(ptr(dy), ptr(idx), ptr(act), ptr(scale), ptr(dx), n, h, w, c,
                                           dy.shape[1], dy.shape[2], stream_ptr()), 'hnd_maxpool3x3s2_bwd_relu_scale'))


def bn_finalize(partials, ntiles, c, cs, count, gamma, beta, running_mean, running_var, nbt, momentum, eps,
                scale, shift, save_mean, save_rstd):
    check(_L.hnd_bn_finalize(ptr(partials), ntiles, c, cs, count, ptr(gamma), ptr(beta), ptr(running_mean),
                             ptr(running_var), ptr(nbt), momentum, eps, ptr(scale), ptr(shift), ptr(save_mean),
                             ptr(save_rstd), stream_ptr()), 'hnd_bn_finalize')


def mask_nibbles_like(y):
    """uint8 buffer for the ReLU-mask nibbles of NHWC tensor y: one byte per pixel and group of four channels"""
    assert y.shape[-1] % 4 == 0
    return torch.empty(tuple(y.shape[:-1]) + (y.shape[-1] // 4,), dtype=torch.uint8, device=y.device)


def relu_mask_nibbles(x, bits, stream=None):
    """bits = [x > 0] as nibbles (mask_nibbles_like(x)): for an activation that was stored without its mask"""
    assert bits.dtype == torch.uint8 and bits.numel() * 4 == x.numel() and x.is_contiguous()
    # (a plan entry -- engine's _Step carries its bytes for bench.py's table: no _hbm record here)
    check(_L.hnd_relu_mask_nibbles(ptr(x), ptr(bits), bits.numel(), stream if stream is not None else stream_ptr()),
          'hnd_relu_mask_nibbles')


def affine_relu(x, scale, shift, y, relu, mask_out=None):
    cs = x.shape[-1]
    assert mask_out is None or (mask_out.dtype == torch.uint8 and mask_out.numel() * 4 == y.numel())
    _hbm('affine_relu', 8 * x.numel() + (0 if mask_out is None else mask_out.numel()), lambda: check(
        _L.hnd_affine_relu(ptr(x), ptr(scale), ptr(shift), ptr(y), x.numel() // cs, cs, int(relu), ptr(mask_out),
                           stream_ptr()), 'hnd_affine_relu'))


def bn_bwd_ntiles(npix):
    return _L.hnd_bn_bwd_ntiles(npix)


def bn_bwd_reduce(g, x, scale, shift, mean, rstd, relu, partials):
    cs = x.shape[-1]
    _hbm('bn_bwd_reduce', 8 * x.numel(), lambda: check(
        _L.hnd_bn_bwd_reduce(ptr(g), ptr(x), ptr(scale), ptr(shift), ptr(mean), ptr(rstd), int(relu),
                             x.numel() // cs, cs, ptr(partials), stream_ptr()), 'hnd_bn_bwd_reduce'))


def bn_bwd_finalize(partials, ntiles, c, cs, count, gamma, mean, rstd, dgamma, dbeta, k123):
    check(_L.hnd_bn_bwd_finalize(ptr(partials), ntiles, c, cs, count, ptr(gamma), ptr(mean), ptr(rstd), ptr(dgamma),
                                 ptr(dbeta), ptr(k123), stream_ptr()), 'hnd_bn_bwd_finalize')


def bn_bwd_apply(g, x, scale, shift, k123, relu, dx):
    cs = x.shape[-1]
    _hbm('bn_bwd_apply', 12 * x.numel(), lambda: check(
        _L.hnd_bn_bwd_apply(ptr(g), ptr(x), ptr(scale), ptr(shift), ptr(k123), int(relu), ptr(dx),
                            x.numel() // cs, cs, stream_ptr()), 'hnd_bn_bwd_apply'))


# launches of each loss entry point so far (like HBM_PROFILE, host-side accounting only: which of the two a criterion
# section took -- an all-MSELoss(sum) one never takes the general entry point)
LOSS_LAUNCHES = {'hnd_mse_sum_fwd_bwd': 0, 'hnd_mimic_loss_fwd_bwd': 0}


class MseLaunch(object):
    """Prebuilt multi-pair fused loss + gradient launch."""

    def __init__(self, pairs, device):
        """pairs: list of (teacher, student, grad_or_None, factor, relu_mask)."""
        self.n = len(pairs)
        self.arr = (MsePair * self.n)()
        self.keep = pairs
        for i, (t, s, g, f, rm) in enumerate(pairs):
            assert t.numel() == s.numel() and t.is_contiguous() and s.is_contiguous()
            self.arr[i].teacher, self.arr[i].student, self.arr[i].grad = ptr(t), ptr(s), ptr(g)
            self.arr[i].numel, self.arr[i].factor, self.arr[i].relu_mask = t.numel(), float(f), int(rm)
        self.out = torch.zeros(1 + self.n, dtype=torch.float64, device=device)
        self.scratch = torch.empty(_L.hnd_mse_scratch_elems(), dtype=torch.float64, device=device)

    def run(self):
        nbytes = sum(4 * t.numel() * (3 if g is not None else 2) for t, s, g, f, rm in self.keep)
        LOSS_LAUNCHES['hnd_mse_sum_fwd_bwd'] += 1
        _hbm('mse', nbytes, lambda: check(
            _L.hnd_mse_sum_fwd_bwd(self.arr, self.n, ptr(self.out), ptr(self.scratch), stream_ptr()),
            'hnd_mse_sum_fwd_bwd'))
        return self.out


class MimicLaunch(object):
    """MseLaunch for any elementwise criterion and either reduction (hnd_mimic_loss_fwd_bwd): same caching contract, built
    once per set of pointers, run() returns the device double[1 + n] (total, per term)."""

    def __init__(self, pairs, device):
        """pairs: list of (teacher, student, grad_or_None, factor, relu_mask, kind, param, count); kind is a key of
        _lib.MIMIC_KINDS, param the beta / delta, count the LOGICAL element count a mean divides by (0 = sum).
        Pairs that name the SAME grad tensor (and the same student) form a group: the launch reads the student once, adds
        the gradients of the members in pair order and stores the sum once."""
        self.n = len(pairs)
        self.arr = (MimicPair * self.n)()
        self.keep = pairs
        for a, (t, s, g, f, rm, kind, param, count) in zip(self.arr, pairs):
            assert t.numel() == s.numel() and t.is_contiguous() and s.is_contiguous()
            assert g is None or (g.numel() == s.numel() and g.is_contiguous())
            a.teacher, a.student, a.grad = ptr(t), ptr(s), ptr(g)
            a.numel, a.count, a.factor, a.param = t.numel(), int(count), float(f), float(param)
            a.kind, a.relu_mask = MIMIC_KINDS[kind], int(rm)
        self.out = torch.zeros(1 + self.n, dtype=torch.float64, device=device)
        self.scratch = torch.empty(_L.hnd_mse_scratch_elems(), dtype=torch.float64, device=device)

    def run(self):
        nbytes, grads = 0, set()
        for p in self.keep:                 # (a group: one read of the student and one write of grad for all its members)
            later = p[2] is not None and ptr(p[2]) in grads
            nbytes += 4 * p[0].numel() * (1 if later else 2 if p[2] is None else 3)
            grads.add(ptr(p[2]))
        LOSS_LAUNCHES['hnd_mimic_loss_fwd_bwd'] += 1
        _hbm('mse', nbytes, lambda: check(
            _L.hnd_mimic_loss_fwd_bwd(self.arr, self.n, ptr(self.out), ptr(self.scratch), stream_ptr()),
            'hnd_mimic_loss_fwd_bwd'))
        return self.out


def scale_by_device_scalar(x, scalar_dev):
    check(_L.hnd_scale_by_device_scalar(ptr(x), x.numel(), ptr(scalar_dev), stream_ptr()),
          'hnd_scale_by_device_scalar')


def adam_step_flat(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale=1.0):
    _hbm('adam', 28 * param.numel(), lambda: check(
        _L.hnd_adam_step_flat(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr),
                              float(beta1), float(beta2), float(eps), int(step), float(grad_scale), stream_ptr()),
        'hnd_adam_step_flat'))
    PARAM_EPOCH[0] += 1


def subsample2(x, y):
    n, h, w, c = x.shape
    check(_L.hnd_subsample2(ptr(x), ptr(y), n, h, w, c, y.shape[1], y.shape[2], stream_ptr()), 'hnd_subsample2')


def upsample_nearest_bwd(g_fine, g_coarse, accumulate):
    """backward of F.interpolate(coarse, size=fine.shape, mode='nearest'): g_coarse (+)= the sums of g_fine over the fine
    pixels that read each coarse one (NHWC, same channels).  Domain: the kernel's source index is the exact integer
    floor(Y h / H), torch's is floorf(Y * (float)h / (float)H); they agree for every H < 1500 with h in
    {ceil(H / 2), floor(H / 2), H} (neighbouring FPN levels), not for arbitrary pairs such as (h, H) = (820, 1122)."""
    n, H, W, c = g_fine.shape
    nc, h, w, cc = g_coarse.shape
    assert (n, c) == (nc, cc) and g_fine.is_contiguous() and g_coarse.is_contiguous()
    check(_L.hnd_upsample_nearest_bwd(ptr(g_fine), ptr(g_coarse), n, H, W, h, w, c, int(bool(accumulate)), stream_ptr()),
          'hnd_upsample_nearest_bwd')


def add_inplace(x, y):
    assert x.numel() == y.numel() and x.is_contiguous() and y.is_contiguous()
    check(_L.hnd_add_inplace(ptr(x), ptr(y), x.numel(), stream_ptr()), 'hnd_add_inplace')


def fill(x, value):
    check(_L.hnd_fill(ptr(x), x.numel(), float(value), stream_ptr()), 'hnd_fill')


def quantize_u8(x, c, q, qparams, scratch):
    cs = x.shape[-1]
    check(_L.hnd_quantize_u8(ptr(x), x.numel() // cs, c, cs, ptr(q), ptr(qparams), ptr(scratch), stream_ptr()),
          'hnd_quantize_u8')


def dequantize_u8(q, qparams, x, c):
    cs = x.shape[-1]
    check(_L.hnd_dequantize_u8(ptr(q), ptr(qparams), ptr(x), x.numel() // cs, c, cs, stream_ptr()),
          'hnd_dequantize_u8')


def minmax_scratch_elems():
    return _L.hnd_minmax_scratch_elems()


# ---- the argument checks of the quantiser wrappers below (codec, fake quantiser, fixed range, entropy coder, per channel).
# One set; `flavour` picks the texts, which every family keeps as its callers know them: 'range' (include/hnd_qrange.h),
# 'entropy' (include/hnd_entropy.h) or 'channel' (include/hnd_qchannel.h).  All raise ValueError; the codec and the batch
# fake quantiser assert their buffers as they always have.
def _q_bits(who, bits):
    if isinstance(bits, bool) or not isinstance(bits, int) or not 1 <= bits <= 8:
        raise ValueError('%s: bits=%r outside 1 ... 8' % (who, bits))
    return bits


def _q_geometry(who, x, c, flavour='range', dtype=torch.float32):
    """(npix, cs) of the NHWC buffer x with c real channels"""
    dims_ok = isinstance(x, torch.Tensor) and (x.dim() == 4 if flavour == 'entropy' else x.dim() >= 1)
    if not (dims_ok and x.dtype == dtype and x.is_contiguous()):
        raise ValueError('%s: needs a contiguous %s' % (who, {
            'range': 'fp32 NHWC buffer', 'entropy': '%s NHWC buffer [N, H, W, cs]' % dtype,
            'channel': '%s NHWC buffer' % str(dtype).replace('torch.', '')}[flavour]))
    cs = x.shape[-1]
    cmax = min(cs, QCHANNEL_MAX_C) if flavour == 'channel' else cs
    if isinstance(c, bool) or not isinstance(c, int) or not 0 < c <= cmax or cs % 4 or x.numel() == 0:
        raise ValueError('%s: c=%r real channels in a pixel stride of %d%s' % (who, c, cs, {
            'range': ' floats (0 < c <= stride, stride % 4 == 0)', 'entropy': ' (0 < c <= stride, stride % 4 == 0)',
            'channel': ' floats (0 < c <= stride, c <= %d, stride %% 4 == 0)' % QCHANNEL_MAX_C}[flavour]))
    return x.numel() // cs, cs


def _q_nhwc(who, x, flavour):
    if not (isinstance(x, torch.Tensor) and x.dim() == 4):
        raise ValueError('%s: %s' % (who, 'needs the NHWC buffer [N, H, W, cs]' if flavour == 'channel' else
                                     'x must be [N, H, W, cs]'))
    return x.shape


def _q_qparams(who, qparams, c=None):
    """per tensor (c None): at least the 4 values; per channel: exactly [c, 4]"""
    ok = isinstance(qparams, torch.Tensor) and qparams.dtype == torch.float32 and qparams.is_contiguous()
    if not (ok and (qparams.numel() >= 4 if c is None else qparams.numel() == 4 * c)):
        raise ValueError('%s: qparams must be a contiguous fp32 tensor %s' % (who, 'of 4 values' if c is None else '[%d, 4]' % c))
    return qparams


def _q_scratch(who, scratch, cs=None):
    """per tensor (cs None): minmax_scratch_elems() floats; per channel: qchannel_scratch_elems(cs), a contiguous tensor"""
    if cs is None:
        if not (scratch.dtype == torch.float32 and scratch.numel() >= minmax_scratch_elems()):
            raise ValueError('%s: scratch must hold minmax_scratch_elems() floats' % who)
    elif not (isinstance(scratch, torch.Tensor) and scratch.dtype == torch.float32 and scratch.is_contiguous()
              and scratch.numel() >= qchannel_scratch_elems(cs)):
        raise ValueError('%s: scratch must be a contiguous fp32 buffer of qchannel_scratch_elems(%d) = %d floats'
                         % (who, cs, qchannel_scratch_elems(cs)))
    return scratch


def _q_payload(who, payload, x, c, bits, flavour='range'):
    """the bit-packed payload of the c real channels of x [N, H, W, cs]: exactly codec_packed_bytes uint8 bytes"""
    n, h, w, _ = x.shape
    numel, nbytes = n * c * h * w, codec_packed_bytes(n * c * h * w, bits)
    if not ((flavour != 'channel' or isinstance(payload, torch.Tensor)) and payload.dtype == torch.uint8
            and payload.is_contiguous() and payload.numel() == nbytes > 0):
        raise ValueError('%s: payload must be %s' % (who, '%d uint8 bytes' % nbytes if flavour != 'channel' else
                                                     'a contiguous uint8 buffer of codec_packed_bytes(%d, %d) = %d bytes'
                                                     % (numel, bits, nbytes)))
    return payload


# `strict` in the three checkers below: the per-channel wrappers (and qrange_mask_grad) answer a non-tensor with their
# ValueError; the fixed-range wrappers never tested for one and let the attribute access fail.  Callers see either, so
# both stay.
def _q_like(who, name, t, x, dtype, strict):
    """`name` is a contiguous buffer of x's extent: a float destination (`out`) has x's shape, a byte destination (`q`)
    x's element count -- the codes are handed on flat as well as shaped"""
    same = (lambda: tuple(t.shape) == tuple(x.shape)) if dtype == torch.float32 else (lambda: t.numel() == x.numel())
    if not ((not strict or isinstance(t, torch.Tensor)) and t.dtype == dtype and t.is_contiguous() and same()):
        raise ValueError('%s: %s must be a contiguous %s buffer of x\'s shape'
                         % (who, name, 'fp32' if dtype == torch.float32 else 'uint8'))
    return t


def _q_stats(who, stats, npix, cs, strict):
    if stats is not None and not ((not strict or isinstance(stats, torch.Tensor)) and stats.dtype == torch.float32
                                  and stats.is_contiguous() and stats.numel() == fake_quantize_tiles(npix) * 2 * cs):
        raise ValueError('%s: stats must be a contiguous fp32 buffer [%d, 2, %d]' % (who, fake_quantize_tiles(npix), cs))
    return stats


def _q_mask(who, mask, npix, cs, strict):
    if not ((not strict or isinstance(mask, torch.Tensor)) and mask.dtype == torch.uint8 and mask.is_contiguous()
            and mask.numel() == npix * (cs // 4)):
        raise ValueError('%s: mask must be a contiguous uint8 buffer of %d bytes' % (who, npix * (cs // 4)))
    return mask


# include/hnd_codec.h: the codec at 1 ... 8 bits.  x is the NHWC fp32 buffer [N, H, W, cs] with c real channels.
def codec_packed_bytes(numel, bits):
    """bytes of the bit-packed payload of `numel` values at `bits` bits each: ceil(numel * bits / 8); 0 for bad arguments"""
    return int(_L.hnd_codec_packed_bytes(int(numel), int(bits)))


def quantize_bits(x, c, bits, q, qparams, scratch):
    """quantize_u8 with qmax = 2^bits - 1: one value per byte into q (uint8, x's shape), pad channels 0"""
    cs = x.shape[-1]
    assert q.numel() == x.numel() and q.dtype == torch.uint8
    check(_L.hnd_quantize_bits(ptr(x), x.numel() // cs, c, cs, int(bits), ptr(q), ptr(qparams), ptr(scratch),
                               stream_ptr()), 'hnd_quantize_bits')


def _assert_payload(payload, x, c, bits):
    n, h, w, cs = x.shape
    assert payload.dtype == torch.uint8 and payload.numel() == codec_packed_bytes(n * c * h * w, bits) > 0, \
        (tuple(payload.shape), (n, c, h, w), bits)
    return n, h, w, cs


def quantize_pack_bits(x, c, bits, payload, qparams, scratch):
    """quantise the c real channels of x and pack them, in logical NCHW order, LSB first, into the 1-D uint8 `payload` of
    exactly codec_packed_bytes(N * c * H * W, bits) bytes (format: include/hnd_codec.h)"""
    n, h, w, cs = _assert_payload(payload, x, c, bits)
    check(_L.hnd_quantize_pack_bits(ptr(x), n, h, w, c, cs, int(bits), ptr(payload), ptr(qparams), ptr(scratch),
                                    stream_ptr()), 'hnd_quantize_pack_bits')


def unpack_dequantize_bits(payload, qparams, x, c, bits):
    """the inverse: scale * (q - zero_point) into the c real channels of x [N, H, W, cs], 0 into its pad channels"""
    n, h, w, cs = _assert_payload(payload, x, c, bits)
    check(_L.hnd_unpack_dequantize_bits(ptr(payload), ptr(qparams), ptr(x), n, h, w, c, cs, int(bits), stream_ptr()),
          'hnd_unpack_dequantize_bits')


# include/hnd_qat.h: the fake-quantised bottleneck of the training step
def fake_quantize_tiles(npix):
    """rows of the `stats` buffer of fake_quantize_bits for npix pixels (128 pixels per row); 0 for npix <= 0"""
    return int(_L.hnd_fake_quantize_tiles(int(npix)))


def fake_quantize_bits(x, c, bits, qparams, scratch, out=None, stats=None):
    """quantise and dequantise the c real channels of x [N, H, W, cs] at `bits` bits in one pass -- the bits of
    dequantize_u8(quantize_bits(x)) -- into `out` (default: in place), 0 into the pad channels; `stats`
    [fake_quantize_tiles(npix), 2, cs] receives the per-tile (sum, sum of squares) of what was stored, for bn_finalize.
    Returns the destination."""
    _q_bits('fake_quantize_bits', bits)
    cs = x.shape[-1]
    npix = x.numel() // cs
    out = x if out is None else out
    assert x.is_contiguous() and out.is_contiguous() and x.dtype == out.dtype == torch.float32
    assert tuple(out.shape) == tuple(x.shape), (tuple(out.shape), tuple(x.shape))
    assert qparams.numel() >= 4 and scratch.numel() >= minmax_scratch_elems()
    if stats is not None:
        assert stats.is_contiguous() and stats.dtype == torch.float32 and \
            stats.numel() == fake_quantize_tiles(npix) * 2 * cs, (tuple(stats.shape), npix, cs)
    check(_L.hnd_fake_quantize_bits(ptr(x), ptr(out), npix, c, cs, bits, ptr(qparams), ptr(scratch), ptr(stats),
                                    stream_ptr()), 'hnd_fake_quantize_bits')
    return out


# include/hnd_qrange.h: the fixed (EMA-calibrated) quantisation range.  qparams is device float[4] = {lo, hi, scale, zero_point}
def qrange_abi():
    return int(_L.hnd_qrange_abi())


def qrange_observe(x, c, bits, momentum, state, qparams, scratch):
    """fold the batch min / max of the c real channels of x into state = {running_min, running_max, steps, 0} (the first
    call initialises, then running += momentum * (batch - running)) and write qparams of the running pair at `bits` bits"""
    who = 'qrange_observe'
    _q_bits(who, bits)
    npix, cs = _q_geometry(who, x, c)
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0 < momentum <= 1:
        raise ValueError('%s: momentum=%r outside (0, 1]' % (who, momentum))
    _q_qparams(who, qparams)
    if not (state.dtype == torch.float32 and state.numel() == 4 and state.is_contiguous()):
        raise ValueError('%s: state must be a contiguous fp32 tensor of 4 values' % who)
    _q_scratch(who, scratch)
    check(_L.hnd_qrange_observe(ptr(x), npix, c, cs, float(momentum), bits, ptr(state), ptr(qparams), ptr(scratch),
                                stream_ptr()), 'hnd_qrange_observe')


def qrange_qparams(lo, hi, bits, qparams):
    """qparams of the literal range [lo, hi] at `bits` bits, computed on the device with the codec's formula"""
    who = 'qrange_qparams'
    _q_bits(who, bits)
    try:
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError('%s: the range (%r, %r) is not a pair of numbers' % (who, lo, hi))
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError('%s: the range needs finite lo < hi, got (%r, %r)' % (who, lo, hi))
    _q_qparams(who, qparams)
    check(_L.hnd_qrange_qparams(lo, hi, bits, ptr(qparams), stream_ptr()), 'hnd_qrange_qparams')
    return qparams


def qrange_mask_shape(x):
    """shape of the clip mask of the NHWC buffer x: one byte per 4 channels of a pixel"""
    return tuple(x.shape[:-1]) + (x.shape[-1] // 4,)


def fake_quantize_range(x, c, bits, qparams, out=None, mask=None, stats=None):
    """fake_quantize_bits on the FIXED range of `qparams` (read, not written), one launch: values outside the range take the
    end codes; `mask` (uint8, qrange_mask_shape(x)) receives bit k of byte g = channel 4 g + k was not clipped.  Returns
    the destination."""
    who = 'fake_quantize_range'
    _q_bits(who, bits)
    npix, cs = _q_geometry(who, x, c)
    _q_qparams(who, qparams)
    out = _q_like(who, 'out', x if out is None else out, x, torch.float32, False)
    if mask is not None:
        _q_mask(who, mask, npix, cs, False)
    _q_stats(who, stats, npix, cs, False)
    check(_L.hnd_fake_quantize_range(ptr(x), ptr(out), npix, c, cs, bits, ptr(qparams), ptr(mask), ptr(stats),
                                     stream_ptr()), 'hnd_fake_quantize_range')
    return out


def qrange_mask_grad(g, mask, c):
    """in place: +0 into the real channels of g whose mask bit is 0 (the backward of fake_quantize_range's clipping)"""
    who = 'qrange_mask_grad'
    npix, cs = _q_geometry(who, g, c)
    _q_mask(who, mask, npix, cs, True)
    check(_L.hnd_qrange_mask_grad(ptr(g), ptr(mask), npix, c, cs, stream_ptr()), 'hnd_qrange_mask_grad')
    return g


def quantize_range_bits(x, c, bits, q, qparams):
    """quantize_bits on the fixed range of `qparams` (read, not written): one launch"""
    who = 'quantize_range_bits'
    _q_bits(who, bits)
    npix, cs = _q_geometry(who, x, c)
    _q_qparams(who, qparams)
    _q_like(who, 'q', q, x, torch.uint8, False)
    check(_L.hnd_quantize_range_bits(ptr(x), npix, c, cs, bits, ptr(q), ptr(qparams), stream_ptr()),
          'hnd_quantize_range_bits')


def quantize_pack_range_bits(x, c, bits, payload, qparams):
    """quantize_pack_bits on the fixed range of `qparams` (read, not written): one launch"""
    who = 'quantize_pack_range_bits'
    _q_bits(who, bits)
    _q_geometry(who, x, c)
    _q_qparams(who, qparams)
    n, h, w, cs = _q_nhwc(who, x, 'range')
    _q_payload(who, payload, x, c, bits)
    check(_L.hnd_quantize_pack_range_bits(ptr(x), n, h, w, c, cs, bits, ptr(payload), ptr(qparams), stream_ptr()),
          'hnd_quantize_pack_range_bits')


# include/hnd_entropy.h: the entropy-coded link payload (canonical Huffman code in chunks of 256 symbols).  q is the
# one-value-per-byte uint8 NHWC tensor [N, H, W, cs] of the quantisers above with c real channels; `lengths` is a host
# bytes object of 2^bits code lengths.
def entropy_abi():
    return int(_L.hnd_entropy_abi())


def entropy_chunks(numel):
    """chunks of 256 symbols that `numel` values make; 0 for numel <= 0 or numel > 2^30"""
    return int(_L.hnd_entropy_chunks(int(numel)))


def entropy_capacity(numel):
    """bytes the payload buffer of `numel` values must have: 384 per chunk; 0 for bad arguments"""
    return int(_L.hnd_entropy_capacity(int(numel)))


def entropy_scratch_bytes(numel):
    """bytes of the encoder's scratch buffer; 0 for bad arguments"""
    return int(_L.hnd_entropy_scratch_bytes(int(numel)))


def _entropy_geometry(who, t, c, bits, dtype):
    _q_bits(who, bits)
    _q_geometry(who, t, c, 'entropy', dtype)
    n, h, w, cs = t.shape
    if entropy_chunks(n * c * h * w) == 0:
        raise ValueError('%s: %d values are more than the 2^30 one stream holds' % (who, n * c * h * w))
    return n, h, w, cs


def _entropy_lengths(who, lengths, bits):
    if not isinstance(lengths, (bytes, bytearray)) or len(lengths) != 1 << bits:
        raise ValueError('%s: lengths must be a bytes object of 2^%d code lengths' % (who, bits))
    return bytes(lengths)


def _entropy_words(who, t, name, count):
    if not (isinstance(t, torch.Tensor) and t.dtype in (torch.int32, torch.uint8) and t.is_contiguous()
            and t.numel() * t.element_size() == 4 * count):
        raise ValueError('%s: %s must be a contiguous int32 buffer of %d words' % (who, name, count))
    return t


def code_histogram(q, c, bits, hist):
    """hist (int32[256], zeroed and filled by the call): how often every code occurs in the c real channels of q"""
    who = 'code_histogram'
    n, h, w, cs = _entropy_geometry(who, q, c, bits, torch.uint8)
    _entropy_words(who, hist, 'hist', 256)
    check(_L.hnd_code_histogram(ptr(q), n, h, w, c, cs, bits, ptr(hist), stream_ptr()), 'hnd_code_histogram')
    return hist


def entropy_encode(q, c, bits, lengths, payload, offsets, scratch):
    """offsets (int32[chunks + 1]) and the stream (payload, uint8[entropy_capacity]) of the logical NCHW codes of q under
    the canonical code of `lengths`: three launches, no host synchronisation"""
    who = 'entropy_encode'
    n, h, w, cs = _entropy_geometry(who, q, c, bits, torch.uint8)
    numel = n * c * h * w
    lengths = _entropy_lengths(who, lengths, bits)
    if not (payload.dtype == torch.uint8 and payload.is_contiguous() and payload.numel() == entropy_capacity(numel)):
        raise ValueError('%s: payload must be %d uint8 bytes' % (who, entropy_capacity(numel)))
    _entropy_words(who, offsets, 'offsets', entropy_chunks(numel) + 1)
    if not (scratch.is_contiguous() and scratch.numel() * scratch.element_size() >= entropy_scratch_bytes(numel)):
        raise ValueError('%s: scratch must hold %d bytes' % (who, entropy_scratch_bytes(numel)))
    check(_L.hnd_entropy_encode(ptr(q), n, h, w, c, cs, bits, lengths, ptr(payload), ptr(offsets), ptr(scratch),
                                stream_ptr()), 'hnd_entropy_encode')


def entropy_decode_dequantize(payload, offsets, lengths, qparams, x, c, bits):
    """the inverse, fused with the dequantiser: scale * (q - zero_point) into the c real channels of x [N, H, W, cs], 0 into
    its pad channels, one launch; the bits of unpack_dequantize_bits.  `payload` may be the whole capacity or its first
    offsets[chunks] bytes."""
    who = 'entropy_decode_dequantize'
    n, h, w, cs = _entropy_geometry(who, x, c, bits, torch.float32)
    lengths = _entropy_lengths(who, lengths, bits)
    _q_qparams(who, qparams)
    if not (payload.dtype == torch.uint8 and payload.is_contiguous() and payload.numel() > 0):
        raise ValueError('%s: payload must be a non-empty contiguous uint8 buffer' % who)
    _entropy_words(who, offsets, 'offsets', entropy_chunks(n * c * h * w) + 1)
    check(_L.hnd_entropy_decode_dequantize(ptr(payload), payload.numel(), ptr(offsets), lengths, ptr(qparams), ptr(x),
                                           n, h, w, c, cs, bits, stream_ptr()), 'hnd_entropy_decode_dequantize')
    return x


# include/hnd_qchannel.h: one (scale, zero point) per channel.  qparams is device float[c][4] = {min, max, scale, zero_point}
QCHANNEL_MAX_C = _lib.QCHANNEL_MAX_C


def qchannel_abi():
    return int(_L.hnd_qchannel_abi())


def qchannel_scratch_elems(cs):
    """floats of the `scratch` buffer of the quantising per-channel calls for a pixel stride of cs floats; 0 for a bad cs"""
    return int(_L.hnd_qchannel_scratch_elems(int(cs)))


def qchannel_quantize_bits(x, c, bits, q, qparams, scratch):
    """quantize_bits with the range of every channel its own: one value per byte into q (uint8, x's shape), pad channels 0"""
    who = 'qchannel_quantize_bits'
    _q_bits(who, bits)
    npix, cs = _q_geometry(who, x, c, 'channel')
    _q_like(who, 'q', q, x, torch.uint8, True)
    check(_L.hnd_qchannel_quantize_bits(ptr(x), npix, c, cs, bits, ptr(q), ptr(_q_qparams(who, qparams, c)),
                                        ptr(_q_scratch(who, scratch, cs)), stream_ptr()), 'hnd_qchannel_quantize_bits')


def qchannel_dequantize_u8(q, qparams, x, c):
    """the inverse: scale[ch] * (q - zero_point[ch]) into the c real channels of x, 0 into its pad channels"""
    who = 'qchannel_dequantize_u8'
    npix, cs = _q_geometry(who, x, c, 'channel')
    _q_like(who, 'q', q, x, torch.uint8, True)
    check(_L.hnd_qchannel_dequantize_u8(ptr(q), ptr(_q_qparams(who, qparams, c)), ptr(x), npix, c, cs, stream_ptr()),
          'hnd_qchannel_dequantize_u8')
    return x


def qchannel_quantize_pack_bits(x, c, bits, payload, qparams, scratch):
    """quantize_pack_bits with the range of every channel its own: the payload format is that of include/hnd_codec.h"""
    who = 'qchannel_quantize_pack_bits'
    n, h, w, cs = _q_nhwc(who, x, 'channel')
    _q_bits(who, bits)
    _q_geometry(who, x, c, 'channel')
    _q_payload(who, payload, x, c, bits, 'channel')
    check(_L.hnd_qchannel_quantize_pack_bits(ptr(x), n, h, w, c, cs, bits, ptr(payload), ptr(_q_qparams(who, qparams, c)),
                                             ptr(_q_scratch(who, scratch, cs)), stream_ptr()),
          'hnd_qchannel_quantize_pack_bits')


def qchannel_unpack_dequantize_bits(payload, qparams, x, c, bits):
    """the inverse: scale[ch] * (q - zero_point[ch]) into the c real channels of x [N, H, W, cs], 0 into its pad channels"""
    who = 'qchannel_unpack_dequantize_bits'
    n, h, w, cs = _q_nhwc(who, x, 'channel')
    _q_bits(who, bits)
    _q_geometry(who, x, c, 'channel')
    _q_payload(who, payload, x, c, bits, 'channel')
    check(_L.hnd_qchannel_unpack_dequantize_bits(ptr(payload), ptr(_q_qparams(who, qparams, c)), ptr(x), n, h, w, c, cs,
                                                 bits, stream_ptr()), 'hnd_qchannel_unpack_dequantize_bits')
    return x


def qchannel_fake_quantize_bits(x, c, bits, qparams, scratch, out=None, stats=None):
    """fake_quantize_bits with the range of every channel its own -- the bits of
    qchannel_dequantize_u8(qchannel_quantize_bits(x)) -- into `out` (default: in place), 0 into the pad channels; `stats`
    [fake_quantize_tiles(npix), 2, cs] receives the per-tile (sum, sum of squares) of what was stored, for bn_finalize.
    Returns the destination."""
    who = 'qchannel_fake_quantize_bits'
    _q_bits(who, bits)
    npix, cs = _q_geometry(who, x, c, 'channel')
    out = _q_like(who, 'out', x if out is None else out, x, torch.float32, True)
    _q_stats(who, stats, npix, cs, True)
    check(_L.hnd_qchannel_fake_quantize_bits(ptr(x), ptr(out), npix, c, cs, bits, ptr(_q_qparams(who, qparams, c)),
                                             ptr(_q_scratch(who, scratch, cs)), ptr(stats), stream_ptr()),
          'hnd_qchannel_fake_quantize_bits')
    return out


# include/hnd_qimage.h: one (scale, zero point) per image.  x is the NHWC fp32 buffer [N, H, W, cs] with c real channels;
# qparams is device float[N][4] = {min, max, scale, zero_point}
QIMAGE_MAX_N = _lib.QIMAGE_MAX_N


def qimage_abi():
    return int(_L.hnd_qimage_abi())


def qimage_scratch_elems(n):
    """floats of the `scratch` buffer of the quantising per-image calls for n images; 0 for a bad n"""
    return int(_L.hnd_qimage_scratch_elems(int(n)))


def _qi_geometry(who, x, c):
    """(n, h, w, cs) of the NHWC buffer x [N, H, W, cs] with c real channels"""
    if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError('%s: needs a contiguous float32 NHWC buffer [N, H, W, cs]' % who)
    n, h, w, cs = x.shape
    if isinstance(c, bool) or not isinstance(c, int) or not 0 < c <= cs or cs % 4 or x.numel() == 0:
        raise ValueError('%s: c=%r real channels in a pixel stride of %d floats (0 < c <= stride, stride %% 4 == 0)'
                         % (who, c, cs))
    if n > QIMAGE_MAX_N:
        raise ValueError('%s: %d images, at most %d per call' % (who, n, QIMAGE_MAX_N))
    return n, h, w, cs


def _qi_scratch(who, scratch, n):
    if not (isinstance(scratch, torch.Tensor) and scratch.dtype == torch.float32 and scratch.is_contiguous()
            and scratch.numel() >= qimage_scratch_elems(n)):
        raise ValueError('%s: scratch must be a contiguous fp32 buffer of qimage_scratch_elems(%d) = %d floats'
                         % (who, n, qimage_scratch_elems(n)))
    return scratch


def qimage_quantize_bits(x, c, bits, q, qparams, scratch):
    """quantize_bits with the range of every image its own: one value per byte into q (uint8, x's shape), pad channels 0"""
    who = 'qimage_quantize_bits'
    _q_bits(who, bits)
    n, h, w, cs = _qi_geometry(who, x, c)
    _q_like(who, 'q', q, x, torch.uint8, True)
    check(_L.hnd_qimage_quantize_bits(ptr(x), n, h * w, c, cs, bits, ptr(q), ptr(_q_qparams(who, qparams, n)),
                                      ptr(_qi_scratch(who, scratch, n)), stream_ptr()), 'hnd_qimage_quantize_bits')


def qimage_dequantize_u8(q, qparams, x, c):
    """the inverse: scale[img] * (q - zero_point[img]) into the c real channels of x, 0 into its pad channels"""
    who = 'qimage_dequantize_u8'
    n, h, w, cs = _qi_geometry(who, x, c)
    _q_like(who, 'q', q, x, torch.uint8, True)
    check(_L.hnd_qimage_dequantize_u8(ptr(q), ptr(_q_qparams(who, qparams, n)), ptr(x), n, h * w, c, cs, stream_ptr()),
          'hnd_qimage_dequantize_u8')
    return x


def qimage_quantize_pack_bits(x, c, bits, payload, qparams, scratch):
    """quantize_pack_bits with the range of every image its own: the payload format is that of include/hnd_codec.h"""
    who = 'qimage_quantize_pack_bits'
    _q_bits(who, bits)
    n, h, w, cs = _qi_geometry(who, x, c)
    _q_payload(who, payload, x, c, bits, 'channel')
    check(_L.hnd_qimage_quantize_pack_bits(ptr(x), n, h, w, c, cs, bits, ptr(payload), ptr(_q_qparams(who, qparams, n)),
                                           ptr(_qi_scratch(who, scratch, n)), stream_ptr()),
          'hnd_qimage_quantize_pack_bits')


def qimage_unpack_dequantize_bits(payload, qparams, x, c, bits):
    """the inverse: scale[img] * (q - zero_point[img]) into the c real channels of x [N, H, W, cs], 0 into its pad channels"""
    who = 'qimage_unpack_dequantize_bits'
    _q_bits(who, bits)
    n, h, w, cs = _qi_geometry(who, x, c)
    _q_payload(who, payload, x, c, bits, 'channel')
    check(_L.hnd_qimage_unpack_dequantize_bits(ptr(payload), ptr(_q_qparams(who, qparams, n)), ptr(x), n, h, w, c, cs,
                                               bits, stream_ptr()), 'hnd_qimage_unpack_dequantize_bits')
    return x


def qimage_fake_quantize_bits(x, c, bits, qparams, scratch, out=None, stats=None):
    """fake_quantize_bits with the range of every image its own -- the bits of qimage_dequantize_u8(qimage_quantize_bits(x))
    -- into `out` (default: in place), 0 into the pad channels; `stats` [fake_quantize_tiles(npix), 2, cs] receives the
    per-tile (sum, sum of squares) of what was stored, tiles over all n * h * w pixels, for bn_finalize.  Returns the
    destination."""
    who = 'qimage_fake_quantize_bits'
    _q_bits(who, bits)
    n, h, w, cs = _qi_geometry(who, x, c)
    out = _q_like(who, 'out', x if out is None else out, x, torch.float32, True)
    _q_stats(who, stats, n * h * w, cs, True)
    check(_L.hnd_qimage_fake_quantize_bits(ptr(x), ptr(out), n, h * w, c, cs, bits, ptr(_q_qparams(who, qparams, n)),
                                           ptr(_qi_scratch(who, scratch, n)), ptr(stats), stream_ptr()),
          'hnd_qimage_fake_quantize_bits')
    return out


# include/hnd_istream.h: one entropy stream, one code table and one (scale, zero point) per image.  q is the one-value-per-
# byte uint8 NHWC tensor [N, H, W, cs] of qimage_quantize_bits with c real channels; hist is int32 [N, 256], lengths DEVICE
# uint8 [N, 256], qparams fp32 [N, 4]
ISTREAM_MAX_N = _lib.ISTREAM_MAX_N


def istream_abi():
    return int(_L.hnd_istream_abi())


def istream_chunks_per_image(chw):
    """chunks of 256 symbols one image of `chw` values makes; 0 for chw <= 0 or chw > 2^30"""
    return int(_L.hnd_istream_chunks_per_image(int(chw)))


def istream_capacity(n, chw):
    """bytes the payload buffer of n images of `chw` values must have: 384 per chunk; 0 for bad arguments"""
    return int(_L.hnd_istream_capacity(int(n), int(chw)))


def istream_scratch_bytes(n, chw):
    """bytes of the encoder's scratch buffer; 0 for bad arguments"""
    return int(_L.hnd_istream_scratch_bytes(int(n), int(chw)))


def _istream_geometry(who, t, c, bits, dtype):
    """(n, h, w, cs, chunks per image) of the NHWC buffer t with c real channels"""
    _q_bits(who, bits)
    _q_geometry(who, t, c, 'entropy', dtype)
    n, h, w, cs = t.shape
    if istream_scratch_bytes(n, c * h * w) == 0:
        raise ValueError('%s: %d images of %d values: at most %d images and 2^30 values per call'
                         % (who, n, c * h * w, ISTREAM_MAX_N))
    return n, h, w, cs, istream_chunks_per_image(c * h * w)


def _istream_rows(who, t, name, n, dtype):
    """a contiguous [n, 256] table: the histograms (int32) or the code lengths (uint8) of n images"""
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == (n, 256)):
        raise ValueError('%s: %s must be a contiguous %s tensor [%d, 256]' % (who, name, str(dtype).replace('torch.', ''), n))
    return t


def istream_histogram(q, c, bits, hist):
    """hist (int32 [N, 256], zeroed and filled by the call): row i counts the codes of the c real channels of image i"""
    who = 'istream_histogram'
    n, h, w, cs, _ = _istream_geometry(who, q, c, bits, torch.uint8)
    _istream_rows(who, hist, 'hist', n, torch.int32)
    check(_L.hnd_istream_histogram(ptr(q), n, h, w, c, cs, bits, ptr(hist), stream_ptr()), 'hnd_istream_histogram')
    return hist


def istream_build_tables(hist, bits, lengths):
    """lengths (uint8 [N, 256]): row i is transformer.huffman_lengths(hist[i], bits), made on the device in one launch"""
    who = 'istream_build_tables'
    _q_bits(who, bits)
    if not (isinstance(hist, torch.Tensor) and hist.dim() == 2 and 0 < hist.shape[0] <= ISTREAM_MAX_N):
        raise ValueError('%s: hist must be an int32 tensor [N, 256] of 1 ... %d images' % (who, ISTREAM_MAX_N))
    n = hist.shape[0]
    _istream_rows(who, hist, 'hist', n, torch.int32)
    _istream_rows(who, lengths, 'lengths', n, torch.uint8)
    check(_L.hnd_istream_build_tables(ptr(hist), n, bits, ptr(lengths), stream_ptr()), 'hnd_istream_build_tables')
    return lengths


def istream_encode(q, c, bits, lengths, payload, offsets, scratch):
    """offsets (int32 [N * chunks per image + 1]) and the streams (payload, uint8 [istream_capacity]) of the images of q,
    image i under the canonical code of lengths[i]: three launches, no host synchronisation"""
    who = 'istream_encode'
    n, h, w, cs, cpi = _istream_geometry(who, q, c, bits, torch.uint8)
    _istream_rows(who, lengths, 'lengths', n, torch.uint8)
    cap = istream_capacity(n, c * h * w)
    if not (isinstance(payload, torch.Tensor) and payload.dtype == torch.uint8 and payload.is_contiguous()
            and payload.numel() == cap):
        raise ValueError('%s: payload must be %d uint8 bytes' % (who, cap))
    _entropy_words(who, offsets, 'offsets', n * cpi + 1)
    if not (isinstance(scratch, torch.Tensor) and scratch.is_contiguous()
            and scratch.numel() * scratch.element_size() >= istream_scratch_bytes(n, c * h * w)):
        raise ValueError('%s: scratch must hold %d bytes' % (who, istream_scratch_bytes(n, c * h * w)))
    check(_L.hnd_istream_encode(ptr(q), n, h, w, c, cs, bits, ptr(lengths), ptr(payload), ptr(offsets), ptr(scratch),
                                stream_ptr()), 'hnd_istream_encode')


def istream_decode_dequantize(payload, offsets, lengths, qparams, x, c, bits):
    """the inverse, fused with the dequantiser: scale[img] * (q - zero_point[img]) into the c real channels of x
    [N, H, W, cs], 0 into its pad channels, one launch; the bits of qimage_unpack_dequantize_bits on the same codes.
    `payload` may be the whole capacity or its first offsets[-1] bytes."""
    who = 'istream_decode_dequantize'
    n, h, w, cs, cpi = _istream_geometry(who, x, c, bits, torch.float32)
    _istream_rows(who, lengths, 'lengths', n, torch.uint8)
    _q_qparams(who, qparams, n)
    if not (isinstance(payload, torch.Tensor) and payload.dtype == torch.uint8 and payload.is_contiguous()
            and payload.numel() > 0):
        raise ValueError('%s: payload must be a non-empty contiguous uint8 buffer' % who)
    _entropy_words(who, offsets, 'offsets', n * cpi + 1)
    check(_L.hnd_istream_decode_dequantize(ptr(payload), payload.numel(), ptr(offsets), ptr(lengths), ptr(qparams), ptr(x),
                                           n, h, w, c, cs, bits, stream_ptr()), 'hnd_istream_decode_dequantize')
    return x


def roundtrip_f16(x):
    check(_L.hnd_roundtrip_f16(ptr(x), x.numel(), stream_ptr()), 'hnd_roundtrip_f16')


# ------------------------------------------------------------------------------ Winograd F(2x2, 3x3)
def wino_tiles_pad(n, h, w, tile=2):
    return int(_L.hnd_wino_tiles_pad(n, h, w, tile))


def wino_tiles(oh, ow, tile):
    """tile x tile output tiles that cover the oh x ow outputs of ONE image (the last of a row / column may be ragged)"""
    return ((oh + tile - 1) // tile) * ((ow + tile - 1) // tile)


def _stream(stream):
    return stream if stream is not None else stream_ptr()


class _WinogradWeights(PackedWeight):
    """One k x k conv weight in the Winograd domain: a grouped operand of ncomp = (tile+k-1)^2 GEMM matrices
    [rows_pad][depth], one per component; dgrad: of the transposed conv.  The subclasses name k, the tiles and the
    kernel that fills the buffer."""
    def __init__(self, weight, dgrad, tile):
        cout, cin, kh, kw = weight.shape
        assert kh == self.K and kw == self.K and weight.is_contiguous() and tile in self.TILES
        rows, depth = (cin, cout) if dgrad else (cout, cin)
        assert depth % 32 == 0, 'Winograd path needs a GEMM depth that is a multiple of 32'
        ncomp, rows_pad = (tile + self.K - 1) ** 2, round_up(rows, 64)
        PackedWeight.__init__(self, torch.empty(ncomp * rows_pad * depth, dtype=torch.float32, device=weight.device),
                              rows, depth, depth, groups=ncomp, group_stride=rows_pad * depth)
        self.src, self.dgrad, self.tile, self.ncomp, self.depth = weight, dgrad, tile, ncomp, depth
        self.repack()

    def fill(self):
        check(getattr(_L, self.KERNEL)(ptr(self.src), ptr(self.buf), self.src.shape[0], self.src.shape[1],
                                       int(self.dgrad), self.tile, stream_ptr()), self.KERNEL)


class WinoWeights(_WinogradWeights):
    """U = G g G^T of one 3x3 conv weight, [(tile+2)^2][rows_pad][depth]; tile = 2 (F(2x2,3x3)), 4 (F(4x4,3x3)) or 6
    (F(6x6,3x3))."""
    K, TILES, KERNEL = 3, (2, 4, 6), 'hnd_wino_weights'

    def __init__(self, weight, dgrad=False, tile=2):
        _WinogradWeights.__init__(self, weight, dgrad, tile)


class _WinogradLaunch(object):
    """What the Winograd launches of one stride-1 K x K correlation with padding `pad` share.  The input half: x [N,H,W,C]
    -> V = B^T d B in `v`, BN(+ReLU) prologue on load.  With a weight operand `ww` the rest as well: the ncomp =
    (tile+K-1)^2 component GEMMs V -> M as ONE grouped igemm launch (tiles_pad rows per component, `m`) and the output
    transform M -> y [N,OH,OW,ldc].  v / m are caller-provided scratch (see scratch_elems).  A subclass names K, ROUND (the
    rounding of cout), the two transforms (INPUT, OUTPUT: plan labels, 'hnd_' + INPUT the entry point), _tiles_pad,
    _input_args and, where it has an output, _run_output and _output_bytes."""

    def __init__(self, x, v, tile, pad, pro_scale, pro_shift, pro_relu, ww=None, y=None, m=None):
        n, h, w, c = _nhwc(x)
        oh, ow = h + 2 * pad - self.K + 1, w + 2 * pad - self.K + 1
        self.x, self.y, self.ww, self.pad, self.tile = x, y, ww, pad, tile
        self.geom = (n, h, w, c, oh, ow)
        self.ncomp, self.dgrad = (tile + self.K - 1) ** 2, ww is not None and bool(ww.dgrad)
        self.tiles_pad, self.tiles = self._tiles_pad(n, oh, ow, tile), n * wino_tiles(oh, ow, tile)
        rows = self.ncomp * self.tiles_pad
        assert v.numel() >= rows * c
        if pro_scale is not None and pro_shift is None:
            pro_shift = _zeros(c, x.device)
        self.pro = (pro_scale, pro_shift, int(pro_relu))
        self.v = v[:rows * c].view(1, 1, rows, c)
        self.input_bytes = 4 * (n * h * w * c + self.ncomp * self.tiles * c)           # read x once, write V
        if ww is None:
            return
        assert tuple(y.shape[:3]) == (n, oh, ow) and c == ww.depth
        self.cout = round_up(ww.rows, self.ROUND)
        assert self.cout <= y.shape[3] and m.numel() >= rows * self.cout
        self.m = m[:rows * self.cout].view(1, 1, rows, self.cout)
        self.gemm = conv_desc(self.v, ww, self.m, kh=1, kw=1, oh=1, ow=rows, sh=1, dh=1, bh=0, sw=1, dw=1, bw=0,
                              cout=self.cout, rows_per_image=self.ncomp * wino_tiles(oh, ow, tile),
                              w_group_rows=self.tiles_pad)
        self.gemm.flops = 2 * self.ncomp * self.tiles * ww.rows * ww.depth             # multiplies actually executed
        self.gemm.alg_flops = 2 * n * oh * ow * ww.rows * self.K ** 2 * ww.depth       # the direct convolution it computes
        self.flops, self.variant = self.gemm.flops, self.gemm.variant

    @classmethod
    def _scratch_elems(cls, n, oh, ow, cin, cout, tile):
        rows = (tile + cls.K - 1) ** 2 * cls._tiles_pad(n, oh, ow, tile)
        return rows * cin, rows * round_up(cout, cls.ROUND)

    def _run_input(self, stream=None):
        name = 'hnd_' + self.INPUT
        check(getattr(_L, name)(*self._input_args(), _stream(stream)), name)

    def step(self, tag):
        """the input transform as an engine plan entry"""
        return (_Step(self._run_input, self.INPUT, self.input_bytes), tag + '.wino_in')

    def launches(self, tag):
        """[(launch, tag)] for an engine plan: the two transforms carry no flops (not event-timed by bench.py), the
        GEMM launch is an ordinary igemm launch with the multiplies it really executes."""
        return [self.step(tag), (self.gemm, tag),
                (_Step(self._run_output, self.OUTPUT, self._output_bytes()), tag + '.wino_out')]

    def run(self, stream=None):
        self._run_input(stream)
        self.gemm.run(stream)
        self._run_output(stream)


class WinoConv(_WinogradLaunch):
    """One stride-1 pad-1 3x3 convolution (or its data gradient) as input transform -> (tile+2)^2 GEMMs in one igemm
    launch -> output transform.  x [N,H,W,C] -> y [N,H,W,ldc]."""
    K, ROUND, INPUT, OUTPUT = 3, 4, 'wino_input', 'wino_output'
    _tiles_pad = staticmethod(wino_tiles_pad)

    def __init__(self, x, ww, y, v, m, pro_scale=None, pro_shift=None, pro_relu=False, epi_scale=None, epi_shift=None,
                 res1=None, mask=None, relu=False, mask_out=None):
        """mask_out: uint8 nibbles of the STORED output (mask_nibbles_like(y)), written by the output transform (tile 4 / 6)"""
        _WinogradLaunch.__init__(self, x, v, ww.tile, 1, pro_scale, pro_shift, pro_relu, ww, y, m)
        self.geom = self.geom[:4]                                                   # (oh, ow) == (h, w)
        self.epi = (epi_scale, epi_shift, res1, mask, int(relu))
        self.mask_out = mask_out
        assert mask_out is None or (self.tile in (4, 6) and self.cout == y.shape[3] and mask_out.dtype == torch.uint8
                                    and tuple(mask_out.shape) == tuple(y.shape[:3]) + (y.shape[3] // 4,))
        for t in (res1, mask):
            assert t is None or tuple(t.shape) == tuple(y.shape)

    @classmethod
    def scratch_elems(cls, n, h, w, cin, cout, tile=2):
        return cls._scratch_elems(n, h, w, cin, cout, tile)

    def _input_args(self):
        return (ptr(self.x), ptr(self.v)) + self.geom + (ptr(self.pro[0]), ptr(self.pro[1]), self.pro[2], self.tile)

    def _run_output(self, stream=None):
        n, h, w, c = self.geom
        es, eb, r1, mk, relu = self.epi
        check(_L.hnd_wino_output(ptr(self.m), ptr(self.y), n, h, w, self.cout, self.y.shape[3], ptr(es), ptr(eb),
                                 ptr(r1), ptr(mk), relu, self.tile, ptr(self.mask_out), _stream(stream)), 'hnd_wino_output')

    def _output_bytes(self):
        n, h, w, c = self.geom
        extra = sum(1 for t in (self.epi[2], self.epi[3]) if t is not None)
        b_out = 4 * (self.ncomp * self.tiles * self.cout + (1 + extra) * n * h * w * self.cout)  # read M (+ res / mask), write y
        return b_out + n * h * w * self.cout // 4 if self.mask_out is not None else b_out


class Wino2Weights(_WinogradWeights):
    """F(tile x tile, 2x2) weights (tile 4 or 6) of one 2x2 conv, [(tile+1)^2][rows_pad][depth]."""
    K, TILES, KERNEL = 2, (4, 6), 'hnd_wino2_weights'

    def __init__(self, weight, dgrad=False, tile=4):
        _WinogradWeights.__init__(self, weight, dgrad, tile)


class _Wino2Launch(_WinogradLaunch):
    """the F(tile x tile, 2x2) launches (tile 4 or 6, padding 0 or 1): geom = (n, h, w, c, oh, ow)"""
    K, ROUND, INPUT, OUTPUT = 2, 2, 'wino2_input', 'wino2_output'

    @staticmethod
    def _tiles_pad(n, oh, ow, tile):
        return int(_L.hnd_wino2_tiles_pad(n, oh, ow, tile))

    def _input_args(self):
        return (ptr(self.x), ptr(self.v)) + self.geom[:4] + (self.pad, ptr(self.pro[0]), ptr(self.pro[1]), self.pro[2],
                                                             self.tile)


class Wino2Conv(_Wino2Launch):
    """One 2x2 correlation with padding `pad` in {0, 1} (a head conv, or -- with Wino2Weights(dgrad=True) and padding
    1 - pad_of_the_conv -- its data gradient): x [N,H,W,C] -> y [N,H+2pad-1,W+2pad-1,ldc].  Optional BN(+ReLU)
    prologue on load; optional per-block BN statistics of the stored output (stats: [stats_blocks][2][cout])."""

    def __init__(self, x, ww, y, v, m, pad, pro_scale=None, pro_shift=None, pro_relu=False, epi_scale=None,
                 epi_shift=None, relu=False, stats=None, bwd_stats=None):
        """bwd_stats = (x_raw, scale, shift, mean, rstd, relu, partials): this launch is the DATA gradient that produces
        the gradient w.r.t. the output of a train-mode BatchNorm(+ReLU) over x_raw; its output transform then also makes
        the BatchNorm-backward partial sums (hnd_wino26_output_bnbwd_stats; F(6x6,2x2), plain epilogue only)."""
        assert pad in (0, 1)
        _Wino2Launch.__init__(self, x, v, ww.tile, pad, pro_scale, pro_shift, pro_relu, ww, y, m)
        n, h, w, c, oh, ow = self.geom
        self.epi = (epi_scale, epi_shift, int(relu))
        self.stats = stats
        if stats is not None:
            assert stats.numel() >= self.stats_blocks(n, oh, ow, self.cout, self.tile) * 2 * self.cout
        self.bwd_stats = bwd_stats
        if bwd_stats is not None:
            assert self.tile == 6 and stats is None and epi_scale is None and epi_shift is None and not relu
            assert 512 % self.cout == 0 and tuple(bwd_stats[0].shape) == tuple(y.shape) and y.shape[3] == self.cout
            assert bwd_stats[6].numel() >= self.stats_blocks(n, oh, ow, self.cout, 6) * 2 * self.cout

    @classmethod
    def scratch_elems(cls, n, oh, ow, cin, cout, tile=4):
        return cls._scratch_elems(n, oh, ow, cin, cout, tile)

    @staticmethod
    def stats_blocks(n, oh, ow, cout, tile=4):
        return int(_L.hnd_wino2_stats_blocks(n, oh, ow, cout, tile))

    def _run_output(self, stream=None):
        n, h, w, c, oh, ow = self.geom
        if self.bwd_stats is not None:
            xr, sc, sh, mu, rs, relu, part = self.bwd_stats
            check(_L.hnd_wino26_output_bnbwd_stats(ptr(self.m), ptr(self.y), n, oh, ow, self.cout, self.y.shape[3],
                                                   ptr(xr), ptr(sc), ptr(sh), ptr(mu), ptr(rs), int(relu), ptr(part),
                                                   _stream(stream)), 'hnd_wino26_output_bnbwd_stats')
            return
        check(_L.hnd_wino2_output(ptr(self.m), ptr(self.y), n, oh, ow, self.cout, self.y.shape[3], ptr(self.epi[0]),
                                  ptr(self.epi[1]), self.epi[2], ptr(self.stats), self.tile, _stream(stream)),
              'hnd_wino2_output')

    def _output_bytes(self):
        n, h, w, c, oh, ow = self.geom
        return 4 * (self.ncomp * self.tiles * self.cout + (2 if self.bwd_stats is not None else 1) * n * oh * ow * self.cout)


class Wino2InputTransform(_Wino2Launch):
    """V = B^T d B of a 2x2 conv's input alone (no weights, no GEMM, no output: _run_input and step only): what Wino2Wgrad
    needs from the forward pass of a conv whose FORWARD is not on the Winograd path (the head's 64 -> 256 conv: its component
    GEMMs would be 64 deep and HBM-bound, but its weight gradient in the Winograd domain executes 2.9x fewer multiplies than
    the direct one)."""

    def __init__(self, x, v, pad, cout, tile=6, pro_scale=None, pro_shift=None, pro_relu=False):
        assert pad in (0, 1) and tile in (4, 6) and x.shape[3] % 32 == 0
        _Wino2Launch.__init__(self, x, v, tile, pad, pro_scale, pro_shift, pro_relu)

    @classmethod
    def scratch_elems(cls, n, oh, ow, cin, tile=6):
        return cls._scratch_elems(n, oh, ow, cin, 0, tile)[0]


class Wino2Wgrad(object):
    """dW of a 2x2 head conv in the Winograd domain (F(2x2 taps, 4x4 tile)): reuses the forward pass's transformed
    input `fwd.v`, transforms dy (z), reduces the 25 component products over the tiles in ONE grouped split-K
    wgrad launch and inverse-transforms into dw [cout, cin, 2, 2]."""

    def __init__(self, fwd, dy, dw, z, s, slabs=None):
        assert isinstance(fwd, _Wino2Launch) and not fwd.dgrad
        n, h, w, c, oh, ow = fwd.geom
        cout, cin = dw.shape[0], dw.shape[1]
        assert tuple(dw.shape) == (cout, cin, 2, 2) and dw.is_contiguous() and cin == c and cout % 2 == 0
        assert tuple(dy.shape[:3]) == (n, oh, ow) and dy.shape[3] >= cout
        self.tile, self.ncomp, self.tiles = fwd.tile, fwd.ncomp, n * wino_tiles(oh, ow, fwd.tile)
        nc = self.ncomp
        assert z.numel() >= nc * fwd.tiles_pad * cout and s.numel() >= nc * cout * cin
        self.fwd, self.dy, self.dw, self.z, self.s = fwd, dy, dw, z, s
        self.geom = (n, oh, ow, cout, dy.shape[3], cin)
        # A conv with 64 OUTPUT channels (encoder.5: 256 -> 64) is 64 rows x 256 columns, which only the LDS-staged kernel
        # takes (0.50 of the matrix peak); with the operands swapped it is the 64-column x 256-row shape of the ring
        # kernel (round 5).  The output transform then reads s transposed.
        d = self.grouped_desc(fwd, cout, False, z, s)
        self.swapped = False
        if (int(_L.hnd_conv2d_wgrad_variant(C.byref(d))) != 3
                and int(_L.hnd_conv2d_wgrad_variant(C.byref(self.grouped_desc(fwd, cout, True, z, s)))) == 3
                and os.environ.get('HND_WGRAD_SWAP', '1') != '0'):
            d, self.swapped = self.grouped_desc(fwd, cout, True, z, s), True
        need = _L.hnd_conv2d_wgrad_workspace(C.byref(d))
        if slabs is None or slabs.numel() * 4 < need:
            slabs = torch.empty((need + 3) // 4, dtype=torch.float32, device=dy.device)
        d.slabs = ptr(slabs)
        self.gemm = WgradLaunch(d, (fwd.v, z, s, slabs), 2 * nc * self.tiles * cout * cin)
        self.gemm.alg_flops = 2 * n * oh * ow * cout * 4 * cin
        self.flops, self.variant = self.gemm.flops, self.gemm.variant

    @staticmethod
    def grouped_desc(fwd, cout, swap=False, z=None, s=None):
        """descriptor of the fwd.ncomp grouped split-K reductions V x Z -> s of a conv with cout output channels; swap: operands
        exchanged -> s comes out [comp][cin][cout].  Without z / s: its geometry alone, to size the workspace."""
        n, h, w, c, oh, ow = fwd.geom
        tiles, tp = n * wino_tiles(oh, ow, fwd.tile), fwd.tiles_pad
        d = WgradDesc()
        d.x, d.dy, d.dw = (ptr(z), ptr(fwd.v), ptr(s)) if swap else (ptr(fwd.v), ptr(z), ptr(s))
        kc, kr = (cout, c) if swap else (c, cout)          # columns ("cin" of the descriptor), rows ("cout")
        d.n, d.h, d.w_, d.cin, d.cin_real = 1, 1, tiles, kc, kc
        d.oh, d.ow, d.cout, d.ldy = 1, tiles, kr, kr
        d.kh, d.kw, d.stride, d.pad, d.splitk = 1, 1, 1, 0, 0
        d.groups = fwd.ncomp
        d.x_group_stride, d.dy_group_stride, d.dw_group_stride = tp * kc, tp * kr, cout * c
        return d

    def _run_dy(self, stream=None):
        n, oh, ow, cout, ldy, cin = self.geom
        check(_L.hnd_wino2_dy(ptr(self.dy), ptr(self.z), n, oh, ow, cout, ldy, self.tile, _stream(stream)), 'hnd_wino2_dy')

    def _run_out(self, stream=None):
        n, oh, ow, cout, ldy, cin = self.geom
        check(_L.hnd_wino2_wgrad_output_t(ptr(self.s), ptr(self.dw), cout, cin, self.tile, int(self.swapped),
                                          _stream(stream)), 'hnd_wino2_wgrad_output')

    def launches(self, tag):
        n, oh, ow, cout, ldy, cin = self.geom
        nc = self.ncomp
        return [(_Step(self._run_dy, 'wino2_dy', 4 * (n * oh * ow * cout + nc * self.tiles * cout)), tag + '.wino_dy'),
                (self.gemm, tag),
                (_Step(self._run_out, 'wino2_wgrad_output', 4 * (nc + 4) * cout * cin), tag + '.wino_out')]

    def run(self, stream=None):
        self._run_dy(stream)
        self.gemm.run(stream)
        self._run_out(stream)


def wino26_bnbwd_step(g, x, scale, shift, k123, relu, dgrad_conv, wgrad):
    """BatchNorm backward "apply" fused into the two transforms that consume its result (hnd_wino26_bnbwd_transforms):
    writes dgrad_conv.v (the input transform of the Wino2Conv data gradient) and wgrad.z (the dy transform of the
    Wino2Wgrad) from g and the raw conv output x, without materialising dy.  Both must be F(6x6,2x2) over the same dy."""
    assert isinstance(dgrad_conv, Wino2Conv) and isinstance(wgrad, Wino2Wgrad) and dgrad_conv.tile == 6 and wgrad.tile == 6
    n, oh, ow, c = _nhwc(g)
    assert tuple(x.shape) == tuple(g.shape) and tuple(dgrad_conv.geom[:4]) == (n, oh, ow, c)
    assert wgrad.geom[:3] == (n, oh, ow) and wgrad.geom[3] == c and wgrad.geom[4] == c
    pad = dgrad_conv.pad

    def fn(stream=None):
        check(_L.hnd_wino26_bnbwd_transforms(ptr(g), ptr(x), ptr(scale), ptr(shift), ptr(k123), int(relu), n, oh, ow, c,
                                             pad, ptr(dgrad_conv.v), ptr(wgrad.z), _stream(stream)),
              'hnd_wino26_bnbwd_transforms')
    # reads g and x, writes the 49 components of both launches' real tiles (over the same dy: the asserts above)
    step = _Step(fn, 'wino2_bnbwd_fused', 4 * (2 * n * oh * ow * c + 49 * (dgrad_conv.tiles + wgrad.tiles) * c))
    step.keep = (g, x, scale, shift, k123, dgrad_conv, wgrad)
    return step


class _Step(object):
    """a plan entry without MFMA work: HBM-bound; `hbm_bytes` = the bytes it must move (bench.py's hbm_roofline)"""
    __slots__ = ('fn', 'flops', 'alg_flops', 'variant', 'kernel', 'hbm_bytes', 'keep')

    def __init__(self, fn, kernel='transform', hbm_bytes=0):
        self.fn, self.flops, self.alg_flops, self.variant = fn, 0, 0, 'transform'
        self.kernel, self.hbm_bytes = kernel, int(hbm_bytes)

    def run(self, stream=None):
        self.fn(stream)


# ------------------------------------------------------------------------------ neural filter (Ext4ResNet)
def adaptive_avgpool_fwd(x, y):
    n, h, w, c = _nhwc(x)
    assert y.shape[0] == n and y.shape[3] == c
    check(_L.hnd_adaptive_avgpool_fwd(ptr(x), ptr(y), n, h, w, c, y.shape[1], y.shape[2], stream_ptr()),
          'hnd_adaptive_avgpool_fwd')


def adaptive_avgpool_bwd(dy, dx):
    n, h, w, c = _nhwc(dx)
    assert dy.shape[0] == n and dy.shape[3] == c
    check(_L.hnd_adaptive_avgpool_bwd(ptr(dy), ptr(dx), n, h, w, c, dy.shape[1], dy.shape[2], stream_ptr()),
          'hnd_adaptive_avgpool_bwd')


def linear_fwd(x, c, weight, bias, out):
    """x NHWC [n, h, w, cs] holding logical [n, c, h, w]; weight [nout, c*h*w] (NCHW flatten order)."""
    n, h, w, cs = _nhwc(x)
    nout = weight.shape[0]
    assert weight.is_contiguous() and weight.shape[1] == c * h * w and tuple(out.shape) == (n, nout)
    check(_L.hnd_linear_fwd(ptr(x), ptr(weight), ptr(bias), ptr(out), n, h * w, c, cs, nout, stream_ptr()),
          'hnd_linear_fwd')


def linear_bwd(x, c, weight, dout, dweight, dbias, dx):
    n, h, w, cs = _nhwc(x)
    nout = weight.shape[0]
    assert dout.is_contiguous() and tuple(dout.shape) == (n, nout)
    assert dweight is None or (dweight.is_contiguous() and dweight.shape == weight.shape)
    assert dx is None or tuple(dx.shape) == tuple(x.shape)
    check(_L.hnd_linear_bwd(ptr(x), ptr(weight), ptr(dout), ptr(dweight), ptr(dbias), ptr(dx), n, h * w, c, cs, nout,
                            stream_ptr()), 'hnd_linear_bwd')


def softmax_rows(x, y):
    assert x.dim() == 2 and x.is_contiguous() and y.shape == x.shape
    check(_L.hnd_softmax_rows(ptr(x), ptr(y), x.shape[0], x.shape[1], stream_ptr()), 'hnd_softmax_rows')


def softmax_ce_rows(logits, labels, loss, dlogits, ignore_index=-100):
    """mean cross entropy of [rows, cols] logits against int64 labels + its gradient, one launch"""
    assert logits.dim() == 2 and logits.is_contiguous() and logits.dtype == torch.float32
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == logits.shape[0]
    assert dlogits.shape == logits.shape and dlogits.is_contiguous() and loss.numel() == 1
    check(_L.hnd_softmax_ce_rows_fwd_bwd(ptr(logits), ptr(labels), logits.shape[0], logits.shape[1], int(ignore_index),
                                         ptr(loss), ptr(dlogits), stream_ptr()), 'hnd_softmax_ce_rows_fwd_bwd')


def channel_sum(x, c, out, scratch=None):
    cs = x.shape[-1]
    need = _L.hnd_channel_sum_scratch_elems(c)
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty(need, dtype=torch.float32, device=x.device)
    check(_L.hnd_channel_sum(ptr(x), ptr(out), x.numel() // cs, c, cs, ptr(scratch), stream_ptr()), 'hnd_channel_sum')


def channel_sum_scratch_elems(c):
    return _L.hnd_channel_sum_scratch_elems(c)


def sgd_step_flat(param, grad, buf, lr, momentum, dampening, weight_decay, nesterov, first_step, grad_scale=1.0):
    check(_L.hnd_sgd_step_flat(ptr(param), ptr(grad), ptr(buf), param.numel(), float(lr), float(momentum),
                               float(dampening), float(weight_decay), int(bool(nesterov)), int(bool(first_step)),
                               float(grad_scale), stream_ptr()), 'hnd_sgd_step_flat')
    PARAM_EPOCH[0] += 1


# include/hnd_optim.h: the state slots of each kind, in descriptor order (None: the kind has no such slot)
OPTIM_STATE_SLOTS = {'adam': ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'), 'adagrad': ('sum', None, None),
                     'rmsprop': ('square_avg', 'momentum_buffer', 'grad_avg')}


def optim_step_flat(kind, param, grad, states, numel=None, step=1, grad_scale=1.0, lr=0.0, weight_decay=0.0, eps=0.0,
                    beta1=0.0, beta2=0.0, momentum=0.0, lr_decay=0.0, amsgrad=False, centered=False):
    """one hnd_optim_step_flat launch.  kind: 'adam' | 'adagrad' | 'rmsprop'; states: up to three tensors (or None) in the
    slot order of OPTIM_STATE_SLOTS[kind]; beta2 is RMSprop's alpha.  Arguments are validated by the library."""
    states = tuple(states) + (None,) * (3 - len(states))
    d = _lib.OptimDesc()
    d.param, d.grad, d.state0, d.state1, d.state2 = ptr(param), ptr(grad), ptr(states[0]), ptr(states[1]), ptr(states[2])
    d.numel, d.step = param.numel() if numel is None else int(numel), int(step)
    d.grad_scale, d.lr, d.weight_decay, d.eps = float(grad_scale), float(lr), float(weight_decay), float(eps)
    d.beta1, d.beta2, d.momentum, d.lr_decay = float(beta1), float(beta2), float(momentum), float(lr_decay)
    d.kind, d.amsgrad, d.centered = _lib.OPTIM_KINDS[kind], int(bool(amsgrad)), int(bool(centered))
    nbuf = 3 + 2 * sum(s is not None for s in states)                  # param r/w, grad r, every state r/w
    _hbm('optim_' + kind, 4 * nbuf * d.numel, lambda: check(_L.hnd_optim_step_flat(C.byref(d), stream_ptr()),
                                                           'hnd_optim_step_flat'))
    PARAM_EPOCH[0] += 1


def interp_out_size(size, scale):
    """F.interpolate(scale_factor=scale) output size: floor(size * scale) in double (torch semantics)."""
    return int(math.floor(float(size) * scale))
