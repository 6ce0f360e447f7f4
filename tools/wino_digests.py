#!/usr/bin/env python3
"""SHA-256 of every buffer the launches of csrc/winograd.hip write, one line per case and buffer: the bit-for-bit gate
of a change to those kernels.  Run once per library (HND_LIB_PATH names it; default: the one in the tree), each in a
process of its own, and `diff` the two outputs.

The cases are the tables of tests/wino_util.py (TABLES, OVER_CASES, WGRAD_CASES, BNBWD_CASES / BNBWD_OVER, OVER_WEIGHTS,
OVER_WGRAD_OUT, OVER_DY) with their seeded operands: drawn on the CPU, except the over-cap cases, whose 150 M elements
come from the device generator under a fixed seed as in tests/test_wino_gpu.py.  Every written buffer starts as NaN
(mask_out: 0xA5), so a digest also covers what a launch must leave alone.  U, V, Z, dW, statistics / partials and mask_out
come straight from the transforms; Y passes through the component GEMMs, which both libraries share.

usage (GPU box):  HND_LIB_PATH=/path/to/libhnd_hip.so python3 tools/wino_digests.py > digests.txt
"""
import hashlib
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hnd_ghnd_object_detectors_amd import _lib, ops  # noqa: E402
from tests import conv_util as U  # noqa: E402
from tests import wino_util as W  # noqa: E402

DEV = 'cuda:0'
NAN = float('nan')


def emit(case, **buffers):
    for name, buf in buffers.items():
        if buf is not None:
            raw = buf.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
            print('%-52s %-8s %s' % (case, name, hashlib.sha256(raw).hexdigest()), flush=True)


def nans(*shape):
    return torch.full(shape, NAN, device=DEV)


def to_nhwc(t_nchw, lanes):
    t = t_nchw.permute(0, 2, 3, 1)
    if t.shape[-1] != lanes:
        t = F.pad(t, (0, lanes - t.shape[-1]))
    return t.contiguous().to(DEV)


def vec(v, lanes):
    return F.pad(v, (0, lanes - v.numel())).to(DEV)


def prologue_kw(c, t):
    kw = dict(pro_relu=c.pro in ('relu', W.SCALE_RELU))
    if 'ps' in t:
        kw['pro_scale'] = vec(t['ps'], c.cin)
    if 'pb' in t:
        kw['pro_shift'] = vec(t['pb'], c.cin)
    return kw


def conv(tag, c, t):
    """a forward / data-gradient case as tests/test_wino_gpu.py launches it"""
    e = U.epi_of(c.epi)
    ldc = W.lanes_out(c) if 'bwd' in e else W.ldc_of(c)
    cls, wcls = (ops.WinoConv, ops.WinoWeights) if c.k == 3 else (ops.Wino2Conv, ops.Wino2Weights)
    ww = wcls(t['wp'].to(DEV).contiguous(), dgrad=c.dgrad, tile=c.tile)
    nv, nm = cls.scratch_elems(c.n, c.oh, c.ow, c.cin, c.cout, c.tile)
    v, m, y = nans(nv), nans(nm), nans(c.n, c.oh, c.ow, ldc)
    stats = mask_out = None
    kw = dict(prologue_kw(c, t), relu='relu' in e)
    if 'es' in e:
        kw['epi_scale'] = vec(t['es'], ldc)
    if 'eb' in e:
        kw['epi_shift'] = vec(t['eb'], ldc)
    if c.k == 3:
        for name, key in (('r1', 'res1'), ('mask', 'mask')):
            if name in e:
                kw[key] = to_nhwc(t[name], ldc)
        if 'mout' in e:
            mask_out = kw['mask_out'] = torch.full((c.n, c.oh, c.ow, ldc // 4), 0xA5, dtype=torch.uint8, device=DEV)
        launch = cls(to_nhwc(t['x'], c.cin), ww, y, v, m, **kw)
    else:
        if 'stats' in e or 'bwd' in e:
            stats = nans(W.stats_blocks(c), 2, W.lanes_out(c))
        if 'stats' in e:
            kw['stats'] = stats
        if 'bwd' in e:
            kw['bwd_stats'] = (to_nhwc(t['bx'], ldc), vec(t['bsc'], ldc), vec(t['bsh'], ldc), vec(t['bmu'], ldc),
                               vec(t['brs'], ldc), 'lin' not in e, stats)
        launch = cls(to_nhwc(t['x'], c.cin), ww, y, v, m, c.pad, **kw)
    launch.run()
    ops.sync_check()
    emit('%s %s' % (tag, W.case_id(c)), U=ww.buf, V=v, Y=y, stats=stats, mask_out=mask_out)


def wgrad(c, route):
    t = W.wgrad_inputs(c)
    nv, nm = ops.Wino2Conv.scratch_elems(c.n, c.oh, c.ow, c.cin, c.cout, c.tile)
    v, m = nans(nv), nans(nm)
    z, s, dw = nans(c.ncomp * c.tiles_pad * c.cout), nans(c.ncomp * c.cout * c.cin), nans(c.cout, c.cin, 2, 2)
    x = to_nhwc(t['x'], c.cin)
    if route == 'fwd':
        fwd = ops.Wino2Conv(x, ops.Wino2Weights(t['wp'].to(DEV).contiguous(), tile=c.tile),
                            torch.empty(c.n, c.oh, c.ow, c.cout, device=DEV), v, m, c.pad, **prologue_kw(c, t))
        fwd.run()
    else:
        fwd = ops.Wino2InputTransform(x, v, c.pad, c.cout, c.tile, **prologue_kw(c, t))
        fwd._run_input()
    ops.Wino2Wgrad(fwd, to_nhwc(t['dy'], c.cout), dw, z, s).run()
    ops.sync_check()
    emit('wgrad %s %s' % (W.case_id(c), route), V=v, Z=z, dW=dw)


def bnbwd(L, n, oh, ow, c, pad, relu, t):
    tp_d, tp_w = int(L.hnd_wino2_tiles_pad(n, oh + 2 * pad - 1, ow + 2 * pad - 1, 6)), int(L.hnd_wino2_tiles_pad(n, oh, ow, 6))
    g, x = [t[k].permute(0, 2, 3, 1).contiguous().to(DEV) for k in ('g', 'x')]
    sc, sh, k123 = t['scale'].to(DEV), t['shift'].to(DEV), t['k123'].to(DEV).contiguous()
    v, z = nans(49 * tp_d * c), nans(49 * tp_w * c)
    _lib.check(L.hnd_wino26_bnbwd_transforms(g.data_ptr(), x.data_ptr(), sc.data_ptr(), sh.data_ptr(), k123.data_ptr(), int(relu),
                                             n, oh, ow, c, pad, v.data_ptr(), z.data_ptr(), ops.stream_ptr()),
               'hnd_wino26_bnbwd_transforms')
    ops.sync_check()
    emit('bnbwd %d-%d-%d-%d-%d-%d' % (n, oh, ow, c, pad, relu), V=v, Z=z)


def main():
    assert torch.cuda.is_available(), 'needs a GPU'
    L = _lib.load()
    print('library: %s' % _lib.LIB_PATH, file=sys.stderr)       # (not part of the output: the two runs must diff empty)
    with ops.emulation('off'):
        for key, cases in W.TABLES.items():
            for c in cases:
                conv('%d-%d-%s' % key, c, W.make_inputs(c))
        for c in W.OVER_CASES:
            conv('over', c, W.over_inputs(c, DEV))
        for c, route, _ in W.WGRAD_CASES:
            wgrad(c, route)
        for case in W.BNBWD_CASES:
            bnbwd(L, *case, W.bnbwd_inputs(*case))
        n, oh, ow, c, pad, relu = W.BNBWD_OVER
        gen = torch.Generator(device=DEV).manual_seed(62000)
        t = dict(g=torch.randn(n, oh, ow, c, generator=gen, device=DEV).permute(0, 3, 1, 2),
                 x=torch.randn(n, oh, ow, c, generator=gen, device=DEV).permute(0, 3, 1, 2),
                 scale=torch.rand(c, generator=gen, device=DEV) + 0.5, shift=torch.randn(c, generator=gen, device=DEV) * 0.5,
                 k123=torch.randn(3, c, generator=gen, device=DEV) * 0.5)
        bnbwd(L, n, oh, ow, c, pad, relu, t)
        # the transforms that no GEMM follows, alone on their second trip
        rows, depth = W.OVER_ROWS, W.OVER_DEPTH
        for k, tile, dgrad in W.OVER_WEIGHTS:
            gen = torch.Generator(device=DEV).manual_seed(63000 + 10 * k + tile)
            cout, cin = (depth, rows) if dgrad else (rows, depth)
            w = torch.randn(cout, cin, k, k, generator=gen, device=DEV)
            u = nans((tile + k - 1) ** 2, rows, depth)
            fn = L.hnd_wino_weights if k == 3 else L.hnd_wino2_weights
            _lib.check(fn(w.data_ptr(), u.data_ptr(), cout, cin, int(dgrad), tile, ops.stream_ptr()), 'weights')
            ops.sync_check()
            emit('over weights %d-%d-%d' % (k, tile, dgrad), U=u)
        for tile, st in W.OVER_WGRAD_OUT:
            gen = torch.Generator(device=DEV).manual_seed(64000 + tile + st)
            s = torch.randn((tile + 1) ** 2, rows, depth, generator=gen, device=DEV)
            dw = nans(rows, depth, 2, 2)
            _lib.check(L.hnd_wino2_wgrad_output_t(s.data_ptr(), dw.data_ptr(), rows, depth, tile, st, ops.stream_ptr()), 'wgrad_output')
            ops.sync_check()
            emit('over wgrad_out %d-%d' % (tile, st), dW=dw)
        for n, oh, ow, cout, tile in W.OVER_DY:
            gen = torch.Generator(device=DEV).manual_seed(65000 + tile)
            dy = torch.randn(n, oh, ow, cout, generator=gen, device=DEV)
            z = nans((tile + 1) ** 2, int(L.hnd_wino2_tiles_pad(n, oh, ow, tile)), cout)
            _lib.check(L.hnd_wino2_dy(dy.data_ptr(), z.data_ptr(), n, oh, ow, cout, cout, tile, ops.stream_ptr()), 'dy')
            ops.sync_check()
            emit('over dy %d-%d-%d-%d-%d' % (n, oh, ow, cout, tile), Z=z)


if __name__ == '__main__':
    main()
