#!/usr/bin/env python
"""Per-shape A/B of the two builds of the bf16x3 emulation GEMM: the persistent kernel (csrc/conv_bx3.hip) against the tiled
one (csrc/conv_bx3_tiled.hip, 64- and 128-row tile), on the step's emulated 1x1 launches at batch 4 / 8 / 16 and on a sweep of
chunks per team for every K.  Each shape: torch.equal on the builds' outputs first, then ms per launch with HIP events, the
builds ALTERNATING (rounds of 10 launches each, 6 rounds, the median round counts); operands re-used, so L2 / MALL-warm like
inside the step.  The crossover of the picker (csrc/conv_bx3.hip: bx3_build) is read from the `c/team` and `x` columns.

    python tools/bench_bx3_tiled.py > profiles/rNN_bx3_tiled_shapes.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hnd_ghnd_object_detectors_amd import ops  # noqa: E402

DEV = torch.device('cuda:0')
# the step's launches of the B-resident emulation kernel at 800 x 1344 (one image's map): name, cin, cout, h, w, stride, extras
STEP = [
    ('layer1.x.conv1 256->64', 256, 64, 200, 336, 1, 'epi'),
    ('layer2.0.conv1 256->128', 256, 128, 200, 336, 1, 'epi'),
    ('layer2.0.downsample 256->512 s2', 256, 512, 200, 336, 2, 'epi'),
    ('layer2.x.conv3 128->512 +res', 128, 512, 100, 168, 1, 'epi+res+mo'),
    ('layer2.x.conv1 512->128', 512, 128, 100, 168, 1, 'epi'),
    ('layer3.0.downsample 512->1024 s2', 512, 1024, 100, 168, 2, 'epi'),
    ('layer3.x.conv3 256->1024 +res', 256, 1024, 50, 84, 1, 'epi+res+mo'),
    ('layer3.x.conv1 1024->256', 1024, 256, 50, 84, 1, 'epi'),
    ('layer3.x.conv1.dgrad 256->1024 mask+res', 256, 1024, 50, 84, 1, 'mask+res'),
    ('layer4.0.downsample 1024->2048 s2', 1024, 2048, 50, 84, 2, 'epi'),
    ('layer4.x.conv3 512->2048 +res', 512, 2048, 25, 42, 1, 'epi+res+mo'),
    ('layer4.x.conv1 2048->512', 2048, 512, 25, 42, 1, 'epi'),
    ('layer4.x.conv3.dgrad 2048->512 mask', 2048, 512, 25, 42, 1, 'mask'),
    ('fpn.inner0 256->256', 256, 256, 200, 336, 1, 'bias+up'),
    ('fpn.inner1 512->256', 512, 256, 100, 168, 1, 'bias+up'),
    ('fpn.inner2 1024->256', 1024, 256, 50, 84, 1, 'bias+up'),
    ('fpn.inner3 2048->256', 2048, 256, 25, 42, 1, 'bias'),
]
BUILDS = [('persistent', 'bx3_tiled=0'), ('tiled 64', 'bx3_tiled=1,bx3_tiled_mi=1'), ('tiled 128', 'bx3_tiled=1,bx3_tiled_mi=2')]


class Keyed(object):
    """a launch that runs under its own HND_DEBUG_PICKER value (the key is read per call)"""
    def __init__(self, key, make):
        self.key = key
        os.environ['HND_DEBUG_PICKER'] = key
        self.l = make()

    def run(self, reps=1):
        os.environ['HND_DEBUG_PICKER'] = self.key
        for _ in range(reps):
            self.l.run()


def timed(launches, rounds=6, reps=10):
    """ms per launch of each, alternating: median over `rounds` of `reps` back-to-back launches"""
    for l in launches:
        l.run(3)
    ms = [[] for _ in launches]
    for _ in range(rounds):
        for i, l in enumerate(launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            l.run(reps)
            b.record()
            torch.cuda.synchronize()
            ms[i].append(a.elapsed_time(b) / reps)
    return [sorted(v)[len(v) // 2] for v in ms]


def one(name, cin, cout, n, h, w, stride, extra, g):
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    m = n * oh * ow
    x = torch.randn(n, h, w, cin, generator=g, device=DEV)
    wt = torch.randn(cout, cin, 1, 1, generator=g, device=DEV) / cin ** 0.5
    pk = ops.pack_weights(wt)
    kw = {}
    if 'epi' in extra:
        kw.update(epi_scale=torch.rand(cout, generator=g, device=DEV) + 0.5, epi_shift=torch.randn(cout, generator=g, device=DEV), relu=True)
    if 'bias' in extra:
        kw.update(epi_shift=torch.randn(cout, generator=g, device=DEV))
    if 'up' in extra:
        kw.update(res1=torch.randn(n, oh // 2, ow // 2, cout, generator=g, device=DEV), res1_up=True)
    elif 'res' in extra:
        kw.update(res1=torch.randn(n, oh, ow, cout, generator=g, device=DEV))
    if 'mask' in extra:
        kw.update(mask_bits=torch.randint(0, 16, (n, oh, ow, cout // 4), generator=g, dtype=torch.uint8, device=DEV))
    ys, launches = [], []
    for _, key in BUILDS:
        y = torch.full((n, oh, ow, cout), float('nan'), device=DEV)
        mo = torch.empty(n, oh, ow, cout // 4, dtype=torch.uint8, device=DEV) if 'mo' in extra else None
        with ops.emulation('force'):
            launches.append(Keyed(key, lambda: ops.conv_forward(x, pk, y, 1, stride, 0, mask_out=mo, **kw)))
        assert launches[-1].l.variant == 'bx3_64', launches[-1].l.variant
        launches[-1].run()
        ys.append(y)
    ops.sync_check()
    same = all(torch.equal(ys[0], y) for y in ys[1:])
    ms = timed(launches)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    teams = 8 * ((cus // 8) // (cout // 64))
    chunks = (m + 63) // 64
    tf = 2.0 * m * cin * cout / 1e9
    print('%-42s %2d %7d %5d %7.2f | %8.4f %6.1f | %8.4f %6.1f %5.2f | %8.4f %6.1f %5.2f | %s'
          % (name, n, m, cin, chunks / teams, ms[0], tf / ms[0], ms[1], tf / ms[1], ms[0] / ms[1], ms[2], tf / ms[2],
             ms[0] / ms[2], 'equal' if same else 'BITS DIFFER'))
    sys.stdout.flush()
    return same


def main():
    g = torch.Generator(device=DEV).manual_seed(0)
    quick = '--quick' in sys.argv
    print('%-42s %2s %7s %5s %7s | %8s %6s | %8s %6s %5s | %8s %6s %5s |' % (
        'shape', 'n', 'M', 'K', 'c/team', 'pers ms', 'TF-eq', 't64 ms', 'TF-eq', 'x', 't128 ms', 'TF-eq', 'x'))
    ok = True
    for n in (4, 8, 16):
        for name, cin, cout, h, w, stride, extra in STEP:
            ok &= one(name, cin, cout, n, h, w, stride, extra, g)
    # chunks per team swept for every K at 256 columns (64 teams on 256 CUs) and for K = 256 at 64 / 1024 columns
    print('# sweep: rows = 64 x chunks, one image of 64 x chunks pixels in a row')
    for cin, cout in ((128, 256), (256, 256), (512, 256), (1024, 256), (2048, 256), (256, 64), (256, 1024), (1024, 1024)):
        teams = 8 * (32 // (cout // 64))
        for cpt in ((1, 4, 16) if quick else (0.5, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32)):
            chunks = max(1, int(cpt * teams))
            ok &= one('sweep %d->%d' % (cin, cout), cin, cout, 1, chunks, 64, 1, 'epi', g)
    if not ok:
        sys.exit('some shape gave different bits on the two builds')


if __name__ == '__main__':
    main()
