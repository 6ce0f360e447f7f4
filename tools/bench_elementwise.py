#!/usr/bin/env python3
"""The HBM-bound elementwise kernels of the step in isolation, at the step's sizes (batch 16, 800x1344), against a torch
elementwise op moving the same bytes (what a plain streaming kernel reaches on this box).

usage (GPU box):  python3 tools/bench_elementwise.py [--reps 30]
                  python3 tools/bench_elementwise.py --mimic-kinds [--rounds 9] [--out profiles/mimic_loss_kinds.txt]
                  (the loss launch per criterion kind beside MseLaunch, on the four maps of the default step)
                  python3 tools/bench_elementwise.py --optim-kinds [--rounds 9] [--out FILE]
                  (hnd_optim_step_flat per kind beside hnd_adam_step_flat, at the student's arena size and at 64 M elements)
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def mimic_kinds(a, out_path=None):
    """The loss launch of the default step (layer1..4 maps of batch 16, 3x800x1333; gradient written, layer4 masked by its
    ReLU) through ops.MseLaunch and through ops.MimicLaunch for every kind, sum and mean.  `rounds` repeats, the variants
    interleaved inside each; a repeat is the mean of `reps` launches between two HIP events.  A kind is judged against the
    MseLaunch median plus that run's own spread of MseLaunch (max - min of its repeats)."""
    from hnd_ghnd_object_detectors_amd import ops
    dev = torch.device('cuda:0')
    n = a.batch
    g = torch.Generator(device=dev).manual_seed(1)
    shapes = [(n, 200, 336, 256), (n, 100, 168, 512), (n, 50, 84, 1024), (n, 25, 42, 2048)]
    maps = []
    for i, shp in enumerate(shapes):        # ReLU outputs on both sides: exact zeros, and |d| on both sides of beta / delta
        t = torch.randn(shp, device=dev, generator=g).clamp_(min=0)
        s = torch.randn(shp, device=dev, generator=g).clamp_(min=0)
        maps.append((t, s, torch.empty(shp, device=dev), 1.0, i == 3))
    nbytes = sum(12 * t.numel() for t, *_ in maps)
    variants = [('MseLaunch (hnd_mse_sum_fwd_bwd)', ops.MseLaunch(maps, dev))]
    for kind, param in (('mse', 0.0), ('l1', 0.0), ('smooth_l1', 0.5), ('huber', 0.5)):
        for red in ('sum', 'mean'):
            pairs = [p + (kind, param, p[0].numel() if red == 'mean' else 0) for p in maps]
            variants.append(('MimicLaunch %s %s' % (kind, red), ops.MimicLaunch(pairs, dev)))
    for _, launch in variants:
        for _ in range(3):
            launch.run()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(a.rounds):
        for i, (_, launch) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                launch.run()
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1) / a.reps)
    ops.sync_check()
    med = [sorted(t)[len(t) // 2] for t in times]
    spread = max(times[0]) - min(times[0])
    lines = ['loss launch on the four maps of the default step (batch %d, %.2f GB moved), %d rounds x %d launches, interleaved'
             % (n, nbytes / 1e9, a.rounds, a.reps),
             '%-34s %9s %9s %9s %8s  %s' % ('launch', 'median ms', 'min ms', 'max ms', 'TB/s', 'vs MseLaunch median + spread')]
    for (name, _), t, m in zip(variants, times, med):
        verdict = '' if t is times[0] else ('within' if m <= med[0] + spread else 'SLOWER by %.4f ms' % (m - med[0] - spread))
        lines.append('%-34s %9.4f %9.4f %9.4f %8.3f  %s' % (name, m, min(t), max(t), nbytes / m / 1e9, verdict))
    lines.append('spread of MseLaunch (max - min of its %d repeats): %.4f ms' % (a.rounds, spread))
    text = '\n'.join(lines)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(text + '\n')


def optim_kinds(a, out_path=None):
    """hnd_optim_step_flat for every kind / flag combination beside hnd_adam_step_flat on the same buffers, at the flat
    arena of the b3ch student (586 566 floats, include/hnd_hip.h) and at 64 M elements.  `rounds` repeats, the variants
    interleaved inside each; a repeat is the mean of `reps` launches between two HIP events.  Bytes per element: the
    parameter and every state are read and written, the gradient is read."""
    from hnd_ghnd_object_detectors_amd import ops
    dev = torch.device('cuda:0')
    lines = []
    for numel in (586566, 64 * 1024 * 1024):
        p, g = torch.randn(numel, device=dev), torch.randn(numel, device=dev)
        s = [torch.rand(numel, device=dev) for _ in range(3)]
        variants = [('hnd_adam_step_flat', 28, lambda: ops.adam_step_flat(p, g, s[0], s[1], 1e-9, 0.9, 0.999, 1e-8, 7))]

        def add(name, kind, states, **hyper):
            nbytes = 4 * (3 + 2 * sum(t is not None for t in states))
            variants.append((name, nbytes, lambda: ops.optim_step_flat(kind, p, g, states, step=7, lr=1e-9, eps=1e-8, **hyper)))
        add('adam weight_decay', 'adam', s[:2], beta1=0.9, beta2=0.999, weight_decay=1e-4)
        add('adam amsgrad', 'adam', s, beta1=0.9, beta2=0.999, amsgrad=True)
        add('adam weight_decay amsgrad', 'adam', s, beta1=0.9, beta2=0.999, weight_decay=1e-4, amsgrad=True)
        add('adagrad', 'adagrad', s[:1], lr_decay=0.1, weight_decay=1e-4)
        add('rmsprop', 'rmsprop', s[:1], beta2=0.99)
        add('rmsprop momentum', 'rmsprop', s[:2], beta2=0.99, momentum=0.9)
        add('rmsprop centered', 'rmsprop', [s[0], None, s[2]], beta2=0.99, centered=True)
        add('rmsprop centered momentum', 'rmsprop', s, beta2=0.99, momentum=0.9, centered=True)
        for _, _, fn in variants:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(a.rounds):
            for i, (_, _, fn) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[i].append(e0.elapsed_time(e1) / a.reps * 1e3)
        ops.sync_check()
        med = [sorted(t)[len(t) // 2] for t in times]
        lines.append('%d elements, %d rounds x %d launches, interleaved' % (numel, a.rounds, a.reps))
        lines.append('%-28s %6s %10s %9s %9s %8s  %s' % ('launch', 'B/elem', 'median us', 'min us', 'max us', 'TB/s',
                                                        'us per (B/elem), hnd_adam_step_flat = 1'))
        for (name, nb, _), t, m in zip(variants, times, med):
            lines.append('%-28s %6d %10.2f %9.2f %9.2f %8.3f  %.3f' % (name, nb, m, min(t), max(t), nb * numel / m / 1e6,
                                                                     (m / nb) / (med[0] / 28)))
        del p, g, s, variants
    text = '\n'.join(lines)
    print(text, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--mimic-kinds', action='store_true', help='only the loss launch, per criterion kind, beside MseLaunch')
    ap.add_argument('--optim-kinds', action='store_true', help='only the optimizer launches of include/hnd_optim.h, per '
                    'kind, beside hnd_adam_step_flat')
    ap.add_argument('--rounds', type=int, default=7, help='--mimic-kinds / --optim-kinds: interleaved repeats of every variant')
    ap.add_argument('--out', help='--mimic-kinds / --optim-kinds: also write the table to this file')
    a = ap.parse_args()
    if a.optim_kinds:
        return optim_kinds(a, a.out)
    if a.mimic_kinds:
        return mimic_kinds(a, a.out)
    from hnd_ghnd_object_detectors_amd import ops
    dev = torch.device('cuda:0')
    n = a.batch
    g = torch.Generator().manual_seed(1)
    rows = []

    def report(name, nbytes, ms):
        rows.append((name, nbytes / 1e9, ms, nbytes / ms / 1e9))
        print('%-34s %7.3f GB  %7.3f ms  %6.3f TB/s' % (name, nbytes / 1e9, ms, nbytes / ms / 1e9), flush=True)

    # ---- reference: torch elementwise ops over the layer1 map (16 x 200 x 336 x 256)
    x = torch.randn(n, 200, 336, 256, device=dev)
    y = torch.empty_like(x)
    report('torch.mul(x, 1.5, out=y)', 8 * x.numel(), timed(lambda: torch.mul(x, 1.5, out=y), a.reps))
    report('torch y.copy_(x)', 8 * x.numel(), timed(lambda: y.copy_(x), a.reps))
    z = torch.randn_like(x)
    report('torch.add(x, z, out=y)', 12 * x.numel(), timed(lambda: torch.add(x, z, out=y), a.reps))

    # ---- affine_relu of the head output (+ mask nibbles)
    sc, sh = torch.rand(256, device=dev) + 0.5, torch.randn(256, device=dev)
    bits = ops.mask_nibbles_like(y)
    report('affine_relu', 8 * x.numel(), timed(lambda: ops.affine_relu(x, sc, sh, y, True), a.reps))
    report('affine_relu + nibbles', 8 * x.numel() + bits.numel(),
           timed(lambda: ops.affine_relu(x, sc, sh, y, True, mask_out=bits), a.reps))

    # ---- BN backward of a 256-channel head tensor
    mu, rs = torch.randn(256, device=dev) * 0.1, torch.rand(256, device=dev) + 0.5
    part = torch.empty(ops.bn_bwd_ntiles(x.numel() // 256), 2, 256, device=dev)
    k123 = torch.randn(3, 256, device=dev)
    report('bn_bwd_reduce', 8 * x.numel(), timed(lambda: ops.bn_bwd_reduce(z, x, sc, sh, mu, rs, True, part), a.reps))
    report('bn_bwd_apply', 12 * x.numel(), timed(lambda: ops.bn_bwd_apply(z, x, sc, sh, k123, True, y), a.reps))

    # ---- fused loss + gradient of the layer1 pair
    ml = ops.MseLaunch([(x, z, y, 1.0, False)], dev)
    report('mse (layer1 pair, + gradient)', 12 * x.numel(), timed(lambda: ml.run(), a.reps))
    del x, y, z, bits, part

    # ---- stem pool: 16 x 400 x 672 x 64 -> 200 x 336
    a0 = torch.randn(n, 400, 672, 64, device=dev)
    x0 = torch.empty(n, 200, 336, 64, device=dev)
    idx = torch.empty(n, 200, 336, 64, dtype=torch.uint8, device=dev)
    report('maxpool_fwd', 4 * a0.numel() + 5 * x0.numel(), timed(lambda: ops.maxpool_fwd(a0, x0, idx), a.reps))
    gx = torch.randn_like(x0)
    dconv = torch.empty_like(a0)
    s64 = torch.rand(64, device=dev) + 0.5
    report('maxpool_bwd_relu_scale', 8 * a0.numel() + 5 * x0.numel(),
           timed(lambda: ops.maxpool_bwd_relu_scale(gx, idx, a0, s64, dconv), a.reps))
    ops.sync_check()


if __name__ == '__main__':
    main()
