#!/usr/bin/env python3
"""Quantisation-aware distillation (include/hnd_qat.h): what the fake-quantised bottleneck costs.

  step     the GHND step of bench.py's configuration (faster_rcnn, b3ch, batch 16, 800 x 1333, resident batch) with
           train.fake_quantize absent and with num_bits = 4, on ONE teacher / student pair of one build: the attribute is
           toggled between rounds (the head's plan is rebuilt by the toggle; one untimed step follows every toggle), rounds
           alternate off / on, a round is the mean of `steps` steps between two HIP events
  launch   hnd_fake_quantize_bits alone (its three launches: min/max partials, qparams, quantise + dequantise + statistics),
           in place with `stats` as the engine calls it, at the bottleneck of that step ([16, H, W], 3 channels on a stride
           of 4) and at the b12ch bottleneck of the same geometry (12 channels on a stride of 32), beside the two codec calls
           it fuses (hnd_quantize_bits then hnd_dequantize_u8); widths 2, 4 and 8

The table gives the median, the minimum and the maximum over the rounds.  Nothing is asserted on the times.  No GPU: fails.

usage (GPU box):  python3 tools/bench_fake_quant.py [--rounds 5] [--steps 6] [--reps 50] [--out profiles/fake_quant.txt]
"""
import argparse
import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS = (2, 4, 8)


def med(t):
    return sorted(t)[len(t) // 2]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_step(a, dev, lines):
    from hnd_ghnd_object_detectors_amd.configs import make_config
    from hnd_ghnd_object_detectors_amd.distillation.tool import DistillationBox
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util
    from hnd_ghnd_object_detectors_amd.synthetic import build_distillation_pair
    from hnd_ghnd_object_detectors_amd.utils import data_util
    config = make_config('faster_rcnn', 'ghnd', 3, batch_size=a.batch, pretrained=False, ckpt_root='/nonexistent')
    with contextlib.redirect_stdout(sys.stderr):
        teacher, student = build_distillation_pair(config, dev, seed=0)
    box = DistillationBox(teacher, student, config['train']['criterion'])
    optimizer = func_util.get_optimizer(student, 'Adam', config['train']['optimizer']['params'])
    loader = data_util.SyntheticDetectionLoader(1, a.batch, a.height, a.width, 'faster_rcnn', seed=1234, rank=0)
    images, targets = next(iter(loader))
    images = [im.to(dev) for im in images]
    targets = [{k: v.to(dev) for k, v in t.items()} for t in targets]
    layer1 = student.backbone.body.layer1

    def step():
        loss = box(images, [dict(t) for t in targets])
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        return loss

    times = {None: [], a.bits: []}
    losses = {}
    for key in (None, a.bits):                      # plans, buffers, code objects of both variants
        layer1.train_fake_quant_bits = key
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for key in (None, a.bits):
            layer1.train_fake_quant_bits = key
            losses[key] = float(step().item())      # (untimed: the toggle rebuilt the head's plan)
            times[key].append(timed(step, a.steps))
    shape = tuple(layer1.head_engine().bottleneck().shape)
    layer1.train_fake_quant_bits = None
    lines.append('GHND step, faster_rcnn b3ch, batch %d, %d x %d, resident batch; %d rounds x %d steps between two HIP '
                 'events, off / on alternating; ms per step' % (a.batch, a.height, a.width, a.rounds, a.steps))
    lines.append('%-34s %10s %9s %9s' % ('train.fake_quantize', 'median ms', 'min ms', 'max ms'))
    for key in (None, a.bits):
        t = times[key]
        lines.append('%-34s %10.3f %9.3f %9.3f' % ('absent' if key is None else 'num_bits = %d' % key, med(t), min(t), max(t)))
    lines.append('difference of the medians: %+.3f ms (%+.2f %%); last losses: absent %.6g, %d bits %.6g'
                 % (med(times[a.bits]) - med(times[None]), 100.0 * (med(times[a.bits]) / med(times[None]) - 1.0),
                    losses[None], a.bits, losses[a.bits]))
    del box, teacher, student, optimizer
    torch.cuda.empty_cache()
    return shape


def bench_launch(a, dev, nhw, lines):
    from hnd_ghnd_object_detectors_amd import ops
    n, h, w = nhw
    for c in (3, 12):
        cs = ops.chan_pad_of(c)
        z = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(7)) * 3 + 0.3
        buf = torch.zeros(n, h, w, cs)
        buf[..., :c] = z
        buf = buf.to(dev)
        npix = n * h * w
        work = buf.clone()
        q = torch.empty(buf.shape, dtype=torch.uint8, device=dev)
        out = torch.empty_like(buf)
        qp, qp2 = torch.empty(4, device=dev), torch.empty(4, device=dev)
        scratch = torch.empty(ops.minmax_scratch_elems(), device=dev)
        stats = torch.empty(ops.fake_quantize_tiles(npix), 2, cs, device=dev)
        variants, checks = [], []
        for bits in WIDTHS:
            def pair(bits=bits):
                ops.quantize_bits(buf, c, bits, q, qp2, scratch)
                ops.dequantize_u8(q, qp2, out, c)
            variants.append(('hnd_fake_quantize_bits (in place, stats)', bits,
                             lambda bits=bits: ops.fake_quantize_bits(work, c, bits, qp, scratch, stats=stats)))
            variants.append(('hnd_quantize_bits + hnd_dequantize_u8', bits, pair))
            work.copy_(buf)
            variants[-2][2]()
            pair()
            ops.sync_check()
            checks.append('%d bits: equal to the codec pair bit for bit: %s' % (bits, bool(torch.equal(work, out))))
        for _, _, fn in variants:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(a.launch_rounds):
            for i, (_, _, fn) in enumerate(variants):
                times[i].append(timed(fn, a.reps) * 1e3)
        ops.sync_check()
        lines.append('')
        lines.append('bottleneck [%d, %d, %d, %d]: NHWC stride %d, %.1f MB of fp32 on the device; %d rounds x %d calls between '
                     'two HIP events, interleaved; us per call' % (n, c, h, w, cs, buf.numel() * 4 / 1e6, a.launch_rounds,
                                                                   a.reps))
        lines.append('%-44s %5s %10s %9s %9s %12s' % ('call', 'bits', 'median us', 'min us', 'max us', 'GB/s (r+w)'))
        for (name, bits, _), t in zip(variants, times):
            moved = buf.numel() * 4 * (3 if name.startswith('hnd_fake') else 3.5)    # min/max read + read + write (+ bytes)
            lines.append('%-44s %5d %10.2f %9.2f %9.2f %12.0f' % (name, bits, med(t), min(t), max(t), moved / med(t) / 1e3))
        lines += checks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--launch_rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--bits', type=int, default=4)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--height', type=int, default=800)
    ap.add_argument('--width', type=int, default=1333)
    ap.add_argument('--no_step', action='store_true', help='only the launch table, at [16, 200, 336]')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    dev = torch.device('cuda:0')
    lines = ['fake-quantised bottleneck (include/hnd_qat.h) on %s' % torch.cuda.get_device_name(0), '']
    shape = (a.batch, 200, 336, 4) if a.no_step else bench_step(a, dev, lines)
    bench_launch(a, dev, shape[:3], lines)
    text = '\n'.join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
