#!/usr/bin/env python3
"""The fixed quantisation range of the bottleneck (include/hnd_qrange.h): what it costs in training, what it saves the codec.

  step     the GHND step of bench.py's configuration (faster_rcnn, b3ch, batch 16, 800 x 1333, resident batch) with
           train.fake_quantize = {num_bits: 4} (the range of each batch) and with range: {type: ema} added, on ONE teacher /
           student pair of one build: the attribute is toggled between rounds (the head's plan is rebuilt by the toggle; one
           untimed step follows every toggle), rounds alternate batch / ema, a round is the mean of `steps` steps between
           two HIP events
  launch   at the bottleneck of that step ([16, H, W], 3 channels on a stride of 4) and at the b12ch bottleneck of the same
           geometry: the three-launch calls hnd_fake_quantize_bits, hnd_quantize_bits and hnd_quantize_pack_bits beside the
           new ones -- hnd_qrange_observe (two launches), hnd_fake_quantize_range (one launch, with mask and stats as the
           engine calls it), hnd_qrange_mask_grad, hnd_quantize_range_bits, hnd_quantize_pack_range_bits -- and the range
           path of a training step as a sum (observe + fake_quantize_range + mask_grad)

The table gives the median, the minimum and the maximum over the rounds.  Nothing is asserted on the times.  No GPU: fails.

usage (GPU box):  python3 tools/bench_qrange.py [--rounds 5] [--steps 6] [--reps 50] [--out profiles/qrange.txt]
"""
import argparse
import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    layer1.train_fake_quant_bits = a.bits
    modes = {'batch': None, 'ema': {'momentum': a.momentum, 'frozen': False}}

    def step():
        loss = box(images, [dict(t) for t in targets])
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        return loss

    times = {k: [] for k in modes}
    losses = {}
    for key in modes:                               # plans, buffers, code objects of both variants
        layer1.train_fake_quant_range = modes[key]
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for key in modes:
            layer1.train_fake_quant_range = modes[key]
            losses[key] = float(step().item())      # (untimed: the toggle rebuilt the head's plan)
            times[key].append(timed(step, a.steps))
    shape = tuple(layer1.head_engine().bottleneck().shape)
    host = layer1.fake_quant_range_host()
    layer1.train_fake_quant_range = None
    layer1.train_fake_quant_bits = None
    lines.append('GHND step, faster_rcnn b3ch, batch %d, %d x %d, resident batch, train.fake_quantize.num_bits = %d; %d rounds x '
                 '%d steps between two HIP events, batch / ema alternating; ms per step'
                 % (a.batch, a.height, a.width, a.bits, a.rounds, a.steps))
    lines.append('%-34s %10s %9s %9s' % ('train.fake_quantize.range', 'median ms', 'min ms', 'max ms'))
    for key in modes:
        t = times[key]
        lines.append('%-34s %10.3f %9.3f %9.3f' % ('absent (batch)' if key == 'batch' else '{type: ema, momentum: %g}' % a.momentum,
                                                   med(t), min(t), max(t)))
    spread = max(max(times[k]) - min(times[k]) for k in modes)
    diff = med(times['ema']) - med(times['batch'])
    lines.append('difference of the medians (ema - batch): %+.3f ms (%+.2f %%); widest min-max spread of either mode: %.3f ms '
                 '-> %s' % (diff, 100.0 * diff / med(times['batch']), spread,
                            'within the spread' if abs(diff) <= spread else 'BEYOND the spread'))
    lines.append('last losses: batch %.6g, ema %.6g; running range after %d observations: [%.5g, %.5g]'
                 % (losses['batch'], losses['ema'], int(host['steps']), host['min'], host['max']))
    del box, teacher, student, optimizer
    torch.cuda.empty_cache()
    return shape


def bench_launch(a, dev, nhw, lines):
    from hnd_ghnd_object_detectors_amd import ops
    n, h, w = nhw
    bits = a.bits
    for c in (3, 12):
        cs = ops.chan_pad_of(c)
        z = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(7)) * 3 + 0.3
        buf = torch.zeros(n, h, w, cs)
        buf[..., :c] = z
        buf = buf.to(dev)
        npix = n * h * w
        work, grad = buf.clone(), torch.randn_like(buf)
        q = torch.empty(buf.shape, dtype=torch.uint8, device=dev)
        payload = torch.empty(ops.codec_packed_bytes(npix * c, bits), dtype=torch.uint8, device=dev)
        qp, fixed, state = torch.empty(4, device=dev), torch.empty(4, device=dev), torch.zeros(4, device=dev)
        scratch = torch.empty(ops.minmax_scratch_elems(), device=dev)
        stats = torch.empty(ops.fake_quantize_tiles(npix), 2, cs, device=dev)
        mask = torch.empty(ops.qrange_mask_shape(buf), dtype=torch.uint8, device=dev)
        ops.qrange_qparams(-8.0, 8.5, bits, fixed)          # about 0.4 % of N(0.3, 3) clipped at each end

        def range_path():
            ops.qrange_observe(work, c, bits, a.momentum, state, qp, scratch)
            ops.fake_quantize_range(work, c, bits, qp, mask=mask, stats=stats)
            ops.qrange_mask_grad(grad, mask, c)
        variants = [
            ('hnd_fake_quantize_bits (3 launches)', lambda: ops.fake_quantize_bits(work, c, bits, qp, scratch, stats=stats)),
            ('hnd_qrange_observe (2 launches)', lambda: ops.qrange_observe(buf, c, bits, a.momentum, state, qp, scratch)),
            ('hnd_fake_quantize_range (mask, stats)', lambda: ops.fake_quantize_range(work, c, bits, fixed, mask=mask, stats=stats)),
            ('hnd_fake_quantize_range (no mask)', lambda: ops.fake_quantize_range(work, c, bits, fixed, stats=stats)),
            ('hnd_qrange_mask_grad', lambda: ops.qrange_mask_grad(grad, mask, c)),
            ('observe + fake_quantize_range + mask_grad', range_path),
            ('hnd_quantize_bits (3 launches)', lambda: ops.quantize_bits(buf, c, bits, q, qp, scratch)),
            ('hnd_quantize_range_bits (1 launch)', lambda: ops.quantize_range_bits(buf, c, bits, q, fixed)),
            ('hnd_quantize_pack_bits (3 launches)', lambda: ops.quantize_pack_bits(buf, c, bits, payload, qp, scratch)),
            ('hnd_quantize_pack_range_bits (1 launch)', lambda: ops.quantize_pack_range_bits(buf, c, bits, payload, fixed)),
        ]
        for _, fn in variants:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(a.launch_rounds):
            for i, (_, fn) in enumerate(variants):
                times[i].append(timed(fn, a.reps) * 1e3)
        ops.sync_check()
        lines.append('')
        lines.append('bottleneck [%d, %d, %d, %d] at %d bits: NHWC stride %d, %.1f MB of fp32 on the device; %d rounds x %d calls '
                     'between two HIP events, interleaved; us per call' % (n, c, h, w, bits, cs, buf.numel() * 4 / 1e6,
                                                                           a.launch_rounds, a.reps))
        lines.append('%-44s %10s %9s %9s' % ('call', 'median us', 'min us', 'max us'))
        for (name, _), t in zip(variants, times):
            lines.append('%-44s %10.2f %9.2f %9.2f' % (name, med(t), min(t), max(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--launch_rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--bits', type=int, default=4)
    ap.add_argument('--momentum', type=float, default=0.01)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--height', type=int, default=800)
    ap.add_argument('--width', type=int, default=1333)
    ap.add_argument('--no_step', action='store_true', help='only the launch table, at [16, 200, 336]')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    dev = torch.device('cuda:0')
    lines = ['fixed quantisation range of the bottleneck (include/hnd_qrange.h) on %s' % torch.cuda.get_device_name(0), '']
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
