#!/usr/bin/env python3
"""Per-image scales for the bottleneck codec and the fake quantiser (include/hnd_qimage.h): what they cost and buy.

  step     the GHND step of bench.py's configuration (faster_rcnn, b3ch, batch 16, 800 x 1333, resident batch) with
           train.fake_quantize = {num_bits: 4} and with {num_bits: 4, per_image: true}, on ONE teacher / student pair of
           one build: the attribute is toggled between rounds (the head's plan is rebuilt by the toggle; one untimed step
           follows every toggle), rounds alternate off / on, a round is the mean of `steps` steps between two HIP events
  launch   every export of the header beside its per-tensor twin (the yardstick) at the b3ch batch-16 bottleneck
           [16, 3, 200, 336] on a stride of 4, at [1, 3, 200, 336] and at the b12ch bottleneck [16, 12, 200, 336]; 4 bits
  rms      the reconstruction RMS error of per-image against per-tensor quantisation on a [4, 3, 5, 7] input whose image i
           is scaled by 4^(i mod 4), at 2, 4 and 8 bits

The tables give the median, the minimum and the maximum over the rounds.  Nothing is asserted on the times.  No GPU: fails.

usage (GPU box):  python3 tools/bench_qimage.py [--rounds 5] [--steps 6] [--reps 50] [--out profiles/qimage.txt]
"""
import argparse
import contextlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEOMETRIES = ((16, 3, 200, 336), (1, 3, 200, 336), (16, 12, 200, 336))
RMS_SHAPE, RMS_WIDTHS = (4, 3, 5, 7), (2, 4, 8)


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

    def step():
        loss = box(images, [dict(t) for t in targets])
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        return loss

    times, losses = {False: [], True: []}, {}
    for key in (False, True):                       # plans, buffers, code objects of both variants
        layer1.train_fake_quant_per_image = key
        for _ in range(2):
            step()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for key in (False, True):
            layer1.train_fake_quant_per_image = key
            losses[key] = float(step().item())      # (untimed: the toggle rebuilt the head's plan)
            times[key].append(timed(step, a.steps))
    layer1.train_fake_quant_per_image = False
    lines.append('GHND step, faster_rcnn b3ch, batch %d, %d x %d, resident batch, train.fake_quantize.num_bits = %d; %d rounds '
                 'x %d steps between two HIP events, off / on alternating; ms per step'
                 % (a.batch, a.height, a.width, a.bits, a.rounds, a.steps))
    lines.append('%-34s %10s %9s %9s' % ('train.fake_quantize.per_image', 'median ms', 'min ms', 'max ms'))
    for key in (False, True):
        t = times[key]
        lines.append('%-34s %10.3f %9.3f %9.3f' % ('absent' if not key else 'true', med(t), min(t), max(t)))
    lines.append('difference of the medians: %+.3f ms (%+.2f %%); last losses: absent %.6g, per image %.6g'
                 % (med(times[True]) - med(times[False]), 100.0 * (med(times[True]) / med(times[False]) - 1.0),
                    losses[False], losses[True]))
    del box, teacher, student, optimizer
    torch.cuda.empty_cache()


def bench_launch(a, dev, shape, lines):
    from hnd_ghnd_object_detectors_amd import ops
    n, c, h, w = shape
    bits = a.bits
    cs = ops.chan_pad_of(c)
    z = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(7)) * 3 + 0.3
    z = z * torch.tensor([4.0 ** (i % 4) for i in range(n)]).view(-1, 1, 1, 1)
    buf = torch.zeros(n, h, w, cs)
    buf[..., :c] = z
    buf = buf.to(dev)
    npix, nbytes = n * h * w, ops.codec_packed_bytes(n * c * h * w, bits)
    work, out = buf.clone(), torch.empty_like(buf)
    q = torch.empty(buf.shape, dtype=torch.uint8, device=dev)
    payload = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    qp, qpc = torch.empty(4, device=dev), torch.empty(n, 4, device=dev)
    scratch = torch.empty(ops.minmax_scratch_elems(), device=dev)
    scratch_c = torch.empty(ops.qimage_scratch_elems(n), device=dev)
    stats = torch.empty(ops.fake_quantize_tiles(npix), 2, cs, device=dev)
    ops.quantize_bits(buf, c, bits, q, qp, scratch)                      # (valid codes and qparams for the inverses)
    ops.quantize_pack_bits(buf, c, bits, payload, qp, scratch)
    qc, payload_c = q.clone(), payload.clone()
    ops.qimage_quantize_bits(buf, c, bits, qc, qpc, scratch_c)
    ops.qimage_quantize_pack_bits(buf, c, bits, payload_c, qpc, scratch_c)
    pairs = [
        ('quantize_bits', lambda: ops.quantize_bits(buf, c, bits, q, qp, scratch),
         lambda: ops.qimage_quantize_bits(buf, c, bits, qc, qpc, scratch_c)),
        ('dequantize_u8', lambda: ops.dequantize_u8(q, qp, out, c), lambda: ops.qimage_dequantize_u8(qc, qpc, out, c)),
        ('quantize_pack_bits', lambda: ops.quantize_pack_bits(buf, c, bits, payload, qp, scratch),
         lambda: ops.qimage_quantize_pack_bits(buf, c, bits, payload_c, qpc, scratch_c)),
        ('unpack_dequantize_bits', lambda: ops.unpack_dequantize_bits(payload, qp, out, c, bits),
         lambda: ops.qimage_unpack_dequantize_bits(payload_c, qpc, out, c, bits)),
        ('fake_quantize_bits (in place, stats)', lambda: ops.fake_quantize_bits(work, c, bits, qp, scratch, stats=stats),
         lambda: ops.qimage_fake_quantize_bits(work, c, bits, qpc, scratch_c, stats=stats)),
    ]
    variants = [fn for _, twin, new in pairs for fn in (twin, new)]
    for fn in variants:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(a.launch_rounds):
        for i, fn in enumerate(variants):
            times[i].append(timed(fn, a.reps) * 1e3)
    ops.sync_check()
    lines.append('')
    lines.append('bottleneck [%d, %d, %d, %d]: NHWC stride %d, %.1f MB of fp32 on the device, %d bits; %d rounds x %d calls '
                 'between two HIP events, interleaved; us per call' % (n, c, h, w, cs, buf.numel() * 4 / 1e6, bits,
                                                                       a.launch_rounds, a.reps))
    lines.append('%-40s %22s %22s %8s' % ('export', 'per tensor (hnd_*)', 'per image (hnd_qimage_*)', 'ratio'))
    lines.append('%-40s %22s %22s' % ('', 'median (min .. max)', 'median (min .. max)'))
    for k, (name, _, _) in enumerate(pairs):
        t, u = times[2 * k], times[2 * k + 1]
        lines.append('%-40s %8.2f (%5.2f .. %5.2f) %8.2f (%5.2f .. %5.2f) %8.2f'
                     % (name, med(t), min(t), max(t), med(u), min(u), max(u), med(u) / med(t)))


def rms_table(a, dev, lines):
    from hnd_ghnd_object_detectors_amd import ops
    n, c, h, w = RMS_SHAPE
    cs = ops.chan_pad_of(c)
    z = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(15 + c)) * 3 + 0.3          # tests/codec_util.py's recipe
    z = z * torch.tensor([4.0 ** (i % 4) for i in range(n)]).view(-1, 1, 1, 1)
    buf = torch.zeros(n, h, w, cs)
    buf[..., :c] = z.permute(0, 2, 3, 1)
    buf = buf.to(dev)
    q, out = torch.empty(buf.shape, dtype=torch.uint8, device=dev), torch.empty_like(buf)
    qp, qpc = torch.empty(4, device=dev), torch.empty(n, 4, device=dev)
    scratch = torch.empty(ops.minmax_scratch_elems(), device=dev)
    scratch_c = torch.empty(ops.qimage_scratch_elems(n), device=dev)
    lines.append('')
    lines.append('reconstruction RMS error on [%d, %d, %d, %d], image i scaled by 4^(i mod 4)' % RMS_SHAPE)
    lines.append('%5s %14s %14s %8s' % ('bits', 'per tensor', 'per image', 'ratio'))
    want = buf[..., :c].double()
    for bits in RMS_WIDTHS:
        ops.quantize_bits(buf, c, bits, q, qp, scratch)
        ops.dequantize_u8(q, qp, out, c)
        flat = float(torch.sqrt(((out[..., :c].double() - want) ** 2).mean()))
        ops.qimage_quantize_bits(buf, c, bits, q, qpc, scratch_c)
        ops.qimage_dequantize_u8(q, qpc, out, c)
        per = float(torch.sqrt(((out[..., :c].double() - want) ** 2).mean()))
        lines.append('%5d %14.4e %14.4e %8.3f' % (bits, flat, per, per / flat))


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
    ap.add_argument('--no_step', action='store_true', help='only the launch and RMS tables')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    dev = torch.device('cuda:0')
    lines = ['per-image scales (include/hnd_qimage.h) on %s' % torch.cuda.get_device_name(0), '']
    if not a.no_step:
        bench_step(a, dev, lines)
    for shape in GEOMETRIES:
        bench_launch(a, dev, shape, lines)
    rms_table(a, dev, lines)
    text = '\n'.join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
