#!/usr/bin/env python3
"""The entropy-coded link payload of the bottleneck (include/hnd_entropy.h): what it costs and how many bytes it saves.

At the b3ch and b12ch bottleneck shapes ([N, 200, 336], batch 1 and 16) and at 2, 4 and 8 bits: the histogram launch, the
encoder's three launches, the decoder's one launch, and beside them the yardsticks hnd_quantize_pack_bits (three launches)
and hnd_unpack_dequantize_bits (one launch) of include/hnd_codec.h; then nbytes and link_bytes of the stream beside
hnd_codec_packed_bytes.  The input is a normal tensor (N(0.3, 3), the range of the batch) and the same tensor on a fixed range
that clips about 5 % at each end (codes pile up at the ends, as after distillation on a fixed range); with --ckpt and
--config the bottleneck of that distilled student on synthetic images is measured as well.  The table built from a tensor's
own histogram (transformer.huffman_lengths) is used; the host time of the read-back and the builder is printed once.

The table gives the median, the minimum and the maximum over the rounds.  Nothing is asserted.  No GPU: fails.

usage (GPU box):  python3 tools/bench_entropy.py [--launch_rounds 7] [--reps 30] [--out profiles/entropy.txt]
"""
import argparse
import os
import sys
import time

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


def bench_tensor(a, dev, buf, c, bits, label, lines, fixed_range=None):
    """buf: fp32 NHWC [n, h, w, cs] on the device"""
    from hnd_ghnd_object_detectors_amd import ops
    from hnd_ghnd_object_detectors_amd.structure.transformer import huffman_lengths
    n, h, w, cs = buf.shape
    numel = n * c * h * w
    q = torch.empty(buf.shape, dtype=torch.uint8, device=dev)
    qp = torch.empty(4, device=dev)
    mm = torch.empty(ops.minmax_scratch_elems(), device=dev)
    packed = torch.empty(ops.codec_packed_bytes(numel, bits), dtype=torch.uint8, device=dev)
    payload = torch.empty(ops.entropy_capacity(numel), dtype=torch.uint8, device=dev)
    offsets = torch.empty(ops.entropy_chunks(numel) + 1, dtype=torch.int32, device=dev)
    scratch = torch.empty(ops.entropy_scratch_bytes(numel) // 4, dtype=torch.int32, device=dev)
    hist = torch.empty(256, dtype=torch.int32, device=dev)
    out = torch.empty_like(buf)
    if fixed_range is None:
        ops.quantize_bits(buf, c, bits, q, qp, mm)
        ops.quantize_pack_bits(buf, c, bits, packed, qp, mm)
    else:
        ops.qrange_qparams(fixed_range[0], fixed_range[1], bits, qp)
        ops.quantize_range_bits(buf, c, bits, q, qp)
        ops.quantize_pack_range_bits(buf, c, bits, packed, qp)
    ops.code_histogram(q, c, bits, hist)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lengths = huffman_lengths(hist.cpu().tolist(), bits)
    host_ms = (time.perf_counter() - t0) * 1e3
    ops.entropy_encode(q, c, bits, lengths, payload, offsets, scratch)
    nbytes = int(offsets[-1].item())
    link = nbytes + 4 * offsets.numel() + (1 << bits) + 8
    variants = [
        ('hnd_code_histogram (1 launch)', lambda: ops.code_histogram(q, c, bits, hist)),
        ('hnd_entropy_encode (3 launches)', lambda: ops.entropy_encode(q, c, bits, lengths, payload, offsets, scratch)),
        ('hnd_entropy_decode_dequantize (1 launch)',
         lambda: ops.entropy_decode_dequantize(payload, offsets, lengths, qp, out, c, bits)),
        ('hnd_quantize_pack_bits (3 launches)', lambda: ops.quantize_pack_bits(buf, c, bits, packed, qp, mm)),
        ('hnd_unpack_dequantize_bits (1 launch)', lambda: ops.unpack_dequantize_bits(packed, qp, out, c, bits)),
    ]
    for _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(a.launch_rounds):
        for i, (_, fn) in enumerate(variants):
            times[i].append(timed(fn, a.reps) * 1e3)
    ops.sync_check()
    flat = ops.codec_packed_bytes(numel, bits)
    lines.append('')
    lines.append('%s [%d, %d, %d, %d] at %d bits (stride %d): packed %d B, entropy nbytes %d B (%.3f of packed, %.3f bits per '
                 'value), link_bytes %d B (%.3f of packed); longest code %d; read-back + huffman_lengths %.2f ms on the host'
                 % (label, n, c, h, w, bits, cs, flat, nbytes, nbytes / flat, 8.0 * nbytes / numel, link, link / flat,
                    max(lengths), host_ms))
    lines.append('%-44s %10s %9s %9s' % ('call', 'median us', 'min us', 'max us'))
    for (name, _), t in zip(variants, times):
        lines.append('%-44s %10.2f %9.2f %9.2f' % (name, med(t), min(t), max(t)))


def student_bottleneck(a, dev):
    """the bottleneck of a distilled student on synthetic images, or None when no checkpoint was given"""
    if not (a.ckpt and a.config):
        return None
    from hnd_ghnd_object_detectors_amd import engine as E
    from hnd_ghnd_object_detectors_amd.hipnn import to_nhwc
    from hnd_ghnd_object_detectors_amd.models import get_model, load_ckpt
    from hnd_ghnd_object_detectors_amd.models.mimic.split_rcnn import split_rcnn_model
    from hnd_ghnd_object_detectors_amd.myutils.common import yaml_util
    config = yaml_util.load_yaml_file(a.config)
    student = get_model(config['student_model'], dev)
    load_ckpt(a.ckpt, model=student)
    student.eval()
    head, _ = split_rcnn_model(student, None)
    head.eval()
    images = [torch.rand(3, 800, 1333, generator=torch.Generator().manual_seed(k)).to(dev) for k in range(a.student_batch)]
    with torch.no_grad():
        z = head(images)[0]
    return to_nhwc(z).clone(), z.shape[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launch_rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--height', type=int, default=200)
    ap.add_argument('--width', type=int, default=336)
    ap.add_argument('--ckpt', default=None, help='checkpoint of a distilled student (with --config)')
    ap.add_argument('--config', default=None)
    ap.add_argument('--student_batch', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    from hnd_ghnd_object_detectors_amd import ops
    dev = torch.device('cuda:0')
    lines = ['entropy-coded link payload of the bottleneck (include/hnd_entropy.h) on %s; %d rounds x %d calls between two HIP '
             'events, interleaved; us per call' % (torch.cuda.get_device_name(0), a.launch_rounds, a.reps)]
    for c in (3, 12):
        for n in (1, 16):
            cs = ops.chan_pad_of(c)
            z = torch.randn(n, a.height, a.width, c, generator=torch.Generator().manual_seed(7)) * 3 + 0.3
            buf = torch.zeros(n, a.height, a.width, cs)
            buf[..., :c] = z
            buf = buf.to(dev)
            for bits in (2, 4, 8):
                bench_tensor(a, dev, buf, c, bits, 'normal tensor, range of the batch,', lines)
            bench_tensor(a, dev, buf, c, 4, 'normal tensor, fixed range [-4.6, 5.2],', lines, fixed_range=(-4.6, 5.2))
    lines.append('')
    student = student_bottleneck(a, dev)
    if student is None:
        lines.append('a trained student\'s bottleneck: NOT MEASURED (no distilled checkpoint was given: --ckpt / --config)')
    else:
        for bits in (2, 4, 8):
            bench_tensor(a, dev, student[0], student[1], bits, 'distilled student %s,' % os.path.basename(a.ckpt), lines)
    text = '\n'.join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
