#!/usr/bin/env python3
"""Per-image entropy streams with device-built tables (include/hnd_istream.h): what they cost and what crosses the link.

  launch   the four exports (histogram, table build, encode, decode) and the whole ImageStreamQuantizer call at the b3ch
           bottleneck at batch 1 and 16 ([1, 3, 200, 336], [16, 3, 200, 336]) and the b12ch one ([16, 12, 200, 336]), 4 bits,
           beside the two things a user can do without them, on the same build:
             Quantizer(4, per_image=True, packed=True) and its unpacking Dequantizer call;
             n separate Quantizer(4, entropy=True) calls on z[i:i+1], each with its histogram read-back and host table.
  sizes    nbytes and link_bytes of the streams against the packed payload on the N(0.3, 3) input of profiles/entropy.txt

Medians of interleaved rounds; the whole-call rows end in a device synchronisation (the read-backs of the n-calls yardstick
are host work a HIP event pair would not see), the export rows are timed between two HIP events.  Nothing is asserted on the
times.  No GPU: fails.

usage (GPU box):  python3 tools/bench_istream.py [--rounds 9] [--reps 50] [--out profiles/istream.txt]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEOMETRIES = ((1, 3, 200, 336), (16, 3, 200, 336), (16, 12, 200, 336))


def med(t):
    return sorted(t)[len(t) // 2]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def walled(fn, reps):
    """us per call, host clock, the device drained before and after: host work between launches counts"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def bench_shape(a, dev, shape, lines):
    from hnd_ghnd_object_detectors_amd import ops
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    n, c, h, w = shape
    bits, chw = a.bits, c * h * w
    z = (torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(7)) * 3 + 0.3).to(dev)      # profiles/entropy.txt's input
    parts = [z[i:i + 1].contiguous() for i in range(n)]
    streams, packed, single = T.ImageStreamQuantizer(bits), T.Quantizer(bits, per_image=True, packed=True), \
        T.Quantizer(bits, entropy=True)
    deq = T.Dequantizer(bits)
    sb, pb = streams(z, None)[0], packed(z, None)[0]
    q, _, _, hist, lengths, payload, offsets, scratch = streams._bufs[next(iter(streams._bufs))]
    out = torch.empty_like(sb.origin)
    singles = [single(p, None)[0] for p in parts[:1]]
    rows = [
        ('hnd_istream_histogram', timed, lambda: ops.istream_histogram(q, c, bits, hist)),
        ('hnd_istream_build_tables', timed, lambda: ops.istream_build_tables(hist, bits, lengths)),
        ('hnd_istream_encode', timed, lambda: ops.istream_encode(q, c, bits, lengths, payload, offsets, scratch)),
        ('hnd_istream_decode_dequantize', timed,
         lambda: ops.istream_decode_dequantize(payload, offsets, lengths, sb.qparams, out, c, bits)),
        ('hnd_qimage_unpack_dequantize_bits', timed,
         lambda: ops.qimage_unpack_dequantize_bits(pb.payload, pb.qparams, out, c, bits)),
        ('ImageStreamQuantizer(%d) call' % bits, walled, lambda: streams(z, None)),
        ('Quantizer(%d, per_image, packed) call' % bits, walled, lambda: packed(z, None)),
        ('%d x Quantizer(%d, entropy=True) on z[i:i+1]' % (n, bits), walled, lambda: [single(p, None) for p in parts]),
        ('Dequantizer on the streams', walled, lambda: deq(sb, None)),
        ('Dequantizer on the packed payload', walled, lambda: deq(pb, None)),
    ]
    for _, _, fn in rows:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in rows]
    for _ in range(a.rounds):
        for i, (_, clock, fn) in enumerate(rows):
            times[i].append(clock(fn, a.reps if clock is timed else max(1, a.reps // 5)))
    ops.sync_check()
    sb = streams(z, None)[0]
    lines.append('')
    lines.append('bottleneck [%d, %d, %d, %d] at %d bits: %d chunks per image; %d rounds, interleaved; us per call'
                 % (n, c, h, w, bits, sb.chunks_per_image, a.rounds))
    lines.append('%-48s %10s %10s %10s  %s' % ('', 'median', 'min', 'max', 'clock'))
    for (name, clock, _), t in zip(rows, times):
        lines.append('%-48s %10.2f %10.2f %10.2f  %s' % (name, med(t), min(t), max(t),
                                                         'HIP events' if clock is timed else 'host, drained'))
    one = singles[0]
    lines.append('sizes: packed payload %d B (link %d B); streams nbytes %d B = %.3f of packed, link_bytes %d B = %.3f of the '
                 'packed link; image 0 alone as Quantizer(entropy=True): nbytes %d B, link %d B (its message here: %d B)'
                 % (pb.nbytes, pb.link_bytes, sb.nbytes, sb.nbytes / pb.nbytes, sb.link_bytes, sb.link_bytes / pb.link_bytes,
                    one.nbytes, one.link_bytes, sb.image_link_bytes[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--bits', type=int, default=4)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    dev = torch.device('cuda:0')
    lines = ['per-image entropy streams (include/hnd_istream.h) on %s' % torch.cuda.get_device_name(0)]
    for shape in GEOMETRIES:
        bench_shape(a, dev, shape, lines)
    text = '\n'.join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
