#!/usr/bin/env python3
"""The bottleneck codec at 1 ... 8 bits (include/hnd_codec.h) beside the 8-bit exports it extends, at the b3ch bottleneck of
one image ([1, 3, 200, 336]) and of an eval batch of four ([4, 3, 204, 340]).

  quantise     hnd_quantize_u8 (the path before hnd_codec.h)  |  hnd_quantize_bits  |  hnd_quantize_pack_bits
               each is three launches: min/max partials, qparams, then quantise (+ pack)
  dequantise   hnd_dequantize_u8 on the one-value-per-byte tensor  |  hnd_unpack_dequantize_bits on the payload
               one launch each

Widths 1, 4 and 8.  Interleaved rounds; a repeat is the mean of `reps` calls between two HIP events, after a warm-up of every
variant; the table gives the median, the minimum and the maximum over the rounds, and the bytes that cross the link in
either form.  Before timing, the packed payload is unpacked on the host and compared with the bytes of hnd_quantize_bits,
and the two dequantised buffers with each other.  Nothing is asserted on the times.  No GPU: fails.

usage (GPU box):  python3 tools/bench_codec_bits.py [--rounds 9] [--reps 50] [--out profiles/codec_bits.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1, 3, 200, 336), (4, 3, 204, 340))
WIDTHS = (1, 4, 8)


def host_unpack(payload, numel, bits):
    stream = np.unpackbits(payload, bitorder='little')[:numel * bits].reshape(numel, bits).astype(np.uint16)
    return (stream << np.arange(bits, dtype=np.uint16)[None, :]).sum(1).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    from hnd_ghnd_object_detectors_amd import ops
    dev = torch.device('cuda:0')
    lines = ['bottleneck codec, %d rounds x %d calls between two HIP events, interleaved; us per call' % (a.rounds, a.reps)]
    for shape in SHAPES:
        n, c, h, w = shape
        cs = ops.chan_pad_of(c)
        numel = n * c * h * w
        z = torch.randn(shape, generator=torch.Generator().manual_seed(7)) * 3 + 0.3
        buf = torch.zeros(n, h, w, cs)
        buf[..., :c] = z.permute(0, 2, 3, 1)
        buf = buf.to(dev)
        q = torch.empty(buf.shape, dtype=torch.uint8, device=dev)
        qp = torch.empty(4, device=dev)
        scratch = torch.empty(ops.minmax_scratch_elems(), device=dev)
        out_q, out_p = torch.empty_like(buf), torch.empty_like(buf)
        variants = [('hnd_quantize_u8', 8, numel, lambda: ops.quantize_u8(buf, c, q, qp, scratch))]
        checks = []
        for bits in WIDTHS:
            nbytes = ops.codec_packed_bytes(numel, bits)
            qb = torch.empty_like(q)
            payload = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            qpb, qpp = torch.empty_like(qp), torch.empty_like(qp)
            variants.append(('hnd_quantize_bits', bits, numel,
                             lambda bits=bits, qb=qb, qpb=qpb: ops.quantize_bits(buf, c, bits, qb, qpb, scratch)))
            variants.append(('hnd_quantize_pack_bits', bits, nbytes,
                             lambda bits=bits, payload=payload, qpp=qpp: ops.quantize_pack_bits(buf, c, bits, payload, qpp,
                                                                                                scratch)))
            variants.append(('hnd_dequantize_u8', bits, numel,
                             lambda qb=qb, qpb=qpb: ops.dequantize_u8(qb, qpb, out_q, c)))
            variants.append(('hnd_unpack_dequantize_bits', bits, nbytes,
                             lambda bits=bits, payload=payload, qpp=qpp: ops.unpack_dequantize_bits(payload, qpp, out_p, c,
                                                                                                    bits)))
            for _, _, _, fn in variants[-4:]:
                fn()
            ops.sync_check()
            same_bytes = bool((host_unpack(payload.cpu().numpy(), numel, bits) ==
                               qb.cpu()[..., :c].permute(0, 3, 1, 2).contiguous().view(-1).numpy()).all())
            checks.append('%d bits: payload unpacks to the bytes of hnd_quantize_bits: %s; the two dequantised buffers are '
                          'equal: %s' % (bits, same_bytes, bool(torch.equal(out_q, out_p))))
        for _, _, _, fn in variants:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in variants]
        for _ in range(a.rounds):
            for i, (_, _, _, fn) in enumerate(variants):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[i].append(e0.elapsed_time(e1) * 1e3 / a.reps)
        ops.sync_check()
        lines.append('')
        lines.append('bottleneck %s: %d values, NHWC stride %d (%.1f KB of fp32 on the device)'
                     % (list(shape), numel, cs, buf.numel() * 4 / 1024.0))
        lines.append('%-28s %5s %12s %10s %9s %9s' % ('export', 'bits', 'link bytes', 'median us', 'min us', 'max us'))
        for (name, bits, nbytes, _), t in zip(variants, times):
            lines.append('%-28s %5d %12d %10.2f %9.2f %9.2f' % (name, bits, nbytes, sorted(t)[len(t) // 2], min(t), max(t)))
        lines += checks
    text = '\n'.join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
