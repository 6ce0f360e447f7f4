#!/usr/bin/env python3
"""Several loss terms on ONE student tensor, at the layer-1 map of the benchmark ([16, 200, 336, 256], 1.1 GB): the grouped
loss launch (pairs that share `grad`: student read once, each teacher once, the summed gradient stored once) beside what a
caller would need without it -- the same terms in one launch with a gradient buffer each, then hnd_add_inplace per extra
term.

  variant                      passes over the map
  grouped launch of m          m + 2                  (m teachers, the student, the gradient)
  separate buffers, then add   3 m + 3 (m - 1)        (teacher + student + gradient per term; read 2, write 1 per add)

Interleaved rounds; a repeat is the mean of `reps` calls between two HIP events, after a warm-up of every variant.  The
grouped gradient is first compared with the separate-buffers one on the same inputs (rel-L2; both add the same fp32
values in the same order).  No GPU: fails.

usage (GPU box):  python3 tools/bench_mimic_shared.py [--rounds 7] [--reps 30] [--out profiles/mimic_shared_terms.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = (('mse', 0.0, False), ('l1', 0.0, True), ('smooth_l1', 0.5, True))     # (kind, param, mean?) of member k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    from hnd_ghnd_object_detectors_amd import ops
    dev = torch.device('cuda:0')
    shp = (a.batch, 200, 336, 256)
    g = torch.Generator(device=dev).manual_seed(1)
    s = torch.randn(shp, device=dev, generator=g).clamp_(min=0)
    ts = [torch.randn(shp, device=dev, generator=g).clamp_(min=0) for _ in KINDS]
    numel = s.numel()
    shared = torch.empty(shp, device=dev)
    own = [torch.empty(shp, device=dev) for _ in KINDS]
    variants, checks = [], []
    for m in (2, 3):
        def pairs(grads):
            return [(ts[k], s, grads[k], 1.0, True, KINDS[k][0], KINDS[k][1], numel if KINDS[k][2] else 0) for k in range(m)]
        grouped = ops.MimicLaunch(pairs([shared] * m), dev)
        separate = ops.MimicLaunch(pairs(own), dev)

        def run_separate(launch=separate, m=m):
            launch.run()
            for k in range(1, m):
                ops.add_inplace(own[0], own[k])
        variants.append(('grouped launch of %d' % m, (m + 2) * 4 * numel, grouped.run))
        variants.append(('%d buffers in one launch, then %d add_inplace' % (m, m - 1), (3 * m + 3 * (m - 1)) * 4 * numel,
                         run_separate))
        grouped.run()
        run_separate()
        ops.sync_check()
        checks.append('m = %d: rel-L2 of the grouped gradient against separate buffers + add %.2e, terms equal: %s'
                      % (m, float((shared - own[0]).norm() / own[0].norm()), bool(torch.equal(grouped.out, separate.out))))
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
            times[i].append(e0.elapsed_time(e1) / a.reps)
    ops.sync_check()
    lines = ['terms on one student tensor, layer-1 map %s (%.2f GB), %d rounds x %d calls, interleaved'
             % (list(shp), 4 * numel / 1e9, a.rounds, a.reps),
             '%-46s %9s %9s %9s %9s %8s' % ('variant', 'GB moved', 'median ms', 'min ms', 'max ms', 'TB/s')]
    med = []
    for (name, nbytes, _), t in zip(variants, times):
        med.append(sorted(t)[len(t) // 2])
        lines.append('%-46s %9.2f %9.4f %9.4f %9.4f %8.3f' % (name, nbytes / 1e9, med[-1], min(t), max(t), nbytes / med[-1] / 1e9))
    for i, m in enumerate((2, 3)):
        lines.append('m = %d: the grouped launch takes %.2fx the time of the alternative (traffic alone: %.2fx)'
                     % (m, med[2 * i] / med[2 * i + 1], (m + 2) / (3 * m + 3 * (m - 1))))
    lines += checks
    text = '\n'.join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    assert all(med[2 * i] <= med[2 * i + 1] for i in range(2)), 'the grouped launch is slower than the alternative'


if __name__ == '__main__':
    main()
