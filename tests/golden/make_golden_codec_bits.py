#!/usr/bin/env python
"""Generate tests/golden/tiny_codec_bits.npz FROM THE REFERENCE ITSELF: the reference's own Quantizer(b) / Dequantizer(b)
(src/structure/transformer.py:131-153, imported unmodified over oracle/shim) for b = 1 ... 7 on the reference-made bottleneck
tensor that tiny_eval_quantized.npz already holds as ``quantized/z`` (the 8-bit row is in that fixture).

Per width b the file holds what the reference emitted:
  b<b>/bytes        uint8 [N, 3, h, w]   QuantizedTensor.tensor (one value per byte: the reference never packs)
  b<b>/scale        float32              float(QuantizedTensor.scale)
  b<b>/zero_point   float32              QuantizedTensor.zero_point
  b<b>/dequantized  float32 [N, 3, h, w] Dequantizer(b) of it
and ``oracle_vs_reference_equal``: whether oracle/myutils_r.quantize_tensor / dequantize_tensor, called directly, gave the
same bytes, scale, zero point and floats at every width (asserted before writing, stored as the other generators store
their oracle-vs-reference figure).  ``z`` itself is not copied: the tests read it from tiny_eval_quantized.npz.

usage:  python tests/golden/make_golden_codec_bits.py
"""
import json
import os
import sys
from collections import OrderedDict

sys.dont_write_bytecode = True       # importing the reference must not leave __pycache__ files in it

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import shim_install  # noqa: E402

shim_install.install()
from oracle.myutils_r import dequantize_tensor, quantize_tensor  # noqa: E402
from structure.transformer import Dequantizer, Quantizer  # noqa: E402  (reference)

NAME = 'tiny_codec_bits'
SOURCE = 'tiny_eval_quantized'
WIDTHS = tuple(range(1, 8))


def main():
    src = np.load(os.path.join(HERE, SOURCE + '.npz'))
    z = torch.from_numpy(src['quantized/z'])
    assert z.dtype == torch.float32 and z.dim() == 4 and float(z.max()) > float(z.min())
    out = OrderedDict()
    equal = True
    for b in WIDTHS:
        qz, _ = Quantizer(b)(z.clone(), None)
        deq, _ = Dequantizer(b)(qz, None)
        assert qz.tensor.dtype == torch.uint8 and int(qz.tensor.max()) <= 2 ** b - 1
        out['b%d/bytes' % b] = qz.tensor.numpy()
        out['b%d/scale' % b] = np.float32(float(qz.scale))
        out['b%d/zero_point' % b] = np.float32(float(qz.zero_point))
        out['b%d/dequantized' % b] = deq.numpy()
        o_q = quantize_tensor(z.clone(), b)
        equal = equal and torch.equal(o_q.tensor, qz.tensor) and float(o_q.scale) == float(qz.scale) and \
            int(o_q.zero_point) == int(qz.zero_point) and torch.equal(dequantize_tensor(o_q), deq)
        print('   %d bits: scale %.6g zero point %d, %d distinct values' % (
            b, float(qz.scale), int(qz.zero_point), int(qz.tensor.unique().numel())))
    assert equal, 'oracle/myutils_r.py disagrees with the reference classes'
    out['oracle_vs_reference_equal'] = np.bool_(equal)
    out['meta'] = np.array(json.dumps({'source': SOURCE, 'key': 'quantized/z', 'shape': list(z.shape),
                                       'widths': list(WIDTHS)}))
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **out)
    print('   wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
