"""include/hnd_entropy.h restated with numpy, for the tests of the entropy-coded link payload: the canonical codes of a table
of lengths, the chunked encoder, a decoder that knows nothing of the encoder's tables (it walks the stream bit by bit through
a dictionary of codes), the link_bytes arithmetic, an unconstrained heapq Huffman as the yardstick of the length builder, and
the seeded inputs the GPU tests share.  Independent of transformer.huffman_lengths: `valid_lengths` below builds the tables
the kernel tests use.

A plain module: no fixtures, no pytest settings; importing it loads neither the library nor the launch helpers."""
import heapq

import numpy as np
import torch

CHUNK = 256
MAX_LEN = 12
CHUNK_BYTES = CHUNK * MAX_LEN // 8           # 384

# (n, c, h, w): one short chunk, c = 1 in cs = 4 | exactly 3 full chunks | 546 symbols, a tail of 34, chunks that straddle
# channels and images | cs = 8
SHAPES = [(1, 1, 1, 5), (1, 3, 16, 16), (2, 3, 7, 13), (1, 6, 5, 52)]
GEOMETRIC = (1, 2, 128, 128)                 # 32 768 symbols at 4 bits: code k occurs 1, 1, 2, 4, ..., 2^14 times


def stride_of(shape):
    """the pixel stride the tests give a shape: 4 for up to 4 channels, 8 for the 6-channel case"""
    return 4 if shape[1] <= 4 else 8


def chunks(numel):
    return (numel + CHUNK - 1) // CHUNK if 0 < numel <= 1 << 30 else 0


def capacity(numel):
    return chunks(numel) * CHUNK_BYTES


def link_bytes(nbytes, numel, bits):
    """stream + offsets + lengths + scale and zero point"""
    return nbytes + 4 * (chunks(numel) + 1) + (1 << bits) + 8


def kraft(lengths):
    """the Kraft sum in units of 2^-12 (4096 is 1)"""
    return sum(1 << (MAX_LEN - int(l)) for l in lengths if l)


def canonical_codes(lengths):
    """{symbol: (code, length)}: the symbols with a non-zero length sorted by (length, symbol); the first gets code 0, each
    next one (code + 1) << (len_next - len_cur)"""
    order = sorted((int(l), s) for s, l in enumerate(lengths) if l)
    assert order and all(1 <= l <= MAX_LEN for l, _ in order) and kraft(lengths) <= 1 << MAX_LEN
    codes, code, cur = {}, 0, order[0][0]
    for k, (l, s) in enumerate(order):
        if k:
            code = (code + 1) << (l - cur)
            cur = l
        codes[s] = (code, l)
    return codes


def encode(symbols, lengths):
    """(payload bytes of the whole stream, offsets uint32[nchunks + 1]) of the flat symbol array"""
    symbols = np.asarray(symbols).reshape(-1)
    codes = canonical_codes(lengths)
    out, offsets = [], [0]
    for c0 in range(0, symbols.size, CHUNK):
        bits = []
        for s in symbols[c0:c0 + CHUNK].tolist():
            if s in codes:                                           # a symbol whose length is 0 emits no bits
                v, l = codes[s]
                bits += [(v >> (l - 1 - j)) & 1 for j in range(l)]   # most significant code bit first
        chunk = np.packbits(np.array(bits, dtype=np.uint8), bitorder='little')      # stream bit k = bit k % 8 of byte k / 8
        out.append(chunk)
        offsets.append(offsets[-1] + chunk.size)
    return np.concatenate(out).astype(np.uint8), np.array(offsets, dtype=np.uint32)


def decode(payload, offsets, lengths, numel):
    """the flat symbol array back; checks what the format promises about every chunk on the way"""
    by_code = {(v, l): s for s, (v, l) in canonical_codes(lengths).items()}
    payload, offsets = np.asarray(payload, dtype=np.uint8), np.asarray(offsets)
    assert offsets.size == chunks(numel) + 1 and int(offsets[0]) == 0
    out = []
    for k in range(chunks(numel)):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        stream = np.unpackbits(payload[lo:hi], bitorder='little').tolist()
        want, got, pos, v, l = min(CHUNK, numel - k * CHUNK), [], 0, 0, 0
        while len(got) < want:
            v, l, pos = (v << 1) | stream[pos], l + 1, pos + 1
            assert l <= MAX_LEN
            if (v, l) in by_code:
                got.append(by_code[(v, l)])
                v = l = 0
        assert hi - lo == (pos + 7) // 8 and not any(stream[pos:]), 'chunk %d: size or pad bits' % k
        out += got
    return np.array(out, dtype=np.uint8)


def heap_huffman_depths(hist):
    """{symbol: depth} of an unconstrained Huffman tree of the occurring symbols (heapq; ties by insertion order)"""
    heap = [(int(w), s, (s,)) for s, w in enumerate(hist) if w]
    depth = {s: 0 for _, s, _ in heap}
    heapq.heapify(heap)
    tick = len(hist)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    return depth


def valid_lengths(hist, bits):
    """a valid table for the histogram, made WITHOUT the builder under test: the heapq Huffman depths where they fit in 12
    bits, else the flat code; one occurring symbol gets 1"""
    depth = heap_huffman_depths(hist)
    if len(depth) == 1:
        return bytes(1 if s in depth else 0 for s in range(1 << bits))
    if max(depth.values()) > MAX_LEN:
        return bytes(bits if s in depth else 0 for s in range(1 << bits))
    return bytes(depth.get(s, 0) for s in range(1 << bits))


def normal_histogram(bits, total=20000, seed=7):
    """counts of a normal-shaped tensor quantised at `bits` on a range of +-3 sigma"""
    z = torch.randn(total, generator=torch.Generator().manual_seed(seed)).numpy()
    q = np.clip(np.rint((z + 3.0) / 6.0 * ((1 << bits) - 1)), 0, (1 << bits) - 1).astype(np.int64)
    return np.bincount(q, minlength=1 << bits).tolist()


GEOMETRIC_HIST = [1] + [1 << k for k in range(15)]                  # 1, 1, 2, 4, ..., 2^14 at 4 bits: Huffman depth 15


# ---- inputs of the GPU tests
_INPUTS = {}


def make_input(shape):
    """a seeded normal logical NCHW tensor with max > min"""
    shape = tuple(shape)
    if shape not in _INPUTS:
        z = torch.randn(*shape, generator=torch.Generator().manual_seed(31 + sum(shape))) * 2.0 + 0.4
        assert float(z.max()) > float(z.min())
        _INPUTS[shape] = z
    return _INPUTS[shape]


def geometric_input():
    """GEOMETRIC-shaped tensor whose code under static_range [0, 15] at 4 bits is k exactly GEOMETRIC_HIST[k] times (scale
    1, zero point 0: the value k quantises to the code k).  The first quarter is in ascending order -- the first chunk holds
    every rare (long) code, later ones a single short code -- and the rest is shuffled."""
    if 'geometric' not in _INPUTS:
        codes = np.repeat(np.arange(16), GEOMETRIC_HIST)
        half = codes.size // 4
        perm = torch.randperm(codes.size - half, generator=torch.Generator().manual_seed(5)).numpy()
        codes[half:] = codes[half:][perm]
        _INPUTS['geometric'] = torch.from_numpy(codes.astype(np.float32)).view(*GEOMETRIC)
    return _INPUTS['geometric']


def logical_codes(q, c):
    """flat logical NCHW codes (numpy uint8) of the one-value-per-byte NHWC tensor q"""
    return q.cpu()[..., :c].permute(0, 3, 1, 2).contiguous().view(-1).numpy()
