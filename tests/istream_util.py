"""Shared by the tests of include/hnd_istream.h (tests/test_istream_cpu.py, tests/test_istream_gpu.py,
tests/test_guard_bands_istream_gpu.py): the case table, the inputs (tests/qimage_util.make_input: every image has a range of
its own; plus a batch of special images), the per-image arithmetic of the format, and a restatement of the DEVICE table
builder -- ranks, the place of every leaf in every level, the walk back; no symbol sets -- which tests/test_istream_cpu.py
holds to transformer.huffman_lengths byte for byte.

A plain module: no fixtures, no pytest settings; importing it loads neither the library nor the launch helpers."""
import bisect

import numpy as np
import torch

from tests import entropy_util as EU
from tests import qimage_util as QI

MAX_N = 65535
LEVELS = EU.MAX_LEN                 # 12 levels of package-merge: the longest code

# (logical NCHW shape, pixel stride): the smallest shapes at which each mechanism can go wrong
SHAPES_ALL_WIDTHS = [((1, 3, 5, 7), 4),          # one short chunk; the n = 1 anchor
                     ((3, 3, 5, 7), 4)]          # h * w * cs = 140: images 1 and 2 start off the 16-byte grid
SHAPES_THREE_WIDTHS = [((4, 1, 16, 16), 4),      # exactly one chunk per image, c = 1
                       ((2, 3, 16, 16), 4),      # exactly three chunks
                       ((2, 5, 9, 31), 8),       # cs = 8, a short last chunk in every image
                       ((2, 3, 47, 45), 4),      # hw = 2115: two decode tiles, the second of 67 pixels
                       ((2, 17, 3, 5), 20)]      # two decode channel groups
ALL_WIDTHS, THREE_WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8), (2, 4, 8)
SPECIAL = ((4, 3, 32, 32), 4)                    # a live image, a constant one, a two-level one, a skewed one
CASES = [(shape, cs, bits) for shape, cs in SHAPES_ALL_WIDTHS for bits in ALL_WIDTHS] + \
        [(shape, cs, bits) for shape, cs in SHAPES_THREE_WIDTHS for bits in THREE_WIDTHS] + \
        [(SPECIAL[0], SPECIAL[1], bits) for bits in THREE_WIDTHS]
CASE_IDS = ['%s-cs%d-b%d' % ('x'.join(map(str, s)), cs, b) for s, cs, b in CASES]
GUARD_CASES = [((3, 3, 5, 7), 4, 3), ((2, 5, 9, 31), 8, 8), ((2, 17, 3, 5), 20, 4)]

# the skewed image: the value k occurs SKEWED_COUNTS[k] times and the value 255 fills the rest, so on its own range [0, 255]
# at 8 bits (scale 1, zero point 0) the code k occurs that often: Fibonacci counts, an unconstrained Huffman tree deeper than 12
SKEWED_COUNTS = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987]


def chunks_per_image(chw):
    return EU.chunks(chw)


def capacity(n, chw):
    return n * EU.capacity(chw) if 1 <= n <= MAX_N and 0 < n * chw <= 1 << 30 else 0


def scratch_bytes(n, chw):
    return 4 * n * EU.chunks(chw) if 1 <= n <= MAX_N and 0 < n * chw <= 1 << 30 else 0


def image_link_bytes(nbytes, chw, bits):
    """one image's message: its stream, its cpi + 1 offsets, its table, scale and zero point"""
    return nbytes + 4 * (chunks_per_image(chw) + 1) + (1 << bits) + 8


def skewed_histogram():
    """the 8-bit histogram of the skewed image of the special batch"""
    hist = [0] * 256
    hist[:len(SKEWED_COUNTS)] = SKEWED_COUNTS
    hist[255] = SPECIAL[0][1] * SPECIAL[0][2] * SPECIAL[0][3] - sum(SKEWED_COUNTS)
    assert hist[255] > 0
    return hist


_INPUTS = {}


def make_input(shape):
    """qimage_util.make_input; for the special shape, image 1 is a constant, image 2 has two levels and image 3 is the
    skewed one (shuffled, so every chunk holds long and short codes)"""
    key = tuple(shape)
    if key not in _INPUTS:
        z = QI.make_input(key).clone()
        if key == SPECIAL[0]:
            g = torch.Generator().manual_seed(11)
            z[1] = -2.5
            z[2] = torch.where(torch.rand(key[1:], generator=g) < 0.3, torch.tensor(1.5), torch.tensor(-0.25))
            values = np.repeat(np.arange(256), skewed_histogram()).astype(np.float32)
            z[3] = torch.from_numpy(values)[torch.randperm(values.size, generator=g)].view(key[1:])
        _INPUTS[key] = z
    return _INPUTS[key]


def image_symbols(q, c):
    """per image, the flat logical symbols (numpy uint8) of the one-value-per-byte NHWC codes q (a CPU tensor or an array)"""
    q = np.asarray(q)
    return [q[i, :, :, :c].transpose(2, 0, 1).reshape(-1) for i in range(q.shape[0])]


def device_lengths(hist, bits):
    """The table builder of include/hnd_istream.h as the kernel does it.  The occurring symbols ranked by (count, symbol) are
    the leaves and level 1; level j + 1 merges the leaves with the pairs of level j (an odd last item dropped), a leaf before
    a package of equal weight, every item placed by a binary search in the other list; only the weights and `place[j][r]`,
    where leaf r stands in level j + 1, are kept.  Walk back from the last level with k = 2 m - 2: a of the first k items are
    leaves (ranks < a grow by one bit), the other k - a are packages: the first 2 (k - a) items of the level below."""
    nsym = 1 << bits
    counts = [int(v) for v in hist][:nsym]
    leaves = sorted((w, s) for s, w in enumerate(counts) if w)
    m = len(leaves)
    out = [0] * nsym
    if m == 1:
        out[leaves[0][1]] = 1
    if m < 2:
        return bytes(out)
    leaf = [w for w, _ in leaves]
    items, place = list(leaf), [list(range(m))]
    for _ in range(LEVELS - 1):
        pack = [items[2 * i] + items[2 * i + 1] for i in range(len(items) // 2)]
        merged = [None] * (m + len(pack))
        at = [r + bisect.bisect_left(pack, leaf[r]) for r in range(m)]          # packages lighter than the leaf come first
        for r in range(m):
            merged[at[r]] = leaf[r]
        for b, w in enumerate(pack):
            merged[b + bisect.bisect_right(leaf, w)] = w                        # leaves no heavier than the package come first
        assert None not in merged and merged == sorted(merged) and max(merged) < 1 << 63
        place.append(at)
        items = merged
    length, k = [0] * m, min(2 * m - 2, len(items))
    for j in range(LEVELS - 1, -1, -1):
        a = bisect.bisect_left(place[j], k)
        for r in range(a):
            length[r] += 1
        k = 2 * (k - a)
    for r, (_, s) in enumerate(leaves):
        out[s] = length[r]
    return bytes(out)
