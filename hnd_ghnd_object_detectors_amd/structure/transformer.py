"""Bottleneck transformers (mirror of the reference's src/structure/transformer.py:131-174).

The reference applies them ONLY at evaluation time with ``-transform_bottleneck`` (src/models/mimic/base.py:54-57;
mimic_runner.py:90 disables them while distilling).  ``Quantizer`` / ``Dequantizer`` run as fused HIP kernels
(global min/max -> affine quantise to 1 ... 8 bits, one value per byte as in the reference or bit-packed as the link
payload, include/hnd_codec.h, or entropy-coded in chunks, include/hnd_entropy.h; dequantise) on the NHWC bottleneck buffer;
the 16-bit variants are a half round trip.  ``per_image=True`` (an extension, include/hnd_qimage.h) gives every image of a
batch a scale and a zero point of its own; ``ImageStreamQuantizer`` (an extension, include/hnd_istream.h) adds an
entropy-coded stream and a device-built code table per image.  ``per_channel=True`` (an extension, include/hnd_qchannel.h) gives every channel
of the bottleneck a scale and a zero point of its own, in the plain, the packed and the fake quantiser.
``FakeQuantizer`` (an extension) is the pair as one call (include/hnd_qat.h) -- the launch the TRAINING step runs on the
bottleneck tensor when ``train.fake_quantize`` is set (engine.HeadEngine.forward).
``JpegCompressor`` / ``JpegDecompressor`` (:94-128: the uint8 bottleneck image through a JPEG file)
and ``DataLogger`` (:58-91: pickled sizes of the bottleneck for the reference's cost analysis) are host-side file /
bookkeeping utilities: the quantisation they contain runs on the same HIP kernel, the rest is PIL / pickle as in the
reference.

Input pipeline (reference :32-55): ``ToTensor`` keeps the decoded uint8 image as a
``DecodedImage`` instead of materialising a float CHW copy on the host, ``RandomHorizontalFlip`` only flips the
(tiny) targets and marks the image; the /255, the flip and the model's normalise/resize/pad then run as ONE HIP
kernel inside ``CustomRCNNTransform`` (hnd_transform_image_u8): 4x fewer host->device bytes, no host float work.
"""
import math
import os
import random

import numpy as np
import torch

from .. import ops
from ..hipnn import attach, to_nhwc


class Compose(object):
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, image, target):
        for t in self.transforms:
            image, target = t(image, target)
        return image, target


class DecodedImage(object):
    """A decoded image waiting for the device: uint8 [H, W, 3] (``hwc``) or [3, H, W], plus a pending horizontal
    flip.  Quacks like the float CHW tensor the reference's dataset yields where the host looks at it
    (``.shape``, ``.to(device)``, ``.device``); the float values only ever exist inside the transform kernel."""

    def __init__(self, data, hwc, flip=False):
        assert data.dtype == torch.uint8 and data.dim() == 3 and data.shape[2 if hwc else 0] == 3
        self.data, self.hwc, self.flip = data, hwc, flip

    @property
    def shape(self):
        d = self.data.shape
        return torch.Size((3, d[0], d[1]) if self.hwc else tuple(d))

    @property
    def device(self):
        return self.data.device

    @property
    def is_cuda(self):
        return self.data.is_cuda

    def dim(self):
        return 3

    def to(self, *args, **kwargs):
        kwargs = {k: v for k, v in kwargs.items() if k != 'dtype'}
        args = tuple(a for a in args if not isinstance(a, torch.dtype))
        return DecodedImage(self.data.to(*args, **kwargs), self.hwc, self.flip)

    def pin_memory(self, *args, **kwargs):
        """DataLoader(pin_memory=True) calls this on batch elements that have it"""
        return DecodedImage(self.data.pin_memory(*args, **kwargs), self.hwc, self.flip)

    def float_chw(self):
        """What the reference's ToTensor (+ flip) would have produced -- for checks, not used by the product path."""
        x = self.data.permute(2, 0, 1) if self.hwc else self.data
        x = x.float() / 255
        return x.flip(-1) if self.flip else x


def flip_coco_person_keypoints(kps, width):
    """COCO left/right joint swap + x mirror, zeroing invisible joints (reference :12-20)."""
    order = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
    out = kps[:, order]
    out[..., 0] = width - out[..., 0]
    out[out[..., 2] == 0] = 0
    return out


class RandomHorizontalFlip(object):
    """reference :32-49.  A DecodedImage is flipped lazily (inside the device kernel); tensors are flipped here."""

    def __init__(self, prob, rng=None):
        self.prob = prob
        self.rng = rng          # None: Python's global ``random`` like the reference; a random.Random: a stream of its own

    def __call__(self, image, target):
        if (self.rng or random).random() >= self.prob:
            return image, target
        width = image.shape[-1]
        if isinstance(image, DecodedImage):
            image = DecodedImage(image.data, image.hwc, not image.flip)
        else:
            image = image.flip(-1)
        boxes = target['boxes']
        boxes[:, [0, 2]] = width - boxes[:, [2, 0]]
        target['boxes'] = boxes
        if 'masks' in target:
            target['masks'] = target['masks'].flip(-1)
        if 'keypoints' in target:
            target['keypoints'] = flip_coco_person_keypoints(target['keypoints'], width)
        return image, target


class ToTensor(object):
    """reference :52-55 (functional.to_tensor).  With ``decoded`` (default) PIL images / uint8 arrays stay uint8
    (DecodedImage: the /255 happens inside the device transform kernel); ``decoded=False`` returns the float CHW
    tensor on the host exactly like the reference."""

    def __init__(self, decoded=True):
        self.decoded = decoded

    def __call__(self, image, target):
        image, target = self._defer(image, target)
        if not self.decoded and isinstance(image, DecodedImage):
            image = image.float_chw().contiguous()
        return image, target

    def _defer(self, image, target):
        if isinstance(image, DecodedImage) or (torch.is_tensor(image) and image.dtype != torch.uint8):
            return image, target
        if torch.is_tensor(image):          # uint8 tensor: [H, W, 3] unless it is unambiguously [3, H, W]
            return DecodedImage(image.contiguous(), hwc=image.shape[0] != 3), target
        arr = np.asarray(image)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise TypeError('ToTensor expects an RGB uint8 image, got %s %s' % (arr.dtype, arr.shape))
        return DecodedImage(torch.from_numpy(np.array(arr, order="C")), hwc=True), target       # copy: PIL memory is read-only


class DataLogger(object):
    """reference :58-91: records, per call, the pickled size (KB) of the bottleneck tensor as it is, as int16
    (``z.short()``, the reference's "fp16" figure) and quantised to ``num_bits``, plus its C / H / W; passes z through.
    A bottleneck transformer for analysis runs (``models.get_model(..., bottleneck_transformer=DataLogger())``)."""

    def __init__(self, num_bits=8):
        self.num_bits4quant = num_bits
        self.data_size_list, self.fp16_data_size_list = [], []
        self.quantized_data_size_list, self.tensor_shape_list = [], []

    def get_data(self):
        return (self.data_size_list.copy(), self.fp16_data_size_list, self.quantized_data_size_list.copy(),
                self.tensor_shape_list.copy())

    def clear(self):
        for lst in (self.data_size_list, self.fp16_data_size_list, self.quantized_data_size_list,
                    self.tensor_shape_list):
            lst.clear()

    def __call__(self, z, target):
        from ..myutils.common import file_util
        if z is None:
            sizes = (0.0, 0.0, 0.0)
        elif not isinstance(z, torch.Tensor):
            sizes = (file_util.get_binary_object_size(z), None, None)
        else:
            plain = z.detach().cpu().contiguous()               # logical NCHW values, as the reference pickles them
            # 1 ... 8 bits: the real quantiser, whose uint8 tensor the reference pickles at any of these widths
            qz, _ = Quantizer(self.num_bits4quant)(z, None) if self.num_bits4quant in range(1, 9) else (plain.half(), None)
            if isinstance(qz, QuantizedTensor):                  # what crosses the link: uint8 tensor + scale + zero point
                qz = _HostQuantized(qz.tensor.cpu().contiguous(), float(qz.scale), int(qz.zero_point))
            sizes = (file_util.get_binary_object_size(plain), file_util.get_binary_object_size(plain.short()),
                     file_util.get_binary_object_size(qz))
        self.data_size_list.append(sizes[0])
        self.fp16_data_size_list.append(sizes[1])
        self.quantized_data_size_list.append(sizes[2])
        self.tensor_shape_list.append([0, 0, 0] if z is None else [z.shape[1], z.shape[2], z.shape[3]])
        return z, target


class _HostQuantized(object):
    """host copy of a quantised bottleneck (uint8 tensor, python scale / zero point): what myutils' QuantizedTensor
    pickles to"""

    def __init__(self, tensor, scale, zero_point):
        self.tensor, self.scale, self.zero_point = tensor, scale, zero_point


class JpegCompressor(object):
    """reference :94-114: a 3-channel bottleneck ([3, H, W] or [1, 3, H, W]) is quantised to uint8 (HIP kernel),
    written as a JPEG file and replaced by ``(file path, quantised tensor)``; anything else passes through"""

    def __init__(self, jpeg_quality=95, tmp_dir_path='./tmp/', per_channel=False, per_image=False):
        if _check_per_channel('JpegCompressor', per_channel):
            raise ValueError('JpegCompressor(per_channel=True): the JPEG file carries one scale and zero point; per-channel '
                             'scales are built for Quantizer / FakeQuantizer at 1 ... 8 bits only')
        if _check_per_image('JpegCompressor', per_image):
            raise ValueError('JpegCompressor(per_image=True): a JPEG file is one image with one scale and zero point already; '
                             'per-image scales are built for Quantizer / FakeQuantizer at 1 ... 8 bits only')
        self.jpeg_quality, self.tmp_dir_path = jpeg_quality, tmp_dir_path
        os.makedirs(tmp_dir_path, exist_ok=True)
        self._quantizer = Quantizer(8)

    def save_image(self, z, output_file_path):
        from PIL import Image
        qz, _ = self._quantizer(z if z.dim() == 4 else z.unsqueeze(0), None)
        hwc = qz.tensor[0].permute(1, 2, 0).cpu().numpy()
        Image.fromarray(np.ascontiguousarray(hwc)).save(output_file_path, format='jpeg', quality=self.jpeg_quality)
        return qz

    def __call__(self, z, target):
        if isinstance(z, torch.Tensor) and ((z.dim() == 3 and z.shape[0] == 3) or
                                            (z.dim() == 4 and z.shape[0] == 1 and z.shape[1] == 3)):
            file_path = os.path.join(self.tmp_dir_path, '{}.jpg'.format(hash(z)))
            return (file_path, self.save_image(z, file_path)), target
        return z, target


class JpegDecompressor(object):
    """reference :117-128: ``(file path, quantised tensor)`` -> decoded RGB * 255 de-quantised with the stored scale /
    zero point: ``scale * (pixel - zero_point)``, as [1, 3, H, W] (target_dim 4) or [3, H, W], on the device the
    quantised tensor lives on"""

    def __init__(self, tmp_dir_path='./tmp/', target_dim=4):
        self.tmp_dir_path, self.target_dim = tmp_dir_path, target_dim

    def __call__(self, z, target):
        if isinstance(z, tuple) and isinstance(z[0], str):
            from PIL import Image
            qz = z[1]
            arr = np.array(Image.open(z[0]).convert("RGB"), dtype=np.uint8)          # a writable copy
            pix = torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1).float().div(255).to(qz.tensor.device)
            img = qz.scale * (pix * 255.0 - qz.zero_point)      # functional.to_tensor(img) * 255.0 in the reference
            return (img if self.target_dim != 4 else img.unsqueeze(0)), target
        return z, target


class QuantizedTensor(object):
    """myutils tensor_util.QuantizedTensor: .tensor (uint8, logical NCHW), .scale, .zero_point.  scale / zero_point
    are 0-dim DEVICE tensors (views of the kernel's qparams) so no host sync is forced; int()/float() work.
    ``per_channel`` (an extension, include/hnd_qchannel.h): qparams is [c, 4], scale / zero_point are its 1-D views
    qparams[:, 2] / qparams[:, 3], and ``num_bits`` is the width it was quantised at.  ``per_image`` (an extension,
    include/hnd_qimage.h): the same with one row of qparams per image, [n, 4]."""

    def __init__(self, tensor, scale, zero_point, qparams=None, origin=None, channels=None, per_channel=False,
                 num_bits=None, per_image=False):
        self.tensor, self.scale, self.zero_point = tensor, scale, zero_point
        self.qparams, self.origin, self.channels = qparams, origin, channels
        self.per_channel, self.per_image, self.num_bits = bool(per_channel), bool(per_image), num_bits


class PackedBottleneck(object):
    """The quantised bottleneck as it crosses the link (``Quantizer(num_bits, packed=True)``): ``payload`` is a 1-D uint8
    device tensor of exactly ceil(numel * num_bits / 8) bytes holding the values of the logical NCHW tensor ``shape``
    back to back, ``num_bits`` each, least significant bit first (format: include/hnd_codec.h); ``scale`` /
    ``zero_point`` are 0-dim device views of ``qparams`` as in QuantizedTensor.  An extension: the reference ships the
    one-value-per-byte tensor whatever the width.  ``per_channel`` (include/hnd_qchannel.h): the same payload format beside a
    ``qparams`` of shape [c, 4]; ``scale`` / ``zero_point`` are its 1-D views qparams[:, 2] / qparams[:, 3].  ``per_image``
    (include/hnd_qimage.h): the same payload format beside a ``qparams`` of shape [n, 4], one row per image."""

    def __init__(self, payload, shape, num_bits, qparams, origin=None, per_channel=False, per_image=False):
        self.payload, self.shape, self.num_bits = payload, tuple(int(s) for s in shape), num_bits
        self.qparams, self.origin, self.per_channel, self.per_image = qparams, origin, bool(per_channel), bool(per_image)
        if self.per_channel and self.per_image:
            raise ValueError('PackedBottleneck(per_channel=True, per_image=True): the qparams are per channel or per image')
        rows = self.per_channel or self.per_image
        self.scale, self.zero_point = (qparams[:, 2], qparams[:, 3]) if rows else (qparams[2], qparams[3])

    @property
    def nbytes(self):
        return self.payload.numel()

    @property
    def link_bytes(self):
        """everything that crosses the link: the payload and one (scale, zero point) per tensor, per channel or per image"""
        return self.nbytes + 8 * (self.shape[1] if self.per_channel else self.shape[0] if self.per_image else 1)


MAX_CODE_LEN = 12          # longest code of include/hnd_entropy.h


def check_code_lengths(who, lengths, num_bits, complete=False):
    """the table of include/hnd_entropy.h as bytes: 2^num_bits lengths in 0 ... 12, at least one non-zero, Kraft sum <= 1;
    ``complete``: every length non-zero (a fixed table must be able to code any tensor).  Anything else is refused by name."""
    try:
        table = [int(v) for v in lengths]
        ok = all(float(v) == int(v) and not isinstance(v, bool) for v in lengths)
    except (TypeError, ValueError):
        table, ok = [], False
    if not ok or len(table) != 1 << num_bits:
        raise ValueError('%s: code_lengths must be %d integers (one per code of %d bits)' % (who, 1 << num_bits, num_bits))
    if any(not 0 <= v <= MAX_CODE_LEN for v in table):
        raise ValueError('%s: code_lengths outside 0 ... %d' % (who, MAX_CODE_LEN))
    if complete and not all(table):
        raise ValueError('%s: a fixed table of code_lengths must be complete: every one of the %d lengths non-zero'
                         % (who, 1 << num_bits))
    if not any(table):
        raise ValueError('%s: code_lengths has no non-zero length' % who)
    if sum(1 << (MAX_CODE_LEN - v) for v in table if v) > 1 << MAX_CODE_LEN:
        raise ValueError('%s: code_lengths has a Kraft sum above 1: no prefix code has these lengths' % who)
    return bytes(table)


def huffman_lengths(hist, num_bits, max_len=MAX_CODE_LEN):
    """Code lengths (bytes, 2^num_bits of them) of an optimal prefix code of the histogram ``hist`` whose longest code is
    ``max_len`` bits -- the ``lengths`` of include/hnd_entropy.h.  Deterministic host code.

    Method: package-merge (Larmore & Hirschberg 1990).  The occurring symbols, sorted by (count, symbol), are the leaves.
    Starting from the leaves, max_len - 1 times: pair the current list's items in order (an odd last item is dropped) and
    merge the pairs ("packages") with the leaves, by weight, a leaf before a package of equal weight.  The first 2 m - 2
    items of the final list are taken (m = occurring symbols) and a symbol's length is the number of taken items that contain
    it.  The result is an optimal code under the length limit, so its Kraft sum is exactly 1 for m >= 2, its cost
    sum(hist * len) never exceeds the flat code's num_bits * sum(hist) (the flat code is one of the candidates), and it
    equals the unconstrained Huffman cost wherever that tree is no deeper than max_len.  Absent symbols get 0; a single
    occurring symbol gets 1.  Should the cost ever exceed the flat code's, the flat code (num_bits for every occurring
    symbol) is returned instead."""
    nsym = 1 << num_bits
    counts = [int(v) for v in hist][:nsym]
    if len(counts) != nsym or any(v < 0 for v in counts) or any(int(v) for v in list(hist)[nsym:]):
        raise ValueError('huffman_lengths: hist must hold a count >= 0 for each of the %d codes and 0 beyond them' % nsym)
    if not num_bits <= max_len <= MAX_CODE_LEN:
        raise ValueError('huffman_lengths: max_len=%r outside %d ... %d' % (max_len, num_bits, MAX_CODE_LEN))
    leaves = sorted((counts[s], s) for s in range(nsym) if counts[s])
    if not leaves:
        raise ValueError('huffman_lengths: an empty histogram')
    lengths = [0] * nsym
    if len(leaves) == 1:
        lengths[leaves[0][1]] = 1
        return bytes(lengths)
    leaf_items = [(w, (s,)) for w, s in leaves]                  # (weight, the symbols it contains, with multiplicity)
    items = leaf_items
    for _ in range(max_len - 1):
        packages = [(items[i][0] + items[i + 1][0], items[i][1] + items[i + 1][1]) for i in range(0, len(items) - 1, 2)]
        merged, a, b = [], 0, 0
        while a < len(leaf_items) or b < len(packages):
            if b == len(packages) or (a < len(leaf_items) and leaf_items[a][0] <= packages[b][0]):
                merged.append(leaf_items[a])
                a += 1
            else:
                merged.append(packages[b])
                b += 1
        items = merged
    for _, symbols in items[:2 * len(leaves) - 2]:
        for s in symbols:
            lengths[s] += 1
    if sum(c * l for c, l in zip(counts, lengths)) > num_bits * sum(counts):
        lengths = [num_bits if c else 0 for c in counts]
    return bytes(lengths)


class EntropyBottleneck(object):
    """The quantised bottleneck as an entropy-coded stream (``Quantizer(num_bits, entropy=True)``; format:
    include/hnd_entropy.h): ``payload`` is a 1-D uint8 device tensor of the stream's CAPACITY of which the first ``nbytes``
    are the stream, ``offsets`` an int32 device tensor of chunks + 1 byte offsets, ``lengths`` the host ``bytes`` of the
    2^num_bits code lengths; ``scale`` / ``zero_point`` are 0-dim device views of ``qparams`` as in QuantizedTensor."""

    def __init__(self, payload, offsets, lengths, shape, num_bits, qparams, origin=None):
        self.payload, self.offsets, self.lengths = payload, offsets, bytes(lengths)
        self.shape, self.num_bits = tuple(int(s) for s in shape), num_bits
        self.qparams, self.scale, self.zero_point, self.origin = qparams, qparams[2], qparams[3], origin
        self._nbytes = None

    @property
    def nbytes(self):
        """bytes of the stream: offsets[chunks], one small device read, cached"""
        if self._nbytes is None:
            self._nbytes = int(self.offsets[-1].item()) & 0xFFFFFFFF
        return self._nbytes

    @property
    def link_bytes(self):
        """everything that crosses the link: the stream, the offsets, the table of lengths, scale and zero point"""
        return self.nbytes + 4 * self.offsets.numel() + (1 << self.num_bits) + 8


class ImageStreamBottleneck(object):
    """The quantised bottleneck as one self-contained entropy stream PER IMAGE (``ImageStreamQuantizer``; format:
    include/hnd_istream.h): ``payload`` is a 1-D uint8 device tensor of the streams' CAPACITY of which the first ``nbytes``
    are the images' streams back to back, ``offsets`` an int32 device tensor of n * chunks_per_image + 1 byte offsets,
    ``lengths`` a DEVICE uint8 tensor [n, 256] (row i: the code lengths of image i), ``qparams`` [n, 4] as
    include/hnd_qimage.h writes it; ``scale`` / ``zero_point`` are its [n] views.  ``image(i)`` cuts image i's message out
    as an ordinary EntropyBottleneck."""

    def __init__(self, payload, offsets, lengths, shape, num_bits, qparams, origin=None):
        self.payload, self.offsets, self.lengths = payload, offsets, lengths
        self.shape, self.num_bits = tuple(int(s) for s in shape), num_bits
        self.qparams, self.scale, self.zero_point, self.origin = qparams, qparams[:, 2], qparams[:, 3], origin
        self.chunks_per_image = -(-(self.shape[1] * self.shape[2] * self.shape[3]) // 256)
        self._bounds = None

    def _image_bounds(self):
        """where every image's stream begins, and the end of the last: offsets[::chunks_per_image], one small device read,
        cached"""
        if self._bounds is None:
            self._bounds = [int(v) & 0xFFFFFFFF for v in self.offsets[::self.chunks_per_image].cpu().tolist()]
        return self._bounds

    @property
    def nbytes(self):
        """bytes of all streams: offsets[n * chunks_per_image]"""
        return self._image_bounds()[-1]

    @property
    def image_nbytes(self):
        """bytes of every image's stream"""
        b = self._image_bounds()
        return [hi - lo for lo, hi in zip(b[:-1], b[1:])]

    @property
    def image_link_bytes(self):
        """per image, everything of it that crosses the link: its stream, its chunks_per_image + 1 offsets, its table of
        lengths, its scale and zero point"""
        return [v + 4 * (self.chunks_per_image + 1) + (1 << self.num_bits) + 8 for v in self.image_nbytes]

    @property
    def link_bytes(self):
        return sum(self.image_link_bytes)

    def image(self, i):
        """image i's link message as an EntropyBottleneck of shape [1, c, h, w] that shares nothing with this object: a copy
        of its stream in a buffer of its own (so 16-byte aligned wherever the stream began), its offsets rebased to 0, its
        code lengths as host bytes and a copy of qparams[i].  The per-tensor Dequantizer takes it as it is."""
        n, c, h, w = self.shape
        if isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < n:
            raise IndexError('ImageStreamBottleneck.image(%r): the batch holds images 0 ... %d' % (i, n - 1))
        bounds, cpi = self._image_bounds(), self.chunks_per_image
        lo, hi = bounds[i], bounds[i + 1]
        payload = self.payload.new_zeros(max(hi - lo, 1))          # an image whose table is all zero has no bytes
        payload[:hi - lo] = self.payload[lo:hi]
        offsets = self.offsets[i * cpi:(i + 1) * cpi + 1] - (lo - (1 << 32) if lo >= 1 << 31 else lo)     # int32 wraps
        lengths = bytes(self.lengths[i, :1 << self.num_bits].cpu().tolist())
        return EntropyBottleneck(payload, offsets.contiguous(), lengths, (1, c, h, w), self.num_bits, self.qparams[i].clone())


SUPPORTED_BITS = tuple(range(1, 9)) + (16,)


def _check_bits(who, num_bits, packed=False):
    if isinstance(num_bits, bool) or num_bits not in SUPPORTED_BITS or (packed and num_bits == 16):
        raise NotImplementedError('%s(num_bits=%r%s): the HIP bottleneck codec implements num_bits in %s%s' % (
            who, num_bits, ', packed=True' if packed else '', list(SUPPORTED_BITS),
            ' and packs 1 ... 8 bits only (16 is a half round trip, nothing to pack)' if packed else ''))


def _check_per_channel(who, per_channel):
    """``per_channel`` of Quantizer / FakeQuantizer / JpegCompressor: a bool, anything else is refused by name"""
    if not isinstance(per_channel, bool):
        raise ValueError('%s: per_channel=%r must be a bool' % (who, per_channel))
    return per_channel


def _check_per_channel_combination(who, num_bits, static_range, entropy=False):
    """per-channel scales (include/hnd_qchannel.h) exist for the per-batch range at 1 ... 8 bits, plain, packed and fake
    quantised; every other combination is refused by name"""
    if entropy:
        raise ValueError('%s(per_channel=True, entropy=True): the entropy coder has no per-channel form' % who)
    if static_range is not None:
        raise ValueError('%s(per_channel=True, static_range=%r): a fixed range has no per-channel form (per-channel scales '
                         'come from the min / max of the tensor in front of the call)' % (who, static_range))
    if num_bits == 16:
        raise ValueError('%s(num_bits=16, per_channel=True): per-channel scales need a width of 1 ... 8 bits (16 is a half '
                         'round trip, no scale)' % who)


def _check_per_image(who, per_image):
    """``per_image`` of Quantizer / FakeQuantizer / JpegCompressor: a bool, anything else is refused by name"""
    if not isinstance(per_image, bool):
        raise ValueError('%s: per_image=%r must be a bool' % (who, per_image))
    return per_image


def _check_per_image_combination(who, num_bits, static_range, entropy=False, per_channel=False):
    """per-image scales (include/hnd_qimage.h) exist for the per-batch range at 1 ... 8 bits, plain, packed and fake
    quantised; every other combination is refused by name"""
    if per_channel:
        raise ValueError('%s(per_image=True, per_channel=True): the scales are per image or per channel, the combination is '
                         'not built' % who)
    if entropy:
        raise ValueError('%s(per_image=True, entropy=True): the entropy coder has no per-image form' % who)
    if static_range is not None:
        raise ValueError('%s(per_image=True, static_range=%r): a fixed range has no per-image form (per-image scales come '
                         'from the min / max of each image in front of the call)' % (who, static_range))
    if num_bits == 16:
        raise ValueError('%s(num_bits=16, per_image=True): per-image scales need a width of 1 ... 8 bits (16 is a half '
                         'round trip, no scale)' % who)


class _StaticRange(object):
    """``static_range`` of Quantizer / FakeQuantizer (include/hnd_qrange.h): None (min / max of the tensor in front of the
    call, three launches), a pair ``[lo, hi]`` (a fixed range: hnd_qrange_qparams runs once per pair and device, and every
    call is then ONE launch), or ``'trained'``: the pair comes from the range a student was distilled with -- resolved by
    ``models.load_ckpt(path, model=student)`` from the checkpoint's ``bottleneck_range`` or by ``mimic_runner.distill``
    from the live state; calling the quantiser before that raises."""

    def _init_static_range(self, static_range):
        who = type(self).__name__
        self._static, self._trained, self._static_qparams = None, False, {}
        if static_range is None:
            return
        if self.num_bits == 16:
            raise ValueError('%s(num_bits=16, static_range=%r): a fixed range needs a width of 1 ... 8 bits (16 is a half '
                             'round trip, no range)' % (who, static_range))
        if isinstance(static_range, str):
            if static_range != 'trained':
                raise ValueError('%s: static_range=%r must be [lo, hi] or \'trained\'' % (who, static_range))
            self._trained = True
            return
        if not isinstance(static_range, (list, tuple)) or len(static_range) != 2:
            raise ValueError('%s: static_range=%r must be [lo, hi] or \'trained\'' % (who, static_range))
        self.set_static_range(*static_range)

    @property
    def static_range(self):
        """None, the pair (lo, hi) in use, or 'trained' while that is unresolved"""
        return self._static if self._static is not None else ('trained' if self._trained else None)

    def set_static_range(self, lo, hi):
        who = type(self).__name__
        if self.num_bits == 16:
            raise ValueError('%s(num_bits=16).set_static_range: a fixed range needs a width of 1 ... 8 bits' % who)
        ok = all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in (lo, hi))
        if not ok or not float(lo) < float(hi):
            raise ValueError('%s: static_range needs finite lo < hi, got [%r, %r]' % (who, lo, hi))
        self._static, self._static_qparams = (float(lo), float(hi)), {}

    def resolve_trained_range(self, info):
        """info: the ``bottleneck_range`` dict of a checkpoint ({'min', 'max', 'steps', 'num_bits', 'momentum'}); a no-op
        unless static_range is 'trained'"""
        who = type(self).__name__
        if not self._trained:
            return False
        if not isinstance(info, dict) or not all(k in info for k in ('min', 'max', 'num_bits')):
            raise ValueError('%s(static_range=\'trained\'): no bottleneck_range to resolve it from (the student was not '
                             'distilled with train.fake_quantize.range: ema)' % who)
        if int(info['num_bits']) != self.num_bits:
            raise ValueError('%s(num_bits=%d, static_range=\'trained\'): the range was trained at %d bits'
                             % (who, self.num_bits, int(info['num_bits'])))
        if info.get('steps', 1) <= 0:
            raise ValueError('%s(static_range=\'trained\'): the trained range has observed no batch yet' % who)
        self.set_static_range(float(info['min']), float(info['max']))
        return True

    def _check_resolved(self):
        if self._static is None and self._trained:
            raise RuntimeError('%s(static_range=\'trained\') was called before its range was resolved: load the student '
                               'with load_ckpt(path, model=student) or run it under distill()' % type(self).__name__)

    def _static_qparams_on(self, device):
        """None when no static range is configured; else the device qparams of the pair (one launch per pair and device)"""
        self._check_resolved()
        if self._static is None:
            return None
        if device not in self._static_qparams:
            qp = torch.empty(4, dtype=torch.float32, device=device)
            ops.qrange_qparams(self._static[0], self._static[1], self.num_bits, qp)
            self._static_qparams[device] = qp
        return self._static_qparams[device]


class _PerChannelKeyword(type):
    """``Quantizer(..., per_channel=..., per_image=...)``: the keywords are taken off the call here and handed to
    ``_init_per_channel`` / ``_init_per_image`` once ``__init__`` has run, so ``Quantizer.__init__`` keeps the parameter list
    it has had since the entropy coder (callers and tools that read it by ``inspect.signature`` see no change)"""

    def __call__(cls, *args, per_channel=False, per_image=False, **kwargs):
        self = super().__call__(*args, **kwargs)
        self._init_per_channel(per_channel)
        self._init_per_image(per_image)
        return self


class Quantizer(_StaticRange, metaclass=_PerChannelKeyword):
    """reference :131-140 at any width the reference's uint8 tensor can hold: 1 ... 8 bits (qmax = 2^num_bits - 1), or
    16 (half round trip).  ``packed=True`` returns the bit-packed link payload (PackedBottleneck) instead of the
    one-value-per-byte QuantizedTensor.  ``static_range``: see _StaticRange (an extension).  ``entropy=True`` (an extension,
    1 ... 8 bits, not with ``packed``) runs the same quantise path and then entropy-codes its bytes (EntropyBottleneck,
    include/hnd_entropy.h): a histogram launch, one 1 KB read-back (the table depends on the data), huffman_lengths on the
    host and the encoder's three launches.  ``code_lengths`` (with ``entropy``) fixes the table instead -- all 2^num_bits
    lengths non-zero -- and the call then has neither the histogram nor the read-back.  ``per_channel=True`` (an extension,
    1 ... 8 bits, plain or ``packed``; not with ``entropy`` or ``static_range``): min / max, scale and zero point per channel
    (include/hnd_qchannel.h); the result carries ``per_channel=True`` and a ``qparams`` of shape [c, 4].  ``per_image=True``
    (an extension, 1 ... 8 bits, plain or ``packed``; not with ``per_channel``, ``entropy`` or ``static_range``): min / max,
    scale and zero point per IMAGE of the batch (include/hnd_qimage.h), so image i gets the codes ``Quantizer(num_bits)``
    gives z[i:i+1] alone; the result carries ``per_image=True`` and a ``qparams`` of shape [n, 4].  The range of an image
    runs over its whole [c, h, w] slice of the batch tensor, padding included."""

    def __init__(self, num_bits=8, packed=False, static_range=None, entropy=False, code_lengths=None):
        _check_bits('Quantizer', num_bits, packed)
        self.num_bits, self.packed, self.entropy = num_bits, bool(packed), bool(entropy)
        self.per_channel = False            # (the keyword: _PerChannelKeyword / _init_per_channel)
        self.per_image = False              # (the keyword: _PerChannelKeyword / _init_per_image)
        if self.entropy and self.packed:
            raise ValueError('Quantizer(entropy=True, packed=True): the link payload is either entropy-coded or bit-packed')
        if self.entropy and num_bits == 16:
            raise ValueError('Quantizer(num_bits=16, entropy=True): entropy coding needs a width of 1 ... 8 bits (16 is a '
                             'half round trip, no codes)')
        if code_lengths is not None and not self.entropy:
            raise ValueError('Quantizer(code_lengths=...) needs entropy=True: the table belongs to the entropy coder')
        self.code_lengths = None if code_lengths is None else \
            check_code_lengths('Quantizer(entropy=True)', code_lengths, num_bits, complete=True)
        self._bufs, self._entropy_bufs = {}, {}
        self._init_static_range(static_range)

    def _init_per_channel(self, per_channel):
        self.per_channel = _check_per_channel('Quantizer', per_channel)
        if self.per_channel:
            _check_per_channel_combination('Quantizer', self.num_bits, self.static_range, self.entropy)

    def _init_per_image(self, per_image):
        self.per_image = _check_per_image('Quantizer', per_image)
        if self.per_image:
            _check_per_image_combination('Quantizer', self.num_bits, self.static_range, self.entropy, self.per_channel)

    def _entropy_code(self, q, c, qparams, shape, origin):
        """q (uint8 NHWC, one value per byte) -> EntropyBottleneck: [histogram, one 1 KB read-back, huffman_lengths] unless
        the table is fixed, then the three launches of the encoder (include/hnd_entropy.h)"""
        key = (tuple(q.shape), c, q.device)
        if key not in self._entropy_bufs:
            numel = q.numel() // q.shape[-1] * c
            self._entropy_bufs[key] = (
                torch.empty(ops.entropy_capacity(numel), dtype=torch.uint8, device=q.device),
                torch.empty(ops.entropy_chunks(numel) + 1, dtype=torch.int32, device=q.device),
                torch.empty(ops.entropy_scratch_bytes(numel) // 4, dtype=torch.int32, device=q.device),
                torch.empty(256, dtype=torch.int32, device=q.device))
        payload, offsets, scratch, hist = self._entropy_bufs[key]
        lengths = self.code_lengths
        if lengths is None:
            ops.code_histogram(q, c, self.num_bits, hist)
            lengths = huffman_lengths(hist.cpu().tolist(), self.num_bits)
        ops.entropy_encode(q, c, self.num_bits, lengths, payload, offsets, scratch)
        return EntropyBottleneck(payload, offsets, lengths, shape, self.num_bits, qparams, origin=origin)

    def __call__(self, z, target):
        self._check_resolved()
        buf = to_nhwc(z)                    # [N, H, W, cs] fp32 bottleneck (pad channels are 0)
        c = z.shape[1]
        if self.num_bits == 16:             # z.half(): stored back as the fp32 value of the half
            ops.roundtrip_f16(buf)
            return z, target
        key = (tuple(buf.shape), c, buf.device)
        if key not in self._bufs:
            n, h, w, cs = buf.shape
            qshape = (ops.codec_packed_bytes(n * c * h * w, self.num_bits),) if self.packed else buf.shape
            self._bufs[key] = (torch.empty(qshape, dtype=torch.uint8, device=buf.device),
                               torch.empty((c, 4) if self.per_channel else (n, 4) if self.per_image else (4,),
                                           dtype=torch.float32, device=buf.device),
                               torch.empty(ops.qchannel_scratch_elems(cs) if self.per_channel else
                                           ops.qimage_scratch_elems(n) if self.per_image else
                                           ops.minmax_scratch_elems(), dtype=torch.float32, device=buf.device))
        q, qparams, scratch = self._bufs[key]
        bits, per_channel, per_image = self.num_bits, self.per_channel, self.per_image
        fixed = None if per_channel or per_image else self._static_qparams_on(buf.device)
        # per flavour: the packing call, the one-value-per-byte call (closures: their argument lists differ; one of the two
        # runs) and the qparams the result carries
        if per_channel:                     # a scale and a zero point per channel (include/hnd_qchannel.h)
            qp = qparams
            pack = lambda: ops.qchannel_quantize_pack_bits(buf, c, bits, q, qp, scratch)
            plain = lambda: ops.qchannel_quantize_bits(buf, c, bits, q, qp, scratch)
        elif per_image:                     # a scale and a zero point per image (include/hnd_qimage.h)
            qp = qparams
            pack = lambda: ops.qimage_quantize_pack_bits(buf, c, bits, q, qp, scratch)
            plain = lambda: ops.qimage_quantize_bits(buf, c, bits, q, qp, scratch)
        elif fixed is not None:             # one launch on the fixed range (include/hnd_qrange.h)
            qp = fixed
            pack = lambda: ops.quantize_pack_range_bits(buf, c, bits, q, qp)
            plain = lambda: ops.quantize_range_bits(buf, c, bits, q, qp)
        else:                               # min / max of this tensor
            qp = qparams
            pack = lambda: ops.quantize_pack_bits(buf, c, bits, q, qp, scratch)
            plain = lambda: ops.quantize_u8(buf, c, q, qp, scratch) if bits == 8 else \
                ops.quantize_bits(buf, c, bits, q, qp, scratch)
        if self.packed:
            pack()
            return PackedBottleneck(q, z.shape, bits, qp, origin=buf, per_channel=per_channel, per_image=per_image), target
        plain()
        if self.entropy:                    # never per channel or per image: the combination checks refuse the pair by name
            assert not per_channel and not per_image
            return self._entropy_code(q, c, qp, z.shape, buf), target
        qt = q[..., :c].permute(0, 3, 1, 2)
        rows = per_channel or per_image
        scale, zero_point = (qp[:, 2], qp[:, 3]) if rows else (qp[2], qp[3])
        return QuantizedTensor(attach(qt, q), scale, zero_point, qp, origin=buf, channels=c, per_channel=per_channel,
                               num_bits=bits if rows else None, per_image=per_image), target


class ImageStreamQuantizer(object):
    """Per-image scales AND an entropy-coded stream per image (an extension, include/hnd_istream.h; 1 ... 8 bits): image i of a
    batch gets the codes, the code table, the bytes and the qparams it gets alone, and ``ImageStreamBottleneck.image(i)`` is
    a message that decodes without its neighbours.  ``Quantizer(entropy=True, per_image=True)`` stays refused: this class is
    that combination.  The call is ops.qimage_quantize_bits (the launches of ``Quantizer(num_bits, per_image=True)``),
    ops.istream_histogram, ops.istream_build_tables -- the tables are made on the device, nothing is read back -- and
    ops.istream_encode; nothing in it synchronises with the host.  ``code_lengths`` fixes one complete table for every image
    instead (checked as Quantizer's; tiled to [n, 256] once per batch size and device): the call then has neither the
    histogram nor the table launch.  The buffers of a call are reused by the next call on the same shape."""

    def __init__(self, num_bits=8, code_lengths=None):
        if isinstance(num_bits, bool) or not isinstance(num_bits, int) or not 1 <= num_bits <= 8:
            raise ValueError('ImageStreamQuantizer(num_bits=%r): per-image entropy streams need a width of 1 ... 8 bits '
                             '(16 is a half round trip, no codes)' % (num_bits,))
        self.num_bits = num_bits
        self.code_lengths = None if code_lengths is None else \
            check_code_lengths('ImageStreamQuantizer', code_lengths, num_bits, complete=True)
        self._bufs, self._tables = {}, {}

    def _buffers(self, buf, c):
        """per (shape, c, device): q, qparams, the quantiser's scratch, hist, lengths, payload, offsets, the encoder's scratch"""
        key = (tuple(buf.shape), c, buf.device)
        if key not in self._bufs:
            n, h, w, _ = buf.shape
            chw, dev = c * h * w, buf.device
            words = ops.istream_scratch_bytes(n, chw) // 4
            if not words:
                raise ValueError('ImageStreamQuantizer: %d images of %d values: at most %d images and 2^30 values per call'
                                 % (n, chw, ops.ISTREAM_MAX_N))
            self._bufs[key] = (torch.empty(buf.shape, dtype=torch.uint8, device=dev),
                               torch.empty((n, 4), dtype=torch.float32, device=dev),
                               torch.empty(ops.qimage_scratch_elems(n), dtype=torch.float32, device=dev),
                               torch.empty((n, 256), dtype=torch.int32, device=dev),
                               torch.empty((n, 256), dtype=torch.uint8, device=dev),
                               torch.empty(ops.istream_capacity(n, chw), dtype=torch.uint8, device=dev),
                               torch.empty(words + 1, dtype=torch.int32, device=dev),
                               torch.empty(words, dtype=torch.int32, device=dev))
        return self._bufs[key]

    def _fixed_table(self, n, device):
        if (n, device) not in self._tables:
            row = torch.tensor(list(self.code_lengths) + [0] * (256 - len(self.code_lengths)), dtype=torch.uint8)
            self._tables[(n, device)] = row.repeat(n, 1).to(device)
        return self._tables[(n, device)]

    def __call__(self, z, target):
        buf = to_nhwc(z)                    # [N, H, W, cs] fp32 bottleneck (pad channels are 0)
        c, bits = z.shape[1], self.num_bits
        q, qparams, qscratch, hist, lengths, payload, offsets, scratch = self._buffers(buf, c)
        ops.qimage_quantize_bits(buf, c, bits, q, qparams, qscratch)
        if self.code_lengths is None:
            ops.istream_histogram(q, c, bits, hist)
            ops.istream_build_tables(hist, bits, lengths)
        else:
            lengths = self._fixed_table(buf.shape[0], buf.device)
        ops.istream_encode(q, c, bits, lengths, payload, offsets, scratch)
        return ImageStreamBottleneck(payload, offsets, lengths, z.shape, bits, qparams, origin=buf), target


class Dequantizer(object):
    """reference :143-153.  A QuantizedTensor of any width goes through the one dequantise kernel (the width lives in its
    scale); a PackedBottleneck is unpacked and dequantised in one launch and must have been packed at ``num_bits``; an
    EntropyBottleneck is decoded and dequantised in one launch and must have been coded at ``num_bits``.  A per-channel
    QuantizedTensor / PackedBottleneck (``per_channel=True``, include/hnd_qchannel.h) is recognised by that attribute and
    must have been quantised at ``num_bits``; so is a per-image one (``per_image=True``, include/hnd_qimage.h).  An
    ImageStreamBottleneck (include/hnd_istream.h) is decoded and dequantised in one launch, every image under its own table
    and qparams, and must have been coded at ``num_bits``."""

    def __init__(self, num_bits=8):
        _check_bits('Dequantizer', num_bits)
        self.num_bits = num_bits

    def __call__(self, qz, target):
        if isinstance(qz, PackedBottleneck):
            if qz.num_bits != self.num_bits:
                raise ValueError('Dequantizer(num_bits=%d) was handed a payload packed at %d bits'
                                 % (self.num_bits, qz.num_bits))
            n, c, h, w = qz.shape
            out = qz.origin if qz.origin is not None else \
                torch.empty((n, h, w, ops.chan_pad_of(c)), dtype=torch.float32, device=qz.payload.device)
            if qz.per_channel:
                ops.qchannel_unpack_dequantize_bits(qz.payload, qz.qparams, out, c, qz.num_bits)
            elif getattr(qz, 'per_image', False):
                ops.qimage_unpack_dequantize_bits(qz.payload, qz.qparams, out, c, qz.num_bits)
            else:
                ops.unpack_dequantize_bits(qz.payload, qz.qparams, out, c, qz.num_bits)
            return attach(out[..., :c].permute(0, 3, 1, 2), out), target
        if isinstance(qz, EntropyBottleneck):
            if qz.num_bits != self.num_bits:
                raise ValueError('Dequantizer(num_bits=%d) was handed a payload entropy-coded at %d bits'
                                 % (self.num_bits, qz.num_bits))
            n, c, h, w = qz.shape
            out = qz.origin if qz.origin is not None else \
                torch.empty((n, h, w, ops.chan_pad_of(c)), dtype=torch.float32, device=qz.payload.device)
            ops.entropy_decode_dequantize(qz.payload, qz.offsets, qz.lengths, qz.qparams, out, c, qz.num_bits)
            return attach(out[..., :c].permute(0, 3, 1, 2), out), target
        if isinstance(qz, ImageStreamBottleneck):
            if qz.num_bits != self.num_bits:
                raise ValueError('Dequantizer(num_bits=%d) was handed per-image streams entropy-coded at %d bits'
                                 % (self.num_bits, qz.num_bits))
            n, c, h, w = qz.shape
            out = qz.origin if qz.origin is not None else \
                torch.empty((n, h, w, ops.chan_pad_of(c)), dtype=torch.float32, device=qz.payload.device)
            ops.istream_decode_dequantize(qz.payload, qz.offsets, qz.lengths, qz.qparams, out, c, qz.num_bits)
            return attach(out[..., :c].permute(0, 3, 1, 2), out), target
        if isinstance(qz, QuantizedTensor) and qz.per_channel and qz.num_bits != self.num_bits:
            raise ValueError('Dequantizer(num_bits=%d) was handed a per-channel tensor quantised at %d bits'
                             % (self.num_bits, qz.num_bits))
        if isinstance(qz, QuantizedTensor) and getattr(qz, 'per_image', False) and qz.num_bits != self.num_bits:
            raise ValueError('Dequantizer(num_bits=%d) was handed a per-image tensor quantised at %d bits'
                             % (self.num_bits, qz.num_bits))
        if self.num_bits == 16 or not isinstance(qz, QuantizedTensor):
            return qz, target
        q = qz.tensor._hnd
        out = qz.origin if qz.origin is not None else torch.empty(q.shape, dtype=torch.float32, device=q.device)
        if qz.per_channel:
            ops.qchannel_dequantize_u8(q, qz.qparams, out, qz.channels)
        elif getattr(qz, 'per_image', False):
            ops.qimage_dequantize_u8(q, qz.qparams, out, qz.channels)
        else:
            ops.dequantize_u8(q, qz.qparams, out, qz.channels)
        z = out[..., :qz.channels].permute(0, 3, 1, 2)
        return attach(z, out), target


FAKE_QUANT_BITS = tuple(range(1, 9))


def check_fake_quant_bits(who, num_bits):
    """the widths the fake-quantising launch (include/hnd_qat.h) takes; anything else is refused by name"""
    if isinstance(num_bits, bool) or not isinstance(num_bits, int) or num_bits not in FAKE_QUANT_BITS:
        raise ValueError('%s: num_bits=%r is outside 1 ... 8, the widths the fake-quantised bottleneck implements '
                         '(16 is the half round trip of Quantizer(16))' % (who, num_bits))
    return num_bits


class FakeQuantizer(_StaticRange):
    """``[Quantizer(num_bits), Dequantizer(num_bits)]`` as ONE codec call (include/hnd_qat.h): z -> the dequantised tensor,
    bit for bit what the pair returns, written back into z's buffer.  1 ... 8 bits; an extension (the reference has no
    such class).  ``qparams`` holds {min, max, scale, zero_point} of the newest call, on the device.  ``static_range``: see
    _StaticRange; the call is then hnd_fake_quantize_range alone.  ``per_channel=True`` (not with ``static_range``): the pair
    ``[Quantizer(num_bits, per_channel=True), Dequantizer(num_bits)]`` as one call (include/hnd_qchannel.h); ``qparams`` is
    then [c, 4].  ``per_image=True`` (not with ``static_range`` or ``per_channel``): the pair
    ``[Quantizer(num_bits, per_image=True), Dequantizer(num_bits)]`` as one call (include/hnd_qimage.h); ``qparams`` is then
    [n, 4]."""

    def __init__(self, num_bits=8, static_range=None, per_channel=False, per_image=False):
        self.num_bits = check_fake_quant_bits('FakeQuantizer', num_bits)
        self.per_channel = _check_per_channel('FakeQuantizer', per_channel)
        if self.per_channel:
            _check_per_channel_combination('FakeQuantizer', num_bits, static_range)
        self.per_image = _check_per_image('FakeQuantizer', per_image)
        if self.per_image:
            _check_per_image_combination('FakeQuantizer', num_bits, static_range, per_channel=self.per_channel)
        self._bufs = {}
        self.qparams = None
        self._init_static_range(static_range)

    def __call__(self, z, target):
        self._check_resolved()
        buf = to_nhwc(z)                    # [N, H, W, cs] fp32 bottleneck (pad channels are 0)
        c, cs, dev = z.shape[1], buf.shape[-1], buf.device
        fixed = self._static_qparams_on(dev)
        if fixed is not None:               # one launch on the fixed range (include/hnd_qrange.h)
            self.qparams = fixed
            ops.fake_quantize_range(buf, c, self.num_bits, fixed)
        else:
            # per flavour: the call, the key of its two buffers, the shape of qparams and the floats of scratch
            if self.per_channel:            # a scale and a zero point per channel (include/hnd_qchannel.h)
                call, key, qshape, nscratch = ops.qchannel_fake_quantize_bits, (dev, c, cs), (c, 4), ops.qchannel_scratch_elems
            elif self.per_image:            # a scale and a zero point per image (include/hnd_qimage.h)
                n = buf.shape[0]
                call, key, qshape, nscratch = ops.qimage_fake_quantize_bits, (dev, 'n', n), (n, 4), \
                    lambda cs: ops.qimage_scratch_elems(n)
            else:
                call, key, qshape, nscratch = ops.fake_quantize_bits, dev, (4,), lambda cs: ops.minmax_scratch_elems()
            if key not in self._bufs:
                self._bufs[key] = (torch.empty(qshape, dtype=torch.float32, device=dev),
                                   torch.empty(nscratch(cs), dtype=torch.float32, device=dev))
            self.qparams, scratch = self._bufs[key]
            call(buf, c, self.num_bits, self.qparams, scratch)
        if getattr(z, '_hnd', None) is buf:         # a HIP-path tensor: a view of the buffer just rewritten
            return z, target
        return attach(buf[..., :c].permute(0, 3, 1, 2), buf), target


def resolve_trained_ranges(transformer, info):
    """hand ``info`` (a checkpoint's ``bottleneck_range``, or the live range of a student under distillation) to every
    component of ``transformer`` (a Compose, a single component or None) whose static_range is 'trained'; returns how many
    took it.  info None: refused by name if any component waits for one."""
    parts = getattr(transformer, 'transforms', None)
    parts = ([] if transformer is None else [transformer]) if parts is None else list(parts)
    return sum(1 for t in parts if isinstance(t, _StaticRange) and t.resolve_trained_range(info))


TRANSFORMER_CLASS_DICT = {'jpeg_compressor': JpegCompressor, 'jpeg_decompressor': JpegDecompressor,
                          'quantizer': Quantizer, 'dequantizer': Dequantizer, 'fake_quantizer': FakeQuantizer,
                          'image_stream_quantizer': ImageStreamQuantizer}


def get_bottleneck_transformer(transformer_config):
    components = []
    for name in transformer_config['order']:
        if name not in TRANSFORMER_CLASS_DICT:
            raise KeyError('transformer `{}` is not expected'.format(name))
        components.append(TRANSFORMER_CLASS_DICT[name](**transformer_config['components'][name]['params']))
    return Compose(components) if components else None
