"""CPU: per-image entropy streams (include/hnd_istream.h) on a machine without a GPU -- the header through _lib's reader, the
symbols, the version, the size queries, the refusals of the C entry points (all before any HIP call: host memory stands in
for the device pointers), the restatement of the device table builder (tests/istream_util.device_lengths) against
transformer.huffman_lengths byte for byte, the classes of structure/transformer.py and the guard ledger of the header."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import entropy_util as EU
from tests import istream_util as IU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'hnd_istream.h')
EXPORTS = ['hnd_istream_abi', 'hnd_istream_build_tables', 'hnd_istream_capacity', 'hnd_istream_chunks_per_image',
           'hnd_istream_decode_dequantize', 'hnd_istream_encode', 'hnd_istream_histogram', 'hnd_istream_scratch_bytes']


@pytest.fixture(scope='module', autouse=True)
def built():
    """the package loads libhnd_hip.so on import (there is no fallback), so it is built first"""
    import __graft_entry__ as g
    g.build()


# ------------------------------------------------------------------------------------------ header and library
def test_header_parses_and_the_library_exports_what_it_declares():
    from hnd_ghnd_object_detectors_amd import _lib
    header = _lib.parse_header(open(HEADER).read(), 'hnd_istream.h')
    assert sorted(header.functions) == EXPORTS and not header.structs and not header.enums
    assert header.defines == {'HND_ISTREAM_ABI': 1, 'HND_ISTREAM_MAX_N': IU.MAX_N}
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(hnd_[a-z0-9_]+)\s*\(', text))) == EXPORTS
    lib = _lib.load()
    assert list(_lib.ISTREAM_SYMBOLS) == EXPORTS == sorted(_lib.ISTREAM_HEADER.functions)
    assert all(getattr(lib, name) is not None for name in EXPORTS)
    assert lib.hnd_istream_abi() == _lib.ISTREAM_ABI == 1
    # the other eight headers do not move
    assert tuple(_lib.HEADERS) == ('hnd_hip.h', 'hnd_optim.h', 'hnd_codec.h', 'hnd_qat.h')
    assert [len(t) for t in (_lib.EXPORTED_SYMBOLS, _lib.OPTIM_SYMBOLS, _lib.CODEC_SYMBOLS, _lib.QAT_SYMBOLS)] == [94, 2, 5, 3]
    assert (len(_lib.QRANGE_SYMBOLS), len(_lib.ENTROPY_SYMBOLS)) == (7, 7)
    assert (_lib.ENTROPY_ABI, _lib.QIMAGE_ABI, _lib.QCHANNEL_ABI, _lib.QRANGE_ABI) == (1, 1, 1, 1)


def test_size_queries_are_the_entropy_coder_s_per_image():
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    for chw in (1, 105, 255, 256, 257, 768, 6345, (1 << 30) - 1, 1 << 30):
        assert lib.hnd_istream_chunks_per_image(chw) == EU.chunks(chw) == -(-chw // 256)
        for n in (1, 2, 3, 16, IU.MAX_N):
            if n * chw > 1 << 30:
                assert lib.hnd_istream_capacity(n, chw) == lib.hnd_istream_scratch_bytes(n, chw) == 0
                continue
            assert lib.hnd_istream_capacity(n, chw) == n * EU.capacity(chw) == IU.capacity(n, chw)
            assert lib.hnd_istream_scratch_bytes(n, chw) == 4 * n * EU.chunks(chw) == IU.scratch_bytes(n, chw)
    for chw in (0, -1, (1 << 30) + 1, 1 << 40):
        assert lib.hnd_istream_chunks_per_image(chw) == lib.hnd_istream_capacity(1, chw) == 0
        assert lib.hnd_istream_scratch_bytes(1, chw) == 0
    for n in (0, -1, IU.MAX_N + 1):
        assert lib.hnd_istream_capacity(n, 105) == lib.hnd_istream_scratch_bytes(n, 105) == 0
    # every offset of the largest call fits 32 bits
    assert max(IU.capacity(n, (1 << 30) // n) for n in (1, 2, 4095, IU.MAX_N)) < 1 << 32


def check_every_refusal(lib):
    """every refusal of the header comment returns HND_ERR_INVALID (-1) with the export's name in the error string; nothing is
    launched, so host memory stands in for the device pointers"""
    host = (ctypes.c_double * 64)()
    addr = ctypes.addressof(host)
    p = addr + (-addr) % 16

    def histogram(q=p, n=2, h=2, w=2, c=3, cs=4, bits=4, hist=p):
        return lib.hnd_istream_histogram(q, n, h, w, c, cs, bits, hist, None)

    def build(hist=p, n=2, bits=4, lengths=p):
        return lib.hnd_istream_build_tables(hist, n, bits, lengths, None)

    def encode(q=p, n=2, h=2, w=2, c=3, cs=4, bits=4, lengths=p, payload=p, offsets=p, scratch=p):
        return lib.hnd_istream_encode(q, n, h, w, c, cs, bits, lengths, payload, offsets, scratch, None)

    def decode(payload=p, payload_bytes=768, offsets=p, lengths=p, qparams=p, x=p, n=2, h=2, w=2, c=3, cs=4, bits=4):
        return lib.hnd_istream_decode_dequantize(payload, payload_bytes, offsets, lengths, qparams, x, n, h, w, c, cs, bits, None)

    geometry = (dict(c=0), dict(c=-3), dict(c=5, cs=4), dict(c=3, cs=6), dict(n=0), dict(n=-2), dict(h=0), dict(w=-1),
                dict(n=IU.MAX_N + 1, h=1, w=1, c=1), dict(n=1 << 15, h=1 << 15, w=2, c=1))
    calls = {'hnd_istream_histogram': (histogram, ('q', 'hist'), ('q', 'hist'), geometry),
             'hnd_istream_build_tables': (build, ('hist', 'lengths'), ('hist',), (dict(n=0), dict(n=-1), dict(n=IU.MAX_N + 1))),
             'hnd_istream_encode': (encode, ('q', 'lengths', 'payload', 'offsets', 'scratch'),
                                    ('q', 'payload', 'offsets', 'scratch'), geometry),
             'hnd_istream_decode_dequantize': (decode, ('payload', 'offsets', 'lengths', 'qparams', 'x'),
                                               ('payload', 'offsets', 'qparams', 'x'), geometry)}
    for name, (call, pointers, aligned, bad) in calls.items():
        def refused(rc):
            return rc == -1 and name.encode() in lib.hnd_last_error_string()
        for ptr in pointers:
            assert refused(call(**{ptr: None})), (name, ptr)
        for ptr in aligned:
            assert refused(call(**{ptr: p + 4})), (name, ptr, 'alignment')
        for bits in (0, 9, -1, 16):
            assert refused(call(bits=bits)), (name, bits)
        for kw in bad:
            assert refused(call(**kw)), (name, kw)
    for nbytes in (0, -4, 1 << 32):
        assert decode(payload_bytes=nbytes) == -1 and b'hnd_istream_decode_dequantize' in lib.hnd_last_error_string()
    assert all(v == 0.0 for v in host)                                    # nothing wrote the stand-in memory


def test_every_export_validates_before_any_hip_call():
    from hnd_ghnd_object_detectors_amd import _lib
    check_every_refusal(_lib.load())


def test_ops_wrappers_refuse_by_name():
    from hnd_ghnd_object_detectors_amd import ops
    q = torch.zeros(2, 2, 2, 4, dtype=torch.uint8)
    hist, lengths = torch.zeros(2, 256, dtype=torch.int32), torch.zeros(2, 256, dtype=torch.uint8)
    payload, offsets, scratch = torch.zeros(768, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match='istream_histogram: bits=9'):
        ops.istream_histogram(q, 3, 9, hist)
    with pytest.raises(ValueError, match='istream_histogram: c=5'):
        ops.istream_histogram(q, 5, 4, hist)
    with pytest.raises(ValueError, match=r'istream_histogram: hist must be a contiguous int32 tensor \[2, 256\]'):
        ops.istream_histogram(q, 3, 4, hist[:1])
    with pytest.raises(ValueError, match='istream_build_tables: bits=True'):
        ops.istream_build_tables(hist, True, lengths)
    with pytest.raises(ValueError, match='istream_build_tables: hist must be'):
        ops.istream_build_tables(hist.view(-1), 4, lengths)
    with pytest.raises(ValueError, match='istream_build_tables: lengths must be'):
        ops.istream_build_tables(hist, 4, lengths.int())
    with pytest.raises(ValueError, match='istream_encode: lengths must be'):
        ops.istream_encode(q, 3, 4, bytes(16), payload, offsets, scratch)
    with pytest.raises(ValueError, match='istream_encode: payload must be 768'):
        ops.istream_encode(q, 3, 4, lengths, payload[:767], offsets, scratch)
    with pytest.raises(ValueError, match='istream_encode: offsets must be'):
        ops.istream_encode(q, 3, 4, lengths, payload, offsets[:2], scratch)
    with pytest.raises(ValueError, match='istream_encode: scratch must hold 8'):
        ops.istream_encode(q, 3, 4, lengths, payload, offsets, scratch[:1])
    with pytest.raises(ValueError, match=r'istream_decode_dequantize: qparams must be a contiguous fp32 tensor \[2, 4\]'):
        ops.istream_decode_dequantize(payload, offsets, lengths, torch.zeros(4), torch.zeros(2, 2, 2, 4), 3, 4)
    with pytest.raises(ValueError, match='istream_decode_dequantize: payload must be'):
        ops.istream_decode_dequantize(payload[:0], offsets, lengths, torch.zeros(2, 4), torch.zeros(2, 2, 2, 4), 3, 4)
    assert ops.istream_abi() == 1 and ops.ISTREAM_MAX_N == IU.MAX_N
    assert (ops.istream_chunks_per_image(105), ops.istream_capacity(3, 105), ops.istream_scratch_bytes(3, 105)) == (1, 1152, 12)


# ------------------------------------------------------------------------------------------ the device table builder, restated
def _fibonacci_histogram():
    """an 8-bit histogram whose unconstrained Huffman tree is deeper than 12: 20 Fibonacci counts among zeros"""
    hist, a, b = [0] * 256, 1, 1
    for k in range(20):
        hist[3 + 11 * k] = a
        a, b = b, a + b
    return hist


def _histograms():
    cases = [('normal-b%d' % bits, bits, EU.normal_histogram(bits)) for bits in range(1, 9)]
    for bits in (1, 4, 8):
        nsym = 1 << bits
        cases.append(('one-b%d' % bits, bits, [0] * (nsym - 1) + [37]))
        cases.append(('two-b%d' % bits, bits, [5] + [0] * (nsym - 2) + [900]))
        cases.append(('equal-b%d' % bits, bits, [100] * nsym))
    cases.append(('equal-odd-b8', 8, [7] * 201 + [0] * 55))
    cases.append(('tied-runs-b8', 8, [1 + (s // 9) % 5 for s in range(256)]))
    cases.append(('tied-runs-b5', 5, [3, 3, 3, 6, 6, 6, 6, 12, 12, 0, 0, 3, 24, 24, 24, 1] * 2))
    cases.append(('near-2^30-b8', 8, [(1 << 30) // 256 - (s % 3) for s in range(256)]))
    cases.append(('near-2^30-b2', 2, [(1 << 30) - 6, 1, 2, 3]))
    cases.append(('geometric-b4', 4, list(EU.GEOMETRIC_HIST)))
    cases.append(('fibonacci-b8', 8, _fibonacci_histogram()))
    cases.append(('skewed-image-b8', 8, IU.skewed_histogram()))
    return cases


HISTS = _histograms()


@pytest.mark.parametrize('name,bits,hist', HISTS, ids=[n for n, _, _ in HISTS])
def test_device_algorithm_restated_equals_the_host_routine_byte_for_byte(name, bits, hist):
    from hnd_ghnd_object_detectors_amd.structure.transformer import huffman_lengths
    want = huffman_lengths(hist, bits)
    got = IU.device_lengths(hist, bits)
    assert isinstance(got, bytes) and got == want, (name, list(got), list(want))
    assert got == IU.device_lengths(list(hist) + [0] * (256 - len(hist)), bits)      # a device row has 256 entries
    if name.startswith(('fibonacci', 'skewed', 'geometric')):
        # the precondition: the unconstrained tree is deeper than 12, so the length limit binds
        assert max(EU.heap_huffman_depths(hist).values()) > EU.MAX_LEN and max(got) == EU.MAX_LEN
    if sum(1 for w in hist if w) > 1:
        assert EU.kraft(got) == 1 << EU.MAX_LEN


def test_an_empty_histogram_gives_an_empty_table_on_the_device_only():
    from hnd_ghnd_object_detectors_amd.structure.transformer import huffman_lengths
    assert IU.device_lengths([0] * 16, 4) == bytes(16)               # the header's rule; the host routine refuses it
    with pytest.raises(ValueError, match='an empty histogram'):
        huffman_lengths([0] * 16, 4)


# ------------------------------------------------------------------------------------------ the classes
def test_quantizer_class_refuses_by_name_and_the_pair_stays_refused():
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    sig = inspect.signature(T.ImageStreamQuantizer.__init__)
    assert list(sig.parameters) == ['self', 'num_bits', 'code_lengths']
    assert [p.default for p in list(sig.parameters.values())[1:]] == [8, None]
    for bad in (16, 0, 9, 4.0, True, None, '4'):
        with pytest.raises(ValueError, match='ImageStreamQuantizer.*1 ... 8'):
            T.ImageStreamQuantizer(bad)
    with pytest.raises(ValueError, match='ImageStreamQuantizer: a fixed table of code_lengths must be complete'):
        T.ImageStreamQuantizer(2, code_lengths=[1, 2, 0, 2])
    with pytest.raises(ValueError, match='ImageStreamQuantizer: .*Kraft sum above 1'):
        T.ImageStreamQuantizer(2, code_lengths=[1, 1, 2, 2])
    with pytest.raises(ValueError, match='ImageStreamQuantizer: .*outside 0 ... 12'):
        T.ImageStreamQuantizer(2, code_lengths=[1, 2, 3, 13])
    with pytest.raises(ValueError, match='ImageStreamQuantizer: .*must be 4 integers'):
        T.ImageStreamQuantizer(2, code_lengths=[1, 2, 3])
    q = T.ImageStreamQuantizer(2, code_lengths=[1, 2, 3, 3])
    assert q.num_bits == 2 and q.code_lengths == bytes([1, 2, 3, 3])
    assert T.ImageStreamQuantizer().num_bits == 8 and T.ImageStreamQuantizer(5).code_lengths is None
    with pytest.raises(ValueError, match='the entropy coder has no per-image form'):
        T.Quantizer(4, entropy=True, per_image=True)
    assert list(inspect.signature(T.Quantizer.__init__).parameters) == ['self', 'num_bits', 'packed', 'static_range', 'entropy',
                                                                         'code_lengths']


def test_registry_configuration_and_split_model():
    from hnd_ghnd_object_detectors_amd.models.mimic import split_rcnn as S
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    import yaml
    assert T.TRANSFORMER_CLASS_DICT['image_stream_quantizer'] is T.ImageStreamQuantizer
    cfg = yaml.safe_load('order: [image_stream_quantizer, dequantizer]\n'
                         'components:\n'
                         '  image_stream_quantizer: {params: {num_bits: 4}}\n'
                         '  dequantizer: {params: {num_bits: 4}}\n')
    quantizer, dequantizer = T.get_bottleneck_transformer(cfg).transforms
    assert isinstance(quantizer, T.ImageStreamQuantizer) and quantizer.num_bits == 4 and isinstance(dequantizer, T.Dequantizer)
    assert list(inspect.signature(S.split_rcnn_model_image_streams).parameters) == ['model', 'num_bits', 'code_lengths']
    with pytest.raises(ValueError, match='split_rcnn_model_image_streams needs a quantization width'):
        S.split_rcnn_model_image_streams(None, None)
    with pytest.raises(ValueError, match='ImageStreamQuantizer'):
        S.split_rcnn_model_image_streams(None, 16)


def _hand_made():
    """two images of 300 values at 2 bits (cpi = 2): streams of 5 + 2 and 0 + 3 bytes"""
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    payload = torch.arange(100, 100 + 2 * 2 * 384, dtype=torch.int64).to(torch.uint8)
    offsets = torch.tensor([0, 5, 7, 7, 10], dtype=torch.int32)
    lengths = torch.zeros(2, 256, dtype=torch.uint8)
    lengths[0, :4] = torch.tensor([1, 2, 3, 3], dtype=torch.uint8)
    lengths[1, :4] = torch.tensor([2, 2, 2, 2], dtype=torch.uint8)
    qparams = torch.tensor([[-1.0, 2.0, 1.0, 1.0], [0.0, 6.0, 2.0, 0.0]])
    return T.ImageStreamBottleneck(payload, offsets, lengths, (2, 3, 10, 10), 2, qparams), payload


def test_bottleneck_link_bytes_and_image_rebasing_on_hand_made_tensors():
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    sb, payload = _hand_made()
    assert sb.chunks_per_image == 2 and sb.shape == (2, 3, 10, 10) and sb.num_bits == 2
    assert sb.nbytes == 10 and sb.image_nbytes == [7, 3]
    assert sb.image_link_bytes == [7 + 4 * 3 + 4 + 8, 3 + 4 * 3 + 4 + 8] == \
        [IU.image_link_bytes(7, 300, 2), IU.image_link_bytes(3, 300, 2)]
    assert sb.link_bytes == 10 + 2 * (12 + 4 + 8)
    assert torch.equal(sb.scale, torch.tensor([1.0, 2.0])) and torch.equal(sb.zero_point, torch.tensor([1.0, 0.0]))
    assert sb.scale.data_ptr() == sb.qparams.data_ptr() + 8
    for i, (lo, hi, offs, table) in enumerate([(0, 7, [0, 5, 7], [1, 2, 3, 3]), (7, 10, [0, 0, 3], [2, 2, 2, 2])]):
        eb = sb.image(i)
        assert isinstance(eb, T.EntropyBottleneck) and eb.shape == (1, 3, 10, 10) and eb.num_bits == 2
        assert eb.payload.data_ptr() % 16 == 0 and eb.payload.data_ptr() != payload.data_ptr() + lo
        assert torch.equal(eb.payload, payload[lo:hi]) and eb.offsets.tolist() == offs and eb.offsets.dtype == torch.int32
        assert eb.lengths == bytes(table) and eb.nbytes == hi - lo
        assert torch.equal(eb.qparams, sb.qparams[i]) and eb.qparams.data_ptr() != sb.qparams[i].data_ptr()
        assert float(eb.scale) == float(sb.scale[i]) and float(eb.zero_point) == float(sb.zero_point[i])
        assert eb.link_bytes == sb.image_link_bytes[i] == EU.link_bytes(hi - lo, 300, 2)
    for bad in (-1, 2, True, 0.0):
        with pytest.raises(IndexError, match='ImageStreamBottleneck.image'):
            sb.image(bad)
    with pytest.raises(ValueError, match='per-image streams entropy-coded at 2 bits'):
        T.Dequantizer(4)(sb, None)


def test_offsets_beyond_2_31_are_read_unsigned_and_rebased():
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    big = (1 << 31) + 40
    offsets = torch.tensor([0, big - (1 << 32), big + 9 - (1 << 32)], dtype=torch.int32)
    sb = T.ImageStreamBottleneck(torch.zeros(16, dtype=torch.uint8), offsets, torch.zeros(2, 256, dtype=torch.uint8),
                                 (2, 1, 1, 5), 2, torch.zeros(2, 4))
    assert sb.chunks_per_image == 1 and sb.image_nbytes == [big, 9] and sb.nbytes == big + 9
    rebased = offsets[1:3] - (big - (1 << 32))
    assert rebased.tolist() == [0, 9]


# ------------------------------------------------------------------------------------------ the guard ledger
def test_every_export_of_the_header_has_a_guard_case_or_a_reason():
    loaded = 'hnd_ghnd_object_detectors_amd.ops' in sys.modules
    from tests import test_guard_bands_istream_gpu as T
    # importing the guard-band module must not touch the GPU: it loads neither the library nor the launch helpers
    assert loaded or 'hnd_ghnd_object_detectors_amd.ops' not in sys.modules
    covered = set().union(*T.LEDGER.values())
    assert covered and all(T.LEDGER.values())
    assert all(isinstance(reason, str) and reason for reason in T.NO_DEVICE_OUTPUT.values())
    assert not covered & set(T.NO_DEVICE_OUTPUT)
    assert covered | set(T.NO_DEVICE_OUTPUT) == set(EXPORTS)
    assert all(callable(getattr(T, name, None)) and name.startswith('test_') for name in T.LEDGER)
