"""CPU: the entropy-coded link payload (include/hnd_entropy.h) on a machine without a GPU -- the length builder
(transformer.huffman_lengths) against an unconstrained heapq Huffman, the numpy restatement of the format
(tests/entropy_util.py) round-tripping its own streams, the keyword refusals of Quantizer / Dequantizer, the refusals of the
C entry points (all before any HIP call: host memory stands in for the device pointers), the size queries, and the guard
ledger of the header."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

from tests import entropy_util as EU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'hnd_entropy.h')
EXPORTS = ['hnd_code_histogram', 'hnd_entropy_abi', 'hnd_entropy_capacity', 'hnd_entropy_chunks', 'hnd_entropy_decode_dequantize',
           'hnd_entropy_encode', 'hnd_entropy_scratch_bytes']


@pytest.fixture(scope='module', autouse=True)
def built():
    """the package loads libhnd_hip.so on import (there is no fallback), so it is built first"""
    import __graft_entry__ as g
    g.build()


def _histograms():
    """(name, bits, hist)"""
    cases = []
    for bits in (1, 2, 4, 8):
        nsym = 1 << bits
        cases.append(('uniform', bits, [100] * nsym))
        cases.append(('one', bits, [0] * (nsym - 1) + [37]))
        cases.append(('two', bits, [5] + [0] * (nsym - 2) + [900]))
        cases.append(('normal', bits, EU.normal_histogram(bits)))
    cases.append(('geometric', 4, list(EU.GEOMETRIC_HIST)))
    return cases


HISTS = _histograms()
HIST_IDS = ['%s-b%d' % (n, b) for n, b, _ in HISTS]


# ------------------------------------------------------------------------------------------ the length builder
@pytest.mark.parametrize('name,bits,hist', HISTS, ids=HIST_IDS)
def test_huffman_lengths_are_valid_optimal_and_deterministic(name, bits, hist):
    from hnd_ghnd_object_detectors_amd.structure.transformer import huffman_lengths
    lengths = huffman_lengths(hist, bits)
    assert isinstance(lengths, bytes) and len(lengths) == 1 << bits
    assert lengths == huffman_lengths(list(hist), bits) == huffman_lengths(np.array(hist), bits)      # same input, same bytes
    assert max(lengths) <= 12
    assert all((l == 0) == (w == 0) for l, w in zip(lengths, hist))              # absent symbols, and only they, get 0
    present = sum(1 for w in hist if w)
    if present == 1:
        assert sorted(lengths)[-1] == 1 and sum(lengths) == 1
    else:
        assert EU.kraft(lengths) == 1 << 12                                      # complete: the Kraft sum is exactly 1
    cost = sum(w * l for w, l in zip(hist, lengths))
    assert cost <= bits * sum(hist)
    depth = EU.heap_huffman_depths(hist)
    if present > 1 and max(depth.values()) <= 12:
        assert cost == sum(hist[s] * d for s, d in depth.items())
    if name == 'geometric':
        assert max(depth.values()) == 15 and max(lengths) == 12                  # capped, and still a valid table
    EU.canonical_codes(lengths)


def test_huffman_lengths_refuses_what_is_not_a_histogram():
    from hnd_ghnd_object_detectors_amd.structure.transformer import huffman_lengths
    for hist, bits in (([0] * 16, 4), ([1, 2, 3], 4), ([1, -1] + [0] * 14, 4), ([1] * 16 + [3], 4)):
        with pytest.raises(ValueError, match='huffman_lengths'):
            huffman_lengths(hist, bits)
    with pytest.raises(ValueError, match='max_len'):
        huffman_lengths([1] * 256, 8, max_len=7)
    assert huffman_lengths([3] * 16 + [0] * 240, 4) == bytes([4] * 16)            # a device histogram has 256 entries


# ------------------------------------------------------------------------------------------ the restated format
def test_canonical_codes_are_the_header_s_assignment():
    codes = EU.canonical_codes(bytes([2, 1, 3, 3]))
    assert codes == {1: (0, 1), 0: (2, 2), 2: (6, 3), 3: (7, 3)}
    payload, offsets = EU.encode([1, 0, 2, 3], bytes([2, 1, 3, 3]))
    # stream bits, first to last: 0 | 1 0 | 1 1 0 | 1 1 1 -> byte 0 = bits 0..7 LSB first, byte 1 = the ninth bit
    assert payload.tolist() == [0b11011010, 0b1] and offsets.tolist() == [0, 2]


@pytest.mark.parametrize('name,bits,hist', HISTS, ids=HIST_IDS)
def test_numpy_encoder_and_decoder_round_trip(name, bits, hist):
    from hnd_ghnd_object_detectors_amd.structure.transformer import huffman_lengths
    total = sum(hist)
    scale = max(1, total // 700)                                                 # about 700 symbols: a few chunks and a tail
    symbols = np.repeat(np.arange(1 << bits), [-(-w // scale) if w else 0 for w in hist]).astype(np.uint8)
    symbols = symbols[np.random.RandomState(3).permutation(symbols.size)]
    for lengths in (huffman_lengths(hist, bits), EU.valid_lengths(hist, bits)):
        payload, offsets = EU.encode(symbols, lengths)
        assert offsets.size == EU.chunks(symbols.size) + 1 and int(offsets[-1]) == payload.size <= EU.capacity(symbols.size)
        assert np.array_equal(EU.decode(payload, offsets, lengths, symbols.size), symbols)
        assert EU.link_bytes(payload.size, symbols.size, bits) == payload.size + 4 * offsets.size + (1 << bits) + 8


# ------------------------------------------------------------------------------------------ Python refusals
def test_quantizer_and_dequantizer_refuse_by_name():
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    sig = inspect.signature(T.Quantizer.__init__)
    assert list(sig.parameters) == ['self', 'num_bits', 'packed', 'static_range', 'entropy', 'code_lengths']
    assert [p.default for p in list(sig.parameters.values())[1:]] == [8, False, None, False, None]
    with pytest.raises(ValueError, match='entropy=True, packed=True'):
        T.Quantizer(4, packed=True, entropy=True)
    with pytest.raises(ValueError, match='num_bits=16, entropy=True'):
        T.Quantizer(16, entropy=True)
    with pytest.raises(ValueError, match='code_lengths.*needs entropy=True'):
        T.Quantizer(2, code_lengths=[2, 2, 2, 2])
    with pytest.raises(ValueError, match='must be complete'):
        T.Quantizer(2, entropy=True, code_lengths=[1, 2, 0, 2])
    with pytest.raises(ValueError, match='Kraft sum above 1'):
        T.Quantizer(2, entropy=True, code_lengths=[1, 1, 2, 2])
    with pytest.raises(ValueError, match='outside 0 ... 12'):
        T.Quantizer(2, entropy=True, code_lengths=[1, 2, 3, 13])
    with pytest.raises(ValueError, match='must be 4 integers'):
        T.Quantizer(2, entropy=True, code_lengths=[1, 2, 3])
    with pytest.raises(ValueError, match='must be 4 integers'):
        T.Quantizer(2, entropy=True, code_lengths=[1, 2, 3, 2.5])
    q = T.Quantizer(2, entropy=True, code_lengths=[1, 2, 3, 3])
    assert q.entropy and q.code_lengths == bytes([1, 2, 3, 3]) and not q.packed
    plain = T.Quantizer(4)
    assert not plain.entropy and plain.code_lengths is None
    eb = T.EntropyBottleneck(None, None, bytes([1, 1]), (1, 1, 1, 2), 1, [0.0, 1.0, 1.0, 0.0])
    with pytest.raises(ValueError, match='entropy-coded at 1 bits'):
        T.Dequantizer(4)(eb, None)


def test_configuration_and_split_model_reach_the_keyword():
    from hnd_ghnd_object_detectors_amd.models.mimic import split_rcnn as S
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    import yaml
    cfg = yaml.safe_load('order: [quantizer, dequantizer]\n'
                         'components:\n'
                         '  quantizer: {params: {num_bits: 4, entropy: true}}\n'
                         '  dequantizer: {params: {num_bits: 4}}\n')
    quantizer, dequantizer = T.get_bottleneck_transformer(cfg).transforms
    assert isinstance(quantizer, T.Quantizer) and quantizer.entropy and quantizer.num_bits == 4
    assert list(inspect.signature(S.split_rcnn_model_entropy).parameters) == ['model', 'quantization', 'static_range',
                                                                               'code_lengths']
    assert list(inspect.signature(S.split_rcnn_model).parameters) == ['model', 'quantization', 'packed']
    assert list(inspect.signature(S.split_rcnn_model_ranged).parameters) == ['model', 'quantization', 'static_range', 'packed']
    with pytest.raises(ValueError, match='split_rcnn_model_entropy needs a quantization width'):
        S.split_rcnn_model_entropy(None, None)


# ------------------------------------------------------------------------------------------ C ABI
def test_entropy_symbols_resolve_and_the_other_tables_do_not_move():
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    assert list(_lib.ENTROPY_SYMBOLS) == EXPORTS == sorted(_lib.ENTROPY_HEADER.functions)
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(hnd_[a-z0-9_]+)\s*\(', text))) == EXPORTS
    assert lib.hnd_entropy_abi() == _lib.ENTROPY_ABI == 1
    assert not _lib.ENTROPY_HEADER.structs and not _lib.ENTROPY_HEADER.enums
    assert tuple(_lib.HEADERS) == ('hnd_hip.h', 'hnd_optim.h', 'hnd_codec.h', 'hnd_qat.h')
    assert [len(t) for t in (_lib.EXPORTED_SYMBOLS, _lib.OPTIM_SYMBOLS, _lib.CODEC_SYMBOLS, _lib.QAT_SYMBOLS)] == [94, 2, 5, 3]
    assert len(_lib.QRANGE_SYMBOLS) == 7


def test_size_queries_match_the_arithmetic():
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    for numel in (1, 5, 255, 256, 257, 546, 768, 32768, (1 << 30) - 1, 1 << 30):
        assert lib.hnd_entropy_chunks(numel) == EU.chunks(numel) == -(-numel // 256)
        assert lib.hnd_entropy_capacity(numel) == EU.capacity(numel) == 384 * -(-numel // 256)
        assert lib.hnd_entropy_scratch_bytes(numel) == 4 * EU.chunks(numel)
    for numel in (0, -1, -256, (1 << 30) + 1, 1 << 40):
        assert lib.hnd_entropy_chunks(numel) == lib.hnd_entropy_capacity(numel) == lib.hnd_entropy_scratch_bytes(numel) == 0


def test_every_export_validates_before_any_hip_call():
    """every refusal of the header comment returns HND_ERR_INVALID (-1) with the export's name in the error string; nothing is
    launched, so host memory stands in for the device pointers"""
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    host = (ctypes.c_double * 64)()
    addr = ctypes.addressof(host)
    p = addr + (-addr) % 16
    good = bytes([1, 2, 3, 3]) + bytes(12)                  # a valid table at 2 bits ... 4 bits (absent symbols)

    def histogram(q=p, n=1, h=2, w=2, c=3, cs=4, bits=4, hist=p):
        return lib.hnd_code_histogram(q, n, h, w, c, cs, bits, hist, None)

    def encode(q=p, n=1, h=2, w=2, c=3, cs=4, bits=4, lengths=good, payload=p, offsets=p, scratch=p):
        return lib.hnd_entropy_encode(q, n, h, w, c, cs, bits, lengths, payload, offsets, scratch, None)

    def decode(payload=p, payload_bytes=384, offsets=p, lengths=good, qparams=p, x=p, n=1, h=2, w=2, c=3, cs=4, bits=4):
        return lib.hnd_entropy_decode_dequantize(payload, payload_bytes, offsets, lengths, qparams, x, n, h, w, c, cs, bits, None)

    calls = {'hnd_code_histogram': (histogram, ('q', 'hist')),
             'hnd_entropy_encode': (encode, ('q', 'lengths', 'payload', 'offsets', 'scratch')),
             'hnd_entropy_decode_dequantize': (decode, ('payload', 'offsets', 'lengths', 'qparams', 'x'))}
    for name, (call, pointers) in calls.items():
        def refused(rc):
            return rc == -1 and name.encode() in lib.hnd_last_error_string()
        for ptr in pointers:
            assert refused(call(**{ptr: None})), (name, ptr)
            if ptr != 'lengths':
                assert refused(call(**{ptr: p + 4})), (name, ptr, 'alignment')
        for bits in (0, 9, -1, 16):
            assert refused(call(bits=bits)), (name, bits)
        for kw in (dict(c=0), dict(c=-3), dict(c=5, cs=4), dict(c=3, cs=6), dict(n=0), dict(h=0), dict(w=-1),
                   dict(n=1 << 15, h=1 << 15, w=2, c=1)):
            assert refused(call(**kw)), (name, kw)
        if 'lengths' in pointers:
            for table, why in ((bytes([13, 1]) + bytes(14), b'above 12'), (bytes([1, 1, 2]) + bytes(13), b'Kraft'),
                               (bytes(16), b'non-zero')):
                assert refused(call(lengths=table)) and why in lib.hnd_last_error_string(), (name, why)
    for nbytes in (0, -4):
        assert decode(payload_bytes=nbytes) == -1 and b'hnd_entropy_decode_dequantize' in lib.hnd_last_error_string()
    assert all(v == 0.0 for v in host)                                    # nothing wrote the stand-in memory


def test_ops_wrappers_refuse_by_name():
    import torch
    from hnd_ghnd_object_detectors_amd import ops
    q = torch.zeros(1, 2, 2, 4, dtype=torch.uint8)
    hist = torch.zeros(256, dtype=torch.int32)
    with pytest.raises(ValueError, match='code_histogram: bits=9'):
        ops.code_histogram(q, 3, 9, hist)
    with pytest.raises(ValueError, match='code_histogram: c=5'):
        ops.code_histogram(q, 5, 4, hist)
    with pytest.raises(ValueError, match='code_histogram: hist must be'):
        ops.code_histogram(q, 3, 4, hist[:8])
    with pytest.raises(ValueError, match='entropy_encode: lengths must be'):
        ops.entropy_encode(q, 3, 4, bytes(4), torch.zeros(384, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), hist)
    with pytest.raises(ValueError, match='entropy_encode: payload must be 384'):
        ops.entropy_encode(q, 3, 4, bytes([4] * 16), torch.zeros(383, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), hist)
    with pytest.raises(ValueError, match='entropy_decode_dequantize: offsets must be'):
        ops.entropy_decode_dequantize(torch.zeros(384, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32), bytes([4] * 16),
                                      torch.zeros(4), torch.zeros(1, 2, 2, 4), 3, 4)
    assert ops.entropy_abi() == 1 and ops.entropy_chunks(546) == 3 and ops.entropy_capacity(546) == 1152


# ------------------------------------------------------------------------------------------ the guard ledger
def test_every_export_of_the_header_has_a_guard_case_or_a_reason():
    loaded = 'hnd_ghnd_object_detectors_amd.ops' in sys.modules
    from tests import test_guard_bands_entropy_gpu as T
    # importing the guard-band module must not touch the GPU: it loads neither the library nor the launch helpers
    assert loaded or 'hnd_ghnd_object_detectors_amd.ops' not in sys.modules
    covered = set().union(*T.LEDGER.values())
    assert covered and all(T.LEDGER.values())
    assert all(isinstance(reason, str) and reason for reason in T.NO_DEVICE_OUTPUT.values())
    assert not covered & set(T.NO_DEVICE_OUTPUT)
    assert covered | set(T.NO_DEVICE_OUTPUT) == set(EXPORTS)
    assert all(callable(getattr(T, name, None)) and name.startswith('test_') for name in T.LEDGER)
