"""CPU: include/hnd_codec.h (symbols, version, the packed size, argument validation), the guard ledger of that header
(tests/test_guard_bands_codec_gpu.py), the construction rules of Quantizer / Dequantizer at 1 ... 8 and 16 bits, and the
oracle against the reference-made fixture tests/golden/tiny_codec_bits.npz."""
import ctypes
import os
import re
import sys

import pytest
import torch

from tests import golden_util as G
from tests.test_lib_cpu import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_EXPORTS = ('hnd_quantize_bits', 'hnd_quantize_pack_bits', 'hnd_unpack_dequantize_bits')


@pytest.fixture(scope='module', autouse=True)
def built():
    """the package loads libhnd_hip.so on import (there is no fallback), so it is built first"""
    import __graft_entry__ as g
    g.build()


# ------------------------------------------------------------------------------------------ C ABI
def test_codec_symbols_resolve_and_stay_out_of_the_main_table():
    """(that no header's names are in another's tuple: tests/test_lib_cpu.py, over all four headers)"""
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    assert list(_lib.CODEC_SYMBOLS) == sorted(('hnd_codec_abi', 'hnd_codec_packed_bytes') + DEVICE_EXPORTS)
    for name in _lib.CODEC_SYMBOLS:
        assert getattr(lib, name).argtypes is not None
    assert lib.hnd_codec_abi() == _lib.CODEC_ABI == 1
    assert lib.hnd_abi_version() == _lib.ABI_VERSION == 12              # (untouched)
    assert re.search(r'#define HND_CODEC_ABI 1\b', open(os.path.join(ROOT, 'include', 'hnd_codec.h')).read())


@pytest.mark.parametrize('numel', [1, 3, 7, 8, 9, 105, 2 ** 33 + 5])
def test_packed_bytes_is_the_ceiling_of_numel_times_bits_over_eight(numel):
    from hnd_ghnd_object_detectors_amd import _lib, ops
    lib = _lib.load()
    for bits in range(1, 9):
        assert lib.hnd_codec_packed_bytes(numel, bits) == (numel * bits + 7) // 8 == ops.codec_packed_bytes(numel, bits)
    for bits in (0, 9):
        assert lib.hnd_codec_packed_bytes(numel, bits) == 0
    for bad in (0, -1, -numel):
        assert lib.hnd_codec_packed_bytes(bad, 4) == 0


def test_codec_entry_points_validate_before_any_hip_call():
    """every refusal of the header comment returns HND_ERR_INVALID (-1) with the export's name in the error string; nothing
    is launched, so host memory stands in for the device pointers"""
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    host = (ctypes.c_double * 64)()
    p = ctypes.addressof(host)

    def quantize(x=p, npix=4, c=3, cs=4, bits=4, q=p, qparams=p, scratch=p):
        return 'hnd_quantize_bits', lib.hnd_quantize_bits(x, npix, c, cs, bits, q, qparams, scratch, None)

    def pack(x=p, n=1, h=2, w=2, c=3, cs=4, bits=4, payload=p, qparams=p, scratch=p):
        return 'hnd_quantize_pack_bits', lib.hnd_quantize_pack_bits(x, n, h, w, c, cs, bits, payload, qparams, scratch, None)

    def unpack(payload=p, qparams=p, x=p, n=1, h=2, w=2, c=3, cs=4, bits=4):
        return 'hnd_unpack_dequantize_bits', lib.hnd_unpack_dequantize_bits(payload, qparams, x, n, h, w, c, cs, bits, None)

    def refused(result):
        name, rc = result
        return rc == -1 and name.encode() in lib.hnd_last_error_string()

    for call, pointers, extents in ((quantize, ('x', 'q', 'qparams', 'scratch'), ('npix',)),
                                    (pack, ('x', 'payload', 'qparams', 'scratch'), ('n', 'h', 'w')),
                                    (unpack, ('payload', 'qparams', 'x'), ('n', 'h', 'w'))):
        for name in pointers:
            assert refused(call(**{name: None})), (call.__name__, name)
        for bits in (0, 9, -1, 16):
            assert refused(call(bits=bits)), (call.__name__, bits)
        for c in (0, -3):
            assert refused(call(c=c)), (call.__name__, c)
        assert refused(call(c=3, cs=2)), call.__name__                   # cs < c
        for name in extents:
            for bad in (0, -2):
                assert refused(call(**{name: bad})), (call.__name__, name, bad)


# ------------------------------------------------------------------------------------------ the guard ledger of hnd_codec.h
def test_every_codec_export_that_writes_device_memory_has_a_guard_case():
    """the rule of tests/test_guard_ledger_cpu.py for include/hnd_codec.h: no export without a guard case"""
    from hnd_ghnd_object_detectors_amd import _lib
    loaded = 'hnd_ghnd_object_detectors_amd.ops' in sys.modules
    from tests import test_guard_bands_codec_gpu as T
    assert loaded or 'hnd_ghnd_object_detectors_amd.ops' not in sys.modules      # importing it does not touch the GPU
    covered = set().union(*T.LEDGER.values())
    assert covered == set(DEVICE_EXPORTS) and all(T.LEDGER.values())
    assert all(isinstance(reason, str) and reason for reason in T.NO_DEVICE_OUTPUT.values())
    assert set(T.NO_DEVICE_OUTPUT) == {'hnd_codec_abi', 'hnd_codec_packed_bytes'}
    assert not covered & set(T.NO_DEVICE_OUTPUT)
    assert covered | set(T.NO_DEVICE_OUTPUT) == set(_lib.CODEC_SYMBOLS) == set(_declared('hnd_codec.h'))
    assert all(callable(getattr(T, name, None)) and name.startswith('test_') for name in T.LEDGER)


# ------------------------------------------------------------------------------------------ host classes
def test_quantizer_builds_at_every_width_the_reference_byte_tensor_holds():
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    for bits in range(1, 9):
        q, p = T.Quantizer(bits), T.Quantizer(bits, packed=True)
        assert (q.num_bits, q.packed, p.num_bits, p.packed) == (bits, False, bits, True)
        assert T.Dequantizer(bits).num_bits == bits
    assert T.Quantizer().num_bits == 8 and not T.Quantizer().packed and T.Quantizer(16).num_bits == 16


@pytest.mark.parametrize('args', [(0,), (9,), (12,), (16, True)])
def test_unsupported_widths_are_refused_by_name_with_the_supported_list(args):
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    with pytest.raises(NotImplementedError) as err:
        T.Quantizer(*args)
    msg = str(err.value)
    assert 'Quantizer' in msg and 'num_bits=%d' % args[0] in msg and '[1, 2, 3, 4, 5, 6, 7, 8, 16]' in msg
    assert len(args) == 1 or 'packed' in msg


def test_yaml_section_with_four_packed_bits_builds():
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    tr = T.get_bottleneck_transformer({'order': ['quantizer', 'dequantizer'], 'components': {
        'quantizer': {'params': {'num_bits': 4, 'packed': True}}, 'dequantizer': {'params': {'num_bits': 4}}}})
    quantizer, dequantizer = tr.transforms
    assert isinstance(quantizer, T.Quantizer) and (quantizer.num_bits, quantizer.packed) == (4, True)
    assert isinstance(dequantizer, T.Dequantizer) and dequantizer.num_bits == 4


def test_split_takes_the_width_and_the_packed_flag():
    """the reference's two arguments first, `packed` after them and off by default (the split itself runs on the GPU:
    tests/test_codec_bits_gpu.py)"""
    import inspect
    from hnd_ghnd_object_detectors_amd.models.mimic import split_rcnn
    sig = inspect.signature(split_rcnn.split_rcnn_model)
    assert list(sig.parameters) == ['model', 'quantization', 'packed'] and sig.parameters['packed'].default is False


# ------------------------------------------------------------------------------------------ oracle vs the reference-made fixture
@pytest.mark.parametrize('bits', range(1, 8))
def test_oracle_reproduces_the_reference_at_every_width(bits):
    """oracle/myutils_r.quantize_tensor(z, b) on the reference's own bottleneck tensor gives the bytes, scale, zero point
    and dequantised floats the reference's Quantizer(b) / Dequantizer(b) produced (tests/golden/make_golden_codec_bits.py)"""
    from oracle.myutils_r import dequantize_tensor, quantize_tensor
    fix = G.load_raw('tiny_codec_bits')
    assert bool(fix['oracle_vs_reference_equal'])
    z = torch.from_numpy(G.load_raw('tiny_eval_quantized')['quantized/z'])
    q = quantize_tensor(z.clone(), bits)
    assert torch.equal(q.tensor, torch.from_numpy(fix['b%d/bytes' % bits]))
    assert float(q.scale) == float(fix['b%d/scale' % bits]) and float(q.zero_point) == float(fix['b%d/zero_point' % bits])
    assert torch.equal(dequantize_tensor(q), torch.from_numpy(fix['b%d/dequantized' % bits]))


def test_host_pack_restates_the_payload_format_of_the_header():
    """tests/codec_util.host_pack, the reference of the GPU byte tests, against the header's rule spelt out value by value:
    value i occupies bits [i * bits, (i + 1) * bits) of the stream, bit k of the stream is bit k % 8 of byte k // 8"""
    from tests import codec_util as CU
    g = torch.Generator().manual_seed(5)
    for bits in range(1, 9):
        for numel in (1, 3, 8, 13):
            v = torch.randint(0, 1 << bits, (numel,), generator=g).to(torch.uint8)
            expect = bytearray((numel * bits + 7) // 8)
            for i, val in enumerate(v.tolist()):
                for j in range(bits):
                    if (val >> j) & 1:
                        k = i * bits + j
                        expect[k // 8] |= 1 << (k % 8)
            packed = CU.host_pack(v, bits)
            assert packed.tobytes() == bytes(expect), (bits, numel)
            assert torch.equal(CU.host_unpack(packed, (numel,), bits), v)
