"""CPU: include/hnd_qimage.h (the header through _lib's reader, symbols, version, argument validation), the numpy
restatement of tests/qimage_util.py pinned to the per-image oracle, the constant-image rule, the refusals of the host classes
and of the config section, the link size, the reconstruction property, the guard ledger of
tests/test_guard_bands_qimage_gpu.py, and the preconditions that make the one-step comparison of tests/test_qimage_gpu.py
fair."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import hnd_oracle as O
from tests import golden_util as G
from tests import model_util as MU
from tests import qat_util as QU
from tests import qimage_util as QI
from tests.test_lib_cpu import HEADER_NAMES, _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'hnd_qimage.h')
EXPORTS = ['hnd_qimage_abi', 'hnd_qimage_dequantize_u8', 'hnd_qimage_fake_quantize_bits', 'hnd_qimage_quantize_bits',
           'hnd_qimage_quantize_pack_bits', 'hnd_qimage_scratch_elems', 'hnd_qimage_unpack_dequantize_bits']


@pytest.fixture(scope='module', autouse=True)
def built():
    """the package loads libhnd_hip.so on import (there is no fallback), so it is built first"""
    import __graft_entry__ as g
    g.build()


def bits_of(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------ C ABI
def test_header_parses_and_the_library_exports_what_it_declares():
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    header = _lib.parse_header(open(HEADER).read(), 'hnd_qimage.h')
    assert not header.structs and not header.enums and sorted(header.functions) == EXPORTS
    assert list(_lib.QIMAGE_SYMBOLS) == EXPORTS == _declared('hnd_qimage.h') == sorted(_lib.QIMAGE_HEADER.functions)
    for name in EXPORTS:
        assert getattr(lib, name).argtypes is not None, name
    value = int(re.search(r'#define HND_QIMAGE_ABI (\d+)\b', open(HEADER).read()).group(1))
    assert lib.hnd_qimage_abi() == _lib.QIMAGE_ABI == value == 1
    assert header.defines['HND_QIMAGE_MAX_N'] == _lib.QIMAGE_MAX_N == 65535
    assert header.defines['HND_QIMAGE_PART_BLOCKS'] == _lib.QIMAGE_PART_BLOCKS == 128


def test_no_name_is_in_another_headers_tuple_and_the_other_headers_stand():
    from hnd_ghnd_object_detectors_amd import _lib
    assert tuple(_lib.HEADERS) == HEADER_NAMES
    others = set(_lib.EXPORTED_SYMBOLS) | set(_lib.OPTIM_SYMBOLS) | set(_lib.CODEC_SYMBOLS) | set(_lib.QAT_SYMBOLS) | \
        set(_lib.QRANGE_SYMBOLS) | set(_lib.ENTROPY_SYMBOLS) | set(_lib.QCHANNEL_SYMBOLS)
    assert not others & set(EXPORTS)
    assert [len(h.functions) for h in _lib.HEADERS.values()] == [94, 2, 5, 3]
    assert len(_lib.QRANGE_SYMBOLS) == 7 and len(_lib.QCHANNEL_SYMBOLS) == 7
    lib = _lib.load()
    assert lib.hnd_abi_version() == 12 and lib.hnd_codec_abi() == 1 and lib.hnd_qat_abi() == 1       # (untouched)
    assert lib.hnd_qrange_abi() == 1 and lib.hnd_entropy_abi() == 1 and lib.hnd_qchannel_abi() == 1


def test_scratch_query():
    from hnd_ghnd_object_detectors_amd import _lib, ops
    lib = _lib.load()
    for n in (1, 2, 16, 1000, 65535):
        elems = lib.hnd_qimage_scratch_elems(n)
        assert elems == ops.qimage_scratch_elems(n) == n * _lib.QIMAGE_PART_BLOCKS * 2     # whole partials [n][B][2]
    for bad in (0, -4, 65536):
        assert lib.hnd_qimage_scratch_elems(bad) == 0


def _refusal_calls(lib, p):
    """{export: (call(**overrides), its pointer arguments, its aligned arguments)}: host memory stands in for the device
    pointers, nothing is launched"""
    def quantize(x=p, n=2, hw=4, c=3, cs=4, bits=4, q=p, qparams=p, scratch=p):
        return lib.hnd_qimage_quantize_bits(x, n, hw, c, cs, bits, q, qparams, scratch, None)

    def dequantize(q=p, qparams=p, x=p, n=2, hw=4, c=3, cs=4):
        return lib.hnd_qimage_dequantize_u8(q, qparams, x, n, hw, c, cs, None)

    def pack(x=p, n=2, h=2, w=2, c=3, cs=4, bits=4, payload=p, qparams=p, scratch=p):
        return lib.hnd_qimage_quantize_pack_bits(x, n, h, w, c, cs, bits, payload, qparams, scratch, None)

    def unpack(payload=p, qparams=p, x=p, n=2, h=2, w=2, c=3, cs=4, bits=4):
        return lib.hnd_qimage_unpack_dequantize_bits(payload, qparams, x, n, h, w, c, cs, bits, None)

    def fake(x=p, y=p, n=2, hw=4, c=3, cs=4, bits=4, qparams=p, scratch=p, stats=None):
        return lib.hnd_qimage_fake_quantize_bits(x, y, n, hw, c, cs, bits, qparams, scratch, stats, None)

    return {'hnd_qimage_quantize_bits': (quantize, ('x', 'q', 'qparams', 'scratch'), ('x',), ('q',)),
            'hnd_qimage_dequantize_u8': (dequantize, ('q', 'qparams', 'x'), ('x',), ('q',)),
            'hnd_qimage_quantize_pack_bits': (pack, ('x', 'payload', 'qparams', 'scratch'), ('x',), ()),
            'hnd_qimage_unpack_dequantize_bits': (unpack, ('payload', 'qparams', 'x'), ('x',), ()),
            'hnd_qimage_fake_quantize_bits': (fake, ('x', 'y', 'qparams', 'scratch'), ('x', 'y'), ())}


def check_every_refusal(lib):
    """every refusal of the header comment returns HND_ERR_INVALID (-1) with the export's name in the error string"""
    host = (ctypes.c_double * 64)()
    p = ctypes.addressof(host)
    p += (-p) % 16
    count = 0
    for export, (call, pointers, aligned16, aligned4) in _refusal_calls(lib, p).items():
        def refused(rc):
            return rc == -1 and export.encode() in lib.hnd_last_error_string()
        names = call.__code__.co_varnames
        for name in pointers:
            assert refused(call(**{name: None})), (export, name)
        for name in aligned16:
            assert refused(call(**{name: p + 4})), (export, name, 'misaligned')
        for name in aligned4:
            assert refused(call(**{name: p + 2})), (export, name, 'misaligned')
        if 'bits' in names:
            for bits in (0, 9, -1, 16):
                assert refused(call(bits=bits)), (export, bits)
        for c, cs in ((0, 4), (-3, 4), (5, 4), (3, 5), (3, 6), (3, 7)):                # c <= 0, cs < c, cs % 4
            assert refused(call(c=c, cs=cs)), (export, c, cs)
        for n in (0, -1, 65536):                                                        # n outside 1 ... HND_QIMAGE_MAX_N
            assert refused(call(n=n)), (export, n)
        sizes = [{'hw': 0}, {'hw': -2}, {'hw': 2 ** 62}] if 'hw' in names else [{'h': 0}, {'w': -1}, {'h': -2, 'w': -2}]
        for kw in sizes:
            assert refused(call(**kw)), (export, kw)
        if export == 'hnd_qimage_fake_quantize_bits':                                   # the tile count leaves an int
            assert refused(call(n=65535, hw=2 ** 40, c=1, cs=4)), export
        count += 1
    assert count == 5


def test_every_export_validates_before_any_hip_call():
    from hnd_ghnd_object_detectors_amd import _lib
    check_every_refusal(_lib.load())


# ------------------------------------------------------------------------------------------ restatement vs the oracle
@pytest.mark.parametrize('shape,cs,bits', QI.CASES)
def test_restatement_is_the_per_image_oracle_bit_for_bit(shape, cs, bits):
    """codes, scale, zero point and the dequantised floats on every image of the input table"""
    z = QI.make_input(shape)
    ref, got = QI.oracle(shape, bits), QI.restated(shape, bits)
    assert all(float(z[i].max()) != float(z[i].min()) for i in range(shape[0]))     # (the table has no constant image)
    assert torch.equal(got.codes, ref.codes)
    assert torch.equal(bits_of(got.scale), bits_of(ref.scale)) and torch.equal(got.zero_point, ref.zero_point)
    assert torch.equal(bits_of(got.lo), bits_of(ref.lo)) and torch.equal(bits_of(got.hi), bits_of(ref.hi))
    assert torch.equal(bits_of(got.dequantized), bits_of(ref.dequantized))
    # the ranges differ as the table says: the gain 4^(i mod 4) shows in the scales, so the batch's range fits no image but
    # the widest
    if shape[0] >= 2:
        assert float(ref.scale[1]) > 2 * float(ref.scale[0])
        assert not torch.equal(QI.restate_per_tensor(z, bits), got.dequantized)
    # the payload is hnd_codec.h's: it unpacks to the codes
    assert torch.equal(QI.CU.host_unpack(got.payload, shape, bits), ref.codes)


@pytest.mark.parametrize('bits', [1, 4, 8])
def test_constant_images_reconstruct_exactly(bits):
    z = QI.with_constants((5, 3, 2, 3))
    got = QI.restate(z, bits)
    for i, v, zp, q in zip((0, 1, 4), QI.CONSTANTS, (0.0, 1.0, 0.0), (1, 0, 0)):
        assert torch.equal(bits_of(got.dequantized[i]), bits_of(z[i])), (i, v)
        assert float(got.zero_point[i]) == zp and bool((got.codes[i] == q).all())
        assert float(got.scale[i]) == (abs(v) if v else 1.0) and float(got.lo[i]) == float(got.hi[i]) == v
    # ... and the live images beside them are the oracle's
    live = [2, 3]
    ref = QI.oracle_per_image(z[live], bits)                                # (the oracle cannot take a constant image)
    assert torch.equal(got.codes[live], ref.codes)
    assert torch.equal(bits_of(got.dequantized[live]), bits_of(ref.dequantized))


@pytest.mark.parametrize('bits', QI.RMS_WIDTHS)
def test_per_image_reconstruction_beats_per_tensor_on_the_scaled_input(bits):
    """a property of the seeded input whose images differ in range by 4^i: the batch's step is the widest image's"""
    z = QI.make_input(QI.RMS_SHAPE)
    per_image = QI.rms_error(z, QI.restated(QI.RMS_SHAPE, bits).dequantized)
    per_tensor = QI.rms_error(z, QI.restate_per_tensor(z, bits))
    print('\n[%d bits] RMS error per image %.4e, per tensor %.4e, ratio %.3f' % (bits, per_image, per_tensor,
                                                                               per_image / per_tensor))
    assert per_image < per_tensor


def test_restated_stats_order_adds_every_row_once_and_the_fused_step_rounds_once():
    y = torch.randn(130, 8, generator=torch.Generator().manual_seed(3))
    st = QI.restate_stats(y, 8)
    assert tuple(st.shape) == (2, 2, 8)
    assert np.allclose(st[:, 0].sum(0).numpy(), y.sum(0).numpy(), rtol=1e-5, atol=1e-5)
    assert np.allclose(st[:, 1].sum(0).numpy(), (y * y).sum(0).numpy(), rtol=1e-5)
    # fma32 against exact rational arithmetic rounded once
    from fractions import Fraction
    g = torch.Generator().manual_seed(5)
    v, acc = torch.randn(2000, generator=g).numpy(), (torch.randn(2000, generator=g) * 3).abs().numpy()
    got = QI.fma32(v, acc)
    rounded_twice = 0
    for a, b, r in zip(v, acc, got):
        exact = Fraction(float(a)) ** 2 + Fraction(float(b))
        lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
        assert abs(Fraction(float(r)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
        rounded_twice += int(np.float32(a * a) + b != r)
    assert rounded_twice > 0                                                 # (the fused step is not the rounded product)


# ------------------------------------------------------------------------------------------ host classes and config
def test_constructors_take_the_keyword_and_refuse_by_name():
    import inspect
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    for bits in range(1, 9):
        assert T.Quantizer(bits, per_image=True).per_image and T.FakeQuantizer(bits, per_image=True).per_image
        assert T.Quantizer(bits, packed=True, per_image=True).packed
    assert not T.Quantizer(4).per_image and not T.FakeQuantizer(4).per_image                # the default is what it was
    assert not T.Quantizer(4, per_channel=True).per_image and T.Quantizer(4, per_channel=True).per_channel
    assert list(inspect.signature(T.Quantizer.__init__).parameters) == ['self', 'num_bits', 'packed', 'static_range',
                                                                       'entropy', 'code_lengths']
    with pytest.raises(ValueError, match=r'Quantizer\(per_image=True, per_channel=True\)'):
        T.Quantizer(4, per_image=True, per_channel=True)
    with pytest.raises(ValueError, match=r'FakeQuantizer\(per_image=True, per_channel=True\)'):
        T.FakeQuantizer(4, per_image=True, per_channel=True)
    with pytest.raises(ValueError, match=r'Quantizer\(per_image=True, entropy=True\)'):
        T.Quantizer(4, entropy=True, per_image=True)
    for rng in ([-1.0, 1.0], 'trained'):
        with pytest.raises(ValueError, match=r'Quantizer\(per_image=True, static_range='):
            T.Quantizer(4, static_range=rng, per_image=True)
        with pytest.raises(ValueError, match=r'FakeQuantizer\(per_image=True, static_range='):
            T.FakeQuantizer(4, static_range=rng, per_image=True)
    with pytest.raises(ValueError, match=r'Quantizer\(num_bits=16, per_image=True\)'):
        T.Quantizer(16, per_image=True)
    with pytest.raises(ValueError, match=r'JpegCompressor\(per_image=True\)'):
        T.JpegCompressor(per_image=True)
    for bad in (1, 0, 'true', None):
        with pytest.raises(ValueError, match='Quantizer: per_image=.*must be a bool'):
            T.Quantizer(4, per_image=bad)
        with pytest.raises(ValueError, match='FakeQuantizer: per_image=.*must be a bool'):
            T.FakeQuantizer(4, per_image=bad)
        with pytest.raises(ValueError, match='JpegCompressor: per_image=.*must be a bool'):
            T.JpegCompressor(per_image=bad)
    # the registry passes the key through (yaml quantizer.params: {num_bits: b, per_image: true})
    tr = T.get_bottleneck_transformer({'order': ['quantizer', 'dequantizer'], 'components': {
        'quantizer': {'params': {'num_bits': 3, 'per_image': True, 'packed': True}},
        'dequantizer': {'params': {'num_bits': 3}}}})
    assert tr.transforms[0].per_image and tr.transforms[0].packed and tr.transforms[0].num_bits == 3
    tr = T.get_bottleneck_transformer({'order': ['fake_quantizer'], 'components': {
        'fake_quantizer': {'params': {'num_bits': 2, 'per_image': True}}}})
    assert tr.transforms[0].per_image


def test_dequantizer_refuses_another_width_and_link_bytes_count_the_images():
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    qp = torch.zeros(2, 4)
    qt = T.QuantizedTensor(torch.zeros(2, 3, 2, 2, dtype=torch.uint8), qp[:, 2], qp[:, 3], qp, channels=3,
                           per_image=True, num_bits=3)
    assert qt.per_image and not qt.per_channel
    with pytest.raises(ValueError, match=r'Dequantizer\(num_bits=4\).*per-image.*3 bits'):
        T.Dequantizer(4)(qt, None)
    payload = torch.zeros(9, dtype=torch.uint8)                              # 24 values at 3 bits
    pb = T.PackedBottleneck(payload, (2, 3, 2, 2), 3, qp, per_image=True)
    assert pb.per_image and not pb.per_channel and tuple(pb.scale.shape) == tuple(pb.zero_point.shape) == (2,)
    assert pb.link_bytes == 9 + 8 * 2
    with pytest.raises(ValueError, match=r'Dequantizer\(num_bits=4\).*packed at 3 bits'):
        T.Dequantizer(4)(pb, None)
    flat = T.PackedBottleneck(payload, (2, 3, 2, 2), 3, torch.zeros(4))
    assert not flat.per_image and flat.scale.dim() == 0 and flat.link_bytes == 9 + 8
    per_channel = T.PackedBottleneck(payload, (2, 3, 2, 2), 3, torch.zeros(3, 4), per_channel=True)
    assert per_channel.link_bytes == 9 + 8 * 3                               # (what it was)
    with pytest.raises(ValueError, match=r'PackedBottleneck\(per_channel=True, per_image=True\)'):
        T.PackedBottleneck(payload, (2, 3, 2, 2), 3, qp, per_channel=True, per_image=True)


def test_ops_wrappers_refuse_by_name():
    from hnd_ghnd_object_detectors_amd import ops
    x = torch.zeros(2, 2, 2, 4)
    q = torch.zeros(2, 2, 2, 4, dtype=torch.uint8)
    qp, scratch = torch.zeros(2, 4), torch.zeros(ops.qimage_scratch_elems(2))
    for bits in (0, 9, 16, True, 4.0):
        with pytest.raises(ValueError, match='qimage_quantize_bits.*outside 1 ... 8'):
            ops.qimage_quantize_bits(x, 3, bits, q, qp, scratch)
        with pytest.raises(ValueError, match='qimage_fake_quantize_bits.*outside 1 ... 8'):
            ops.qimage_fake_quantize_bits(x, 3, bits, qp, scratch)
    with pytest.raises(ValueError, match='qimage_quantize_bits: c=5'):
        ops.qimage_quantize_bits(x, 5, 4, q, qp, scratch)
    with pytest.raises(ValueError, match=r'qimage_quantize_bits: needs a contiguous float32 NHWC buffer \[N, H, W, cs\]'):
        ops.qimage_quantize_bits(x.view(8, 4), 3, 4, q, qp, scratch)
    with pytest.raises(ValueError, match=r'qimage_quantize_bits: qparams.*\[2, 4\]'):
        ops.qimage_quantize_bits(x, 3, 4, q, torch.zeros(4), scratch)
    with pytest.raises(ValueError, match=r'qimage_dequantize_u8: qparams.*\[2, 4\]'):
        ops.qimage_dequantize_u8(q, torch.zeros(3, 4), x, 3)
    with pytest.raises(ValueError, match='qimage_fake_quantize_bits: scratch'):
        ops.qimage_fake_quantize_bits(x, 3, 4, qp, torch.zeros(8))
    with pytest.raises(ValueError, match='qimage_fake_quantize_bits: stats'):
        ops.qimage_fake_quantize_bits(x, 3, 4, qp, scratch, stats=torch.zeros(3))
    with pytest.raises(ValueError, match='qimage_fake_quantize_bits: out must'):
        ops.qimage_fake_quantize_bits(x, 3, 4, qp, scratch, out=torch.zeros(3))
    with pytest.raises(ValueError, match='qimage_quantize_pack_bits: payload'):
        ops.qimage_quantize_pack_bits(x, 3, 4, torch.zeros(5, dtype=torch.uint8), qp, scratch)
    with pytest.raises(ValueError, match='qimage_unpack_dequantize_bits: payload'):
        ops.qimage_unpack_dequantize_bits(torch.zeros(7, dtype=torch.uint8), qp, x, 3, 4)
    with pytest.raises(ValueError, match='qimage_dequantize_u8: q must'):
        ops.qimage_dequantize_u8(torch.zeros(3, dtype=torch.uint8), qp, x, 3)


def _plain(o):
    if isinstance(o, dict):
        return {k: _plain(v) for k, v in o.items()}
    return [_plain(v) for v in o] if isinstance(o, (list, tuple)) else o


def test_config_key_round_trips_and_is_refused_with_the_ema_range_and_per_channel(tmp_path):
    import yaml
    from hnd_ghnd_object_detectors_amd import configs
    from hnd_ghnd_object_detectors_amd.myutils.common import yaml_util
    from hnd_ghnd_object_detectors_amd.utils import main_util
    cfg = configs.make_config('faster_rcnn', 'ghnd', 6, fake_quantize_bits=4, fake_quantize_per_image=True)
    assert cfg['train']['fake_quantize'] == {'num_bits': 4, 'per_image': True}
    assert configs.fake_quantize_per_image_of(cfg) is True and configs.fake_quantize_bits_of(cfg) == 4
    assert configs.fake_quantize_range_of(cfg) is None and configs.fake_quantize_per_channel_of(cfg) is False
    path = tmp_path / 'c.yaml'
    with open(path, 'w') as fp:
        yaml.safe_dump(_plain(cfg), fp, sort_keys=False, default_flow_style=None)
    loaded = yaml_util.load_yaml_file(str(path))
    assert loaded == _plain(cfg) and configs.fake_quantize_per_image_of(loaded) is True
    # without the key: what it was
    base = _plain(configs.make_config('faster_rcnn', 'ghnd', 3, fake_quantize_bits=4))
    assert base['train']['fake_quantize'] == {'num_bits': 4} and configs.fake_quantize_per_image_of(base) is False
    assert configs.fake_quantize_per_image_of(_plain(configs.make_config())) is False
    per_channel = configs.make_config(fake_quantize_bits=4, fake_quantize_per_channel=True)
    assert per_channel['train']['fake_quantize'] == {'num_bits': 4, 'per_channel': True}
    assert configs.fake_quantize_per_image_of(per_channel) is False
    # --json, as mimic_runner.main applies it
    main_util.overwrite_config(base, json.dumps({'train': {'fake_quantize': {'num_bits': 2, 'per_image': True}}}))
    assert configs.fake_quantize_per_image_of(base) is True and configs.fake_quantize_bits_of(base) == 2
    # with range: batch it is allowed; with range: ema or per_channel refused by name, through make_config and the section
    ok = configs.make_config(fake_quantize_bits=4, fake_quantize_range={'type': 'batch'}, fake_quantize_per_image=True)
    assert configs.fake_quantize_per_image_of(ok) is True
    with pytest.raises(ValueError, match='per_image together with range: {type: ema}'):
        configs.make_config(fake_quantize_bits=4, fake_quantize_range={'type': 'ema'}, fake_quantize_per_image=True)
    with pytest.raises(ValueError, match='per_image together with per_channel'):
        configs.make_config(fake_quantize_bits=4, fake_quantize_per_channel=True, fake_quantize_per_image=True)
    base['train']['fake_quantize']['range'] = {'type': 'ema', 'momentum': 0.1}
    with pytest.raises(ValueError, match='per_image together with range: {type: ema}'):
        configs.fake_quantize_range_of(base)
    for bad in (1, 0, 'true', None):
        cfg = configs.make_config(fake_quantize_bits=4)
        cfg['train']['fake_quantize']['per_image'] = bad
        with pytest.raises(ValueError, match='fake_quantize.per_image=.*must be a bool'):
            configs.fake_quantize_per_image_of(cfg)
    with pytest.raises(ValueError, match='num_bits'):
        configs.make_config(fake_quantize_per_image=True)


def test_layer_attribute_defaults_to_off_and_refuses_the_fixed_range_and_per_channel():
    import inspect
    from hnd_ghnd_object_detectors_amd import engine as E
    from hnd_ghnd_object_detectors_amd.models.mimic.resnet_layer import Bottleneck4LargeResNet
    layer = Bottleneck4LargeResNet(6, None, None)
    assert layer.train_fake_quant_per_image is False
    layer.train_fake_quant_bits, layer.train_fake_quant_per_image = 4, True
    assert layer.fake_quant_bits_checked() == 4
    layer.train_fake_quant_per_image = 1
    with pytest.raises(ValueError, match='train_fake_quant_per_image.*must be a bool'):
        layer.fake_quant_bits_checked()
    layer.train_fake_quant_per_image = True
    layer.train_fake_quant_per_channel = True
    with pytest.raises(ValueError, match='train_fake_quant_per_image together with train_fake_quant_per_channel'):
        layer.fake_quant_bits_checked()
    layer.train_fake_quant_per_channel = False
    layer.train_fake_quant_range = {'momentum': 0.1, 'frozen': False}
    with pytest.raises(ValueError, match='train_fake_quant_per_image together with train_fake_quant_range'):
        layer.fake_quant_bits_checked()
    layer.train_fake_quant_range = None
    assert layer.fake_quant_bits_checked() == 4
    assert inspect.signature(E.HeadEngine.forward).parameters['fake_quant_per_image'].default is False


def test_split_model_entry_exists_and_the_old_ones_keep_their_signatures():
    import inspect
    from hnd_ghnd_object_detectors_amd.models.mimic import split_rcnn as S
    assert list(inspect.signature(S.split_rcnn_model).parameters) == ['model', 'quantization', 'packed']
    assert list(inspect.signature(S.split_rcnn_model_per_channel).parameters) == ['model', 'num_bits', 'packed']
    assert list(inspect.signature(S.split_rcnn_model_per_image).parameters) == ['model', 'num_bits', 'packed']
    with pytest.raises(ValueError, match='split_rcnn_model_per_image needs a quantization width'):
        S.split_rcnn_model_per_image(None, None)


# ------------------------------------------------------------------------------------------ the guard ledger
def test_every_export_that_writes_device_memory_has_a_guard_case():
    loaded = 'hnd_ghnd_object_detectors_amd.ops' in sys.modules
    from tests import test_guard_bands_qimage_gpu as T
    assert loaded or 'hnd_ghnd_object_detectors_amd.ops' not in sys.modules     # importing it does not touch the GPU
    declared = set(_declared('hnd_qimage.h'))
    covered = set().union(*T.LEDGER.values())
    assert covered and all(T.LEDGER.values())
    assert all(isinstance(reason, str) and reason for reason in T.NO_DEVICE_OUTPUT.values())
    assert not covered & set(T.NO_DEVICE_OUTPUT), sorted(covered & set(T.NO_DEVICE_OUTPUT))
    everything = covered | set(T.NO_DEVICE_OUTPUT)
    assert everything == declared == set(EXPORTS), (sorted(declared - everything), sorted(everything - declared))
    assert set(T.NO_DEVICE_OUTPUT) == {'hnd_qimage_abi', 'hnd_qimage_scratch_elems'}                # queries only
    assert all(callable(getattr(T, name, None)) and name.startswith('test_') for name in T.LEDGER)


# ------------------------------------------------------------------------------------------ the one-step preconditions
def _oracles(name):
    z, meta = G.load(name)
    cfg = MU.config_for(meta)
    t_sd, s_sd = MU.oracle_states(meta['seed'], meta['model'], meta.get('bch', 3), meta.get('num_classes', 91))
    ms = meta['min_size'] if isinstance(meta['min_size'], list) else [meta['min_size']]
    kw = dict(terms=MU.terms_of(cfg), min_size=tuple(ms), max_size=meta['max_size'])
    images, _ = G.case_inputs(meta)
    return t_sd, s_sd, kw, images


def test_one_step_cases_are_at_least_two_with_a_low_width():
    assert len(QI.ONE_STEP_CASES) >= 2 and len(set(QI.ONE_STEP_CASES)) == len(QI.ONE_STEP_CASES)
    assert any(bits <= 3 for _, bits in QI.ONE_STEP_CASES)
    assert all(name in QI.SCAN_FIXTURES and 1 <= bits <= 8 for name, bits in QI.ONE_STEP_CASES)
    assert set(QI.ONE_STEP_MARGINS) == set(QI.ONE_STEP_CASES)


@pytest.mark.parametrize('name,bits', QI.ONE_STEP_CASES)
def test_oracle_alone_meets_the_preconditions_of_the_one_step_comparison(name, bits, monkeypatch):
    """per image, the fp32 and the fp64 oracle take the same rounding decisions on the bottleneck tensor from the fixture's
    initial state, every decision keeps qat_util.MARGIN code units from its tie, the two images' qparams differ, and the
    margins are the listed ones"""
    t_sd, s_sd, kw, images = _oracles(name)
    capture = {}

    def fq(z):
        capture[z.dtype] = QI.decide_codes_per_image(z.detach(), bits)
        return QI.ste_per_image(z, bits)
    monkeypatch.setattr(O, 'student_layer1', QU.make_student_layer1(bits, fake_quant=fq))
    O.DistillOracle(t_sd, s_sd, dtype=torch.float64, **kw).forward(images)
    O.DistillOracle(t_sd, s_sd, **kw).forward(images)
    caps32, caps64 = capture[torch.float32], capture[torch.float64]
    assert len(caps64) == 2
    half, zp = QI.check_preconditions_per_image(caps32, caps64, '%s at %d bits' % (name, bits))
    assert QI.qparams_differ(caps32) and QI.qparams_differ(caps64)
    print('\n[%s, %d bits, per image] %d images; nearest tie %.2e code units, nearest integer of -min/scale %.2e'
          % (name, bits, len(caps32), half, zp))
    listed = QI.ONE_STEP_MARGINS[(name, bits)]
    assert abs(half - listed[0]) <= 0.05 * listed[0] and abs(zp - listed[1]) <= 0.05 * listed[1], (half, zp, listed)
    assert all(len(torch.unique(c['codes'])) > 1 for c in caps64)           # the quantiser is at work on every image
