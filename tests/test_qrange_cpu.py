"""CPU: include/hnd_qrange.h (symbols, version, argument validation), the config plumbing of train.fake_quantize.range, the
host classes' refusals, the layer attribute, and the preconditions that make the GPU one-step comparison of
tests/test_qrange_gpu.py fair: on every (fixture, width, lo, hi) case the fp32 and the fp64 oracle with the clipped
straight-through estimator of tests/qrange_util.py take the same code and the same pass decision for every element, none
within qat_util.MARGIN of a half-integer, with both ends of the range really clipping."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
import yaml

from oracle import hnd_oracle as O
from tests import golden_util as G
from tests import model_util as MU
from tests import qat_util as QU
from tests import qrange_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'hnd_qrange.h')
EXPORTS = ['hnd_fake_quantize_range', 'hnd_qrange_abi', 'hnd_qrange_mask_grad', 'hnd_qrange_observe', 'hnd_qrange_qparams',
           'hnd_quantize_pack_range_bits', 'hnd_quantize_range_bits']


@pytest.fixture(scope='module', autouse=True)
def built():
    """the package loads libhnd_hip.so on import (there is no fallback), so it is built first"""
    import __graft_entry__ as g
    g.build()


# ------------------------------------------------------------------------------------------ C ABI
def test_qrange_symbols_resolve_and_the_other_tables_do_not_move():
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    assert list(_lib.QRANGE_SYMBOLS) == EXPORTS == sorted(_lib.QRANGE_HEADER.functions)
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r'\b(hnd_[a-z0-9_]+)\s*\(', text))) == EXPORTS      # (found without the reader of _lib.py)
    for name in EXPORTS:
        assert getattr(lib, name).argtypes is not None
    value = int(re.search(r'#define HND_QRANGE_ABI (\d+)\b', open(HEADER).read()).group(1))
    assert lib.hnd_qrange_abi() == _lib.QRANGE_ABI == value == 1
    assert not _lib.QRANGE_HEADER.structs and not _lib.QRANGE_HEADER.enums
    # the four pinned headers, their tuples and their versions
    assert tuple(_lib.HEADERS) == ('hnd_hip.h', 'hnd_optim.h', 'hnd_codec.h', 'hnd_qat.h')
    tuples = (_lib.EXPORTED_SYMBOLS, _lib.OPTIM_SYMBOLS, _lib.CODEC_SYMBOLS, _lib.QAT_SYMBOLS)
    assert [len(t) for t in tuples] == [94, 2, 5, 3]
    assert not set(EXPORTS) & {n for t in tuples for n in t}
    assert lib.hnd_abi_version() == _lib.ABI_VERSION == 12 and lib.hnd_codec_abi() == _lib.CODEC_ABI == 1
    assert lib.hnd_qat_abi() == _lib.QAT_ABI == 1


def _host():
    host = (ctypes.c_double * 64)()
    addr = ctypes.addressof(host)
    return host, addr + (-addr) % 16          # 16-byte aligned host memory standing in for the device pointers


def _refusals(lib, name, call, pointers, aligned, geometry=True, npix_name='npix'):
    """the refusals every export with a buffer geometry shares"""
    def refused(rc):
        return rc == -1 and name.encode() in lib.hnd_last_error_string()

    for ptr in pointers:
        assert refused(call(**{ptr: None})), (name, ptr)
    for ptr in aligned:
        assert refused(call(**{ptr: call.p + 4})), (name, ptr, 'alignment')
    if 'bits' in call.__code__.co_varnames:
        for bits in (0, 9, -1, 16):
            assert refused(call(bits=bits)), (name, bits)
    if geometry:
        for c in (0, -3):
            assert refused(call(c=c)), (name, c)
        assert refused(call(c=5, cs=4)), name                              # cs < c
        for cs in (5, 6, 7):
            assert refused(call(c=3, cs=cs)), (name, cs)                   # cs % 4 != 0
        for npix in (0, -2):
            assert refused(call(**{npix_name: npix})), (name, npix)
    return refused


def test_every_export_validates_before_any_hip_call():
    """every refusal of the header comment returns HND_ERR_INVALID (-1) with the export's name in the error string; nothing
    is launched, so host memory stands in for the device pointers"""
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    host, p = _host()

    def observe(x=p, npix=4, c=3, cs=4, momentum=0.1, bits=4, state=p, qparams=p, scratch=p):
        return lib.hnd_qrange_observe(x, npix, c, cs, momentum, bits, state, qparams, scratch, None)
    observe.p = p
    refused = _refusals(lib, 'hnd_qrange_observe', observe, ('x', 'state', 'qparams', 'scratch'), ('x', 'state', 'qparams'))
    for m in (0.0, -0.1, 1.5, float('nan')):
        assert refused(observe(momentum=m)), m

    def qparams(lo=-1.0, hi=1.0, bits=4, qparams=p):
        return lib.hnd_qrange_qparams(lo, hi, bits, qparams, None)
    qparams.p = p
    refused = _refusals(lib, 'hnd_qrange_qparams', qparams, ('qparams',), ('qparams',), geometry=False)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float('nan'), 1.0), (0.0, float('nan')), (float('-inf'), 1.0), (0.0, float('inf'))):
        assert refused(qparams(lo=lo, hi=hi)), (lo, hi)

    def fake(x=p, y=p, npix=4, c=3, cs=4, bits=4, qparams=p, mask=None, stats=None):
        return lib.hnd_fake_quantize_range(x, y, npix, c, cs, bits, qparams, mask, stats, None)
    fake.p = p
    _refusals(lib, 'hnd_fake_quantize_range', fake, ('x', 'y', 'qparams'), ('x', 'y', 'qparams'))

    def mask_grad(g=p, mask=p, npix=4, c=3, cs=4):
        return lib.hnd_qrange_mask_grad(g, mask, npix, c, cs, None)
    mask_grad.p = p
    _refusals(lib, 'hnd_qrange_mask_grad', mask_grad, ('g', 'mask'), ('g',))

    def quantize(x=p, npix=4, c=3, cs=4, bits=4, q=p, qparams=p):
        return lib.hnd_quantize_range_bits(x, npix, c, cs, bits, q, qparams, None)
    quantize.p = p
    _refusals(lib, 'hnd_quantize_range_bits', quantize, ('x', 'q', 'qparams'), ('x', 'qparams'))

    def pack(x=p, n=1, h=2, w=2, c=3, cs=4, bits=4, payload=p, qparams=p):
        return lib.hnd_quantize_pack_range_bits(x, n, h, w, c, cs, bits, payload, qparams, None)
    pack.p = p
    refused = _refusals(lib, 'hnd_quantize_pack_range_bits', pack, ('x', 'payload', 'qparams'), ('x', 'qparams'), npix_name='n')
    for dim in ('h', 'w'):
        assert refused(pack(**{dim: 0})), dim
    assert all(v == 0.0 for v in host)                                    # nothing wrote the stand-in memory


def test_ops_wrappers_refuse_by_name():
    from hnd_ghnd_object_detectors_amd import ops
    x = torch.zeros(1, 1, 1, 4)
    qp = torch.zeros(4)
    for bits in (0, 9, 16, True, 4.0):
        for name, call in (('qrange_observe', lambda b: ops.qrange_observe(x, 3, b, 0.1, qp, qp, qp)),
                           ('qrange_qparams', lambda b: ops.qrange_qparams(0.0, 1.0, b, qp)),
                           ('fake_quantize_range', lambda b: ops.fake_quantize_range(x, 3, b, qp)),
                           ('quantize_range_bits', lambda b: ops.quantize_range_bits(x, 3, b, None, qp)),
                           ('quantize_pack_range_bits', lambda b: ops.quantize_pack_range_bits(x, 3, b, None, qp))):
            with pytest.raises(ValueError, match=name + '.*outside 1 ... 8'):
                call(bits)
    for c in (0, 5, True):
        with pytest.raises(ValueError, match='fake_quantize_range: c='):
            ops.fake_quantize_range(x, c, 4, qp)
        with pytest.raises(ValueError, match='qrange_mask_grad: c='):
            ops.qrange_mask_grad(x, torch.zeros(1, dtype=torch.uint8), c)
    with pytest.raises(ValueError, match='fake_quantize_range: c='):
        ops.fake_quantize_range(torch.zeros(1, 1, 1, 6), 3, 4, qp)       # a stride that is no multiple of 4
    with pytest.raises(ValueError, match='fake_quantize_range: mask'):
        ops.fake_quantize_range(x, 3, 4, qp, mask=torch.zeros(2, dtype=torch.uint8))
    with pytest.raises(ValueError, match='qrange_mask_grad: mask'):
        ops.qrange_mask_grad(x, torch.zeros(1, dtype=torch.float32), 3)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float('nan'), 1.0), (0.0, float('inf')), ('a', 1.0)):
        with pytest.raises(ValueError, match='qrange_qparams: the range'):
            ops.qrange_qparams(lo, hi, 4, qp)
    for m in (0, -1.0, 1.5, True):
        with pytest.raises(ValueError, match='qrange_observe: momentum'):
            ops.qrange_observe(x, 3, 4, m, qp, qp, qp)
    assert ops.qrange_abi() == 1 and ops.qrange_mask_shape(torch.zeros(2, 3, 5, 8)) == (2, 3, 5, 2)


# ------------------------------------------------------------------------------------------ host classes
def test_static_range_of_the_quantisers_is_checked_at_construction():
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    for cls in (T.Quantizer, T.FakeQuantizer):
        assert cls(4).static_range is None
        assert cls(4, static_range=[-1, 2.5]).static_range == (-1.0, 2.5)
        q = cls(4, static_range='trained')
        assert q.static_range == 'trained'
        with pytest.raises(RuntimeError, match=cls.__name__ + r".*'trained'.*before its range was resolved"):
            q(torch.zeros(1, 3, 2, 2), None)
        with pytest.raises(ValueError, match=cls.__name__ + r".*no bottleneck_range"):
            q.resolve_trained_range(None)
        with pytest.raises(ValueError, match=cls.__name__ + r'.*trained at 2 bits'):
            q.resolve_trained_range({'min': -1.0, 'max': 1.0, 'steps': 3.0, 'num_bits': 2, 'momentum': 0.01})
        assert q.resolve_trained_range({'min': -1.0, 'max': 1.0, 'steps': 3.0, 'num_bits': 4, 'momentum': 0.01})
        assert q.static_range == (-1.0, 1.0)
        q.set_static_range(0.0, 3.0)
        assert q.static_range == (0.0, 3.0)
        for bad in ([1.0, 1.0], [2.0, 1.0], [0.0, float('inf')], [float('nan'), 1.0], [0.0], 'ema', [0.0, '1']):
            with pytest.raises(ValueError, match=cls.__name__ + '.*static_range'):
                cls(4, static_range=bad)
        with pytest.raises(ValueError, match=cls.__name__ + '.*static_range.*lo < hi'):
            q.set_static_range(1.0, 1.0)
    with pytest.raises(ValueError, match=r'Quantizer\(num_bits=16, static_range'):
        T.Quantizer(16, static_range=[0.0, 1.0])
    with pytest.raises(ValueError, match=r'Quantizer\(num_bits=16, static_range'):
        T.Quantizer(16, static_range='trained')
    assert T.Quantizer(16).static_range is None
    tr = T.get_bottleneck_transformer({'order': ['quantizer', 'dequantizer'], 'components': {
        'quantizer': {'params': {'num_bits': 3, 'packed': True, 'static_range': 'trained'}},
        'dequantizer': {'params': {'num_bits': 3}}}})
    assert T.resolve_trained_ranges(tr, {'min': -2.0, 'max': 2.0, 'steps': 1.0, 'num_bits': 3}) == 1
    assert tr.transforms[0].static_range == (-2.0, 2.0)
    assert T.resolve_trained_ranges(None, None) == 0 and T.resolve_trained_ranges(T.Compose([T.Quantizer(3)]), None) == 0


def test_split_model_takes_the_static_range_beside_its_pinned_signature():
    import inspect
    from hnd_ghnd_object_detectors_amd.models.mimic import split_rcnn as S
    assert list(inspect.signature(S.split_rcnn_model).parameters) == ['model', 'quantization', 'packed']
    assert list(inspect.signature(S.split_rcnn_model_ranged).parameters) == ['model', 'quantization', 'static_range', 'packed']
    with pytest.raises(ValueError, match='split_rcnn_model_ranged.*static_range.*needs a quantization width'):
        S.split_rcnn_model_ranged(None, None, [0.0, 1.0])
    with pytest.raises(ValueError, match=r'Quantizer\(num_bits=16, static_range'):
        S.split_rcnn_model_ranged(None, 16, [0.0, 1.0])
    with pytest.raises(ValueError, match='packed=True.*needs a quantization width'):
        S.split_rcnn_model(None, None, packed=True)


# ------------------------------------------------------------------------------------------ config
def _plain(o):
    if isinstance(o, dict):
        return {k: _plain(v) for k, v in o.items()}
    return [_plain(v) for v in o] if isinstance(o, (list, tuple)) else o


@pytest.mark.parametrize('momentum', [None, 0.05, 1])
def test_range_section_round_trips_through_yaml_and_json(momentum, tmp_path):
    from hnd_ghnd_object_detectors_amd import configs
    from hnd_ghnd_object_detectors_amd.myutils.common import yaml_util
    from hnd_ghnd_object_detectors_amd.utils import main_util
    section = {'type': 'ema'} if momentum is None else {'type': 'ema', 'momentum': momentum}
    want = {'momentum': 0.01 if momentum is None else float(momentum), 'frozen': False}
    cfg = configs.make_config('faster_rcnn', 'ghnd', 3, fake_quantize_bits=4, fake_quantize_range=section)
    assert cfg['train']['fake_quantize'] == {'num_bits': 4, 'range': section}
    assert configs.fake_quantize_bits_of(cfg) == 4 and configs.fake_quantize_range_of(cfg) == want
    path = tmp_path / 'c.yaml'
    with open(path, 'w') as fp:
        yaml.safe_dump(_plain(cfg), fp, sort_keys=False, default_flow_style=None)
    loaded = yaml_util.load_yaml_file(str(path))
    assert loaded == _plain(cfg) and configs.fake_quantize_range_of(loaded) == want
    # --json on a config without the key, and on one with {num_bits: b} alone
    for base in (_plain(configs.make_config('faster_rcnn', 'ghnd', 3)),
                 _plain(configs.make_config('faster_rcnn', 'ghnd', 3, fake_quantize_bits=2))):
        assert configs.fake_quantize_range_of(base) is None
        main_util.overwrite_config(base, json.dumps({'train': {'fake_quantize': {'num_bits': 4, 'range': section}}}))
        assert configs.fake_quantize_bits_of(base) == 4 and configs.fake_quantize_range_of(base) == want
        assert base['train']['batch_size'] == 4


def test_num_bits_alone_and_type_batch_keep_the_per_batch_range():
    from hnd_ghnd_object_detectors_amd import configs
    for bits in (1, 4, 8):
        cfg = configs.make_config(fake_quantize_bits=bits)
        assert cfg['train']['fake_quantize'] == {'num_bits': bits}
        assert configs.fake_quantize_bits_of(cfg) == bits and configs.fake_quantize_range_of(cfg) is None
        cfg = configs.make_config(fake_quantize_bits=bits, fake_quantize_range={'type': 'batch'})
        assert configs.fake_quantize_bits_of(cfg) == bits and configs.fake_quantize_range_of(cfg) is None
    assert configs.fake_quantize_range_of(configs.make_config()) is None


def test_bad_range_sections_are_refused_at_config_time():
    from hnd_ghnd_object_detectors_amd import configs
    bad_ranges = ['ema', None, {}, {'type': 'learned'}, {'momentum': 0.1}, {'type': 'batch', 'momentum': 0.1},
                  {'type': 'ema', 'momentum': 0}, {'type': 'ema', 'momentum': -0.1}, {'type': 'ema', 'momentum': 1.5},
                  {'type': 'ema', 'momentum': True}, {'type': 'ema', 'momentum': '0.1'}, {'type': 'ema', 'decay': 0.9}]
    for bad in bad_ranges:
        cfg = configs.make_config()
        cfg['train']['fake_quantize'] = {'num_bits': 4, 'range': bad}
        for fn in (configs.fake_quantize_bits_of, configs.fake_quantize_range_of):
            with pytest.raises(ValueError, match='train.fake_quantize must be'):
                fn(cfg)
    for section in ({'bits': 4}, {'num_bits': 4, 'ranges': {'type': 'ema'}}, {'range': {'type': 'ema'}}, 4):
        cfg = configs.make_config()
        cfg['train']['fake_quantize'] = section
        with pytest.raises(ValueError, match='train.fake_quantize must be'):
            configs.fake_quantize_range_of(cfg)
    cfg = configs.make_config()
    cfg['train']['fake_quantize'] = {'num_bits': 12, 'range': {'type': 'ema'}}
    with pytest.raises(ValueError, match='fake_quantize.num_bits.*outside 1 ... 8'):
        configs.fake_quantize_range_of(cfg)
    with pytest.raises(ValueError, match='train.fake_quantize must be'):
        configs.make_config(fake_quantize_range={'type': 'ema'})         # a range without a width


# ------------------------------------------------------------------------------------------ the layer attribute
def test_layer_attribute_registers_a_non_persistent_buffer_once_it_is_on():
    from hnd_ghnd_object_detectors_amd.models.mimic.resnet_layer import Bottleneck4LargeResNet
    layer = Bottleneck4LargeResNet(3, None, None)
    keys = list(layer.state_dict())
    assert layer.train_fake_quant_range is None and 'qrange_state' not in dict(layer.named_buffers())
    assert layer.fake_quant_range_host() is None
    layer.train_fake_quant_range = None                                   # (off stays off: no buffer)
    assert 'qrange_state' not in dict(layer.named_buffers())
    layer.train_fake_quant_range = {'momentum': 0.05, 'frozen': False}
    assert layer.train_fake_quant_range['momentum'] == 0.05 and layer.train_fake_quant_range['frozen'] is False
    assert torch.equal(layer.qrange_state, torch.zeros(4)) and layer.qrange_state.dtype == torch.float32
    assert list(layer.state_dict()) == keys                               # checkpoints do not change
    layer.load_state_dict(Bottleneck4LargeResNet(3, None, None).state_dict(), strict=True)
    for bad in ({'momentum': 0}, {'momentum': 2.0}, {'momentum': True}, {'frozen': True}, {'momentum': 0.1, 'frozen': 1},
                {'momentum': 0.1, 'ema': True}, 0.1, {'momentum': 0.1, 'range': [0.0, 1.0]},
                {'momentum': 0.1, 'frozen': True, 'range': [1.0, 1.0]}):
        with pytest.raises(ValueError, match='train_fake_quant_range'):
            layer.train_fake_quant_range = bad
    # without a width the range is inert; a frozen range with nothing observed is refused by name
    assert layer._fake_quant_range_arg() is None
    layer.train_fake_quant_bits = 4
    arg = layer._fake_quant_range_arg()
    assert arg['state'] is layer.qrange_state and arg['momentum'] == 0.05 and not arg['frozen'] and arg['range'] is None
    layer.train_fake_quant_range = {'momentum': 0.05, 'frozen': True}
    with pytest.raises(RuntimeError, match='frozen but qrange_state holds no range'):
        layer._fake_quant_range_arg()
    layer.train_fake_quant_range = {'momentum': 0.05, 'frozen': True, 'range': [-1.5, 2.0]}
    assert layer.qrange_state.tolist() == [-1.5, 2.0, 1.0, 0.0]
    assert layer._fake_quant_range_arg()['range'] == (-1.5, 2.0)
    assert layer.fake_quant_range_host() == {'min': -1.5, 'max': 2.0, 'steps': 1.0}
    # the refusals of fake_quant_bits_checked apply unchanged
    handle = layer.encoder.register_forward_hook(lambda m, i, o: None)
    with pytest.raises(NotImplementedError, match='fake quantisation.*backbone.body.layer1.encoder'):
        layer.fake_quant_bits_checked()
    handle.remove()
    layer.train_fake_quant_range = None
    assert layer.train_fake_quant_range is None and list(layer.state_dict()) == keys


# ------------------------------------------------------------------------------------------ numpy restatement, estimator
def test_numpy_restatement_marks_the_boundaries_as_the_header_states():
    qp = R.qparams_np(-1.0, 2.0, 2)                                       # scale 1, zero point 1, qmax 3
    assert qp.tolist() == [-1.0, 2.0, 1.0, 1.0]
    x = np.zeros((1, 12), dtype=np.float32)
    #             u: -0.5  -0.5001  3.5    3.4999  0.5   1.5   2.5   -7     9     nan   0
    x[0, :11] = [-1.5, -1.5001, 2.5, 2.4999, -0.5, 0.5, 1.5, -8.0, 8.0, np.nan, -1.0]
    y, mask, u = R.fake_quantize_range_np(x, 11, 2, qp)
    assert R.mask_bits(mask, 11)[0].tolist() == [True, False, False, True, True, True, True, False, False, False, True]
    assert mask.shape == (1, 3) and int(mask[0, 2]) >> 3 == 0 and all(int(b) < 16 for b in mask[0])
    assert y[0, :9].tolist() == [-1.0, -1.0, 2.0, 2.0, -1.0, 1.0, 1.0, -1.0, 2.0] and np.isnan(y[0, 9]) and y[0, 11] == 0


def _oracles(name):
    z, meta = G.load(name)
    cfg = MU.config_for(meta)
    t_sd, s_sd = MU.oracle_states(meta['seed'], meta['model'], meta.get('bch', 3), meta.get('num_classes', 91))
    ms = meta['min_size'] if isinstance(meta['min_size'], list) else [meta['min_size']]
    kw = dict(terms=MU.terms_of(cfg), min_size=tuple(ms), max_size=meta['max_size'])
    images, _ = G.case_inputs(meta)
    return t_sd, s_sd, kw, images


@pytest.mark.parametrize('name,bits,lo,hi', R.ONE_STEP_RANGE_CASES)
def test_oracle_alone_meets_the_preconditions_of_the_one_step_comparison(name, bits, lo, hi, monkeypatch):
    t_sd, s_sd, kw, images = _oracles(name)
    capture = {}
    monkeypatch.setattr(O, 'student_layer1', QU.make_student_layer1(bits, fake_quant=R.clipped_ste(bits, lo, hi, capture)))
    O.DistillOracle(t_sd, s_sd, dtype=torch.float64, **kw).forward(images)
    O.DistillOracle(t_sd, s_sd, **kw).forward(images)
    cap32, cap64 = capture[torch.float32], capture[torch.float64]
    m32, m64 = R.check_range_preconditions(cap32, cap64, bits, '%s at %d bits on [%g, %g]' % (name, bits, lo, hi))
    zp_raw = -np.float32(lo) / cap32['scale']
    print('\n[%s, %d bits, [%g, %g]] %d values; nearest half-integer fp32 %.2e / fp64 %.2e code units; clipped below %.2f %%, '
          'above %.2f %%, passing %.2f %%; -lo / scale %.4f' % (name, bits, lo, hi, cap32['codes'].numel(), m32[0], m64[0],
                                                               100 * m32[1], 100 * m32[2], 100 * m32[3], zp_raw))
    assert abs(zp_raw - round(zp_raw)) >= QU.MARGIN                       # the zero point's int() is no close call either
    # the numpy restatement (what the GPU kernel is held to) takes the oracle's decisions on the oracle's tensor
    z = cap32['z'].permute(0, 2, 3, 1).reshape(-1, cap32['z'].shape[1]).numpy()
    cs = (z.shape[1] + 3) // 4 * 4
    buf = np.zeros((z.shape[0], cs), dtype=np.float32)
    buf[:, :z.shape[1]] = z
    qp = R.qparams_np(lo, hi, bits)
    y, mask, _ = R.fake_quantize_range_np(buf, z.shape[1], bits, qp)
    passed = cap32['passed'].permute(0, 2, 3, 1).reshape(-1, z.shape[1]).numpy()
    assert int(qp[3]) == cap32['zero_point'] and np.array_equal(R.mask_bits(mask, z.shape[1]), passed)


def test_clipped_estimator_has_no_gradient_where_the_value_was_clipped():
    z = torch.tensor([-3.0, -0.9, 0.1, 0.7, 1.9, 4.0], dtype=torch.float64, requires_grad=True)
    capture = {}
    y = R.clipped_ste(2, -1.0, 2.0, capture)(z)
    (y * torch.arange(1.0, 7.0, dtype=torch.float64)).sum().backward()
    assert capture[torch.float64]['passed'].tolist() == [False, True, True, True, True, False]
    assert z.grad.tolist() == [0.0, 2.0, 3.0, 4.0, 5.0, 0.0]
    assert y.detach().tolist() == [-1.0, -1.0, 0.0, 1.0, 2.0, 2.0]
