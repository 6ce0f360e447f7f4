"""CPU: include/hnd_qat.h (symbols, version, argument validation), the config plumbing of train.fake_quantize, the
straight-through helper of tests/qat_util.py, and the preconditions that make the GPU one-step comparison of
tests/test_fake_quant_gpu.py fair: on every (fixture, width) pair in use the fp32 and the fp64 oracle take the same rounding
decisions, none of them within 1e-4 of a tie."""
import ctypes
import json
import os
import re

import pytest
import torch
import yaml

from oracle import hnd_oracle as O
from tests import golden_util as G
from tests import model_util as MU
from tests import qat_util as QU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'hnd_qat.h')


@pytest.fixture(scope='module', autouse=True)
def built():
    """the package loads libhnd_hip.so on import (there is no fallback), so it is built first"""
    import __graft_entry__ as g
    g.build()


# ------------------------------------------------------------------------------------------ C ABI
def test_qat_symbols_resolve_and_the_other_tables_do_not_move():
    """(that no header's names are in another's tuple: tests/test_lib_cpu.py, over all four headers)"""
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    assert list(_lib.QAT_SYMBOLS) == ['hnd_fake_quantize_bits', 'hnd_fake_quantize_tiles', 'hnd_qat_abi']
    for name in _lib.QAT_SYMBOLS:
        assert getattr(lib, name).argtypes is not None
    header = open(HEADER).read()
    value = int(re.search(r'#define HND_QAT_ABI (\d+)\b', header).group(1))
    assert lib.hnd_qat_abi() == _lib.QAT_ABI == value == 1
    assert lib.hnd_abi_version() == _lib.ABI_VERSION == 12 and lib.hnd_codec_abi() == _lib.CODEC_ABI == 1   # (untouched)


def test_tile_count_is_the_ceiling_of_npix_over_the_rows_the_header_states():
    from hnd_ghnd_object_detectors_amd import _lib, ops
    lib = _lib.load()
    rows = int(re.search(r'#define HND_FAKE_QUANT_TILE_ROWS (\d+)\b', open(HEADER).read()).group(1))
    assert rows == 128
    for npix in (1, 70, 127, 128, 129, 3 * 37 * 41, 2 ** 31 + 5):
        assert lib.hnd_fake_quantize_tiles(npix) == (npix + rows - 1) // rows == ops.fake_quantize_tiles(npix)
    for bad in (0, -1, -128):
        assert lib.hnd_fake_quantize_tiles(bad) == 0


def test_fake_quantize_validates_before_any_hip_call():
    """every refusal of the header comment returns HND_ERR_INVALID (-1) with the export's name in the error string; nothing
    is launched, so host memory stands in for the device pointers"""
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    host = (ctypes.c_double * 64)()
    p = ctypes.addressof(host)

    def call(x=p, y=p, npix=4, c=3, cs=4, bits=4, qparams=p, scratch=p, stats=None):
        return lib.hnd_fake_quantize_bits(x, y, npix, c, cs, bits, qparams, scratch, stats, None)

    def refused(rc):
        return rc == -1 and b'hnd_fake_quantize_bits' in lib.hnd_last_error_string()

    for name in ('x', 'y', 'qparams', 'scratch'):
        assert refused(call(**{name: None})), name
    for bits in (0, 9, -1, 16):
        assert refused(call(bits=bits)), bits
    for c in (0, -3):
        assert refused(call(c=c)), c
    assert refused(call(c=5, cs=4))                                      # cs < c
    for cs in (5, 6, 7):
        assert refused(call(c=3, cs=cs)), cs                             # cs % 4 != 0
    for npix in (0, -2):
        assert refused(call(npix=npix)), npix


def test_ops_wrapper_refuses_a_bad_width_by_name():
    from hnd_ghnd_object_detectors_amd import ops
    x = torch.zeros(1, 1, 1, 4)
    for bits in (0, 9, 16, True, 4.0):
        with pytest.raises(ValueError, match='fake_quantize_bits.*outside 1 ... 8'):
            ops.fake_quantize_bits(x, 3, bits, None, None)


# ------------------------------------------------------------------------------------------ host classes and config
def test_fake_quantizer_builds_at_1_to_8_bits_and_is_registered():
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    for bits in range(1, 9):
        assert T.FakeQuantizer(bits).num_bits == bits
    assert T.TRANSFORMER_CLASS_DICT['fake_quantizer'] is T.FakeQuantizer
    tr = T.get_bottleneck_transformer({'order': ['fake_quantizer'],
                                       'components': {'fake_quantizer': {'params': {'num_bits': 3}}}})
    assert isinstance(tr.transforms[0], T.FakeQuantizer) and tr.transforms[0].num_bits == 3
    for bad in (0, 9, 16, True, 2.0):
        with pytest.raises(ValueError, match='FakeQuantizer.*outside 1 ... 8'):
            T.FakeQuantizer(bad)
    assert T.Quantizer(16).num_bits == 16                                # (16 stays with Quantizer)


def _plain(o):
    if isinstance(o, dict):
        return {k: _plain(v) for k, v in o.items()}
    return [_plain(v) for v in o] if isinstance(o, (list, tuple)) else o


@pytest.mark.parametrize('bits', [1, 4, 8])
def test_config_key_round_trips_through_yaml_and_json(bits, tmp_path):
    from hnd_ghnd_object_detectors_amd import configs
    from hnd_ghnd_object_detectors_amd.myutils.common import yaml_util
    from hnd_ghnd_object_detectors_amd.utils import main_util
    cfg = configs.make_config('faster_rcnn', 'ghnd', 3, fake_quantize_bits=bits)
    assert cfg['train']['fake_quantize'] == {'num_bits': bits} and configs.fake_quantize_bits_of(cfg) == bits
    path = tmp_path / 'c.yaml'
    with open(path, 'w') as fp:                                          # the writer of tools/gen_configs.py
        yaml.safe_dump(_plain(cfg), fp, sort_keys=False, default_flow_style=None)
    loaded = yaml_util.load_yaml_file(str(path))
    assert loaded == _plain(cfg) and configs.fake_quantize_bits_of(loaded) == bits
    # --json on a config without the key, as mimic_runner.main applies it
    base = _plain(configs.make_config('faster_rcnn', 'ghnd', 3))
    assert 'fake_quantize' not in base['train'] and configs.fake_quantize_bits_of(base) is None
    main_util.overwrite_config(base, json.dumps({'train': {'fake_quantize': {'num_bits': bits}}}))
    assert configs.fake_quantize_bits_of(base) == bits and base['train']['batch_size'] == 4
    # ... and --json that changes the width of a config that has the key
    main_util.overwrite_config(loaded, json.dumps({'train': {'fake_quantize': {'num_bits': 2}}}))
    assert configs.fake_quantize_bits_of(loaded) == 2


def test_bad_widths_and_a_term_on_the_bottleneck_tensor_are_refused_at_config_time():
    from hnd_ghnd_object_detectors_amd import configs
    for bad in (0, 9, 16, -1, True, '4', 4.0, None):
        if bad is not None:
            with pytest.raises(ValueError, match='fake_quantize.num_bits.*outside 1 ... 8'):
                configs.make_config(fake_quantize_bits=bad)
        cfg = configs.make_config()
        cfg['train']['fake_quantize'] = {'num_bits': bad}
        with pytest.raises(ValueError, match='fake_quantize.num_bits.*outside 1 ... 8'):
            configs.fake_quantize_bits_of(cfg)
    cfg = configs.make_config()
    cfg['train']['fake_quantize'] = {'bits': 4}
    with pytest.raises(ValueError, match='train.fake_quantize must be'):
        configs.fake_quantize_bits_of(cfg)
    cfg = configs.make_config(fake_quantize_bits=4)
    path = 'backbone.body.layer1.encoder'
    cfg['train']['criterion']['terms']['enc'] = {'ts_modules': [path, path], 'factor': 1.0,
                                                 'criterion': {'type': 'MSELoss', 'params': {'reduction': 'sum'}}}
    with pytest.raises(NotImplementedError, match='fake_quantize.*backbone.body.layer1.encoder'):
        configs.fake_quantize_bits_of(cfg)
    del cfg['train']['fake_quantize']
    assert configs.fake_quantize_bits_of(cfg) is None                    # the term alone is fine


def test_absent_key_leaves_the_layer_attribute_at_none():
    """a student built from a config without the key has train_fake_quant_bits None (the reference's training); the
    layer refuses a bad width, a hook on its encoder and -- by the runner's rule -- nothing else"""
    from hnd_ghnd_object_detectors_amd.models.mimic.base import BottleneckBase4Ext
    from hnd_ghnd_object_detectors_amd.models.mimic.resnet_layer import Bottleneck4LargeResNet
    layer = Bottleneck4LargeResNet(3, None, None)
    assert isinstance(layer, BottleneckBase4Ext) and layer.train_fake_quant_bits is None
    assert layer.fake_quant_bits_checked() is None
    layer.train_fake_quant_bits = 4
    assert layer.fake_quant_bits_checked() == 4
    for bad in (0, 9, 16, True):
        layer.train_fake_quant_bits = bad
        with pytest.raises(ValueError, match='train_fake_quant_bits.*outside 1 ... 8'):
            layer.fake_quant_bits_checked()
    layer.train_fake_quant_bits = 4
    handle = layer.encoder.register_forward_hook(lambda m, i, o: None)
    with pytest.raises(NotImplementedError, match='fake quantisation.*backbone.body.layer1.encoder'):
        layer.fake_quant_bits_checked()
    handle.remove()
    assert layer.fake_quant_bits_checked() == 4


# ------------------------------------------------------------------------------------------ the oracle helper
def _oracles(name):
    z, meta = G.load(name)
    cfg = MU.config_for(meta)
    t_sd, s_sd = MU.oracle_states(meta['seed'], meta['model'], meta.get('bch', 3), meta.get('num_classes', 91))
    ms = meta['min_size'] if isinstance(meta['min_size'], list) else [meta['min_size']]
    kw = dict(terms=MU.terms_of(cfg), min_size=tuple(ms), max_size=meta['max_size'])
    images, _ = G.case_inputs(meta)
    return t_sd, s_sd, kw, images


@pytest.mark.parametrize('name,bits', QU.ONE_STEP_CASES)
def test_oracle_alone_meets_the_preconditions_of_the_one_step_comparison(name, bits, monkeypatch):
    """the fp32 and the fp64 oracle, from the fixture's initial state (what the GPU test syncs them to), take the same
    rounding decisions on the bottleneck tensor, and every decision keeps 1e-4 code units from its tie"""
    t_sd, s_sd, kw, images = _oracles(name)
    capture = {}
    monkeypatch.setattr(O, 'student_layer1', QU.make_student_layer1(bits, capture))
    O.DistillOracle(t_sd, s_sd, dtype=torch.float64, **kw).forward(images)
    O.DistillOracle(t_sd, s_sd, **kw).forward(images)
    cap32, cap64 = capture[torch.float32], capture[torch.float64]
    m32, m64 = QU.check_preconditions(cap32, cap64, '%s at %d bits' % (name, bits))
    print('\n[%s, %d bits] %d values, %d distinct codes; nearest tie fp32 %.2e / fp64 %.2e code units, zero point %d '
          '(-min/scale %.4f)' % (name, bits, cap32['codes'].numel(), len(torch.unique(cap32['codes'])), m32[0], m64[0],
                                 cap64['zero_point'], cap64['zp_raw']))
    assert len(torch.unique(cap64['codes'])) > 2 or bits == 1            # the quantiser is really at work


def test_widths_of_the_one_step_comparison_include_a_low_one():
    widths = sorted(b for _, b in QU.ONE_STEP_CASES)
    assert len(set(widths)) >= 2 and widths[0] <= 3 and all(1 <= b <= 8 for b in widths)


def test_straight_through_helper_has_the_gradient_of_z_plus_a_constant(monkeypatch):
    """fp64: the gradient through the patched student_layer1 equals the gradient of the same graph with the fake quantiser
    replaced by z + const, const = the detached quantisation error of the same forward"""
    name, bits = QU.ONE_STEP_CASES[0]
    t_sd, s_sd, kw, images = _oracles(name)
    capture = {}
    monkeypatch.setattr(O, 'student_layer1', QU.make_student_layer1(bits, capture))
    orc = O.DistillOracle(t_sd, s_sd, dtype=torch.float64, **kw)
    loss_a, _, g_a, _ = orc.step(images)
    zq = O.quantize_dequantize(capture[torch.float64]['z'], bits)
    const = (zq - capture[torch.float64]['z']).detach()
    assert float(const.abs().max()) > 0
    monkeypatch.setattr(O, 'student_layer1', QU.make_student_layer1(bits, fake_quant=lambda z: z + const))
    loss_b, _, g_b, _ = O.DistillOracle(t_sd, s_sd, dtype=torch.float64, **kw).step(images)
    assert abs(loss_a - loss_b) <= 1e-12 * abs(loss_a)
    for k in g_a:
        assert float((g_a[k] - g_b[k]).norm()) <= 1e-12 * float(g_a[k].norm()) + 1e-300, k
    # ... and it is not the gradient of the unquantised graph (the quantiser changes what the decoder sees)
    monkeypatch.setattr(O, 'student_layer1', QU.make_student_layer1(bits, fake_quant=lambda z: z))
    _, _, g_c, _ = O.DistillOracle(t_sd, s_sd, dtype=torch.float64, **kw).step(images)
    key = O.B + 'layer1.decoder.1.weight' if O.B + 'layer1.decoder.1.weight' in g_a else next(iter(g_a))
    assert float((g_a[key] - g_c[key]).norm()) > 1e-6 * float(g_c[key].norm())
