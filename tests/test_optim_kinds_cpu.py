"""CPU: include/hnd_optim.h (symbols, version, descriptor layout, argument validation), the guard ledger of that header
(tests/test_guard_bands_optim_gpu.py) and func_util.get_optimizer for Adagrad, RMSprop and Adam with weight_decay / amsgrad."""
import ctypes
import os
import re
import sys

import pytest
import torch

from tests.test_lib_cpu import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def built():
    """the package loads libhnd_hip.so on import (there is no fallback), so it is built first"""
    import __graft_entry__ as g
    g.build()


# ------------------------------------------------------------------------------------------ C ABI
def test_optim_symbols_resolve_and_stay_out_of_the_main_table():
    """(that no header's names are in another's tuple: tests/test_lib_cpu.py, over all four headers)"""
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    assert list(_lib.OPTIM_SYMBOLS) == ['hnd_optim_abi', 'hnd_optim_step_flat']
    for name in _lib.OPTIM_SYMBOLS:
        assert getattr(lib, name).argtypes is not None
    assert lib.hnd_optim_abi() == _lib.OPTIM_ABI == 1
    assert lib.hnd_abi_version() == _lib.ABI_VERSION == 12              # (untouched)
    assert _lib.OPTIM_KINDS == {'adam': 0, 'adagrad': 1, 'rmsprop': 2}  # enum hnd_optim_kind
    header = open(os.path.join(ROOT, 'include', 'hnd_optim.h')).read()
    for name, value in (('HND_OPTIM_ADAM', 0), ('HND_OPTIM_ADAGRAD', 1), ('HND_OPTIM_RMSPROP', 2)):
        assert re.search(r'\b%s = %d\b' % (name, value), header), name
    assert re.search(r'#define HND_OPTIM_ABI 1\b', header)


def test_optim_desc_matches_the_header_layout():
    """(sizeof and every offsetof against the C compiler: tests/test_lib_cpu.py)"""
    from hnd_ghnd_object_detectors_amd import _lib
    assert [n for n, _ in _lib.OptimDesc._fields_] == [
        'param', 'grad', 'state0', 'state1', 'state2', 'numel', 'step', 'grad_scale', 'lr', 'weight_decay', 'eps', 'beta1',
        'beta2', 'momentum', 'lr_decay', 'kind', 'amsgrad', 'centered', 'reserved']
    # the struct of the header, field by field in order
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hnd_optim.h')).read(), flags=re.S)
    body = re.search(r'typedef struct hnd_optim_desc \{(.*?)\} hnd_optim_desc;', text, flags=re.S).group(1)
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            ctype, names = re.match(r'((?:const )?\w+\*?)\s+(.*)', decl).groups()
            fields += [(n.strip(), ctype) for n in names.split(',')]
    ctype_of = {'float*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'int64_t': ctypes.c_int64,
                'double': ctypes.c_double, 'int32_t': ctypes.c_int32}
    assert [(n, ctype_of[t]) for n, t in fields] == list(_lib.OptimDesc._fields_)


def test_optim_entry_point_validates_before_any_hip_call():
    """every refusal of the header comment returns HND_ERR_INVALID (-1) with the function's name in the error string;
    nothing is launched, so host memory stands in for the device pointers"""
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    host = (ctypes.c_double * 64)()
    p = ctypes.addressof(host)
    nan, inf = float('nan'), float('inf')

    def desc(kind, **kw):
        d = _lib.OptimDesc()
        d.param, d.grad, d.state0, d.state1, d.state2 = p, p, p, p, p
        d.numel, d.step, d.grad_scale = 64, 1, 1.0
        d.lr, d.weight_decay, d.eps, d.beta1, d.beta2, d.momentum, d.lr_decay = 1e-3, 0.0, 1e-8, 0.9, 0.99, 0.0, 0.0
        d.kind, d.amsgrad, d.centered = _lib.OPTIM_KINDS.get(kind, kind), 0, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(d):
        rc = lib.hnd_optim_step_flat(None if d is None else ctypes.byref(d), None)
        return rc == -1 and b'hnd_optim_step_flat' in lib.hnd_last_error_string()

    assert refused(None)
    for kind in ('adam', 'adagrad', 'rmsprop'):
        assert refused(desc(kind, param=None)) and refused(desc(kind, grad=None)), kind
        assert refused(desc(kind, state0=None)), kind
        for numel in (0, -4):
            assert refused(desc(kind, numel=numel)), (kind, numel)
        for step in (0, -1):
            assert refused(desc(kind, step=step)), (kind, step)
        for field in ('grad_scale', 'lr', 'weight_decay', 'eps', 'beta1', 'beta2', 'momentum', 'lr_decay'):
            for bad in (nan, inf, -inf):
                assert refused(desc(kind, **{field: bad})), (kind, field, bad)
        for field in ('lr', 'eps', 'weight_decay', 'momentum', 'lr_decay'):
            assert refused(desc(kind, **{field: -1e-3})), (kind, field)
    for kind in (-1, 3, 17):
        assert refused(desc(kind)), kind
    # a state pointer the kind / flags need
    assert refused(desc('adam', state1=None))
    assert refused(desc('adam', amsgrad=1, state2=None))
    assert refused(desc('rmsprop', momentum=0.9, state1=None))
    assert refused(desc('rmsprop', centered=1, state2=None))
    # betas outside [0, 1) (Adam), alpha < 0 (RMSprop)
    for field in ('beta1', 'beta2'):
        for bad in (-0.1, 1.0, 1.5):
            assert refused(desc('adam', **{field: bad})), (field, bad)
    assert refused(desc('rmsprop', beta2=-0.1))


# ------------------------------------------------------------------------------------------ the guard ledger of hnd_optim.h
def test_every_optim_export_that_writes_device_memory_has_a_guard_case():
    """the rule of tests/test_guard_ledger_cpu.py for include/hnd_optim.h: no export without a guard case"""
    from hnd_ghnd_object_detectors_amd import _lib
    loaded = 'hnd_ghnd_object_detectors_amd.ops' in sys.modules
    from tests import test_guard_bands_optim_gpu as T
    assert loaded or 'hnd_ghnd_object_detectors_amd.ops' not in sys.modules      # importing it does not touch the GPU
    covered = set().union(*T.LEDGER.values())
    assert covered and all(T.LEDGER.values())
    assert all(isinstance(reason, str) and reason for reason in T.NO_DEVICE_OUTPUT.values())
    assert not covered & set(T.NO_DEVICE_OUTPUT)
    assert covered | set(T.NO_DEVICE_OUTPUT) == set(_lib.OPTIM_SYMBOLS) == set(_declared('hnd_optim.h'))
    assert all(callable(getattr(T, name, None)) and name.startswith('test_') for name in T.LEDGER)


# ------------------------------------------------------------------------------------------ func_util.get_optimizer
def _params():
    return [torch.nn.Parameter(torch.zeros(3, 5)), torch.nn.Parameter(torch.zeros(7))]


def test_get_optimizer_returns_the_fused_class_with_its_hyper_parameters():
    from hnd_ghnd_object_detectors_amd import optim
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util
    o = func_util.get_optimizer(_params(), 'adagrad', {'lr': 0.05, 'lr_decay': 0.01, 'weight_decay': 1e-4,
                                                       'initial_accumulator_value': 0.1, 'eps': 1e-9})
    assert type(o) is optim.FusedAdagrad and isinstance(o, torch.optim.Adagrad)
    g = o.param_groups[0]
    assert (g['lr'], g['lr_decay'], g['weight_decay'], g['initial_accumulator_value'], g['eps']) == (0.05, 0.01, 1e-4, 0.1, 1e-9)
    assert all(float(o.state[p]['sum'].min()) == float(o.state[p]['sum'].max()) == pytest.approx(0.1) for p in g['params'])
    o = func_util.get_optimizer(torch.nn.Linear(3, 2), 'RMSprop', {'lr': 0.02, 'alpha': 0.9, 'eps': 1e-7, 'weight_decay': 1e-4,
                                                                  'momentum': 0.8, 'centered': True})
    assert type(o) is optim.FusedRMSprop and isinstance(o, torch.optim.RMSprop)
    g = o.param_groups[0]
    assert (g['lr'], g['alpha'], g['eps'], g['weight_decay'], g['momentum'], g['centered']) == (0.02, 0.9, 1e-7, 1e-4, 0.8, True)
    assert len(g['params']) == 2
    assert func_util.get_optimizer(_params(), 'rmsprop', {}).param_groups[0]['alpha'] == 0.99           # torch's defaults
    o = func_util.get_optimizer(_params(), 'Adam', {'lr': 1e-3, 'weight_decay': 1e-4})
    assert type(o) is optim.FusedAdam and o.param_groups[0]['weight_decay'] == 1e-4 and not o.param_groups[0]['amsgrad']
    o = func_util.get_optimizer(_params(), 'adam', {'lr': 1e-3, 'amsgrad': True, 'betas': (0.8, 0.9)})
    assert o.param_groups[0]['amsgrad'] is True and o.param_groups[0]['betas'] == (0.8, 0.9)
    o = func_util.get_optimizer(_params(), 'Adam', {'lr': 1e-3, 'weight_decay': 1e-2, 'amsgrad': True})
    assert (o.param_groups[0]['weight_decay'], o.param_groups[0]['amsgrad']) == (1e-2, True)
    for cls in (optim.FusedAdam, optim.FusedAdagrad, optim.FusedRMSprop):
        assert cls(_params()).grad_scale == 1.0
        with pytest.raises(NotImplementedError, match='closure'):
            cls(_params()).step(lambda: 0.0)


def test_unknown_types_and_keywords_of_other_implementations_are_refused():
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util
    for optim_type in ('AdamW', 'Adadelta', 'LBFGS', 'Adamax'):
        with pytest.raises(ValueError, match=optim_type):
            func_util.get_optimizer(_params(), optim_type, {'lr': 1e-3})
    for optim_type in ('Adam', 'Adagrad', 'RMSprop'):
        for keyword in ('maximize', 'foreach', 'capturable', 'differentiable', 'fused'):
            with pytest.raises(NotImplementedError, match=keyword):
                func_util.get_optimizer(_params(), optim_type, {'lr': 1e-3, keyword: True})
            func_util.get_optimizer(_params(), optim_type, {'lr': 1e-3, keyword: False})       # the default is taken
    # torch's own constructor checks still apply
    for optim_type, params in (('Adagrad', {'lr': -1.0}), ('RMSprop', {'alpha': -0.5}), ('Adam', {'weight_decay': -1e-4}),
                               ('Adagrad', {'initial_accumulator_value': -0.1})):
        with pytest.raises(ValueError):
            func_util.get_optimizer(_params(), optim_type, params)
