"""CPU: the criterion factory, the C ABI of hnd_mimic_loss_fwd_bwd (layout, argument validation) and the reference-made
fixture tests/golden/tiny_ghnd_criteria.npz (four terms, four criteria), pinned by a CPU restatement of the step."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import hnd_oracle as O
from tests import criteria_util as CU
from tests import golden_util as G


@pytest.fixture(scope='module', autouse=True)
def built():
    """the package loads libhnd_hip.so on import (there is no fallback), so it is built first"""
    import __graft_entry__ as g
    g.build()


# ------------------------------------------------------------------------------------------ func_util.get_loss
SPELLINGS = [('mse', 'HipMSELoss', 'mse'), ('MSELoss', 'HipMSELoss', 'mse'), ('mseloss', 'HipMSELoss', 'mse'),
             ('l1', 'HipL1Loss', 'l1'), ('L1Loss', 'HipL1Loss', 'l1'), ('L1LOSS', 'HipL1Loss', 'l1'),
             ('smoothl1', 'HipSmoothL1Loss', 'smooth_l1'), ('SmoothL1Loss', 'HipSmoothL1Loss', 'smooth_l1'),
             ('huber', 'HipHuberLoss', 'huber'), ('HuberLoss', 'HipHuberLoss', 'huber')]


@pytest.mark.parametrize('spelling,cls,kind', SPELLINGS)
@pytest.mark.parametrize('reduction', ['sum', 'mean'])
def test_get_loss_returns_the_criterion_for_every_accepted_spelling(spelling, cls, kind, reduction):
    from hnd_ghnd_object_detectors_amd.distillation import hip_loss
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util
    c = func_util.get_loss(spelling, {'reduction': reduction})
    assert type(c) is getattr(hip_loss, cls)
    assert (c.kind, c.reduction) == (kind, reduction)
    assert c.is_mse_sum() == (kind == 'mse' and reduction == 'sum')


def test_get_loss_applies_params_and_torch_defaults():
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util
    assert func_util.get_loss('SmoothL1Loss', {'reduction': 'sum', 'beta': 0.02}).param == 0.02
    assert func_util.get_loss('SmoothL1Loss', {'reduction': 'sum'}).param == 1.0            # torch's default beta
    assert func_util.get_loss('SmoothL1Loss', {'beta': 0.0}).param == 0.0                    # = L1, as in torch
    assert func_util.get_loss('HuberLoss', {'delta': 2.5}).param == 2.5
    assert func_util.get_loss('huber').param == 1.0
    assert func_util.get_loss('L1Loss').reduction == 'mean'                                  # torch's default reduction
    assert func_util.get_loss('MSELoss', {'reduction': 'sum', 'size_average': None, 'reduce': None}).is_mse_sum()


@pytest.mark.parametrize('loss_type,params', [
    ('MSELoss', {'reduction': 'none'}), ('L1Loss', {'reduction': 'none'}),
    ('MSELoss', {'size_average': False}), ('SmoothL1Loss', {'reduce': True}), ('L1Loss', {'size_average': True}),
    ('KLDivLoss', {'reduction': 'batchmean'}), ('CrossEntropyLoss', {}), ('CosineEmbeddingLoss', {})])
def test_unsupported_criteria_are_refused_with_the_supported_list(loss_type, params):
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util
    with pytest.raises((NotImplementedError, ValueError)) as e:
        func_util.get_loss(loss_type, params)
    msg = str(e.value)
    for word in ('MSELoss', 'L1Loss', 'SmoothL1Loss', 'HuberLoss', "'sum'", "'mean'"):
        assert word in msg, msg
    assert loss_type in msg


def test_bad_thresholds_are_refused():
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util
    for loss_type, params in (('SmoothL1Loss', {'beta': -1.0}), ('SmoothL1Loss', {'beta': float('nan')}),
                              ('HuberLoss', {'delta': 0.0}), ('HuberLoss', {'delta': float('inf')})):
        with pytest.raises(ValueError):
            func_util.get_loss(loss_type, params)


def test_criterion_section_with_mixed_terms_parses_and_org_loss_factor_is_still_refused():
    from hnd_ghnd_object_detectors_amd.distillation import loss as L
    from tests import model_util as MU
    _, meta = G.load('tiny_ghnd_criteria')
    cfg = CU.apply_criteria(MU.config_for(meta), meta['criterion'])
    crit = L.get_loss(cfg['train']['criterion'])
    got = [(t.criterion.kind, t.criterion.reduction, t.criterion.param, t.factor) for t in crit.term_dict.values()]
    assert got == [('smooth_l1', 'mean', 1.0, 1.0), ('l1', 'mean', 0.0, 1.0), ('mse', 'mean', 0.0, 4.0),
                   ('smooth_l1', 'sum', 0.02, 1e-4)]
    cfg['train']['criterion']['params']['org_loss_factor'] = 1.0
    with pytest.raises(NotImplementedError):
        L.get_loss(cfg['train']['criterion'])({}, {})


# ------------------------------------------------------------------------------------------ C ABI
def test_mimic_pair_matches_the_header_layout():
    """(sizeof and every offsetof of both pair structs against the C compiler: tests/test_lib_cpu.py)"""
    from hnd_ghnd_object_detectors_amd import _lib
    assert [n for n, _ in _lib.MimicPair._fields_] == ['teacher', 'student', 'grad', 'numel', 'count', 'factor', 'param',
                                                      'kind', 'relu_mask']
    assert _lib.MIMIC_KINDS == {'mse': 0, 'l1': 1, 'smooth_l1': 2, 'huber': 3}  # enum hnd_mimic_kind
    assert 'hnd_mimic_loss_fwd_bwd' in _lib.EXPORTED_SYMBOLS


def test_mimic_entry_point_validates_before_any_hip_call():
    """every refusal of the header comment returns HND_ERR_INVALID (-1) with the function's name in the error string;
    nothing is launched, so host memory stands in for the device pointers"""
    import __graft_entry__ as g
    g.build()
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    host = (ctypes.c_double * 64)()
    p = ctypes.addressof(host)

    def pairs(n=1, **kw):
        arr = (_lib.MimicPair * n)()
        for a in arr:
            a.teacher, a.student, a.grad, a.numel, a.count = p, p, None, 64, 0
            a.factor, a.param, a.kind, a.relu_mask = 1.0, 1.0, 2, 0
        for k, v in kw.items():
            setattr(arr[n - 1], k, v)
        return arr

    def refused(arr, n, out=p, scratch=p):
        rc = lib.hnd_mimic_loss_fwd_bwd(arr, n, out, scratch, None)
        return rc == -1 and b'hnd_mimic_loss_fwd_bwd' in lib.hnd_last_error_string()

    assert refused(None, 1)
    assert refused(pairs(), 1, out=None) and refused(pairs(), 1, scratch=None)
    assert refused(pairs(), 0) and refused(pairs(), -1) and refused(pairs(9), 9)
    assert refused(pairs(teacher=None), 1) and refused(pairs(student=None), 1)
    assert refused(pairs(2, student=None), 2)                      # the LAST pair of two is checked as well
    for numel in (0, -4, 6, 63):
        assert refused(pairs(numel=numel), 1), numel
    for kind in (-1, 4, 17):
        assert refused(pairs(kind=kind), 1), kind
    for param in (-0.5, float('inf'), float('nan')):
        assert refused(pairs(param=param), 1), param
    assert refused(pairs(count=-1), 1)
    assert refused(pairs(count=65), 1)                             # more logical elements than the buffer holds
    assert refused(pairs(param=1e-30, factor=1e30), 1)             # factor / beta has no fp32 value


# ------------------------------------------------------------------------------------------ the kernel tests' reference
def test_fp64_formulas_are_torchs():
    """the table the kernel is held to IS F.mse_loss / l1_loss / smooth_l1_loss / huber_loss (fp64, autograd gradient)"""
    fns = {'mse': lambda a, b, p: F.mse_loss(a, b, reduction='sum'), 'l1': lambda a, b, p: F.l1_loss(a, b, reduction='sum'),
           'smooth_l1': lambda a, b, p: F.smooth_l1_loss(a, b, reduction='sum', beta=p),
           'huber': lambda a, b, p: F.huber_loss(a, b, reduction='sum', delta=p)}
    t, s, _ = CU.kernel_inputs(3)[1]
    for kind, param in CU.KINDS.items():
        s64 = s.double().requires_grad_(True)
        loss = fns[kind](t.double(), s64, param)            # called as the reference does: criterion(teacher, student)
        loss.backward()
        val, grad = CU.fp64_reference(kind, param, t, s, 1.0, False)
        assert abs(float(loss.detach()) - float(val)) <= 1e-12 * float(val)
        assert float((grad - s64.grad).norm() / s64.grad.norm()) < 1e-12


# ------------------------------------------------------------------------------------------ the reference-made fixture
def test_criteria_fixture_is_reproduced_by_a_cpu_restatement_of_the_step():
    """tiny_ghnd_criteria.npz was written by the reference's own DistillationBox -> backward -> Adam
    (tests/golden/make_golden_criteria.py).  Maps from oracle.hnd_oracle, torch.nn criteria called as
    criterion(teacher, student): loss, per-term values, gradients, parameters after two steps to the bars
    test_oracle_golden.py holds the other tiny fixtures to."""
    z, meta = G.load('tiny_ghnd_criteria')
    crit = meta['criterion']
    assert [(k, v['criterion']['type'], v['criterion']['params'], v['factor']) for k, v in crit.items()] == [
        ('layer1', 'SmoothL1Loss', {'reduction': 'mean'}, 1.0), ('layer2', 'L1Loss', {'reduction': 'mean'}, 1.0),
        ('layer3', 'MSELoss', {'reduction': 'mean'}, 4.0),
        ('layer4', 'SmoothL1Loss', {'reduction': 'sum', 'beta': 0.02}, 1e-4)]
    # what the generator asserted for its seed: no term hides behind another, both zones of each SmoothL1 term populated
    norms = meta['solo_grad_norms']
    assert max(norms.values()) <= 10 * min(norms.values()), norms
    for name in ('layer1', 'layer4'):
        assert 0.05 <= meta['zones'][name]['linear_share'] <= 0.95, meta['zones']
    t_sd = O.init_teacher_state(meta['seed'], meta['model'])
    s_sd = O.init_student_state(t_sd, meta['seed'] + 1000)
    orc = CU.CriteriaOracle(t_sd, s_sd, crit, min_size=(meta['min_size'],), max_size=meta['max_size'], warmup_iters=4,
                            warmup_factor=1e-3)
    images, _ = G.case_inputs(meta)
    for step in range(meta['steps']):
        if step == 0:
            _, _, t_h, s_h, _, _, _ = orc.forward(images, update_buffers=False)
            for k in crit:
                G.compare(z, 'step0/teacher/' + k, t_h[k], 1e-6)
                G.compare(z, 'step0/student/' + k, s_h[k], 1e-6)
                d = (s_h[k] - t_h[k]).detach()
                if 'zero_share' in meta['zones'].get(k, {}):
                    assert math.isclose(float((d == 0).double().mean()), meta['zones'][k]['zero_share'], abs_tol=1e-3)
        loss, per_term, grads, lr = orc.step(images)
        assert abs(loss - float(z['step%d/loss' % step])) <= 1e-6 * abs(loss)
        assert abs(lr - float(z['step%d/lr' % step])) < 1e-12
        for k in crit:
            assert abs(per_term[k] - float(z['step%d/term/%s' % (step, k)])) <= 1e-6 * abs(per_term[k]), k
        for n, g in grads.items():
            if not n.endswith(G.ZERO_GRAD_SUFFIXES):
                G.compare(z, 'step%d/grad/%s' % (step, n), g, 2e-5)
    for n in orc.keys:
        if not n.endswith(G.ZERO_GRAD_SUFFIXES):
            G.compare(z, 'after/param/' + n, orc.s[n], 1e-4, atol=1e-6)
    for n in z.files:
        if n.startswith('after/buffer/'):
            ref = torch.from_numpy(z[n]).double()
            assert float((orc.s[n[len('after/buffer/'):]].double() - ref).abs().max()) <= 1e-5 * (1 + float(ref.abs().max()))
