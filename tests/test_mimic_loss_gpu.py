"""GPU: the fused mimic loss for MSELoss / L1Loss / SmoothL1Loss / HuberLoss with reduction 'sum' or 'mean'
(hnd_mimic_loss_fwd_bwd -> ops.MimicLaunch -> hip_loss.distill_loss -> the YAML's criterion section):
the kernel against torch fp64, its bit identity with the MSE-sum launch, the model against the reference-made fixture
tests/golden/tiny_ghnd_criteria.npz, the mean divisor on the padded bottleneck tensor, the untouched default path, the CLI.
Bars: tests/test_ops_gpu.py::test_mse_fused_loss_and_grad for the kernel (1e-6), tests/test_model_gpu.py for the model."""
import copy
import json
import os
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

from oracle import hnd_oracle as O
from tests import criteria_util as CU
from tests import golden_util as G
from tests import model_util as MU

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FEAT_TOL, LOSS_TOL, GRAD_TOL = 1e-3, 1e-3, 2e-3          # (the model bars of tests/test_model_gpu.py)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


# ------------------------------------------------------------------------------------------ kernel vs torch fp64
KINDS, SHAPES, FACTORS = CU.KINDS, CU.SHAPES, CU.FACTORS
_kernel_inputs, _fp64_reference = CU.kernel_inputs, CU.fp64_reference


@pytest.mark.parametrize('relu_mask', [0, 1])
@pytest.mark.parametrize('reduction', ['sum', 'mean'])
@pytest.mark.parametrize('kind', list(KINDS))
def test_mimic_kernel_matches_torch_fp64(ops, kind, reduction, relu_mask):
    param = KINDS[kind]
    data = _kernel_inputs(21)
    pairs, refs = [], []
    for (t, s, logical), f in zip(data, FACTORS):
        d = (s - t)
        assert float((d == 0).double().mean()) >= 0.10 and float(((d == 0) & (s > 0)).double().mean()) >= 0.03
        if param:
            lin = float((d.abs() > param).double().mean())
            assert 0.05 < lin < 0.95, lin                   # both zones populated
        count = logical if reduction == 'mean' else 0
        w = f / count if count else f
        val, grad = _fp64_reference(kind, param, t, s, w, relu_mask)
        refs.append((val * w, grad))
        pairs.append((t.to(DEV), s.to(DEV), torch.full(t.shape, float('nan'), device=DEV), f, relu_mask, kind, param, count))
    out = ops.MimicLaunch(pairs, DEV).run().cpu()
    ops.sync_check()
    total = float(sum(r[0] for r in refs))
    worst = abs(float(out[0]) - total) / total
    assert worst <= 1e-6
    for i, (term, grad) in enumerate(refs):
        e_t = abs(float(out[1 + i]) - float(term)) / float(term)
        e_g = rel_l2(pairs[i][2].cpu(), grad)
        print('%s %s relu_mask=%d pair %d: term %.2e gradient %.2e' % (kind, reduction, relu_mask, i, e_t, e_g))
        assert e_t <= 1e-6, (i, e_t)
        assert e_g < 1e-6, (i, e_g)
        got = pairs[i][2].cpu()
        zero = (data[i][1] == data[i][0])
        if kind != 'mse':
            assert bool((got[zero] == 0).all())             # sign(0) = 0, in both zones' formulas
        if data[i][0].shape[-1] == 4:
            assert bool((got[..., 3] == 0).all())           # nothing flows into the padded channel


def test_smooth_l1_with_beta_zero_is_the_l1_launch_bit_for_bit(ops):
    data = _kernel_inputs(22)
    outs = []
    for kind in ('l1', 'smooth_l1'):
        pairs = [(t.to(DEV), s.to(DEV), torch.empty(t.shape, device=DEV), f, 1, kind, 0.0, logical)
                 for (t, s, logical), f in zip(data, FACTORS)]
        outs.append((ops.MimicLaunch(pairs, DEV).run().clone(), [p[2] for p in pairs]))
    ops.sync_check()
    assert torch.equal(outs[0][0], outs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


def test_huber_is_delta_times_smooth_l1_of_beta_delta(ops):
    """Huber(delta) = delta * SmoothL1(beta = delta): the extension of this project (the reference's factory has no Huber)
    against the criterion the reference-made fixture pins"""
    data = _kernel_inputs(23)[:4]
    delta = 0.6
    res = []
    for kind, scale in (('huber', 1.0), ('smooth_l1', delta)):
        pairs = [(t.to(DEV), s.to(DEV), torch.empty(t.shape, device=DEV), f * scale, 0, kind, delta, 0)
                 for (t, s, _), f in zip(data, FACTORS)]
        res.append((ops.MimicLaunch(pairs, DEV).run().cpu(), [p[2].cpu() for p in pairs]))
    ops.sync_check()
    assert float(((res[0][0] - res[1][0]).abs() / res[1][0]).max()) <= 1e-6
    for a, b in zip(res[0][1], res[1][1]):
        assert rel_l2(a, b) < 1e-6


# ------------------------------------------------------------------------------------------ bit identity
def test_mse_sum_through_the_new_entry_point_gives_the_bits_of_the_old_one(ops):
    g = gen(12)
    shapes = [(2, 9, 11, 256), (2, 5, 6, 512), (2, 3, 3, 1024), (2, 37, 41, 2048)]       # (the last one: many chunks)
    old, new = [], []
    for i, (shp, f) in enumerate(zip(shapes, [1.0, 0.5, 2.0, 0.3])):
        t = torch.randn(shp, generator=g).to(DEV)
        s = F.relu(torch.randn(shp, generator=g)).to(DEV)
        old.append((t, s, torch.empty(shp, device=DEV), f, i == 3))
        new.append((t, s, torch.empty(shp, device=DEV), f, i == 3, 'mse', 0.0, 0))
    a = ops.MseLaunch(old, DEV).run()
    b = ops.MimicLaunch(new, DEV).run()
    ops.sync_check()
    assert torch.equal(a, b)
    for p, q in zip(old, new):
        assert torch.equal(p[2], q[2])


def test_two_runs_of_a_mixed_launch_are_bit_identical(ops):
    data = _kernel_inputs(24)
    kinds = [('smooth_l1', 0.7, True), ('l1', 0.0, True), ('mse', 0.0, True), ('huber', 1.3, False), ('smooth_l1', 0.1, True)]
    runs = []
    for _ in range(2):
        pairs = [(t.to(DEV), s.to(DEV), torch.empty(t.shape, device=DEV), f, i == 3, k, p, logical if mean else 0)
                 for i, ((t, s, logical), f, (k, p, mean)) in enumerate(zip(data, FACTORS, kinds))]
        ml = ops.MimicLaunch(pairs, DEV)
        first = ml.run().clone()
        assert torch.equal(ml.run(), first)             # replay of the cached launch object
        runs.append((first, [p[2] for p in pairs]))
    ops.sync_check()
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


# ------------------------------------------------------------------------------------------ model
def _sync_oracle(orc, student):
    sd = student.state_dict()
    with torch.no_grad():
        for k, v in orc.s.items():
            if k in sd and v.is_floating_point():
                v.copy_(sd[k].detach().cpu().to(v.dtype))


def _grad_check(name, hip, ref32, ref64, tol=None):
    """the project's gradient rule (tests/test_model_gpu.py): as close to the exact (fp64) gradient as the reference's
    own fp32 path -- within GRAD_TOL, or within 2x the fp32 reference's error"""
    ref64 = ref64.double()
    e_hip = float((hip.cpu().double() - ref64).norm() / ref64.norm())
    e_ref = float((ref32.double() - ref64).norm() / ref64.norm())
    assert e_hip <= max(tol or GRAD_TOL, 2.0 * e_ref), '%s: HIP %.2e vs fp64, reference fp32 %.2e' % (name, e_hip, e_ref)
    return e_hip


def _hooked(model, path):
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import module_util
    return module_util.get_module(model, path).__dict__['distillation_box']['output']


def _to_dev(images, targets):
    return [im.to(DEV) for im in images], [{k: v.to(DEV) for k, v in t.items()} for t in targets]


def _kink_crossings(section, d_hip, d_64):
    """elements of a term whose difference sits on the other side of a kink of its criterion than in the fp64
    restatement: d = 0 for L1, |d| = beta / delta for SmoothL1 / Huber, none for MSE"""
    kind, params = section['type'], section['params']
    if kind == 'L1Loss':
        return int((torch.sign(d_hip) != torch.sign(d_64)).sum())
    if kind == 'SmoothL1Loss':
        beta = params.get('beta', 1.0)
        return int(((d_hip.abs() < beta) != (d_64.abs() < beta)).sum() + ((torch.sign(d_hip) != torch.sign(d_64)) &
                                                                         (d_64.abs() >= beta)).sum())
    if kind == 'HuberLoss':
        delta = params.get('delta', 1.0)
        return int(((d_hip.abs() <= delta) != (d_64.abs() <= delta)).sum() + ((torch.sign(d_hip) != torch.sign(d_64)) &
                                                                             (d_64.abs() > delta)).sum())
    return 0


def test_distill_steps_with_four_criteria_match_the_reference_made_fixture():
    """tiny_ghnd_criteria.npz: SmoothL1(mean) / L1(mean) / MSE(mean) / SmoothL1(sum, beta 0.02) on layer1..4, written by
    the reference's own DistillationBox -> backward -> Adam.  Loss and per-term values within LOSS_TOL, maps within
    FEAT_TOL, every gradient through the project's rule, parameters after two Adam steps as the other tiny fixtures."""
    from hnd_ghnd_object_detectors_amd import ops
    from hnd_ghnd_object_detectors_amd.distillation.tool import DistillationBox
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util
    from hnd_ghnd_object_detectors_amd.utils import main_util
    z, meta = G.load('tiny_ghnd_criteria')
    crit = meta['criterion']
    cfg = CU.apply_criteria(MU.config_for(meta), crit)
    t_sd, s_sd = MU.oracle_states(meta['seed'], meta['model'])
    teacher, student = MU.build_pair(cfg, t_sd, s_sd, DEV)
    box = DistillationBox(teacher, student, cfg['train']['criterion'])
    opt = func_util.get_optimizer(student, 'Adam', {'lr': 1e-3})
    warm = main_util.warmup_lr_scheduler(opt, 4, 1e-3)
    images, targets = G.case_inputs(meta)
    kw = dict(min_size=(meta['min_size'],), max_size=meta['max_size'])
    orc64, orc32 = CU.CriteriaOracle(t_sd, s_sd, crit, dtype=torch.float64, **kw), CU.CriteriaOracle(t_sd, s_sd, crit, **kw)
    worst = {'feat': 0.0, 'loss': 0.0, 'grad': 0.0}
    before = dict(ops.LOSS_LAUNCHES)
    kinks = OrderedDict()
    for step in range(meta['steps']):
        ims, tgs = _to_dev(images, targets)
        _sync_oracle(orc64, student)
        _sync_oracle(orc32, student)
        _, _, t64, s64, _, _, _ = orc64.forward(images, update_buffers=False)
        _, _, g64, _ = orc64.step(images)
        _, _, g32, _ = orc32.step(images)
        loss = box(ims, tgs)
        ref_loss = float(z['step%d/loss' % step])
        worst['loss'] = max(worst['loss'], abs(loss.item() - ref_loss) / abs(ref_loss))
        per_term = loss.per_term.cpu()
        for i, k in enumerate(crit):
            ref = float(z['step%d/term/%s' % (step, k)])
            print('step %d term %s: HIP %.8g reference %.8g' % (step, k, float(per_term[i]), ref))
            worst['loss'] = max(worst['loss'], abs(float(per_term[i]) - ref) / abs(ref))
            path = cfg['train']['criterion']['terms'][k]['ts_modules']
            t_out, s_out = _hooked(teacher, path[0]).cpu(), _hooked(student, path[1]).cpu()
            kinks['step%d/%s' % (step, k)] = (_kink_crossings(crit[k]['criterion'], (s_out - t_out).double(),
                                                              (s64[k] - t64[k]).detach()), s_out.numel())
            if step == 0:
                worst['feat'] = max(worst['feat'], G.compare(z, 'step0/teacher/' + k, t_out.contiguous(), FEAT_TOL),
                                    G.compare(z, 'step0/student/' + k, s_out.contiguous(), FEAT_TOL))
        opt.zero_grad()
        loss.backward()
        assert abs(opt.param_groups[0]['lr'] - float(z['step%d/lr' % step])) < 1e-12
        for n, p in student.named_parameters():
            if p.requires_grad and n not in O.ZERO_GRAD_KEYS:
                key = 'step%d/grad/%s' % (step, n)
                ref32 = torch.from_numpy(z[key]) if key in z.files else g32[n]
                e = _grad_check(n, p.grad, ref32, g64[n])
                worst['grad'] = max(worst['grad'], e)
                if key not in z.files:
                    G.compare(z, key, p.grad, 5e-2)         # checksum form: the stored fingerprint, loosely
        opt.step()
        warm.step()
    line = ('[tiny_ghnd_criteria] maps %.2e, loss / terms %.2e, gradients vs fp64 %.2e; elements across a kink of their '
            'criterion vs the fp64 restatement: %s' % (worst['feat'], worst['loss'], worst['grad'], ', '.join(
                '%s %d of %d' % (k, v[0], v[1]) for k, v in kinks.items())))
    print('\n' + line)
    assert worst['loss'] < LOSS_TOL, worst
    assert ops.LOSS_LAUNCHES['hnd_mimic_loss_fwd_bwd'] == before['hnd_mimic_loss_fwd_bwd'] + meta['steps']
    assert ops.LOSS_LAUNCHES['hnd_mse_sum_fwd_bwd'] == before['hnd_mse_sum_fwd_bwd']      # one launch for ALL terms
    sd = student.state_dict()
    ptol = 5e-3 if worst['grad'] > 1e-4 else 1e-3           # (test_distill_steps_match_reference_golden's rule)
    worst['param'] = max(G.compare(z, 'after/param/' + n, sd[n], ptol, atol=1e-6)
                         for n in O.trainable_keys(s_sd) if n not in O.ZERO_GRAD_KEYS)
    for n in z.files:
        if n.startswith('after/buffer/'):
            ref = torch.from_numpy(z[n]).double()
            got = sd[n[len('after/buffer/'):]].cpu().double()
            assert float((got - ref).abs().max()) <= 1e-4 * (1 + float(ref.abs().max())), n
    from tests.conftest import record_achieved
    record_achieved(line + '; parameters after 2 Adam steps %.2e (held to %.0e)' % (worst['param'], ptol))


def test_mean_reduction_divides_by_the_logical_count_of_the_padded_bottleneck_tensor():
    """MSELoss(reduction='mean') on backbone.body.layer1.encoder: the tensor has 3 channels and is stored with 4, so the
    divisor is N*3*H*W -- dividing by the buffer's element count is a 4/3 error in the term and its gradient."""
    from hnd_ghnd_object_detectors_amd.distillation.tool import DistillationBox
    from hnd_ghnd_object_detectors_amd.hipnn import to_nhwc
    z, meta = G.load('tiny_enc_term')
    mean_mse = {'type': 'MSELoss', 'params': {'reduction': 'mean'}}
    sum_mse = {'type': 'MSELoss', 'params': {'reduction': 'sum'}}
    # (factors: alone, the two terms then give parameter-gradient norms of 193 and 131 in the fp64 restatement)
    criteria = OrderedDict((tn, {'criterion': mean_mse if tn == 'enc' else sum_mse, 'factor': 1.0 if tn == 'enc' else 1e-2})
                           for tn, _, _, _ in meta['terms'])
    paths = {tn: (O.rel_key(tp), O.rel_key(sp)) for tn, tp, sp, _ in meta['terms']}
    cfg = MU.config_for(meta)
    cfg['train']['criterion']['terms'] = OrderedDict(
        (tn, {'ts_modules': [tp, sp], 'criterion': copy.deepcopy(criteria[tn]['criterion']), 'factor': criteria[tn]['factor']})
        for tn, tp, sp, _ in meta['terms'])
    t_sd, s_sd = MU.oracle_states(meta['seed'], meta['model'])
    t_sd = O.init_student_state(t_sd, meta['seed'] + 500)
    cfg['teacher_model'] = copy.deepcopy(cfg['student_model'])
    teacher, student = MU.build_pair(cfg, t_sd, s_sd, DEV)
    box = DistillationBox(teacher, student, cfg['train']['criterion'])
    images, targets = G.case_inputs(meta)
    kw = dict(paths=paths, min_size=(meta['min_size'],), max_size=meta['max_size'], teacher_is_student_arch=True)
    orc64 = CU.CriteriaOracle(t_sd, s_sd, criteria, dtype=torch.float64, **kw)
    orc32 = CU.CriteriaOracle(t_sd, s_sd, criteria, **kw)
    l64, terms64, g64, _ = orc64.step(images)
    _, _, g32, _ = orc32.step(images)
    ims, tgs = _to_dev(images, targets)
    loss = box(ims, tgs)
    enc = _hooked(student, 'backbone.body.layer1.encoder')
    assert enc.shape[1] == 3 and to_nhwc(enc).shape[-1] == 4           # logical 3 channels in a 4-channel buffer
    got = [float(v) for v in loss.per_term.cpu()]
    print('enc term: HIP %.8g fp64 %.8g (a divisor of numel would give %.8g); layer2 term: HIP %.8g fp64 %.8g'
          % (got[0], terms64['enc'], terms64['enc'] * 0.75, got[1], terms64['layer2']))
    assert abs(got[0] - terms64['enc']) <= LOSS_TOL * terms64['enc']
    assert abs(got[1] - terms64['layer2']) <= LOSS_TOL * terms64['layer2']
    assert abs(loss.item() - l64) <= LOSS_TOL * l64
    assert terms64['enc'] > 0.2 * terms64['layer2']                      # the mean term is not hidden behind the other
    loss.backward()
    for n, p in student.named_parameters():
        if p.requires_grad and n not in O.ZERO_GRAD_KEYS:
            _grad_check(n, p.grad, g32[n], g64[n])


def test_all_mse_sum_criterion_takes_the_old_launch_and_its_bits():
    """the default path is untouched: an all-MSELoss(sum) criterion section launches hnd_mse_sum_fwd_bwd through
    ops.MseLaunch -- loss, per-term values, loss gradients and the flat gradient arena are the bits of a direct
    ops.MseLaunch over the same maps -- and never reaches hnd_mimic_loss_fwd_bwd."""
    from hnd_ghnd_object_detectors_amd import ops
    from hnd_ghnd_object_detectors_amd.distillation import hip_loss
    from hnd_ghnd_object_detectors_amd.distillation.tool import DistillationBox
    z, meta = G.load('tiny_ghnd_faster')
    cfg = MU.config_for(meta)
    for term in cfg['train']['criterion']['terms'].values():
        assert term['criterion'] == {'type': 'MSELoss', 'params': {'reduction': 'sum'}}
    t_sd, s_sd = MU.oracle_states(meta['seed'], meta['model'])
    teacher, student = MU.build_pair(cfg, t_sd, s_sd, DEV)
    box = DistillationBox(teacher, student, cfg['train']['criterion'])
    images, targets = G.case_inputs(meta)
    before = dict(ops.LOSS_LAUNCHES)
    loss = box(*_to_dev(images, targets))
    body = student.backbone.body
    launch = body._loss_cache[1]
    assert type(launch) is ops.MseLaunch
    node = loss.grad_fn                 # the _DistillLossFn node (behind the alias node of the StepLoss subclass)
    while not hasattr(node, 'state'):
        node = node.next_functions[0][0]
    assert ops.LOSS_LAUNCHES['hnd_mimic_loss_fwd_bwd'] == before['hnd_mimic_loss_fwd_bwd']
    assert ops.LOSS_LAUNCHES['hnd_mse_sum_fwd_bwd'] == before['hnd_mse_sum_fwd_bwd'] + 1
    step_out = launch.out.clone()
    step_grads = [p[2].clone() for p in launch.keep]
    assert torch.equal(loss.detach(), step_out[0].float()) and torch.equal(loss.per_term, step_out[1:])
    loss.backward()
    arena = body._grad_arena
    step_flat = arena.flat[arena.cur].clone()
    assert float(step_flat.abs().sum()) > 0
    for p in arena.params:
        p.grad = None
    # a direct launch over the same maps, into the step's own gradient buffers, then the same backward plan once more
    direct = ops.MseLaunch([tuple(p) for p in launch.keep], DEV)
    for p in launch.keep:
        p[2].fill_(float('nan'))
    direct_out = direct.run()
    assert torch.equal(direct_out, step_out)
    assert all(torch.equal(p[2], g) for p, g in zip(launch.keep, step_grads))
    hip_loss._DistillLossFn.backward(node, torch.ones((), device=DEV))
    ops.sync_check()
    assert torch.equal(arena.flat[arena.cur], step_flat)
    assert ops.LOSS_LAUNCHES['hnd_mimic_loss_fwd_bwd'] == before['hnd_mimic_loss_fwd_bwd']


def test_mimic_runner_cli_with_the_criterion_replaced_through_json(tmp_path, capsys):
    """the runner end to end on the tiny synthetic setup of test_mimic_runner_cli_end_to_end, the criterion of the YAML
    replaced through --json exactly as the reference's users would: two iterations, a finite loss, and the mean loss of
    the epoch equals what DistillationBox gives for the same seed outside the runner."""
    import math
    from hnd_ghnd_object_detectors_amd import mimic_runner, ops
    from hnd_ghnd_object_detectors_amd.distillation.tool import DistillationBox
    from hnd_ghnd_object_detectors_amd.models import get_model
    from hnd_ghnd_object_detectors_amd.myutils.common import yaml_util
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util, module_util
    from hnd_ghnd_object_detectors_amd.utils import data_util, main_util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg_path = os.path.join(root, 'config', 'hnd', 'faster_rcnn-backbone_resnet50-b3ch.yaml')
    ckpt = str(tmp_path / 'student.pt')
    override = {'teacher_model': {'backbone': {'params': {'pretrained': False}},
                                  'params': {'pretrained': False, 'min_size': 64, 'max_size': 128},
                                  'ckpt': str(tmp_path / 'none.pt')},
                'student_model': {'backbone': {'params': {'pretrained': False}},
                                  'params': {'pretrained': False, 'min_size': 64, 'max_size': 128}, 'ckpt': ckpt},
                'train': {'batch_size': 2, 'log_freq': 1,
                          'criterion': {'terms': {'layer1': {'criterion': {'type': 'SmoothL1Loss',
                                                                           'params': {'reduction': 'mean', 'beta': 0.5}},
                                                             'factor': 2.0}}}}}
    argv = ['--config', cfg_path, '--json', json.dumps(override), '-distill', '--synthetic_batches', '2',
            '--image_size', '64x96', '--num_epochs', '1']
    before = ops.LOSS_LAUNCHES['hnd_mimic_loss_fwd_bwd']
    torch.manual_seed(0)
    mimic_runner.main(mimic_runner.get_argparser().parse_args(argv))
    out = capsys.readouterr().out
    assert 'Epoch: [0]' in out and 'Updating ckpt' in out
    assert ops.LOSS_LAUNCHES['hnd_mimic_loss_fwd_bwd'] == before + 2
    ck = torch.load(ckpt, weights_only=False)
    crit = ck['config']['train']['criterion']['terms']
    assert list(crit) == ['layer1'] and crit['layer1']['criterion']['type'] == 'SmoothL1Loss'
    runner_loss = ck['best_loss']
    assert math.isfinite(runner_loss) and runner_loss > 0

    # the same two iterations outside the runner
    config = yaml_util.load_yaml_file(cfg_path)
    main_util.overwrite_config(config, json.dumps(override))
    config['student_model']['ckpt'] = str(tmp_path / 'none.pt')     # (not the checkpoint the runner has just written)
    torch.manual_seed(0)
    teacher = get_model(config['teacher_model'], DEV)
    module_util.freeze_module_params(teacher)
    student = get_model(config['student_model'], DEV)
    mimic_runner.freeze_modules(student, config['student_model'])
    loader = data_util.SyntheticDetectionLoader(2, 2, 64, 96, config['student_model']['name'])
    box = DistillationBox(teacher, student, config['train']['criterion'])
    opt = func_util.get_optimizer(student, config['train']['optimizer']['type'], config['train']['optimizer']['params'])
    warm = main_util.warmup_lr_scheduler(opt, 1, 1.0 / 1000.0)
    teacher.eval()
    student.train()
    teacher.distill_backbone_only = student.distill_backbone_only = config['student_model']['distill_backbone_only']
    student.backbone.body.layer1.use_bottleneck_transformer = False
    losses = []
    for images, targets in loader:
        loss = box(*_to_dev(images, targets))
        opt.zero_grad()
        loss.backward()
        opt.step()
        warm.step()
        losses.append(loss.item())
    print('runner mean loss %.8g, DistillationBox %s' % (runner_loss, losses))
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    assert runner_loss == pytest.approx(sum(losses) / 2, rel=1e-6)
