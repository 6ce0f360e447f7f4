"""GPU, model level: several loss terms on ONE student tensor.  Their pairs share the position's gradient buffer, the loss
launch adds their gradients and stores the sum once (a group of hnd_mimic_loss_fwd_bwd), and the backward plan runs once.

 * the reference-made fixture tests/golden/tiny_ghnd_shared_terms.npz: MSELoss(sum) + L1Loss(mean) on layer4 (the top,
   ReLU-masked tensor) and SmoothL1Loss(mean) + MSELoss(mean) on layer2 (a layer output below it), the second term of each
   tensor naming the teacher through the alias the reference's users need (`layer4.2`, `layer2.3`);
 * positions with no teacher-side alias -- the bottleneck tensor, a pyramid map, an inner Bottleneck below the top --
   through distill_loss directly: the gradients of [A, B] against those of the single-term runs, g_A + g_B;
 * autograd's grad_output reaches a shared buffer once;
 * the runner's command line.
Bars and helpers: tests/test_mimic_loss_gpu.py (constants imported, helper logic copied)."""
import copy
import json
import math
import os
from collections import OrderedDict

import pytest
import torch

from oracle import hnd_oracle as O
from tests import criteria_util as CU
from tests import golden_util as G
from tests import model_util as MU
from tests.test_mimic_loss_gpu import FEAT_TOL, GRAD_TOL, LOSS_TOL

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NAME = 'tiny_ghnd_shared_terms'


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


def _shared_terms_setup():
    """(z, meta, crit, cfg, teacher, student, box, images, targets, t_sd, s_sd) of the fixture's section"""
    from hnd_ghnd_object_detectors_amd.distillation.tool import DistillationBox
    z, meta = G.load(NAME)
    crit = meta['criterion']
    cfg = MU.config_for(meta)
    proto = copy.deepcopy(cfg['train']['criterion']['terms'])
    cfg['train']['criterion']['terms'] = OrderedDict(
        (k, {'ts_modules': list(c['ts_modules']), 'criterion': copy.deepcopy(c['criterion']), 'factor': c['factor']})
        for k, c in crit.items())
    assert proto                                            # (the YAML's own terms are replaced, as --json would)
    t_sd, s_sd = MU.oracle_states(meta['seed'], meta['model'])
    teacher, student = MU.build_pair(cfg, t_sd, s_sd, DEV)
    box = DistillationBox(teacher, student, cfg['train']['criterion'])
    images, targets = G.case_inputs(meta)
    return z, meta, crit, cfg, teacher, student, box, images, targets, t_sd, s_sd


def test_distill_steps_with_two_terms_on_each_of_two_tensors_match_the_reference_made_fixture():
    """tiny_ghnd_shared_terms.npz, written by the reference's own DistillationBox -> backward -> Adam.  Loss and per-term
    values within LOSS_TOL, maps within FEAT_TOL, every gradient through the project's rule, parameters after two Adam
    steps as the other tiny fixtures; one launch of the general entry point per step."""
    from hnd_ghnd_object_detectors_amd import ops
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util
    from hnd_ghnd_object_detectors_amd.utils import main_util
    z, meta, crit, cfg, teacher, student, box, images, targets, t_sd, s_sd = _shared_terms_setup()
    opt = func_util.get_optimizer(student, 'Adam', {'lr': 1e-3})
    warm = main_util.warmup_lr_scheduler(opt, 4, 1e-3)
    paths = {k: (O.rel_key(c['ts_modules'][0]), O.rel_key(c['ts_modules'][1])) for k, c in crit.items()}
    kw = dict(paths=paths, min_size=(meta['min_size'],), max_size=meta['max_size'])
    orc64, orc32 = CU.CriteriaOracle(t_sd, s_sd, crit, dtype=torch.float64, **kw), CU.CriteriaOracle(t_sd, s_sd, crit, **kw)
    worst = {'feat': 0.0, 'loss': 0.0, 'grad': 0.0}
    before = dict(ops.LOSS_LAUNCHES)
    for step in range(meta['steps']):
        ims, tgs = _to_dev(images, targets)
        _sync_oracle(orc64, student)
        _sync_oracle(orc32, student)
        _, _, g64, _ = orc64.step(images)
        _, _, g32, _ = orc32.step(images)
        loss = box(ims, tgs)
        ref_loss = float(z['step%d/loss' % step])
        worst['loss'] = max(worst['loss'], abs(loss.item() - ref_loss) / abs(ref_loss))
        per_term = loss.per_term.cpu()
        assert len(per_term) == len(crit)
        for i, k in enumerate(crit):
            ref = float(z['step%d/term/%s' % (step, k)])
            print('step %d term %s: HIP %.8g reference %.8g' % (step, k, float(per_term[i]), ref))
            worst['loss'] = max(worst['loss'], abs(float(per_term[i]) - ref) / abs(ref))
            if step == 0:
                tp, sp = crit[k]['ts_modules']
                t_out, s_out = _hooked(teacher, tp).cpu(), _hooked(student, sp).cpu()
                worst['feat'] = max(worst['feat'], G.compare(z, 'step0/teacher/' + k, t_out.contiguous(), FEAT_TOL),
                                    G.compare(z, 'step0/student/' + k, s_out.contiguous(), FEAT_TOL))
        opt.zero_grad()
        loss.backward()
        assert abs(opt.param_groups[0]['lr'] - float(z['step%d/lr' % step])) < 1e-12
        for n, p in student.named_parameters():
            if p.requires_grad and n not in O.ZERO_GRAD_KEYS:
                key = 'step%d/grad/%s' % (step, n)
                ref32 = torch.from_numpy(z[key]) if key in z.files else g32[n]
                worst['grad'] = max(worst['grad'], _grad_check(n, p.grad, ref32, g64[n]))
                if key not in z.files:
                    G.compare(z, key, p.grad, 5e-2)         # checksum form: the stored fingerprint, loosely
        opt.step()
        warm.step()
    line = '[%s] maps %.2e, loss / terms %.2e, gradients vs fp64 %.2e' % (NAME, worst['feat'], worst['loss'], worst['grad'])
    print('\n' + line)
    assert worst['feat'] < FEAT_TOL and worst['loss'] < LOSS_TOL, worst
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


def test_grad_output_reaches_a_shared_gradient_buffer_once():
    """(2 * loss).backward() gives exactly twice the gradients of loss.backward(): a power of two is exact, so a buffer
    listed twice in grad_bufs -- scaled twice -- shows as a factor 4"""
    _, _, _, _, _, student, box, images, targets, _, _ = _shared_terms_setup()
    params = [(n, p) for n, p in student.named_parameters() if p.requires_grad]
    grads = []
    for scale in (1, 2):
        for _, p in params:
            p.grad = None
        loss = box(*_to_dev(images, targets))
        (loss if scale == 1 else loss * scale).backward()
        grads.append([p.grad.clone() for _, p in params])
    torch.cuda.synchronize()
    assert any(float(g.abs().max()) > 0 for g in grads[0])
    for (n, _), a, b in zip(params, grads[0], grads[1]):
        assert torch.equal(b, a * 2), n


# ------------------------------------------------------------------------------------------ positions without an alias
def _position_case(position):
    """(fixture, path of the shared student tensor, path of another term C kept in the runs that have one)"""
    return {'bottleneck tensor': ('tiny_enc_term', 'backbone.body.layer1.encoder', 'backbone.body.layer2'),
            'pyramid map': ('tiny_ghnd_fpn_term', 'backbone.fpn.layer_blocks.1', 'backbone.body.layer3'),
            'inner Bottleneck below the top': ('tiny_ghnd_fpn_term', 'backbone.body.layer2.1', 'backbone.body.layer3')}[position]


@pytest.mark.parametrize('position', ['bottleneck tensor', 'pyramid map', 'inner Bottleneck below the top'])
def test_two_terms_on_a_tensor_without_an_alias_give_the_sum_of_the_single_term_gradients(position):
    """distill_loss([A, B, C]) with A = MSELoss(sum) and B = SmoothL1Loss(mean) on tensor X and C = MSELoss(sum) elsewhere,
    against distill_loss([A, C]) and distill_loss([B]) -- launches and backward plans that exist without this feature and
    are pinned to the reference.  loss_AB = loss_A + loss_B within LOSS_TOL; rel-L2 of g_AB - (g_A + g_B) within GRAD_TOL on
    every parameter gradient (each side an independent fp32 pass held to GRAD_TOL; the achieved figure is printed and
    recorded, orders of magnitude below).  B's factor is the power of two that brings its parameter-gradient norm next to
    A's, found from a first run of B with factor 1, so neither term hides behind the other."""
    from hnd_ghnd_object_detectors_amd.distillation import hip_loss
    from hnd_ghnd_object_detectors_amd.distillation.tool import DistillationBox
    fixture, x_path, c_path = _position_case(position)
    z, meta = G.load(fixture)
    cfg = MU.config_for(meta)
    crit = cfg['train']['criterion']
    proto = next(iter(crit['terms'].values()))['criterion']
    hooks = [x_path, c_path]
    crit['terms'] = OrderedDict(('h%d' % i, {'ts_modules': [p, p], 'criterion': proto, 'factor': 1.0})
                                for i, p in enumerate(hooks))
    t_sd, s_sd = MU.oracle_states(meta['seed'], meta['model'])
    if meta.get('teacher') == 'student_arch':
        t_sd = O.init_student_state(t_sd, meta['seed'] + 500)
        cfg['teacher_model'] = copy.deepcopy(cfg['student_model'])
    teacher, student = MU.build_pair(cfg, t_sd, s_sd, DEV)
    box = DistillationBox(teacher, student, crit)
    images, targets = G.case_inputs(meta)
    params = [(n, p) for n, p in student.named_parameters() if p.requires_grad and n not in O.ZERO_GRAD_KEYS]
    mse_sum = hip_loss.HipMSELoss(reduction='sum')

    def run(with_a, b_factor, with_c):
        """a fresh forward (train-mode BatchNorm: the same maps every time), then the loss over the chosen terms"""
        for _, p in params:
            p.grad = None
        box(*_to_dev(images, targets))
        tx, sx = _hooked(teacher, x_path), _hooked(student, x_path)
        terms = []
        if with_a:
            terms.append(('A', tx, sx, 1e-2, mse_sum))
        if b_factor:
            beta = 0.5 * float((sx.detach() - tx.detach()).abs().median()) + 1e-6   # both zones populated
            terms.append(('B', tx, sx, b_factor, hip_loss.HipSmoothL1Loss(reduction='mean', beta=beta)))
        if with_c:
            terms.append(('C', _hooked(teacher, c_path), _hooked(student, c_path), 1e-2, mse_sum))
        loss = hip_loss.distill_loss(terms)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.item()), [torch.zeros_like(p) if p.grad is None else p.grad.detach().clone() for _, p in params]

    def norm(gs):
        return math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
    loss_a, g_a = run(True, 0.0, True)
    _, g_b1 = run(False, 1.0, False)
    f_b = 2.0 ** round(math.log2(norm(g_a) / norm(g_b1)))
    loss_b, g_b = run(False, f_b, False)
    loss_ab, g_ab = run(True, f_b, True)
    assert 0.1 < norm(g_b) / norm(g_a) < 10.0
    e_loss = abs(loss_ab - (loss_a + loss_b)) / (loss_a + loss_b)
    worst, where = 0.0, None
    for (n, _), ab, a, b in zip(params, g_ab, g_a, g_b):
        ref = a.double() + b.double()
        if float(ref.abs().max()) == 0.0:                   # (no path from X or C to this parameter)
            assert float(ab.abs().max()) == 0.0, n
            continue
        e = float((ab.double() - ref).norm() / ref.norm())
        if e > worst:
            worst, where = e, n
    line = ('[two terms on the %s, %s] loss_AB vs loss_A + loss_B %.2e; worst rel-L2 of g_AB - (g_A + g_B) %.2e (%s); |g_B| / '
            '|g_A| %.2f with factor_B = %g' % (position, x_path, e_loss, worst, where, norm(g_b) / norm(g_a), f_b))
    print('\n' + line)
    assert e_loss < LOSS_TOL, e_loss
    assert worst < GRAD_TOL, (where, worst)
    from tests.conftest import record_achieved
    record_achieved(line)


# ------------------------------------------------------------------------------------------ CLI
def test_mimic_runner_cli_with_a_second_term_on_layer4_through_json(tmp_path, capsys):
    """the runner end to end at the tiny synthetic size of test_mimic_runner_cli_with_the_criterion_replaced_through_json:
    --json adds an L1Loss(mean) term on the student's layer4 beside the YAML's MSELoss(sum) one, the teacher named through
    its alias layer4.2 as a user of the reference would.  Two iterations, a finite loss, one general launch per step."""
    from hnd_ghnd_object_detectors_amd import mimic_runner, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg_path = os.path.join(root, 'config', 'ghnd', 'faster_rcnn-backbone_resnet50-b3ch.yaml')
    ckpt = str(tmp_path / 'student.pt')
    override = {'teacher_model': {'backbone': {'params': {'pretrained': False}},
                                  'params': {'pretrained': False, 'min_size': 64, 'max_size': 128},
                                  'ckpt': str(tmp_path / 'none.pt')},
                'student_model': {'backbone': {'params': {'pretrained': False}},
                                  'params': {'pretrained': False, 'min_size': 64, 'max_size': 128}, 'ckpt': ckpt},
                'train': {'batch_size': 2, 'log_freq': 1,
                          'criterion': {'terms': {'layer4_l1': {
                              'ts_modules': ['backbone.body.layer4.2', 'backbone.body.layer4'],
                              'criterion': {'type': 'L1Loss', 'params': {'reduction': 'mean'}}, 'factor': 100.0}}}}}
    argv = ['--config', cfg_path, '--json', json.dumps(override), '-distill', '--synthetic_batches', '2',
            '--image_size', '64x96', '--num_epochs', '1']
    before = dict(ops.LOSS_LAUNCHES)
    torch.manual_seed(0)
    mimic_runner.main(mimic_runner.get_argparser().parse_args(argv))
    out = capsys.readouterr().out
    assert 'Epoch: [0]' in out and 'Updating ckpt' in out
    assert ops.LOSS_LAUNCHES['hnd_mimic_loss_fwd_bwd'] == before['hnd_mimic_loss_fwd_bwd'] + 2
    assert ops.LOSS_LAUNCHES['hnd_mse_sum_fwd_bwd'] == before['hnd_mse_sum_fwd_bwd']
    ck = torch.load(ckpt, weights_only=False)
    terms = ck['config']['train']['criterion']['terms']
    assert 'layer4' in terms and terms['layer4_l1']['ts_modules'][1] == terms['layer4']['ts_modules'][1]
    assert math.isfinite(ck['best_loss']) and ck['best_loss'] > 0
