#!/usr/bin/env python
"""Generate tests/golden/tiny_ghnd_criteria.npz FROM THE REFERENCE ITSELF: a distillation step whose four terms use four
different criteria (SmoothL1 / L1 / MSE with reduction='mean', SmoothL1(beta) with reduction='sum').

Same recipe as make_golden.py (whose helpers are imported, not copied): the reference's unmodified DistillationBox ->
backward -> Adam over oracle/shim, two steps on the tiny_ghnd_faster geometry with a seed of its own.  The criterion
section below is what the reference's CustomLoss parses (func_util.get_loss(type, params) per term) and is stored in the
fixture's ``meta`` as JSON.  Per-term values are computed with the reference's own criterion objects
(``box.criterion.term_dict``), called the way the reference calls them: criterion(teacher_output, student_output).

Before writing, the generator ASSERTS for its seed that
 (a) the parameter-gradient norm of every term ALONE is within a factor 10 of every other's (no term hides behind another:
     a wrong gradient of any one criterion moves the total by at least ~1/30), and
 (b) both zones of each SmoothL1 term hold at least 5 % of its elements.
HuberLoss is not here: the reference's factory (restated in oracle/myutils_r.py) knows mse / l1 / smoothl1 only.

usage:  python tests/golden/make_golden_criteria.py
"""
import json
import os
import sys
from collections import OrderedDict

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import O, DistillationBox, build_reference_models, func_util, hooked, main_util, make_inputs, \
    module_util, put  # noqa: E402

NAME = 'tiny_ghnd_criteria'
CRITERIA = OrderedDict((
    ('layer1', ({'type': 'SmoothL1Loss', 'params': {'reduction': 'mean'}}, 1.0)),
    ('layer2', ({'type': 'L1Loss', 'params': {'reduction': 'mean'}}, 1.0)),
    ('layer3', ({'type': 'MSELoss', 'params': {'reduction': 'mean'}}, 4.0)),
    ('layer4', ({'type': 'SmoothL1Loss', 'params': {'reduction': 'sum', 'beta': 0.02}}, 1e-4)),
))
CASE = dict(yaml='ghnd/faster_rcnn-backbone_resnet50-b3ch.yaml', model='faster_rcnn', sizes=[(60, 90), (56, 100)],
            min_size=64, max_size=128, steps=2, seed=51)


def criterion_section(config):
    crit = config['train']['criterion']
    for name, (sub, factor) in CRITERIA.items():
        crit['terms'][name]['criterion'] = json.loads(json.dumps(sub))
        crit['terms'][name]['factor'] = factor
    assert list(crit['terms']) == list(CRITERIA)
    return crit


def solo_grad_norms(box, student, images, targets):
    """parameter-gradient norm of each term alone (step-0 weights; BatchNorm buffers restored afterwards)"""
    saved = {k: v.clone() for k, v in student.state_dict().items()}
    full = box.criterion.term_dict
    norms = OrderedDict()
    for name in full:
        box.criterion.term_dict = {k: (v[0], v[1], v[2] if k == name else 0.0) for k, v in full.items()}
        student.zero_grad()
        box([im.clone() for im in images], [{k: v.clone() for k, v in t.items()} for t in targets]).backward()
        norms[name] = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for n, p in student.named_parameters()
                                           if p.requires_grad and n not in O.ZERO_GRAD_KEYS)))
        student.load_state_dict(saved)
    box.criterion.term_dict = full
    student.zero_grad()
    return norms


def main():
    torch.set_num_threads(8)
    case = dict(CASE)
    t_sd = O.init_teacher_state(case['seed'], case['model'])
    s_sd = O.init_student_state(t_sd, case['seed'] + 1000)
    config, teacher, student = build_reference_models(case)
    teacher.load_state_dict(t_sd, strict=True)
    student.load_state_dict(s_sd, strict=True)
    assert module_util.get_updatable_param_names(student) == O.trainable_keys(s_sd)
    crit = criterion_section(config)
    box = DistillationBox(teacher, student, crit)
    opt_cfg = config['train']['optimizer']
    optimizer = func_util.get_optimizer(student, opt_cfg['type'], opt_cfg['params'])
    warm = main_util.warmup_lr_scheduler(optimizer, 4, 1.0 / 1000.0)
    teacher.eval()
    student.train()
    teacher.distill_backbone_only = True
    student.distill_backbone_only = True
    student.backbone.body.layer1.use_bottleneck_transformer = False
    images, targets = make_inputs(case)

    norms = solo_grad_norms(box, student, images, targets)
    print('   solo gradient norms: %s' % ', '.join('%s %.4g' % kv for kv in norms.items()))
    assert max(norms.values()) <= 10.0 * min(norms.values()), 'a term hides behind another: adjust its factor'

    out = OrderedDict()
    zones = OrderedDict()
    for step in range(case['steps']):
        loss = box([im.clone() for im in images], [{k: v.clone() for k, v in t.items()} for t in targets])
        optimizer.zero_grad()
        loss.backward()
        grads = OrderedDict((n, p.grad.detach().clone()) for n, p in student.named_parameters() if p.requires_grad)
        lr_used = optimizer.param_groups[0]['lr']
        optimizer.step()
        warm.step()
        pre = 'step%d/' % step
        out[pre + 'loss'] = np.float64(loss.item())
        out[pre + 'lr'] = np.float64(lr_used)
        for name, (paths, criterion, factor) in box.criterion.term_dict.items():
            t_out, s_out = hooked(teacher, paths[0]), hooked(student, paths[1])
            out[pre + 'term/' + name] = np.float64((criterion(t_out, s_out) * factor).item())
            if step == 0:
                put(out, pre + 'teacher/' + name, t_out)
                put(out, pre + 'student/' + name, s_out)
                if isinstance(criterion, torch.nn.SmoothL1Loss):
                    lin = float(((s_out - t_out).abs() >= criterion.beta).double().mean())
                    zones[name] = {'beta': criterion.beta, 'linear_share': lin}
                    assert 0.05 <= lin <= 0.95, (name, lin)
                if isinstance(criterion, (torch.nn.L1Loss, torch.nn.SmoothL1Loss)):
                    zones.setdefault(name, {})['zero_share'] = float(((s_out - t_out) == 0).double().mean())
        for n, g in grads.items():
            put(out, pre + 'grad/' + n, g, full_limit=20000)
    print('   zones: %s' % json.dumps(zones))
    sd_after = student.state_dict()
    for n in O.trainable_keys(s_sd):
        put(out, 'after/param/' + n, sd_after[n], full_limit=20000)
    for n, v in sd_after.items():
        if 'layer1' in n and ('running_' in n or 'num_batches' in n):
            out['after/buffer/' + n] = v.numpy()
    meta = dict(case)
    meta['criterion'] = OrderedDict((name, {'criterion': sub, 'factor': factor}) for name, (sub, factor) in CRITERIA.items())
    meta['solo_grad_norms'] = norms
    meta['zones'] = zones
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **out)
    print('   loss(step0)=%.6f  wrote %s (%.1f KB)' % (float(out['step0/loss']), path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
