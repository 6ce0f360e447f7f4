#!/usr/bin/env python
"""Generate tests/golden/tiny_ghnd_shared_terms.npz FROM THE REFERENCE ITSELF: a distillation step with TWO terms on each
of two student tensors -- MSELoss(sum) + L1Loss(mean) on layer4 (the top, ReLU-masked tensor of the backward plan) and
SmoothL1Loss(mean) + MSELoss(mean) on layer2 (a layer output below it).

The reference keeps one hook slot per module and keys its outputs by the teacher slot, so two terms that name the same
teacher module collapse into the later one; a reference user who wants two criteria on one map names the teacher through an
alias of the same tensor -- `backbone.body.layer4.2` is the last Bottleneck of layer4, whose output IS the layer's.  The
section below does that; the student path is the plain layer on both terms, so both read one student tensor and autograd
adds their gradients on it.

Same recipe as make_golden_criteria.py (helpers imported from make_golden.py, nothing copied): the reference's unmodified
DistillationBox -> backward -> Adam over oracle/shim, two steps on the tiny_ghnd_faster geometry with a seed of its own.

Before writing, the generator ASSERTS for its seed that
 (a) the parameter-gradient norm of every term ALONE is within a factor 10 of every other's (no term hides behind its group
     partner), and
 (b) both zones of the SmoothL1 term hold at least 5 % of its elements.
Both figures are stored in the fixture's ``meta``.

usage:  python tests/golden/make_golden_shared_terms.py
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

NAME = 'tiny_ghnd_shared_terms'
BODY = 'backbone.body.'
# name -> (teacher path, student path, criterion, factor)
TERMS = OrderedDict((
    ('l4_mse', ('layer4', 'layer4', {'type': 'MSELoss', 'params': {'reduction': 'sum'}}, 2e-4)),
    ('l4_l1', ('layer4.2', 'layer4', {'type': 'L1Loss', 'params': {'reduction': 'mean'}}, 1.0)),
    ('l2_sl1', ('layer2', 'layer2', {'type': 'SmoothL1Loss', 'params': {'reduction': 'mean', 'beta': 0.1}}, 1.0)),
    ('l2_mse', ('layer2.3', 'layer2', {'type': 'MSELoss', 'params': {'reduction': 'mean'}}, 1.0)),
))
CASE = dict(yaml='ghnd/faster_rcnn-backbone_resnet50-b3ch.yaml', model='faster_rcnn', sizes=[(60, 90), (56, 100)],
            min_size=64, max_size=128, steps=2, seed=67)


def criterion_section(config):
    crit = config['train']['criterion']
    crit['terms'] = OrderedDict(
        (name, {'ts_modules': [BODY + tp, BODY + sp], 'criterion': json.loads(json.dumps(sub)), 'factor': factor})
        for name, (tp, sp, sub, factor) in TERMS.items())
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
    assert list(box.criterion.term_dict) == list(TERMS)
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
        total = 0.0
        for name, (paths, criterion, factor) in box.criterion.term_dict.items():
            t_out, s_out = hooked(teacher, paths[0]), hooked(student, paths[1])
            out[pre + 'term/' + name] = np.float64((criterion(t_out, s_out) * factor).item())
            total += float(out[pre + 'term/' + name])
            if step == 0:
                put(out, pre + 'teacher/' + name, t_out)
                put(out, pre + 'student/' + name, s_out)
                if isinstance(criterion, torch.nn.SmoothL1Loss):
                    ad = (s_out - t_out).abs()
                    lin = float((ad >= criterion.beta).double().mean())
                    zones[name] = {'beta': criterion.beta, 'linear_share': lin}
                    assert 0.05 <= lin <= 0.95, (name, lin)
                if isinstance(criterion, (torch.nn.L1Loss, torch.nn.SmoothL1Loss)):
                    zones.setdefault(name, {})['zero_share'] = float(((s_out - t_out) == 0).double().mean())
        # every term is in the loss: nothing collapsed into a later term of the same teacher slot
        assert abs(total - float(out[pre + 'loss'])) <= 1e-5 * abs(total), (total, float(out[pre + 'loss']))
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
    meta['criterion'] = OrderedDict((name, {'ts_modules': [BODY + tp, BODY + sp], 'criterion': sub, 'factor': factor})
                                    for name, (tp, sp, sub, factor) in TERMS.items())
    meta['solo_grad_norms'] = norms
    meta['zones'] = zones
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(HERE, NAME + '.npz')
    np.savez_compressed(path, **out)
    print('   loss(step0)=%.6f  wrote %s (%.1f KB)' % (float(out['step0/loss']), path, os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
