"""CPU restatement of a distillation step whose terms carry their own criterion (tests/golden/tiny_ghnd_criteria.npz):
the oracle's backbone (oracle.hnd_oracle, imported, not edited) for the hooked maps, torch.nn criteria called the way the
reference calls them -- criterion(teacher_output, student_output) -- for the loss."""
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

from oracle import hnd_oracle as O

TORCH_CRITERIA = {'MSELoss': nn.MSELoss, 'L1Loss': nn.L1Loss, 'SmoothL1Loss': nn.SmoothL1Loss, 'HuberLoss': nn.HuberLoss}


def torch_criterion(section):
    """{'type': ..., 'params': {...}} of a YAML term -> the torch.nn module"""
    return TORCH_CRITERIA[section['type']](**section['params'])


class CriteriaOracle(O.DistillOracle):
    """O.DistillOracle with a criterion per term.  `criteria`: name -> {'criterion': {'type', 'params'}, 'factor': f} (the
    `criterion` entry of the fixture's meta); `paths`: name -> (teacher key, student key) relative to backbone.body,
    default the term's own name on both sides."""

    def __init__(self, teacher_sd, student_sd, criteria, paths=None, **kw):
        paths = paths or {}
        terms = OrderedDict((name, paths[name] + (c['factor'],) if name in paths else c['factor'])
                            for name, c in criteria.items())
        super().__init__(teacher_sd, student_sd, terms=terms, **kw)
        self.modules = OrderedDict((name, torch_criterion(c['criterion'])) for name, c in criteria.items())

    def forward(self, images, fixed_sizes=None, update_buffers=True, intermediates=None):
        _, _, t_h, s_h, t_f, s_f, x = super().forward(images, fixed_sizes, update_buffers, intermediates)
        per_term = OrderedDict()
        for name, v in self.terms.items():
            tk, sk, factor = v if isinstance(v, tuple) else (name, name, v)
            per_term[name] = self.modules[name](t_h[tk], s_h[sk]) * factor
        return sum(per_term.values()), per_term, t_h, s_h, t_f, s_f, x


def apply_criteria(config, criteria):
    """put the fixture's criterion section into a config made by configs.make_config (terms of the same names)"""
    terms = config['train']['criterion']['terms']
    assert list(terms) == list(criteria)
    for name, c in criteria.items():
        terms[name]['criterion'] = {'type': c['criterion']['type'], 'params': dict(c['criterion']['params'])}
        terms[name]['factor'] = c['factor']
    return config


# ------------------------------------------------------------------------------------------ kernel-level reference
KINDS = {'mse': 0.0, 'l1': 0.0, 'smooth_l1': 0.7, 'huber': 1.3}         # kind -> beta / delta
# the shapes of test_mse_fused_loss_and_grad, plus a 4-channel buffer holding a 3-channel tensor (count = 3/4 numel)
SHAPES = [(2, 9, 11, 256), (2, 5, 6, 512), (2, 3, 3, 1024), (2, 2, 2, 2048), (2, 7, 9, 4)]
FACTORS = [1.0, 0.5, 2.0, 1.0, 3.0]


def kernel_inputs(seed):
    """(teacher, student) NHWC fp32 pairs, both ReLU outputs; 15 % of the elements have teacher == student exactly (half of
    them positive, so d = 0 meets s > 0), the rest spread over both zones of SmoothL1(0.7) / Huber(1.3)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for shp in SHAPES:
        t = F.relu(torch.randn(shp, generator=g) * 1.5)
        s = F.relu(torch.randn(shp, generator=g) * 1.5)
        same = torch.rand(shp, generator=g) < 0.15
        t = torch.where(same, s, t)
        logical = shp[-1]
        if shp[-1] == 4:                    # padded channel: zero in both operands, not counted by a mean
            t[..., 3] = 0
            s[..., 3] = 0
            logical = 3
        out.append((t, s, t.numel() // shp[-1] * logical))
    return out


def fp64_reference(kind, param, t, s, w, relu_mask):
    """(sum of the criterion over the elements, gradient w.r.t. s with weight w) in fp64 on the same fp32 inputs"""
    d = s.double() - t.double()
    ad = d.abs()
    if kind == 'mse':
        val, grad = d * d, 2 * w * d
    elif kind == 'l1':
        val, grad = ad, w * torch.sign(d)
    elif kind == 'smooth_l1':
        val = torch.where(ad < param, 0.5 * d * d / param, ad - 0.5 * param)
        grad = torch.where(ad < param, w * d / param, w * torch.sign(d))
    else:
        val = torch.where(ad <= param, 0.5 * d * d, param * (ad - 0.5 * param))
        grad = torch.where(ad <= param, w * d, w * param * torch.sign(d))
    if relu_mask:
        grad = grad * (s > 0)
    return val.sum(), grad
