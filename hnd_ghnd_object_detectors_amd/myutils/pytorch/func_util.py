"""Factories the runner calls by name (src/mimic_runner.py:67-70, src/distillation/loss.py:13).

get_optimizer('Adam' / 'SGD' / 'Adagrad' / 'RMSprop') returns the fused flat-arena optimizers, get_loss('MSELoss' / 'L1Loss' / 'SmoothL1Loss' /
'HuberLoss', reduction 'sum' or 'mean') a criterion of the fused HIP loss; schedulers are plain torch (host-side scalars only)."""
import torch
from torch import nn

from ...optim import FusedAdam, FusedSGD, FusedAdagrad, FusedRMSprop
from ...distillation.hip_loss import HipMSELoss, HipL1Loss, HipSmoothL1Loss, HipHuberLoss, SUPPORTED_CRITERIA


def get_optimizer(target, optim_type, optim_params_config):
    params = target.parameters() if isinstance(target, nn.Module) else target
    if optim_type.lower() == 'adam':
        return FusedAdam(params, **optim_params_config)
    if optim_type.lower() == 'sgd':
        return FusedSGD(params, **optim_params_config)
    if optim_type.lower() == 'adagrad':
        return FusedAdagrad(params, **optim_params_config)
    if optim_type.lower() == 'rmsprop':
        return FusedRMSprop(params, **optim_params_config)
    raise ValueError('optim_type `{}` is not expected on the HIP path (SGD, Adam, Adagrad and RMSprop are; the hnd/ghnd '
                     'configs use Adam, the ext config SGD)'.format(optim_type))


def get_scheduler(optimizer, scheduler_type, scheduler_params_config):
    for name in ('StepLR', 'MultiStepLR', 'ExponentialLR', 'CosineAnnealingLR'):
        if scheduler_type.lower() == name.lower():
            return getattr(torch.optim.lr_scheduler, name)(optimizer, **scheduler_params_config)
    raise ValueError('scheduler_type `{}` is not expected'.format(scheduler_type))


LOSS_DICT = {'mse': HipMSELoss, 'mseloss': HipMSELoss, 'l1': HipL1Loss, 'l1loss': HipL1Loss,
             'smoothl1': HipSmoothL1Loss, 'smoothl1loss': HipSmoothL1Loss, 'huber': HipHuberLoss, 'huberloss': HipHuberLoss}


def get_loss(loss_type, param_dict=None):
    param_dict = param_dict or {}
    cls = LOSS_DICT.get(loss_type.lower())
    if cls is None:
        raise ValueError('loss_type `{}` is not expected on the HIP distillation path.  Supported: {}'
                         .format(loss_type, SUPPORTED_CRITERIA))
    return cls(**param_dict)
