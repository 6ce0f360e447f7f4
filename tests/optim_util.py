"""Shared by tests/test_optim_kinds_gpu.py and tests/test_guard_bands_optim_gpu.py: the cases of hnd_optim_step_flat, their
torch.optim reference (CPU, fp64) and yardstick (CPU, fp32), and the bar both files hold the kernel to.

A plain module: importing it touches neither the GPU nor the library."""
from collections import OrderedDict

import torch

# case -> (kind of include/hnd_optim.h, keywords of the torch.optim class)
CASES = OrderedDict([
    ('adam_wd', ('adam', dict(lr=1e-3, weight_decay=1e-2))),
    ('adam_amsgrad', ('adam', dict(lr=1e-3, amsgrad=True))),
    ('adam_wd_amsgrad', ('adam', dict(lr=1e-3, weight_decay=1e-2, amsgrad=True))),
    ('adagrad', ('adagrad', dict(lr=1e-2))),
    ('adagrad_decay_wd_init', ('adagrad', dict(lr=1e-2, lr_decay=0.1, weight_decay=1e-2, initial_accumulator_value=0.1))),
    ('rmsprop', ('rmsprop', dict(lr=1e-2))),
    ('rmsprop_wd', ('rmsprop', dict(lr=1e-2, weight_decay=1e-2))),
    ('rmsprop_momentum', ('rmsprop', dict(lr=1e-2, momentum=0.9))),
    ('rmsprop_centered', ('rmsprop', dict(lr=1e-2, centered=True))),
    ('rmsprop_centered_momentum', ('rmsprop', dict(lr=1e-2, centered=True, momentum=0.9))),
])
TORCH = {'adam': torch.optim.Adam, 'adagrad': torch.optim.Adagrad, 'rmsprop': torch.optim.RMSprop}
# torch's state keys in the slot order of struct hnd_optim_desc
SLOTS = {'adam': ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'), 'adagrad': ('sum', None, None),
         'rmsprop': ('square_avg', 'momentum_buffer', 'grad_avg')}
STEPS = 4
GRAD_SCALE = 0.25           # the kernel gets 4 x the gradient and this factor (exact in fp32)


def used_slots(kind, hyper):
    """the state keys the case has, by slot (None: unused)"""
    a, b, c = SLOTS[kind]
    if kind == 'adam':
        return a, b, (c if hyper.get('amsgrad') else None)
    if kind == 'rmsprop':
        return a, (b if hyper.get('momentum', 0) > 0 else None), (c if hyper.get('centered') else None)
    return a, None, None


def inputs(numel, seed, steps=STEPS):
    """p0 and one independent gradient per step, scaled 10**step (tests/test_ops_gpu.py test_adam_matches_torch)"""
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(numel, generator=g)
    grads = [torch.randn(numel, generator=g) * (10.0 ** step) for step in range(1, steps + 1)]
    return p0, grads


def torch_run(kind, hyper, p0, grads, dtype):
    """the torch.optim class, single-tensor path, on CPU in `dtype`: {'param': ..., state key: ...} after the steps"""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = TORCH[kind]([p], foreach=False, **hyper)
    for g in grads:
        p.grad = g.to(dtype).clone()
        opt.step()
    out = OrderedDict(param=p.detach())
    for k in used_slots(kind, hyper):
        if k is not None:
            out[k] = opt.state[p][k]
    return out


def kernel_hyper(kind, hyper):
    """torch.optim keywords (torch's defaults filled in) -> keywords of ops.optim_step_flat"""
    h = dict(hyper)
    if kind == 'adam':
        beta1, beta2 = h.pop('betas', (0.9, 0.999))
        return dict(lr=h.get('lr', 1e-3), beta1=beta1, beta2=beta2, eps=h.get('eps', 1e-8),
                    weight_decay=h.get('weight_decay', 0), amsgrad=h.get('amsgrad', False))
    if kind == 'adagrad':
        return dict(lr=h.get('lr', 1e-2), lr_decay=h.get('lr_decay', 0), eps=h.get('eps', 1e-10),
                    weight_decay=h.get('weight_decay', 0))
    return dict(lr=h.get('lr', 1e-2), beta2=h.get('alpha', 0.99), eps=h.get('eps', 1e-8), weight_decay=h.get('weight_decay', 0),
                momentum=h.get('momentum', 0), centered=h.get('centered', False))


def initial_states(kind, hyper, numel):
    """CPU tensors of the used slots as torch initialises them (None for an unused slot)"""
    fill = hyper.get('initial_accumulator_value', 0.0) if kind == 'adagrad' else 0.0
    return [None if k is None else torch.full((numel,), fill) for k in used_slots(kind, hyper)]


def kernel_steps(ops, kind, hyper, param, states, grads_dev, first_step=1):
    """hnd_optim_step_flat once per gradient on device buffers the caller owns (4 x gradient, grad_scale 0.25)"""
    kw = kernel_hyper(kind, hyper)
    for i, g in enumerate(grads_dev):
        ops.optim_step_flat(kind, param, g, states, step=first_step + i, grad_scale=GRAD_SCALE, **kw)


def named(kind, hyper, param, states):
    out = OrderedDict(param=param)
    for k, s in zip(used_slots(kind, hyper), states):
        if k is not None:
            out[k] = s
    return out


def err(t, ref64):
    """largest absolute error relative to the buffer's largest magnitude"""
    ref64 = ref64.double()
    return float((t.detach().cpu().double() - ref64).abs().max() / ref64.abs().max().clamp_min(1e-300))


def check_bar(label, got, ref64, ref32):
    """per buffer: err_kernel <= 2 * err_torch_fp32 + 1e-7 against the fp64 run -- the kernel is as close to the exact
    step as torch's own fp32 step; the factor 2 covers a different but equally valid rounding order (FMA contraction,
    scalars rounded once from double).  Prints every pair before asserting; returns the report lines."""
    lines, bad = [], []
    assert list(got) == list(ref64) == list(ref32), (list(got), list(ref64))
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), (label, k)
        e_k, e_t = err(got[k], ref64[k]), err(ref32[k], ref64[k])
        lines.append('%-44s %-16s kernel %.3e   torch fp32 %.3e' % (label, k, e_k, e_t))
        print(lines[-1])
        if not e_k <= 2.0 * e_t + 1e-7:
            bad.append(lines[-1])
    assert not bad, '\n'.join(bad)
    return lines
