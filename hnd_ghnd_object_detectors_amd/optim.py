"""Fused optimizers over one flat parameter arena: Adam (replaces torch.optim.Adam created at
src/mimic_runner.py:67-68), SGD with momentum / weight decay (the neural filter's optimizer,
src/ext_runner.py:118-120 with config/ext/*.yaml), Adagrad and RMSprop (the other two types the reference's
func_util.get_optimizer takes).

Each subclasses its torch.optim class so ``state_dict()`` / ``load_state_dict()`` keep the torch format the reference
checkpoints store under 'optimizer' (src/models/__init__.py:15-17) and LambdaLR / MultiStepLR drive
``param_groups[i]['lr']`` as usual.  ``step()`` is one launch when the trainable tensors and their gradients sit in flat
arenas (the normal case), else one launch per tensor -- never torch math.  Plain Adam (no weight decay, no AMSGrad)
launches hnd_adam_step_flat and SGD hnd_sgd_step_flat (include/hnd_hip.h); Adam with weight_decay / amsgrad, Adagrad and
RMSprop launch hnd_optim_step_flat (include/hnd_optim.h).

Known deviation from torch.optim (all four classes): a parameter the backward plan writes an exact-zero gradient for --
the student's decoder under a lone ``layer1.encoder`` term, for example -- is stepped here, where autograd would leave
``.grad`` at None and torch would skip the tensor.  With zero state and weight_decay == 0 a zero gradient moves nothing
and the two agree; with weight_decay > 0, or with non-zero state (moments, momentum buffers from earlier steps or from
a checkpoint), such a parameter moves here and stays put in torch, and its step count advances.
"""
import torch

from . import ops, parallel

# torch.optim keywords that select another implementation of the same step; the HIP path is the only one here
_REFUSED_KEYWORDS = ('maximize', 'foreach', 'capturable', 'differentiable', 'fused')


def _refuse_keywords(name, kwargs):
    """keywords of torch.optim the HIP path does not take raise when set to a true value; false / None values and the
    remaining keywords are dropped as before"""
    for k in _REFUSED_KEYWORDS:
        if kwargs.get(k):
            raise NotImplementedError('%s: %s=%r is not supported on the HIP path' % (name, k, kwargs[k]))


# ---------------------------------------------------------------------------------------------------- flat arenas
def _arena_offsets(plist):
    """every tensor starts on a 64-float boundary of the arena (the gradient arena of the backward plan has this layout)"""
    offsets, total = [], 0
    for p in plist:
        offsets.append(total)
        total += (p.numel() + 63) // 64 * 64
    return offsets, total


def _grads_are_flat(flat, plist):
    """the gradients as ONE flat view when they lie in an arena of the parameters' layout, else None"""
    base = plist[0].grad.data_ptr()
    for o, p in zip(flat['offsets'], plist):
        if p.grad.data_ptr() != base + o * 4 or not p.grad.is_contiguous():
            return None
    g0 = plist[0].grad
    span = g0.untyped_storage().nbytes() // 4 - (base - g0.untyped_storage().data_ptr()) // 4
    if span < flat['total']:
        return None
    return torch.as_strided(g0, (flat['total'],), (1,), g0.storage_offset())


def _params_in_arena(flat, plist):
    return all(p.data_ptr() == flat['p'].data_ptr() + o * 4 for o, p in zip(flat['offsets'], plist))


class _FlatStateOptimizer(object):
    """What FusedAdam, FusedAdagrad and FusedRMSprop share: the flat parameter arena, one flat arena per state tensor of
    torch's (views of it live under torch's own state keys), the resume from a checkpoint, the choice between one launch
    and one launch per tensor.  A subclass names its state keys (``_state_keys``) and launches (``_launch``)."""

    def _init_flat(self):
        self.grad_scale = 1.0          # extra factor on the gradients (tests); the DP mean comes from parallel
        self._flat = None

    def _state_keys(self, group):
        raise NotImplementedError

    def _launch(self, group, param, grad, states, step, grad_scale):
        raise NotImplementedError

    def _fresh_state(self, p, group, key):
        return torch.zeros_like(p, memory_format=torch.preserve_format)

    def load_state_dict(self, state_dict):
        """the loaded state tensors replace the arena views: the arenas are rebuilt from them on the next step"""
        super().load_state_dict(state_dict)
        self._flat = None

    def _flatten(self, group, plist):
        """move the trainable tensors (and their state) into contiguous arenas; parameters keep their identity (only
        .data is re-pointed), so optimizers / DDP / state_dict are unaffected.  Tensors whose step counts differ (a
        hand-edited checkpoint) cannot share one launch: nothing is touched then and the per-tensor path is used from
        now on (decided once, not per step)."""
        keys = self._state_keys(group)
        ids = [id(p) for p in plist]
        steps = set(int(self.state[p]['step']) if keys[0] in self.state[p] else 0 for p in plist)
        if len(steps) != 1:
            print('%s: per-tensor step counts differ (%s); using one launch per tensor'
                  % (type(self).__name__, sorted(steps)))
            return {'ids': ids, 'per_tensor': True}
        offsets, total = _arena_offsets(plist)
        dev = plist[0].device
        flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        arenas = {k: torch.zeros_like(flat_p) for k in keys}
        for o, p in zip(offsets, plist):
            n = p.numel()
            flat_p[o:o + n].copy_(p.data.reshape(-1))
            p.data = flat_p[o:o + n].view(p.shape)
            st = self.state[p]
            for k in keys:
                if k in st:                           # resumed from a checkpoint (or set up by torch's constructor)
                    arenas[k][o:o + n].copy_(st[k].reshape(-1))
                else:
                    arenas[k][o:o + n].copy_(self._fresh_state(p, group, k).reshape(-1))
                st[k] = arenas[k][o:o + n].view(p.shape)
            if 'step' not in st:
                st['step'] = torch.tensor(0.0)
        return {'ids': ids, 'offsets': offsets, 'total': total, 'p': flat_p, 'state': arenas}

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError('%s.step(closure) is not supported' % type(self).__name__)
        for group in self.param_groups:
            plist = [p for p in group['params'] if p.grad is not None]
            if not plist:
                continue
            keys = self._state_keys(group)
            flat = self._flat
            if flat is None or flat['ids'] != [id(p) for p in plist]:
                flat = self._flatten(group, plist)
                self._flat = flat
            flat_g = _grads_are_flat(flat, plist) if not flat.get('per_tensor') else None
            # gradient all-reduces fired from inside backward (parallel.DistributedStudent): wait stream-side, and
            # fold the 1/world mean of a sum all-reduce into this launch
            grad_scale = self.grad_scale * parallel.finish_pending(flat_g if flat_g is not None else [p.grad for p in plist], plist)
            if flat_g is not None and _params_in_arena(flat, plist):
                step = int(self.state[plist[0]]['step']) + 1
                self._launch(group, flat['p'], flat_g, [flat['state'][k] for k in keys], step, grad_scale)
                for p in plist:
                    self.state[p]['step'] = torch.tensor(float(step))
            else:
                for p in plist:
                    st = self.state[p]
                    if keys[0] not in st:
                        st['step'] = torch.tensor(0.0)
                    for k in keys:
                        if k not in st:
                            st[k] = self._fresh_state(p, group, k)
                    step = int(st['step']) + 1
                    g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                    self._launch(group, p.data, g, [st[k] for k in keys], step, grad_scale)
                    st['step'] = torch.tensor(float(step))
        parallel.end_step()
        return None


class FusedAdam(_FlatStateOptimizer, torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **kwargs):
        _refuse_keywords('FusedAdam', kwargs)
        if kwargs.get('decoupled_weight_decay'):
            raise NotImplementedError('FusedAdam: decoupled_weight_decay=True (AdamW) is not supported on the HIP path')
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad))
        self._init_flat()

    def _state_keys(self, group):
        return ['exp_avg', 'exp_avg_sq'] + (['max_exp_avg_sq'] if group['amsgrad'] else [])

    def _launch(self, group, param, grad, states, step, grad_scale):
        beta1, beta2 = group['betas']
        if group['weight_decay'] == 0 and not group['amsgrad']:
            ops.adam_step_flat(param, grad, states[0], states[1], group['lr'], beta1, beta2, group['eps'], step, grad_scale)
        else:
            ops.optim_step_flat('adam', param, grad, states, step=step, grad_scale=grad_scale, lr=group['lr'],
                                weight_decay=group['weight_decay'], eps=group['eps'], beta1=beta1, beta2=beta2,
                                amsgrad=group['amsgrad'])


class FusedAdagrad(_FlatStateOptimizer, torch.optim.Adagrad):
    """torch.optim.Adagrad (lr_decay, weight_decay, initial_accumulator_value, eps) as one hnd_optim_step_flat launch over
    flat parameter / gradient / ``sum`` arenas."""

    def __init__(self, params, lr=1e-2, lr_decay=0, weight_decay=0, initial_accumulator_value=0, eps=1e-10, **kwargs):
        _refuse_keywords('FusedAdagrad', kwargs)
        # torch's constructor fills state[p]['sum'] with initial_accumulator_value; _flatten copies it into the arena
        super().__init__(params, lr=lr, lr_decay=lr_decay, weight_decay=weight_decay,
                         initial_accumulator_value=initial_accumulator_value, eps=eps)
        self._init_flat()

    def _state_keys(self, group):
        return ['sum']

    def _fresh_state(self, p, group, key):
        return torch.full_like(p, group['initial_accumulator_value'], memory_format=torch.preserve_format)

    def _launch(self, group, param, grad, states, step, grad_scale):
        ops.optim_step_flat('adagrad', param, grad, states, step=step, grad_scale=grad_scale, lr=group['lr'],
                            weight_decay=group['weight_decay'], eps=group['eps'], lr_decay=group['lr_decay'])


class FusedRMSprop(_FlatStateOptimizer, torch.optim.RMSprop):
    """torch.optim.RMSprop (alpha, eps, weight_decay, momentum, centered) as one hnd_optim_step_flat launch over flat
    parameter / gradient / ``square_avg`` (/ ``momentum_buffer`` / ``grad_avg``) arenas."""

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, **kwargs):
        _refuse_keywords('FusedRMSprop', kwargs)
        super().__init__(params, lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum,
                         centered=bool(centered))
        self._init_flat()

    def _state_keys(self, group):
        return ['square_avg'] + (['momentum_buffer'] if group['momentum'] > 0 else []) + \
            (['grad_avg'] if group['centered'] else [])

    def _launch(self, group, param, grad, states, step, grad_scale):
        by_key = dict(zip(self._state_keys(group), states))
        ops.optim_step_flat('rmsprop', param, grad, [by_key.get(k) for k in ops.OPTIM_STATE_SLOTS['rmsprop']], step=step,
                            grad_scale=grad_scale, lr=group['lr'], weight_decay=group['weight_decay'], eps=group['eps'],
                            beta2=group['alpha'], momentum=group['momentum'], centered=group['centered'])


class FusedSGD(torch.optim.SGD):
    """torch.optim.SGD (momentum, dampening, weight_decay, nesterov) as one hnd_sgd_step_flat launch over flat
    parameter / gradient / momentum arenas; ``state_dict()`` keeps torch's ``momentum_buffer`` entries."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **kwargs):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov)
        self.grad_scale = 1.0
        self._flat = None

    def _flatten(self, plist):
        ids = [id(p) for p in plist]
        started = set(self.state[p].get('momentum_buffer') is not None for p in plist)
        if len(started) != 1:           # nothing touched; per-tensor path from now on (decided once)
            print('FusedSGD: some tensors have a momentum buffer and some do not; using one launch per tensor')
            return {'ids': ids, 'per_tensor': True}
        offsets, total = _arena_offsets(plist)
        dev = plist[0].device
        flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        flat_b = torch.zeros_like(flat_p)
        for o, p in zip(offsets, plist):
            n = p.numel()
            flat_p[o:o + n].copy_(p.data.reshape(-1))
            p.data = flat_p[o:o + n].view(p.shape)
            st = self.state[p]
            buf = st.get('momentum_buffer')
            if buf is not None:                       # resumed from a checkpoint
                flat_b[o:o + n].copy_(buf.reshape(-1))
            st['momentum_buffer'] = flat_b[o:o + n].view(p.shape) if buf is not None else None
        return {'ids': ids, 'offsets': offsets, 'total': total, 'p': flat_p, 'b': flat_b, 'started': started.pop()}

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise NotImplementedError('FusedSGD.step(closure) is not supported')
        for group in self.param_groups:
            plist = [p for p in group['params'] if p.grad is not None]
            if not plist:
                continue
            hyper = (group['lr'], group['momentum'], group['dampening'], group['weight_decay'], group['nesterov'])
            flat = self._flat
            if flat is None or flat['ids'] != [id(p) for p in plist]:
                flat = self._flatten(plist)
                self._flat = flat
            flat_g = _grads_are_flat(flat, plist) if not flat.get('per_tensor') else None
            grad_scale = self.grad_scale * parallel.finish_pending(flat_g if flat_g is not None else [p.grad for p in plist], plist)
            if flat_g is not None and _params_in_arena(flat, plist):
                ops.sgd_step_flat(flat['p'], flat_g, flat['b'], *hyper, first_step=not flat['started'],
                                  grad_scale=grad_scale)
                if not flat['started'] and group['momentum'] != 0:
                    for o, p in zip(flat['offsets'], plist):
                        self.state[p]['momentum_buffer'] = flat['b'][o:o + p.numel()].view(p.shape)
                flat['started'] = True
            else:
                for p in plist:
                    st = self.state[p]
                    first = st.get('momentum_buffer') is None
                    if first and group['momentum'] != 0:
                        st['momentum_buffer'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                    ops.sgd_step_flat(p.data, g, st.get('momentum_buffer'), *hyper, first_step=first,
                                      grad_scale=grad_scale)
        parallel.end_step()
        return None
