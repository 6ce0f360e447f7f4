"""GPU: hnd_optim_step_flat (include/hnd_optim.h) against torch.optim, and the host paths of FusedAdam with weight_decay /
amsgrad, FusedAdagrad and FusedRMSprop on the tiny GHND pair.

Reference: the same torch.optim class on CPU in fp64.  Yardstick: that class in fp32 on CPU against the same fp64 run.
Bar, per buffer (the parameter and every state): tests/optim_util.check_bar."""
import copy
import functools

import pytest
import torch

from tests import golden_util as G
from tests import model_util as MU
from tests import optim_util as OU

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


# ------------------------------------------------------------------------------------------ kernel vs torch
@functools.lru_cache(maxsize=None)
def _reference(case, numel):
    """inputs and the two torch runs of a case: computed once, shared, never modified"""
    kind, hyper = OU.CASES[case]
    p0, grads = OU.inputs(numel, seed=1000 + numel)
    return p0, grads, OU.torch_run(kind, hyper, p0, grads, torch.float64), OU.torch_run(kind, hyper, p0, grads, torch.float32)


def _device_buffers(kind, hyper, p0, offset):
    """param and the used states on the device; offset = 1: every buffer starts one float past a 16-byte boundary"""
    def put(t):
        if t is None:
            return None
        base = torch.full((t.numel() + offset,), float('nan'), device=DEV)
        base[offset:].copy_(t)
        return base[offset:]
    return put(p0), [put(s) for s in OU.initial_states(kind, hyper, p0.numel())], put


# numel: less than one vector, a vector and a tail, many vectors and a tail in one block / in several blocks
@pytest.mark.parametrize('numel,offset', [(1, 0), (5, 0), (1021, 0), (10007, 0), (1021, 1)])
@pytest.mark.parametrize('case', list(OU.CASES))
def test_optim_kernel_matches_torch(ops, case, numel, offset):
    kind, hyper = OU.CASES[case]
    p0, grads, ref64, ref32 = _reference(case, numel)
    param, states, put = _device_buffers(kind, hyper, p0, offset)
    grads_dev = [put(g * 4) for g in grads]
    assert all(t.data_ptr() % 16 == 4 * offset for t in [param] + grads_dev + [s for s in states if s is not None])
    OU.kernel_steps(ops, kind, hyper, param, states, grads_dev)
    ops.sync_check()
    OU.check_bar('%s numel %d%s' % (case, numel, ' unaligned' if offset else ''), OU.named(kind, hyper, param, states),
                 ref64, ref32)


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('case', list(OU.CASES))
def test_optim_kernel_is_bit_reproducible(ops, case, offset):
    """the same call twice from the same state gives the same bits (fixed order, one store per element, no atomics)"""
    kind, hyper = OU.CASES[case]
    p0, grads, _, _ = _reference(case, 10007)
    runs = []
    for _ in range(2):
        param, states, put = _device_buffers(kind, hyper, p0, offset)
        OU.kernel_steps(ops, kind, hyper, param, states, [put(g * 4) for g in grads[:2]])
        ops.sync_check()
        runs.append([t.clone() for t in OU.named(kind, hyper, param, states).values()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------ host paths
HOST_CASES = [('Adagrad', dict(lr=1e-2, lr_decay=0.1, weight_decay=1e-4, initial_accumulator_value=0.1)),
              ('RMSprop', dict(lr=1e-3, weight_decay=1e-4, momentum=0.9, centered=True)),
              ('Adam', dict(lr=1e-3, weight_decay=1e-4, amsgrad=True))]


def _to_dev(images, targets):
    return [im.to(DEV) for im in images], [{k: v.to(DEV) for k, v in t.items()} for t in targets]


def _twin(optim_type, hyper, params, dtype):
    """a plain torch.optim optimizer over CPU copies of ALL parameters, in the fused optimizer's order"""
    copies = [torch.nn.Parameter(p.detach().cpu().to(dtype), requires_grad=p.requires_grad) for p in params]
    return copies, getattr(torch.optim, optim_type)(copies, foreach=False, **hyper)


def _twin_step(copies, opt, grads):
    for c, g in zip(copies, grads):
        c.grad = None if g is None else g.to(c.dtype)
    opt.step()


def _arena_of(params, opt, key):
    """one buffer kind ('param' or a torch state key) over the given parameters as one vector, as the arena holds it"""
    return torch.cat([(p if key == 'param' else opt.state[p][key]).detach().reshape(-1).cpu() for p in params])


def _compare(label, keys, fused, twin64, twin32):
    (fp, fo), (p64, o64), (p32, o32) = fused, twin64, twin32
    stepped = [i for i, p in enumerate(fp) if p.grad is not None]
    pick = lambda ps, o: OU.OrderedDict((k, _arena_of([ps[i] for i in stepped], o, k)) for k in ('param',) + tuple(keys))
    OU.check_bar(label, pick(fp, fo), pick(p64, o64), pick(p32, o32))
    for i in stepped:
        assert int(fo.state[fp[i]]['step']) == int(o32.state[p32[i]]['step'])


@pytest.mark.parametrize('optim_type,hyper', HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_fused_optimizer_on_the_tiny_pair_matches_its_torch_twin(ops, monkeypatch, optim_type, hyper):
    """two training steps through func_util.get_optimizer on the flat path (one launch per step, parameters views of one
    storage), the state_dict round trip with a torch twin in both directions, then a third step: on the flat path against
    the twins, and once more from the same state on the per-tensor path, which must give the same bits"""
    from hnd_ghnd_object_detectors_amd import optim
    from hnd_ghnd_object_detectors_amd.distillation.tool import DistillationBox
    from hnd_ghnd_object_detectors_amd.myutils.pytorch import func_util
    z, meta = G.load('tiny_ghnd_faster')
    cfg = MU.config_for(meta)
    t_sd, s_sd = MU.oracle_states(meta['seed'], meta['model'])
    teacher, student = MU.build_pair(cfg, t_sd, s_sd, DEV)
    box = DistillationBox(teacher, student, cfg['train']['criterion'])
    images, targets = G.case_inputs(meta)
    opt = func_util.get_optimizer(student, optim_type, dict(hyper))
    assert type(opt) is getattr(optim, 'Fused' + optim_type)
    params = [p for g in opt.param_groups for p in g['params']]
    twin64, twin32 = _twin(optim_type, hyper, params, torch.float64), _twin(optim_type, hyper, params, torch.float32)
    launches = []
    real = ops.optim_step_flat
    monkeypatch.setattr(ops, 'optim_step_flat', lambda *a, **k: (launches.append(a[0]), real(*a, **k))[1])
    kind = optim_type.lower()
    keys = [k for k in OU.used_slots(kind, hyper) if k is not None]

    def backward():
        loss = box(*_to_dev(images, targets))
        opt.zero_grad()
        loss.backward()
        ops.sync_check()
        return [None if p.grad is None else p.grad.detach().cpu().clone() for p in params]

    for step in (1, 2):
        grads = backward()
        opt.step()
        ops.sync_check()
        for copies, t in (twin64, twin32):
            _twin_step(copies, t, grads)
        assert launches == [kind] * step                                  # the flat path: one launch per step
        stepped = [p for p in params if p.grad is not None]
        assert len(stepped) > 1 and len(set(p.untyped_storage().data_ptr() for p in stepped)) == 1
        for k in keys:
            assert len(set(opt.state[p][k].untyped_storage().data_ptr() for p in stepped)) == 1, k
        _compare('%s tiny pair step %d' % (optim_type, step), keys, (params, opt), twin64, twin32)

    # torch's format in both directions: fused -> twins (the fp64 twin continues from the fp32 state) -> fused.  Deep
    # copies, as through a checkpoint file: state_dict() hands out the live tensors and torch steps 'step' in place
    sd = opt.state_dict()
    assert all(sorted(st) == sorted(keys + ['step']) for st in sd['state'].values())
    for _, t in (twin64, twin32):
        t.load_state_dict(copy.deepcopy(sd))
    opt.load_state_dict(copy.deepcopy(twin32[1].state_dict()))
    grads = backward()
    stepped = [p for p in params if p.grad is not None]
    saved = [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()}) for p in stepped]
    opt.step()
    ops.sync_check()
    assert launches == [kind] * 3
    for copies, t in (twin64, twin32):
        _twin_step(copies, t, grads)
    _compare('%s tiny pair step 3 (after load_state_dict)' % optim_type, keys, (params, opt), twin64, twin32)
    flat_bits = [(p.detach().clone(), {k: opt.state[p][k].clone() for k in keys}) for p in stepped]

    # the same step from the same state with one gradient outside the arena: one launch per tensor, the same bits
    for p, (data, st) in zip(stepped, saved):
        p.data.copy_(data)
        for k in keys:
            opt.state[p][k].copy_(st[k])
        opt.state[p]['step'] = st['step'].clone()
    stepped[-1].grad = stepped[-1].grad.clone()
    opt.step()
    ops.sync_check()
    assert launches == [kind] * (3 + len(stepped))
    for p, (data, st) in zip(stepped, flat_bits):
        assert torch.equal(p.detach(), data)
        assert all(torch.equal(opt.state[p][k], st[k]) for k in keys)
        assert int(opt.state[p]['step']) == 3


def test_plain_adam_and_sgd_still_take_their_own_launches(ops, monkeypatch):
    """FusedAdam(weight_decay=0, amsgrad=False) launches hnd_adam_step_flat and FusedSGD hnd_sgd_step_flat; with
    weight_decay or amsgrad FusedAdam launches hnd_optim_step_flat"""
    from hnd_ghnd_object_detectors_amd import optim
    calls = []
    for name in ('adam_step_flat', 'sgd_step_flat', 'optim_step_flat'):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])

    def one_step(cls, **hyper):
        p = torch.nn.Parameter(torch.randn(77, device=DEV))
        o = cls([p], **hyper)
        p.grad = torch.randn(77, device=DEV)
        o.step()
        ops.sync_check()
        assert bool(torch.isfinite(p).all())
    one_step(optim.FusedAdam, lr=1e-3)
    one_step(optim.FusedSGD, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    one_step(optim.FusedAdam, lr=1e-3, weight_decay=1e-4)
    one_step(optim.FusedAdam, lr=1e-3, amsgrad=True)
    assert calls == ['adam_step_flat', 'sgd_step_flat', 'optim_step_flat', 'optim_step_flat']
