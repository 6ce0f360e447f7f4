"""GPU: hnd_optim_step_flat stays inside the buffers include/hnd_optim.h sizes -- the guard ledger of that header.

As tests/test_guard_bands_gpu.py does for include/hnd_hip.h: the parameter, the gradient and every state buffer of a
launch are views of exactly `numel` floats inside ONE tests/guard_util.Arena filled with 0xFF (fp32 NaN); one launch, then
ops.sync_check(), then arena.check() (no guard byte changed); the results are finite (an over-read would poison them) and
at the bar of tests/test_optim_kinds_gpu.py (tests/optim_util.check_bar).  tests/test_optim_kinds_cpu.py holds LEDGER, with
NO_DEVICE_OUTPUT, to _lib.OPTIM_SYMBOLS.  Importing this module does not touch the GPU."""
import pytest
import torch

from tests import guard_util as G
from tests import optim_util as OU

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

LEDGER = {}          # test function name -> exports of include/hnd_optim.h whose device writes it guards


def covers(*exports):
    def deco(fn):
        LEDGER.setdefault(fn.__name__, set()).update(exports)
        return fn
    return deco


# exports that write no device memory a caller owns: nothing to guard
NO_DEVICE_OUTPUT = {
    'hnd_optim_abi': 'constant',
}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


# every kind, each with all of its state buffers in use
GUARD_CASES = ['adam_wd_amsgrad', 'adagrad_decay_wd_init', 'rmsprop_centered_momentum']


@covers('hnd_optim_step_flat')
@pytest.mark.parametrize('numel', [1, 7, 4099])
@pytest.mark.parametrize('case', GUARD_CASES)
def test_optim_step_stays_inside_buffers_of_exactly_numel_floats(ops, case, numel):
    kind, hyper = OU.CASES[case]
    assert OU.used_slots(kind, hyper) == OU.SLOTS[kind]                    # every state buffer the kind has
    p0, grads = OU.inputs(numel, seed=2000 + numel, steps=1)
    states0 = OU.initial_states(kind, hyper, numel)
    nbuf = 2 + sum(s is not None for s in states0)
    arena = G.Arena(DEV, G.arena_bytes([((numel,), torch.float32)] * nbuf))
    param, grad = arena.load('param', p0), arena.load('grad', grads[0] * 4)
    states = [None if s is None else arena.load('state%d' % i, s) for i, s in enumerate(states0)]
    OU.kernel_steps(ops, kind, hyper, param, states, [grad])
    ops.sync_check()
    arena.check()
    assert torch.equal(grad.cpu(), grads[0] * 4)                          # the gradient is read only
    OU.check_bar('%s numel %d guarded' % (case, numel), OU.named(kind, hyper, param, states),
                 OU.torch_run(kind, hyper, p0, grads, torch.float64), OU.torch_run(kind, hyper, p0, grads, torch.float32))
