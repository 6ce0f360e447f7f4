"""GPU: pairs of one hnd_mimic_loss_fwd_bwd call that share `grad` form a group -- the launch reads the student once and each
teacher once, adds the members' gradients in fp32 in pair order, masks the sum once and stores it once.  Through
ops.MimicLaunch against torch fp64 on the CPU.

Sizes: a chunk is 4096 floats; numel 4 (one vector), 4092 (a tail), 4096 (an exact chunk), 4100 (a chunk plus one vector),
20484 (several workgroups and a tail).  Bars: those of tests/test_mimic_loss_gpu.py::test_mimic_kernel_matches_torch_fp64 --
every term within 1e-6 relative, rel-L2 of the summed gradient against fp64 below 1e-6.  Teachers and student are drawn
independently, so the summed gradient has no systematic cancellation; a torch fp32 evaluation in the kernel's order (terms
summed in fp32 throughout, which the kernel does per thread only) is within 2e-7 on every term and 6e-8 on every summed
gradient of the cases here, checked on the CPU when the seeds were fixed."""
import pytest
import torch
import torch.nn.functional as F

from tests import criteria_util as CU
from tests import guard_util as GU

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NUMELS = (4, 4092, 4096, 4100, 20484)
SMOOTH_BETA, HUBER_DELTA = CU.KINDS['smooth_l1'], CU.KINDS['huber']
PARAM = {'mse': 0.0, 'l1': 0.0, 'smooth_l1': SMOOTH_BETA, 'huber': HUBER_DELTA}
CYCLE = ('mse', 'l1', 'smooth_l1', 'huber')

# grouping -> list of (unit, teacher slot, kind, mean?, factor); pairs of one unit share student and grad.
# `mixed` interleaves its units: two groups (a: 2 members, b: 3), a lone pair and a pair without a gradient.
GROUPINGS = {
    'two': [('a', 0, 'mse', False, 0.5), ('a', 1, 'l1', True, 2.0)],
    'three': [('a', 0, 'mse', True, 1.5), ('a', 1, 'smooth_l1', False, 0.25), ('a', 2, 'huber', True, 3.0)],
    'eight': [('a', i, CYCLE[i % 4], i % 2 == 1, (0.5, 2.0, 0.25, 3.0, 1.0, 1.5, 0.75, 2.5)[i]) for i in range(8)],
    'two_same_teacher': [('a', 0, 'mse', False, 0.5), ('a', 0, 'smooth_l1', True, 2.0)],
    'mixed': [('a', 0, 'l1', False, 0.5), ('b', 0, 'huber', True, 2.0), ('lone', 0, 'smooth_l1', False, 1.0),
              ('a', 1, 'mse', True, 1.5), ('b', 1, 'mse', False, 0.25), ('null', 0, 'l1', True, 3.0),
              ('b', 2, 'smooth_l1', True, 0.75)],
}
SEEDS = {'two': 101, 'three': 102, 'eight': 103, 'two_same_teacher': 104, 'mixed': 105}


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


_CASES = {}


def case(grouping, numel):
    """(students, teachers, reference) of a grouping at a size, made once and never written: students[unit], teachers[(unit,
    slot)] fp32 on the CPU; reference[relu_mask] = (terms, {unit: fp64 gradient}).  For numel = 4 the draw is repeated
    until every two-zone member has both zones in its four elements."""
    key = (grouping, numel)
    if key in _CASES:
        return _CASES[key]
    spec = GROUPINGS[grouping]
    g = torch.Generator().manual_seed(SEEDS[grouping] * 100003 + numel)
    for _ in range(200):
        students, teachers = {}, {}
        for unit, slot, _, _, _ in spec:
            if unit not in students:
                students[unit] = F.relu(torch.randn(numel, generator=g) * 1.5)
            if (unit, slot) not in teachers:
                teachers[(unit, slot)] = F.relu(torch.randn(numel, generator=g) * 1.5)
        shares = [float(((students[u] - teachers[(u, sl)]).abs() > PARAM[k]).double().mean())
                  for u, sl, k, _, _ in spec if PARAM[k]]
        if all(0.05 < v < 0.95 for v in shares):
            break
    else:
        raise AssertionError('no draw with both zones populated')
    ref = {}
    for relu_mask in (0, 1):
        terms, grads = [], {}
        for unit, slot, kind, mean, f in spec:
            w = f / numel if mean else f
            val, grad = CU.fp64_reference(kind, PARAM[kind], teachers[(unit, slot)], students[unit], w, False)
            terms.append(float(val) * w)
            grads[unit] = grads[unit] + grad if unit in grads else grad
        if relu_mask:
            grads = {u: gr * (students[u] > 0) for u, gr in grads.items()}
        ref[relu_mask] = (terms, grads)
    _CASES[key] = (students, teachers, ref)
    return _CASES[key]


def device_pairs(grouping, numel, relu_mask, take=None, load=None):
    """the launch's pair tuples; the pairs of a unit name ONE student tensor and ONE grad tensor (NaN-filled)"""
    take = take or (lambda name, n: torch.full((n,), float('nan'), device=DEV))
    load = load or (lambda name, t: t.to(DEV))
    students, teachers, _ = case(grouping, numel)
    s_dev = {u: load('s_' + u, s) for u, s in students.items()}
    t_dev = {k: load('t_%s%d' % k, t) for k, t in teachers.items()}
    g_dev = {u: None if u == 'null' else take('grad_' + u, numel) for u in students}
    pairs = [(t_dev[(u, sl)], s_dev[u], g_dev[u], f, relu_mask, kind, PARAM[kind], numel if mean else 0)
             for u, sl, kind, mean, f in GROUPINGS[grouping]]
    return pairs, g_dev


def check(grouping, numel, relu_mask, out, g_dev):
    terms, grads = case(grouping, numel)[2][relu_mask]
    out = out.cpu()
    worst_t = max(abs(float(out[1 + i]) - t) / t for i, t in enumerate(terms))
    e_tot = abs(float(out[0]) - sum(terms)) / sum(terms)
    worst_g = 0.0
    for u, gref in grads.items():
        if g_dev[u] is None:
            continue
        got = g_dev[u].cpu()
        assert bool(torch.isfinite(got).all()), u
        worst_g = max(worst_g, rel_l2(got, gref))
    print('%s numel %d relu_mask %d: terms %.2e total %.2e summed gradient %.2e' % (grouping, numel, relu_mask, worst_t,
                                                                                   e_tot, worst_g))
    assert worst_t <= 1e-6 and e_tot <= 1e-6, (worst_t, e_tot)
    assert worst_g < 1e-6, worst_g
    return worst_t, worst_g


@pytest.mark.parametrize('relu_mask', [0, 1])
@pytest.mark.parametrize('numel', NUMELS)
@pytest.mark.parametrize('grouping', list(GROUPINGS))
def test_grouped_launch_matches_torch_fp64(ops, grouping, numel, relu_mask):
    pairs, g_dev = device_pairs(grouping, numel, relu_mask)
    out = ops.MimicLaunch(pairs, DEV).run()
    ops.sync_check()
    check(grouping, numel, relu_mask, out, g_dev)
    if relu_mask:               # the mask acts on the SUM: nothing where the student is not positive
        students = case(grouping, numel)[0]
        for u, gbuf in g_dev.items():
            if gbuf is not None:
                assert bool((gbuf.cpu()[students[u] <= 0] == 0).all())


@pytest.mark.parametrize('grouping', ['three', 'eight', 'mixed'])
def test_two_runs_of_a_grouped_launch_are_bit_identical(ops, grouping):
    runs = []
    for _ in range(2):
        pairs, g_dev = device_pairs(grouping, 20484, 1)
        ml = ops.MimicLaunch(pairs, DEV)
        first = ml.run().clone()
        assert torch.equal(ml.run(), first)             # replay of the cached launch object
        runs.append((first, [g for g in g_dev.values() if g is not None]))
    ops.sync_check()
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


@pytest.mark.parametrize('grouping', ['three', 'two_same_teacher'])
def test_the_value_of_a_grouped_term_is_that_of_the_pair_launched_alone(ops, grouping):
    pairs, _ = device_pairs(grouping, 20484, 1)
    grouped = ops.MimicLaunch(pairs, DEV).run().cpu()
    for i, p in enumerate(pairs):
        alone = ops.MimicLaunch([p[:2] + (torch.empty_like(p[1]),) + p[3:]], DEV).run().cpu()
        ops.sync_check()
        e = abs(float(grouped[1 + i]) - float(alone[1])) / float(alone[1])
        print('%s pair %d: grouped %.17g alone %.17g (%.1e)' % (grouping, i, float(grouped[1 + i]), float(alone[1]), e))
        assert e <= 1e-6


def test_group_of_three_inside_guard_bands(ops):
    """numel 4100 (a chunk plus one vector): every buffer of the launch is a view of one arena with 0xFF guards around it;
    scratch holds exactly hnd_mse_scratch_elems() doubles and loss_out exactly 1 + npairs"""
    from hnd_ghnd_object_detectors_amd import _lib
    numel, nscratch = 4100, int(_lib.load().hnd_mse_scratch_elems())
    specs = [((numel,), torch.float32)] * 5 + [((4,), torch.float64), ((nscratch,), torch.float64)]
    arena = GU.Arena(DEV, GU.arena_bytes(specs))
    pairs, g_dev = device_pairs('three', numel, 1, take=lambda name, n: arena.take(name, n), load=arena.load)
    ml = ops.MimicLaunch(pairs, DEV)
    ml.out = arena.take('out', 1 + len(pairs), torch.float64, fill=0)
    ml.scratch = arena.take('scratch', nscratch, torch.float64)
    assert len(arena.views) == len(specs)
    ml.run()
    ops.sync_check()
    arena.check()
    assert bool(torch.isfinite(ml.out).all())
    check('three', numel, 1, ml.out, g_dev)
