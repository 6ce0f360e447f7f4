"""CPU self-test of tests/guard_util.py: the guard-band arena reports what it must, where it must."""
import pytest
import torch

from tests import guard_util as G


def _arena():
    a = G.Arena('cpu', G.arena_bytes([((3, 5, 7, 64), torch.float32), ((13,), torch.uint8), ((4, 3), torch.int64)]
                                     + 3 * [((6,), torch.int64)]))
    x = a.take('x', (3, 5, 7, 64), torch.float32)
    m = a.take('mask', (13,), torch.uint8)
    i = a.load('idx', torch.arange(12, dtype=torch.int64).view(4, 3))
    return a, x, m, i


def test_views_are_aligned_exact_and_prefilled():
    a, x, m, i = _arena()
    for v in (x, m, i):
        assert v.is_contiguous() and v.data_ptr() % 256 == 0
    assert bool(torch.isnan(x).all())                       # 0xFF as fp32 is a NaN
    assert bool((m == 0xFF).all())                          # as a mask byte every bit is set
    assert torch.equal(i, torch.arange(12).view(4, 3))
    assert bool((a.take('neg', (5,), torch.int32) == -1).all()) and bool((a.take('neg64', (2,), torch.int64) == -1).all())
    assert float(a.take('ws', (6,), torch.float32, fill=0).abs().sum()) == 0.0
    # the end is not rounded: the byte after the 13-byte view is a guard byte
    _, start, end, g = [v for v in a.views if v[0] == 'mask'][0]
    assert end - start == 13 and g == G.MIN_GUARD and int(a.base[end]) == 0xFF
    # G = max(256 KiB, 256 rows of the view's pitch): a [.., 2048] fp32 view asks for 2 MiB
    assert G.guard_bytes((9, 2048), torch.float32) == 256 * 2048 * 4
    assert G.guard_bytes((9, 64), torch.float32) == 256 * 1024 and G.guard_bytes((1 << 20,), torch.float32) == 256 * 1024
    # at least G owned bytes lie between neighbours and at both ends of the arena
    prev_end = 0
    for _, s, e, gg in a.views:
        assert s - prev_end >= gg
        prev_end = e
    assert a.base.numel() - prev_end >= a.views[-1][3]
    with pytest.raises(ValueError, match='too small'):
        G.Arena('cpu', 1 << 20).take('big', (1 << 20,), torch.uint8)


def test_a_clean_sequence_passes():
    a, x, m, i = _arena()
    x.fill_(1.5)
    m.zero_()
    i.add_(1)
    x[-1, -1, -1, -1] = 2.0                                 # the last element of a view is the view's
    m[12] = 7
    a.check()
    a.check()


@pytest.mark.parametrize('name', ['x', 'mask', 'idx'])
@pytest.mark.parametrize('side', ['before', 'after'])
def test_one_damaged_byte_is_reported_with_view_side_and_offset(name, side):
    a = _arena()[0]
    _, start, end, g = [v for v in a.views if v[0] == name][0]
    for off in (0, 1, 4097, g // 2 - 1):                    # (nearer to this view than to its neighbour: bands are shared)
        at = start - 1 - off if side == 'before' else end + off
        a.base[at] = 0                                      # through the arena's own base tensor: in bounds of the allocation
        with pytest.raises(G.GuardDamage) as e:
            a.check()
        assert e.value.reports == [dict(name=name, side=side, first=off, last=off, count=1)], e.value.reports
        assert repr(name) in str(e.value) and side in str(e.value)
        a.base[at] = 0xFF
        a.check()


def test_a_write_at_distance_g_minus_1_is_still_caught():
    a = _arena()[0]
    (_, s0, e0, g0), (_, s1, e1, g1) = a.views[0], a.views[-1]
    for at in (s0 - 1 - (g0 - 1), e1 + (g1 - 1)):           # the outer ends of the first and the last band
        a.base[at] = 0xFE
        with pytest.raises(G.GuardDamage) as e:
            a.check()
        r = e.value.reports
        assert len(r) == 1 and r[0]['first'] == r[0]['last'] == (g0 if at < s0 else g1) - 1 and r[0]['count'] == 1
        assert (r[0]['name'], r[0]['side']) == (('x', 'before') if at < s0 else ('idx', 'after'))
        a.base[at] = 0xFF
    # between two views every byte belongs to some band: G - 1 past `x` is caught, whichever neighbour it is charged to
    a.base[e0 + g0 - 1] = 1
    with pytest.raises(G.GuardDamage) as e:
        a.check()
    assert sum(r['count'] for r in e.value.reports) == 1


def test_a_run_of_damage_reports_first_last_and_count():
    a = _arena()[0]
    _, start, end, g = a.views[0]
    a.base[end:end + 256] = 0                               # "one row too many" of a 64-channel fp32 tensor
    a.base[start - 3:start] = 1
    with pytest.raises(G.GuardDamage) as e:
        a.check()
    assert e.value.reports == [dict(name='x', side='after', first=0, last=255, count=256),
                               dict(name='x', side='before', first=0, last=2, count=3)]


def test_a_whole_band_of_damage_is_reported_without_walking_its_bytes():
    a = _arena()[0]
    (_, s0, e0, g0), (_, s1, e1, g1) = a.views[0], a.views[1]
    a.base[e0:s1] = 0                                       # everything between `x` and `mask`: split where the distances meet
    with pytest.raises(G.GuardDamage) as e:
        a.check()
    gap = s1 - e0
    assert e.value.reports == [dict(name='x', side='after', first=0, last=(gap - 1) // 2, count=(gap - 1) // 2 + 1),
                               dict(name='mask', side='before', first=0, last=gap // 2 - 1, count=gap // 2)]
