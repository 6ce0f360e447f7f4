"""No GPU: hnd_mimic_loss_fwd_bwd refuses, before any HIP call, pairs that share `grad` without being a group (different
student, numel or relu_mask) and gradient ranges that overlap without being identical.  The checks compare pointers only,
so host memory stands in for the device pointers and nothing is ever read through them."""
import ctypes
import re


def _lib():
    import __graft_entry__ as g
    g.build()
    from hnd_ghnd_object_detectors_amd import _lib
    return _lib, _lib.load()


def _refused_naming(lib, arr, n, out, i, j):
    rc = lib.hnd_mimic_loss_fwd_bwd(arr, n, out, out, None)
    msg = lib.hnd_last_error_string().decode()
    assert rc == -1, (rc, msg)
    assert 'hnd_mimic_loss_fwd_bwd' in msg
    assert sorted(int(v) for v in re.findall(r'\b\d+\b', msg.split('pairs', 1)[1])[:2]) == [i, j], msg
    return msg


def test_shared_grad_and_overlapping_grad_ranges_are_validated_on_pointers_alone():
    L, lib = _lib()
    bufs = [(ctypes.c_float * 256)() for _ in range(4)]
    t, s, s2, g = [ctypes.addressof(b) for b in bufs]
    out = ctypes.addressof((ctypes.c_double * 16)())

    def pairs(n, **last):
        arr = (L.MimicPair * n)()
        for a in arr:
            a.teacher, a.student, a.grad, a.numel, a.count = t, s, g, 64, 0
            a.factor, a.param, a.kind, a.relu_mask = 1.0, 1.0, 2, 1
        for k, v in last.items():
            setattr(arr[n - 1], k, v)
        return arr

    assert 'student' in _refused_naming(lib, pairs(2, student=s2), 2, out, 0, 1)
    assert 'numel' in _refused_naming(lib, pairs(2, numel=32), 2, out, 0, 1)
    assert 'relu_mask' in _refused_naming(lib, pairs(2, relu_mask=0), 2, out, 0, 1)
    # the disagreeing member is found wherever it sits: pair 2 against pair 0 of a group of three
    _refused_naming(lib, pairs(3, student=s2), 3, out, 0, 2)
    # [g + 16 floats, + 64 floats) overlaps [g, g + 64 floats): two sets of workgroups would write the same elements
    assert 'overlap' in _refused_naming(lib, pairs(2, grad=g + 16 * 4), 2, out, 0, 1)
    assert 'overlap' in _refused_naming(lib, pairs(2, grad=g + 63 * 4, numel=4), 2, out, 0, 1)
    arr = pairs(3, grad=g + 32 * 4)
    arr[1].grad = None                                      # a pair without a gradient is in nobody's way
    _refused_naming(lib, arr, 3, out, 0, 2)


def test_the_scratch_query_covers_one_slot_per_member_and_workgroup():
    """a grouped launch keeps one partial sum per (member, workgroup): at most 1024 workgroups of up to 8 members"""
    _, lib = _lib()
    assert lib.hnd_mse_scratch_elems() >= 1024 * 8
    assert lib.hnd_abi_version() == 12
