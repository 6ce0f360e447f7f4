"""CPU: the ledger of tests/test_guard_bands_gpu.py against include/hnd_hip.h.

Every export the header declares is either covered by a guard-band case (@covers) or sits in NO_DEVICE_OUTPUT (it writes
no caller-owned device memory: size and variant queries, error strings, the RCCL entry points; one-line reason each).
An export added to the header lands in neither and turns this red."""
import sys

from tests.test_lib_cpu import _declared


def test_every_export_that_writes_device_memory_has_a_guard_case():
    loaded = 'hnd_ghnd_object_detectors_amd.ops' in sys.modules
    from tests import test_guard_bands_gpu as T
    # importing the guard-band module must not touch the GPU: it loads neither the library nor the launch helpers
    assert loaded or 'hnd_ghnd_object_detectors_amd.ops' not in sys.modules
    declared = set(_declared())
    covered = set().union(*T.LEDGER.values())
    assert covered and all(T.LEDGER.values())
    assert all(isinstance(reason, str) and reason for reason in T.NO_DEVICE_OUTPUT.values())
    assert not covered & set(T.NO_DEVICE_OUTPUT), sorted(covered & set(T.NO_DEVICE_OUTPUT))
    everything = covered | set(T.NO_DEVICE_OUTPUT)
    assert everything == declared, (sorted(declared - everything), sorted(everything - declared))
    # every case that declares exports is a test of the module
    assert all(callable(getattr(T, name, None)) and name.startswith('test_') for name in T.LEDGER)
