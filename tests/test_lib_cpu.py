"""CPU: the C-ABI library builds, loads, and exports every symbol the four headers under include/ declare; the binding
hnd_ghnd_object_detectors_amd/_lib.py reads from those headers lays its structs out as the C compiler does, and its reader
refuses what it does not know."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_NAMES = ('hnd_hip.h', 'hnd_optim.h', 'hnd_codec.h', 'hnd_qat.h')
STRUCTS = {'hnd_conv_desc': 'ConvDesc', 'hnd_wgrad_desc': 'WgradDesc', 'hnd_pack_desc': 'PackDesc', 'hnd_image_desc': 'ImageDesc',
           'hnd_boxes_desc': 'BoxesDesc', 'hnd_mse_pair': 'MsePair', 'hnd_mimic_pair': 'MimicPair', 'hnd_optim_desc': 'OptimDesc'}


def _declared(header='hnd_hip.h'):
    """the names a header declares, found WITHOUT the reader of _lib.py"""
    text = open(os.path.join(ROOT, 'include', header)).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(hnd_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    declared = _declared()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared
    assert lib.hnd_abi_version() == _lib.ABI_VERSION == 12


def test_every_export_is_declared_by_exactly_one_header():
    """the optimizer kinds, the bit codec and the fake quantiser came with a header, a version and a symbol tuple of their
    own: no name of theirs is in another header's tuple, and hnd_hip.h still declares exactly the 94 it did"""
    import __graft_entry__ as g
    g.build()
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    tuples = dict(zip(HEADER_NAMES, (_lib.EXPORTED_SYMBOLS, _lib.OPTIM_SYMBOLS, _lib.CODEC_SYMBOLS, _lib.QAT_SYMBOLS)))
    assert tuple(_lib.HEADERS) == HEADER_NAMES
    for header, names in tuples.items():
        assert list(names) == _declared(header) == sorted(_lib.HEADERS[header].functions), header
    every = [n for names in tuples.values() for n in names]
    assert len(every) == len(set(every)) == 104 and [len(tuples[h]) for h in HEADER_NAMES] == [94, 2, 5, 3]
    for name in every:
        assert getattr(lib, name).argtypes is not None, name


def test_ctypes_structs_match_header_layout(tmp_path):
    """sizeof of the eight structs and offsetof of every field, printed by a host C program compiled from the four headers
    with the ROCm toolchain's compiler (no device code), against the classes _lib.py generates"""
    from hnd_ghnd_object_detectors_amd import _lib
    assert {tag for h in _lib.HEADERS.values() for tag in h.structs} == set(STRUCTS)
    lines = ['#include <stddef.h>', '#include <stdio.h>'] + ['#include "%s"' % h for h in HEADER_NAMES] + ['int main(void) {']
    want = {}
    for tag, cls in ((tag, getattr(_lib, name)) for tag, name in STRUCTS.items()):
        assert cls is [h for h in _lib.HEADERS.values() if tag in h.structs][0].structs[tag]
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (tag, tag))
        want[tag] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (tag, field, tag, field))
            want['%s.%s' % (tag, field)] = getattr(cls, field).offset
    (tmp_path / 'layout.c').write_text('\n'.join(lines + ['  return 0;', '}', '']))
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    subprocess.run([hipcc, '-std=c99', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'), str(tmp_path / 'layout.c'), '-o',
                    str(tmp_path / 'layout')], check=True, capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True, timeout=60).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert len(want) == 8 + sum(len(getattr(_lib, name)._fields_) for name in STRUCTS.values()) and len(want) > 140
    assert got == want, sorted(set(got.items()) ^ set(want.items()))


@pytest.mark.parametrize('snippet, line', [
    ('int hnd_f(long n);', 1),                                                       # an unknown type
    ('int hnd_f(const float* x,\n          unsigned int n);', 1),
    ('typedef struct hnd_s {\n  int32_t n;\n  wchar_t* name;\n} hnd_s;', 3),
    ('\n\nint hnd_f(void (*done)(int), void* stream);', 3),                          # a function-pointer parameter
    ('int hnd_f(int n);\ntypedef struct hnd_s {\n  int32_t n;\n', 2),               # an unterminated struct
    ('typedef struct hnd_s {\n  int32_t n\n} hnd_s;', 3),
    ('typedef struct hnd_s {\n  float *a, b;\n} hnd_s;', 2),
    ('typedef enum hnd_e {\n  HND_A = 0,\n  HND_B\n} hnd_e;', 3),                   # an enumerator without its value
    ('#define HND_N 1\n#if HND_N\nint hnd_f(void);\n#endif', 2),
    ('int hnd_f();', 1),
    ('/* never closed\nint hnd_f(void);', 1),
])
def test_reader_refuses_what_is_outside_its_grammar(snippet, line):
    from hnd_ghnd_object_detectors_amd import _lib
    with pytest.raises(_lib.HndLibraryError, match=r'^snippet\.h:%d: ' % line):
        _lib.parse_header(snippet, 'snippet.h')


def test_reader_refuses_a_function_declared_twice():
    from hnd_ghnd_object_detectors_amd import _lib
    once = _lib.parse_header('int hnd_f(int n, void* stream);', 'snippet.h')
    assert once.functions == {'hnd_f': (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p])}
    with pytest.raises(_lib.HndLibraryError, match=r'^snippet\.h:2: hnd_f is declared twice'):
        _lib.parse_header('int hnd_f(int n, void* stream);\nint hnd_f(int64_t n, void* stream);', 'snippet.h')


def test_invalid_arguments_are_reported_not_thrown():
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    assert lib.hnd_conv2d_igemm(None, None) == -1
    assert b'null descriptor' in lib.hnd_last_error_string()
    assert lib.hnd_adam_step_flat(None, None, None, None, 0, 0.0, 0.0, 0.0, 0.0, 0, 1.0, None) == -1


def test_detection_operators_validate_their_arguments():
    """the validation-path entry points (ABI 3 / 4) reject null pointers and bad geometry with HND_ERR_INVALID and a
    message, and treat an empty problem (k = 0) as a successful no-op -- all before any HIP call, so this runs on CPU"""
    from hnd_ghnd_object_detectors_amd import _lib
    lib = _lib.load()
    assert lib.hnd_mask_probs(None, None, 0, 28, 91, None, None) == 0
    assert lib.hnd_mask_probs(None, None, 5, 28, 91, None, None) == -1
    assert b'hnd_mask_probs' in lib.hnd_last_error_string()
    assert lib.hnd_paste_masks(None, None, 0, 28, 800, 1333, None, None) == 0
    assert lib.hnd_paste_masks(None, None, 3, 28, 800, 1333, None, None) == -1
    assert lib.hnd_upsample_bilinear_nhwc(None, 2, 28, 28, 17, 2, None, None) == -1
    assert lib.hnd_heatmaps_to_keypoints(None, 0, 56, 56, 17, 17, None, None, None, None) == 0
    assert lib.hnd_heatmaps_to_keypoints(None, 4, 56, 56, 17, 17, None, None, None, None) == -1
    assert b'hnd_heatmaps_to_keypoints' in lib.hnd_last_error_string()
    assert lib.hnd_nms(None, None, 0, 0.5, None, None, None) == 0
    assert lib.hnd_nms(None, None, 10, 0.5, None, None, None) == -1
    assert lib.hnd_roi_align(None, 1, 8, 8, 64, None, None, 3, 0.25, 7, 7, 2, None, None) == -1
    assert lib.hnd_nms_workspace(4800) == 4800 * 75 * 8


def test_bres2_inline_asm_ring_is_untouched_between_load_and_wait():
    """csrc/conv_bres.hip / conv_bstream.hip / conv_wgrad_ring.hip / conv_bx3.hip / conv_bxs.hip hide their ring loads (A fragments; the parked B-stage
    loads of bstream; both operands of the ring weight gradient) from hipcc -- inline asm `global_load_dwordx4` +
    hand-counted `s_waitcnt vmcnt(N)` -- and the compiler is then free to copy / spill / reuse a ring register before its
    data has landed.  tools/audit_bres_asm.py walks the control-flow graph of the generated assembly (every path, loop
    back edges included) and must find no instruction touching a ring register between its asm load and the wait that
    releases it."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, 'tools', 'audit_bres_asm.py')], capture_output=True,
                         text=True, timeout=1800)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert all(k in res.stdout for k in ('bres2_kernel', 'bstream_kernel', 'wgrad_ring_kernel', 'bx3_kernel', 'bxs_kernel'))
    assert res.stdout.count(' 0 problem(s)') == 5 and ': 0 16-byte loads' not in res.stdout
