"""CPU: the picker between the two builds of the bf16x3 emulation GEMM (csrc/conv_bx3.hip: bx3_build; the tiled build is
csrc/conv_bx3_tiled.hip) and the tiled kernel's resource usage.  No GPU: the CU count falls back to 256 and the picker only
needs non-null, 16-byte-aligned pointer VALUES (nothing is dereferenced).

The crossovers pinned here are the ones read from profiles/r07_bx3_tiled_shapes.txt (tools/bench_bx3_tiled.py on an
MI355X): at batch 16 fpn.inner0 (16 x 200 x 336, 256 -> 256: 263 chunks per team) and layer2.0.conv1 (256 -> 128: 132) run
0.60 x / 0.55 x on the tiled build and stay persistent; layer4.x.conv1 (2048 -> 512: 9 chunks per team) runs 1.30 x tiled."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from hnd_ghnd_object_detectors_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def clean_picker_env():
    old = os.environ.pop('HND_DEBUG_PICKER', None)
    yield
    os.environ.pop('HND_DEBUG_PICKER', None)
    if old is not None:
        os.environ['HND_DEBUG_PICKER'] = old


def desc(n, h, w, cin, cout, stride=1, image=True, groups_rows=0, **extra):
    from hnd_ghnd_object_detectors_amd import _lib
    d = _lib.ConvDesc()
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    d.x, d.w, d.y = 0x10000, 0x20000, 0x30000
    d.n, d.h, d.w_, d.cin = n, h, w, cin
    d.oh, d.ow, d.yh, d.yw, d.cout, d.ldc = oh, ow, oh, ow, cout, cout
    d.y_sh, d.y_oh, d.y_sw, d.y_ow = 1, 0, 1, 0
    d.kh, d.kw = 1, 1
    d.sh, d.dh, d.bh, d.sw, d.dw, d.bw = stride, 1, 0, stride, 1, 0
    d.kdim = cin
    d.w_group_rows, d.w_group_stride = groups_rows, (cout * cin if groups_rows else 0)
    if image:
        d.w_bf16x3 = 0x40000
    for k, v in extra.items():
        setattr(d, k, v)
    return d


def build_of(lib, d):
    return int(lib.hnd_conv2d_igemm_build(ctypes.byref(d))), int(lib.hnd_conv2d_igemm_tile(ctypes.byref(d)))


def test_the_export_exists_is_declared_and_rejects_null(lib):
    from hnd_ghnd_object_detectors_amd import _lib
    assert 'hnd_conv2d_igemm_build' in _lib.EXPORTED_SYMBOLS
    header = open(os.path.join(ROOT, 'include', 'hnd_hip.h')).read()
    assert re.search(r'int\s+hnd_conv2d_igemm_build\s*\(\s*const\s+hnd_conv_desc\s*\*', header)
    assert lib.hnd_conv2d_igemm_build(None) == -1
    assert lib.hnd_abi_version() == 12


def test_the_debug_key_forces_either_build_where_the_kernel_applies_and_nothing_elsewhere(lib):
    ok = desc(16, 50, 84, 1024, 256)
    grouped = desc(1, 64, 64 * 8, 256, 256, groups_rows=512)          # 64 groups of 512 rows: a Winograd component launch
    no_image = desc(16, 50, 84, 1024, 256, image=False)
    stats = desc(16, 50, 84, 1024, 256, stats=0x50000)
    taps = desc(16, 50, 84, 1024, 256)
    taps.kh, taps.kw, taps.bh, taps.bw, taps.kdim = 3, 3, 1, 1, 9 * 1024
    for key, want in (('bx3_tiled=1', 1), ('bx3_tiled=0', 0), ('bres_all,bx3_tiled=1', 1)):
        os.environ['HND_DEBUG_PICKER'] = key
        assert build_of(lib, ok) == (want, 13), key
        assert build_of(lib, grouped) == (want, 13), key
        for d in (no_image, stats, taps):
            b, t = build_of(lib, d)
            assert b == 0 and t != 13, (key, b, t)
    assert lib.hnd_conv2d_igemm_workspace(ctypes.byref(ok)) == 0


def test_the_rule_is_monotone_in_the_row_count_and_lands_where_the_measured_table_says(lib):
    seen_tiled = 0
    for cin in (128, 256, 512, 768, 1024, 1536, 2048):
        for cout in (64, 128, 256, 512, 1024, 2048):
            persistent_from = None
            for rows in list(range(1, 64)) + list(range(64, 4096, 37)):
                b, t = build_of(lib, desc(1, rows, 64, cin, cout))              # M = 64 rows: `rows` chunks
                assert t == 13 and b in (0, 1)
                seen_tiled += b
                if b == 0 and persistent_from is None:
                    persistent_from = rows
                assert not (b == 1 and persistent_from is not None), (cin, cout, rows, persistent_from)
            assert persistent_from is not None, (cin, cout)          # large grids belong to the persistent kernel
    assert seen_tiled > 0
    # the step's launches (800 x 1344 images; profiles/r07_bx3_tiled_shapes.txt)
    assert build_of(lib, desc(16, 200, 336, 256, 256))[0] == 0         # fpn.inner0, batch 16: tiled 0.60 x
    assert build_of(lib, desc(16, 200, 336, 256, 128))[0] == 0         # layer2.0.conv1, batch 16: 0.55 x
    assert build_of(lib, desc(4, 200, 336, 256, 256))[0] == 0          # ... and at batch 4: 0.58 x
    assert build_of(lib, desc(16, 50, 84, 1024, 256))[0] == 0          # layer3.x.conv1, batch 16: 1.04 x / 1.01 x, inside the noise
    assert build_of(lib, desc(4, 50, 84, 1024, 256))[0] == 1           # ... batch 4: 1.51 x
    assert build_of(lib, desc(1, 50, 84, 1024, 256))[0] == 1
    assert build_of(lib, desc(4, 25, 42, 2048, 256))[0] == 1           # fpn.inner3, batch 4: 1.91 x
    assert build_of(lib, desc(16, 25, 42, 2048, 512))[0] == 1          # layer4.x.conv1, batch 16: 1.30 x
    assert build_of(lib, desc(4, 100, 168, 512, 128))[0] == 1          # layer2.x.conv1, batch 4: 1.13 x
    assert build_of(lib, desc(8, 100, 168, 512, 128))[0] == 0          # ... batch 8: 0.88 x
    # grouped launches were not measured: persistent unless forced
    assert build_of(lib, desc(1, 64, 64 * 4, 512, 512, groups_rows=256))[0] == 0


def test_the_tiled_kernel_uses_no_scratch_in_any_instantiation(tmp_path):
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'hnd_ghnd_object_detectors_amd', 'csrc', 'conv_bx3_tiled.hip')
    out = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(ROOT, 'include'),
                          '-ffp-contract=fast', '-Rpass-analysis=kernel-resource-usage', '-c', src, '-o',
                          str(tmp_path / 'conv_bx3_tiled.o')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    names = re.findall(r'Function Name: (\S+)', out)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', out)]
    spills = [int(v) for v in re.findall(r'VGPRs Spill: (\d+)', out)]
    kernels = [n for n in names if 'bx3t_kernel' in n]
    assert len(kernels) == 2 and len(scratch) == len(names) == len(spills), out
    assert not any('bx3_kernel' in n for n in names)            # (tools/audit_bres_asm.py matches kernels by that substring)
    assert scratch == [0] * len(names) and spills == [0] * len(names), out
    text = open(src).read().lower()
    assert 'asm' not in re.sub(r'//.*', '', text)                # compiler-visible loads and LDS only: nothing to audit
