"""Records what the conv kernel pickers of libhnd_hip.so decide, for tests/test_conv_picker_cpu.py to replay.

    HND_LIB_PATH=<libhnd_hip.so of the commit to record> python tests/golden/make_picker_table.py

writes tests/golden/conv_picker_table.npz: a fixed-seed sample of hnd_conv_desc / hnd_wgrad_desc descriptors and a grid of
(rows, K, cout, taps), and under every environment setting of SETTINGS the answers of hnd_conv2d_igemm_tile / _build /
_workspace, hnd_conv2d_wgrad_variant / _workspace and hnd_bf16x3_recommended / hnd_bf16x3s_recommended.  No GPU is needed:
the pickers read pointer VALUES only and take 256 compute units when no device answers (an MI355X has 256).  Every
setting is evaluated in a fresh child process, so a library that reads a switch once per process is recorded correctly.

The table in the repository was made from the library of the commit named in the table's `source` entry (pass it as
argv[1]); it is a refactoring fixture: regenerate it only from a commit whose picker rules are MEANT to differ."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, 'conv_picker_table.npz')

SWITCHES = ('HND_BRES', 'HND_BRES2', 'HND_BSTREAM', 'HND_BXS', 'HND_STEM7', 'HND_THIN_N', 'HND_WGRAD_RING', 'HND_THIN_WGRAD',
            'HND_DEBUG_PICKER')
PICKER_KEYS = ('bres_all', 'bstream_all', 'igemm_tile=0', 'igemm_tile=1', 'igemm_tile=2', 'igemm_tile=3', 'wgrad_ring_taps',
               'bstream_k1024', 'bstream_parity', 'bxs_wn1', 'bx3_tiled=0', 'bx3_tiled=1', 'bx3_tiled_mi=1', 'bx3_tiled_mi=2',
               'bres_all,bx3_tiled=1')
# "NAME=value"; '' = nothing set.  "0" and "1" for every on/off switch, HND_BRES also as a depth.
SETTINGS = ('',) + tuple('%s=%s' % (s, v) for s in SWITCHES[:-1] for v in ('0', '1')) + ('HND_BRES=256',) + \
    tuple('HND_DEBUG_PICKER=' + k for k in PICKER_KEYS)
# Settings that spell out the default (a switch that is on anyway), and bx3_tiled_mi, which picks the tiled build's row tile
# only under bx3_tiled=1 and never shows in a recorded answer: these must change NOTHING; every other setting changes a row.
NO_OPS = ('HND_BRES2=1', 'HND_BSTREAM=1', 'HND_BXS=1', 'HND_STEM7=1', 'HND_THIN_N=1', 'HND_WGRAD_RING=1', 'HND_THIN_WGRAD=1',
          'HND_DEBUG_PICKER=bx3_tiled_mi=1', 'HND_DEBUG_PICKER=bx3_tiled_mi=2')
CONV_ANSWERS = ('conv_tile', 'conv_build', 'conv_workspace')
WGRAD_ANSWERS = ('wgrad_variant', 'wgrad_workspace')
REC_ANSWERS = ('rec_bx3', 'rec_bxs')


def _lib_module():
    sys.path.insert(0, ROOT)
    from hnd_ghnd_object_detectors_amd import _lib
    return _lib


TILE_CODES = tuple(sorted(c for n, c in _lib_module().CONV_TILES.items() if n != 'unused'))      # enum hnd_conv_tile


def field_names(cls):
    return [n for n, _ in cls._fields_]


def fill(desc, names, row):
    for n, v in zip(names, row):
        setattr(desc, n, int(v))
    return desc


def set_env(setting):
    for s in SWITCHES:
        os.environ.pop(s, None)
    if setting:
        k, v = setting.split('=', 1)
        os.environ[k] = v


def evaluate(lib, _lib, conv, wgrad, rec):
    """the recorded answers for the descriptor rows `conv` / `wgrad` and the grid `rec`, under the current environment"""
    out = {k: np.zeros(len(conv), np.int64) for k in CONV_ANSWERS}
    out.update({k: np.zeros(len(wgrad), np.int64) for k in WGRAD_ANSWERS})
    out.update({k: np.zeros(len(rec), np.int64) for k in REC_ANSWERS})
    names, d = field_names(_lib.ConvDesc), _lib.ConvDesc()
    for i, row in enumerate(conv):
        p = ctypes.byref(fill(d, names, row))
        out['conv_tile'][i] = lib.hnd_conv2d_igemm_tile(p)
        out['conv_build'][i] = lib.hnd_conv2d_igemm_build(p)
        out['conv_workspace'][i] = lib.hnd_conv2d_igemm_workspace(p)
    names, d = field_names(_lib.WgradDesc), _lib.WgradDesc()
    for i, row in enumerate(wgrad):
        p = ctypes.byref(fill(d, names, row))
        out['wgrad_variant'][i] = lib.hnd_conv2d_wgrad_variant(p)
        out['wgrad_workspace'][i] = lib.hnd_conv2d_wgrad_workspace(p)
    for i, (rows, k, cout, taps) in enumerate(rec):
        out['rec_bx3'][i] = lib.hnd_bf16x3_recommended(int(rows), int(k), int(cout))
        out['rec_bxs'][i] = lib.hnd_bf16x3s_recommended(int(rows), int(k), int(cout), int(taps))
    return out


# ---- the sample

def conv_is_valid(d):
    """hnd_conv2d_igemm's HND_REQUIREs"""
    taps, px_out, px_y, px_in = d['kh'] * d['kw'], d['n'] * d['oh'] * d['ow'], d['n'] * d['yh'] * d['yw'], d['n'] * d['h'] * d['w_']
    plain = not (d['res1'] or d['res2'] or d['mask'] or d['mask_bits'] or d['relu'])
    return bool(
        d['x'] and d['w'] and d['y'] and min(d['n'], d['h'], d['w_'], d['oh'], d['ow'], d['cout'], d['kh'], d['kw']) > 0 and
        (d['cin'] == 4 or d['cin'] % 32 == 0) and d['kdim'] % 32 == 0 and d['kdim'] >= taps * d['cin'] and
        (d['cin'] != 4 or taps <= 64) and d['ldc'] >= d['cout'] and
        d['w_group_rows'] >= 0 and d['w_group_rows'] % 128 == 0 and (d['w_group_rows'] == 0 or d['w_group_stride'] > 0) and
        max(px_out, px_y, px_in) < 2 ** 31 and (d['res1_mode'] == 0 or (d['res1_h'] > 0 and d['res1_w'] > 0)) and
        (not d['pro_scale'] or d['pro_shift']) and px_y * d['ldc'] < 2 ** 32 - 1 and not (d['mask'] and d['mask_bits']) and
        (not (d['mask_bits'] or d['mask_out']) or (d['ldc'] % 4 == 0 and d['cin'] != 4)) and
        (not d['mask_out'] or d['cout'] % 128 == 0) and px_in * d['cin'] < 2 ** 32 - 1 and
        (not d['bwd_x'] or (d['stats'] and d['bwd_scale'] and d['bwd_shift'] and d['bwd_mean'] and d['bwd_rstd'] and plain and
                            d['cin'] != 4)))


CINS = (4, 32, 64, 128, 256, 512, 768, 1024, 2048, 4096)
COUTS = (3, 4, 64, 128, 192, 256, 512, 1024, 2048)
MAPS = ((7, 11), (25, 42), (50, 84), (100, 168), (200, 336))
# (kh, kw, stride, pad, parity): parity = a stride-2 data gradient's launch, one of four output phases (y_sh = y_sw = 2)
GEOMETRIES = ((1, 1, 1, 0, 0), (1, 1, 2, 0, 0), (3, 3, 1, 1, 0), (3, 3, 2, 1, 0), (2, 2, 1, 0, 0), (2, 2, 1, 1, 0),
              (1, 1, 1, 0, 1), (1, 2, 1, 0, 1), (2, 2, 1, 0, 1))


def conv_sample(rng, names):
    ptr = dict((n, 0x100000 * (i + 1)) for i, n in enumerate(names))          # distinct 16-byte aligned pointer values
    rows = []

    def add(n, h, w, cin, cout, kh, kw, stride, pad, parity, pick):
        """pick(p) -> True with probability p; the optional operands of the launch are drawn with it"""
        d = dict.fromkeys(names, 0)
        d.update(x=ptr['x'], w=ptr['w'], y=ptr['y'], n=n, h=h, w_=w, cin=cin, cout=cout, kh=kh, kw=kw, sh=stride, sw=stride,
                 dh=1, dw=1, bh=-pad, bw=-pad)
        d['oh'], d['ow'] = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
        if d['oh'] < 1 or d['ow'] < 1:
            return
        d['kdim'] = (kh * kw * cin + 31) // 32 * 32
        if parity:
            d.update(yh=2 * d['oh'], yw=2 * d['ow'], y_sh=2, y_sw=2, y_oh=int(rng.randint(2)), y_ow=int(rng.randint(2)))
            if pick(0.5):
                d.update(bh=-(kh - 1), bw=-(kw - 1))
        else:
            d.update(yh=d['oh'], yw=d['ow'], y_sh=1, y_sw=1)
        d['ldc'] = (cout + 3) // 4 * 4 + 64 if pick(0.3) else cout
        if pick(0.15):
            d['w_group_rows'], d['w_group_stride'] = (128, 512)[rng.randint(2)], cout * d['kdim']
        for k in ('stats', 'res2', 'relu', 'mask_out'):
            if pick(0.15):
                d[k] = ptr[k] if k != 'relu' else 1
        if pick(0.15):
            d.update(pro_scale=ptr['pro_scale'], pro_shift=ptr['pro_shift'], pro_relu=int(rng.randint(2)))
        if pick(0.25):
            d['res1'] = ptr['res1']
            if pick(0.4) and d['yh'] % 2 == 0 and d['yw'] % 2 == 0:
                d.update(res1_mode=1, res1_h=d['yh'] // 2, res1_w=d['yw'] // 2)
        which = rng.randint(8)
        if which < 2:
            d['mask' if which else 'mask_bits'] = ptr['mask']
        if pick(0.08):
            d.update(stats=ptr['stats'], res1=0, res1_mode=0, res2=0, mask=0, mask_bits=0, relu=0,
                     **dict((k, ptr[k]) for k in ('bwd_x', 'bwd_scale', 'bwd_shift', 'bwd_mean', 'bwd_rstd')))
        image = rng.randint(6)                       # none (half), w_bf16x3, w_bf16x3s, both
        if image in (3, 5):
            d['w_bf16x3'] = ptr['w_bf16x3']
        if image in (4, 5):
            d['w_bf16x3s'] = ptr['w_bf16x3s']
        if pick(0.04):
            d['y'] += 4
        if d['res1'] and pick(0.04):
            d['res1'] += 4
        if conv_is_valid(d):
            rows.append([d[k] for k in names])

    always, never = (lambda p: True), (lambda p: False)
    draw = lambda p: rng.rand() < p
    # the grid: every channel pair and geometry at a few sizes, once with no optional operand at all and twice drawn
    for cin in CINS:
        for cout in COUTS:
            for g in GEOMETRIES if cin != 4 else ((7, 7, 2, 3, 0), (2, 2, 1, 0, 0), (3, 3, 1, 1, 0)):
                for pick in (never, draw, draw):
                    (h, w), n = MAPS[rng.randint(len(MAPS))], (1, 4, 16)[rng.randint(3)]
                    if g[0] == 7:
                        h, w = 8 * h, 8 * w           # the stem sees the image, not a feature map
                    add(n, h, w, cin, cout, *g, pick=pick)
    # every size for the launches the persistent kernels and their relays are priced on: plain 1x1 and 3x3 stride-2 convs
    for cin in (64, 128, 256, 512, 1024, 2048):
        for cout in (64, 128, 192, 256, 512, 1024, 2048):
            for (h, w) in MAPS:
                for n in (1, 4, 16):
                    add(n, h, w, cin, cout, 1, 1, 1, 0, 0, pick=never)
                    add(n, h, w, cin, cout, 1, 1, 1, 0, 0, pick=draw)
                    if cin <= 512:
                        add(n, h, w, cin, cout, 3, 3, 2, 1, 0, pick=draw)
    # the stem at image sizes, bare (the stem kernel's form) and with operands drawn
    for n in (1, 4, 16):
        for (h, w) in ((64, 96), (200, 336), (800, 1344)):
            add(n, h, w, 4, 64, 7, 7, 2, 3, 0, pick=never)
            add(n, h, w, 4, 64, 7, 7, 2, 3, 0, pick=draw)
    # thin outputs (the 64 -> 3 / 4 decoder convs) and Winograd-component launches (groups of 512 rows) for the emulation
    for cout in (3, 4):
        for (h, w) in MAPS:
            add(4, h, w, 64, cout, 2, 2, 1, 1, 0, pick=never)
            add(4, h, w, 128, cout, 1, 1, 1, 0, 0, pick=draw)
    return np.array(rows, np.int64)


def wgrad_sample(rng, names):
    ptr = dict((n, 0x100000 * (i + 1)) for i, n in enumerate(names))
    rows = []

    def add(n, h, w, cin, cin_real, cout, ldy, k, stride, pad, groups=0, splitk=0, pro=False, misalign=False):
        d = dict.fromkeys(names, 0)
        d.update(x=ptr['x'], dy=ptr['dy'] + (4 if misalign else 0), dw=ptr['dw'], slabs=ptr['slabs'], n=n, h=h, w_=w, cin=cin,
                 cin_real=cin_real, cout=cout, ldy=ldy, kh=k, kw=k, stride=stride, pad=pad, splitk=splitk, groups=groups)
        d['oh'], d['ow'] = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        if pro:
            d.update(pro_scale=ptr['pro_scale'], pro_shift=ptr['pro_shift'], pro_relu=1)
        if groups > 1:
            d.update(x_group_stride=n * h * w * cin, dy_group_stride=n * d['oh'] * d['ow'] * ldy, dw_group_stride=cout * k * k * cin_real)
        assert (cin == 4 or cin % 32 == 0) and 0 < cin_real <= cin and ldy >= cout and ldy % 4 == 0 and d['oh'] > 0 and d['ow'] > 0
        rows.append([d[k_] for k_ in names])

    for splitk in (0, 4, 16):
        for n in (1, 4, 16):
            for (h, w) in ((64, 96), (200, 336), (800, 1344)):
                for cin_real in (3, 4):                                    # the stem
                    add(n, h, w, 4, cin_real, 64, 64, 7, 2, 3, splitk=splitk, misalign=(n == 4 and h == 64))
            for (h, w) in ((25, 42), (100, 168), (200, 336)):
                for pad in (0, 1):                                         # the thin forms, tap problems, leftovers
                    add(n, h, w, 64, 64, 3, 4, 2, 1, pad, splitk=splitk)
                    add(n, h, w, 64, 64, 4, 4, 2, 1, pad, splitk=splitk)
                    add(n, h, w, 4, 3, 64, 64, 2, 1, pad, splitk=splitk)
                    add(n, h, w, 4, 4, 64, 64, 2, 1, pad, splitk=splitk)
                    for cin, cout in ((64, 256), (64, 128), (128, 128), (256, 256), (64, 64)):
                        add(n, h, w, cin, cin, cout, cout, 2, 1, pad, splitk=splitk, pro=(pad == 1 and cin == 64))
                add(n, h, w, 64, 64, 64, 64, 3, 1, 1, splitk=splitk)
                add(n, h, w, 256, 256, 128, 128, 3, 2, 1, splitk=splitk)
                add(n, h, w, 512, 512, 256, 256, 1, 2, 0, splitk=splitk)
                add(n, h, w, 32, 32, 64, 64, 1, 1, 0, splitk=splitk)
                add(n, h, w, 256, 256, 192, 192, 1, 1, 0, splitk=splitk)
            for groups in (0, 16, 36):                                     # grouped 1x1: the Winograd-domain reductions
                for cin, cout in ((64, 128), (64, 256), (64, 512), (128, 128), (128, 256), (256, 256), (512, 128), (64, 64),
                                  (96, 128)):
                    add(n, 30, 44, cin, cin, cout, cout if groups != 16 else cout + 64, 1, 1, 0, groups=groups, splitk=splitk,
                        pro=(cin == 512))
    return np.array(rows, np.int64)


def rec_grid():
    return np.array([(rows, k, cout, taps) for rows in (0, 1, 77, 1024, 1050, 4200, 16800, 67200)
                     for k in (64, 128, 192, 256, 512, 768, 1024, 2048, 4096) for cout in (3, 64, 128, 192, 256, 512, 1024, 2048)
                     for taps in (1, 4, 9)], np.int64)


# ---- recording

def child(inputs, setting, out):
    set_env(setting)
    _lib = _lib_module()
    t = np.load(inputs)
    np.savez(out, **evaluate(_lib.load(), _lib, t['conv'], t['wgrad'], t['rec']))


def main(source):
    assert os.environ.get('HND_LIB_PATH'), 'name the library to record with HND_LIB_PATH'
    _lib = _lib_module()
    rng = np.random.RandomState(20261018)
    conv, wgrad, rec = conv_sample(rng, field_names(_lib.ConvDesc)), wgrad_sample(rng, field_names(_lib.WgradDesc)), rec_grid()
    answers = {}
    with tempfile.TemporaryDirectory() as tmp:
        inputs = os.path.join(tmp, 'inputs.npz')
        np.savez(inputs, conv=conv, wgrad=wgrad, rec=rec)
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), '--child', inputs, s, os.path.join(tmp, '%d.npz' % i)])
                 for i, s in enumerate(SETTINGS)]
        assert all(p.wait() == 0 for p in procs)
        for i, s in enumerate(SETTINGS):
            answers[s] = dict(np.load(os.path.join(tmp, '%d.npz' % i)))
    keys = CONV_ANSWERS + WGRAD_ANSWERS + REC_ANSWERS
    table = {k: np.stack([answers[s][k] for s in SETTINGS]) for k in keys}
    # ---- what keeps the table from being vacuous
    base = answers['']
    counts = {c: int((base['conv_tile'] == c).sum()) for c in TILE_CODES}
    print('%d conv rows, %d wgrad rows, %d grid points, %d settings; tile codes under no setting: %s' %
          (len(conv), len(wgrad), len(rec), len(SETTINGS), counts))
    assert set(np.unique(table['conv_tile'])) <= set(TILE_CODES)
    assert min(counts.values()) >= 5, counts
    assert set(np.unique(base['conv_build'])) == {0, 1}
    ws = base['conv_workspace'] > 0
    assert (ws & np.isin(base['conv_tile'], (11, 12))).any() and (ws & np.isin(base['conv_tile'], (14, 15))).any()
    assert set(np.unique(base['wgrad_variant'])) == {0, 1, 2, 3}
    assert base['rec_bx3'].any() and base['rec_bxs'].any() and not base['rec_bx3'].all() and not base['rec_bxs'].all()
    for s in SETTINGS[1:]:
        changed = sum(int((answers[s][k] != base[k]).sum()) for k in keys)
        print('  %-40s changes %d answers' % (s, changed))
        assert (changed == 0) == (s in NO_OPS), s
    np.savez_compressed(TABLE, conv=conv, wgrad=wgrad, rec=rec, settings=np.array(SETTINGS), source=np.array(source),
                        conv_fields=np.array(field_names(_lib.ConvDesc)), wgrad_fields=np.array(field_names(_lib.WgradDesc)),
                        **{k: v.astype(np.int64) for k, v in table.items()})
    print('wrote %s (%d bytes)' % (TABLE, os.path.getsize(TABLE)))


if __name__ == '__main__':
    if sys.argv[1:2] == ['--child']:
        child(*sys.argv[2:5])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else 'unknown')
