"""Shared by the tests of the fixed quantisation range (include/hnd_qrange.h; tests/test_qrange_cpu.py,
tests/test_qrange_gpu.py, tests/test_guard_bands_qrange_gpu.py): the header's arithmetic restated in numpy fp32, one correctly
rounded operation per step; the CLIPPED straight-through estimator for the oracle; and the literal ranges of the one-step
comparison with the preconditions they were chosen to meet.

A plain module: no fixtures, no pytest settings; importing it loads neither the library nor the launch helpers."""
import numpy as np
import torch

from tests import qat_util as QU

F = np.float32
ROWS = 128                      # HND_FAKE_QUANT_TILE_ROWS

# (fixture, width, lo, hi) of the one-step comparison with a frozen literal range.  Chosen on the CPU from the fp32 / fp64
# oracle alone (tests/test_qrange_cpu.py holds them to it): both oracles take the same code and the same pass decision for
# every element, no u = zero_point + z / scale lies within qat_util.MARGIN of a half-integer (the pass boundaries -0.5 and
# qmax + 0.5 are half-integers), at least 1 % of the elements are clipped at each end and at least half pass.
# Achieved (fp32 / fp64 oracle), printed by the CPU test:
#   tiny_ghnd_faster    2 bits [-9.4, 10.34]:  nearest half-integer 6.76e-04 / 6.76e-04 code units; clipped below 6.92 %, above
#                                             1.16 %, passing 91.92 %; -lo / scale = 1.43 (zero point 1)
#   tiny_ghnd_faster_b6 4 bits [-8.29, 6.17]:  nearest half-integer 8.89e-04 / 8.95e-04 code units; clipped below 3.24 %, above
#                                             4.97 %, passing 91.79 %; -lo / scale = 8.60 (zero point 8)
ONE_STEP_RANGE_CASES = [('tiny_ghnd_faster', 2, -9.4, 10.34), ('tiny_ghnd_faster_b6', 4, -8.29, 6.17)]


# ------------------------------------------------------------------------------------------ numpy fp32 restatement
def qparams_np(lo, hi, bits):
    """{lo, hi, scale, zero_point} of a range, fp32, the header's formula"""
    qmax = F(2 ** bits - 1)
    lo, hi = F(lo), F(hi)
    with np.errstate(all='ignore'):
        scale = F(F(hi - lo) / qmax)
        zp = F(F(0) - F(lo / scale))
    zp = F(0) if zp < 0 else (qmax if zp > qmax else zp)
    return np.array([lo, hi, scale, np.trunc(zp)], dtype=F)


def observe_np(state, x, c, momentum, bits):
    """hnd_qrange_observe on the host: (new state, qparams); x is [npix, cs]"""
    real = x[:, :c]
    lo, hi = F(real.min()), F(real.max())
    rmin, rmax, steps = F(state[0]), F(state[1]), F(state[2])
    m = F(momentum)
    if steps == 0:
        rmin, rmax = lo, hi
    else:
        rmin = F(rmin + F(m * F(lo - rmin)))
        rmax = F(rmax + F(m * F(hi - rmax)))
    new = np.array([rmin, rmax, F(steps + F(1)), 0], dtype=F)
    return new, qparams_np(rmin, rmax, bits)


def fake_quantize_range_np(x, c, bits, qp):
    """hnd_fake_quantize_range on the host: x [npix, cs] fp32 -> (y [npix, cs] fp32, mask [npix, cs // 4] uint8, u [npix, c])"""
    npix, cs = x.shape
    qmax, scale, zp = F(2 ** bits - 1), F(qp[2]), F(qp[3])
    with np.errstate(all='ignore'):
        u = (zp + (x[:, :c] / scale).astype(F)).astype(F)
        r = np.rint(u)
        passed = (r >= 0) & (r <= qmax)                                   # False for a NaN
        cl = np.where(u < 0, F(0), np.where(u > qmax, qmax, u)).astype(F)   # the kernel's clamp: -0 and NaN go through
        code = np.rint(cl).astype(F)
        y = np.zeros((npix, cs), dtype=F)
        y[:, :c] = (scale * (code - zp).astype(F)).astype(F)
    bits_ = np.zeros((npix, cs), dtype=np.uint8)
    bits_[:, :c] = passed
    mask = np.zeros((npix, cs // 4), dtype=np.uint8)
    for k in range(4):
        mask |= (bits_[:, k::4] << k).astype(np.uint8)
    return y, mask, u


def quantize_range_np(x, c, bits, qp):
    """the codes hnd_quantize_range_bits stores: [npix, cs] uint8, pad channels 0 (no NaN in x)"""
    npix, cs = x.shape
    qmax, scale, zp = F(2 ** bits - 1), F(qp[2]), F(qp[3])
    u = (zp + (x[:, :c] / scale).astype(F)).astype(F)
    q = np.zeros((npix, cs), dtype=np.uint8)
    q[:, :c] = np.rint(np.clip(u, F(0), qmax)).astype(np.uint8)
    return q


def mask_bits(mask, c):
    """[npix, cs // 4] uint8 mask -> [npix, c] bool"""
    m = np.asarray(mask)
    out = np.stack([(m >> k) & 1 for k in range(4)], axis=-1).reshape(m.shape[0], -1)
    return out[:, :c].astype(bool)


# ------------------------------------------------------------------------------------------ the oracle's estimator
def range_decisions(z, bits, lo, hi):
    """the quantiser's decisions on z (a torch tensor, fp32 or fp64) for the literal range, in z's dtype:
    dict(u, codes, passed, scale, zero_point, dequantised)"""
    qmax = float(2 ** bits - 1)
    lo_t, hi_t = (torch.tensor(float(np.float32(v)), dtype=z.dtype) for v in (lo, hi))
    scale = (hi_t - lo_t) / qmax
    zp = torch.trunc(torch.clamp(0.0 - lo_t / scale, 0.0, qmax))
    u = zp + z / scale
    r = torch.round(u)
    passed = (r >= 0) & (r <= qmax)
    codes = torch.round(torch.clamp(u, 0.0, qmax))
    return {'u': u.double(), 'codes': codes, 'passed': passed, 'scale': float(scale), 'zero_point': int(zp),
            'dequantised': scale * (codes - zp), 'dtype': z.dtype}


def clipped_ste(bits, lo, hi, capture=None):
    """fake_quant for qat_util.make_student_layer1: forward = quantise -> dequantise on the literal range; backward = the
    identity where the value passed, zero where it was clipped.  capture: dict that receives range_decisions() of the
    unquantised bottleneck tensor under the dtype of the run."""
    def fq(z):
        d = range_decisions(z.detach(), bits, lo, hi)
        if capture is not None:
            capture[z.dtype] = dict(d, z=z.detach().clone())
        fqz = d['dequantised']
        return torch.where(d['passed'], z + (fqz - z).detach(), fqz.detach())
    return fq


def range_margins(cap, bits):
    """(distance of the nearest u from a half-integer, share clipped below, share clipped above, share passing)"""
    u = cap['u']
    half = float(((u - torch.floor(u)) - 0.5).abs().min())
    qmax = 2 ** bits - 1
    n = float(u.numel())
    below = float((torch.round(u) < 0).sum()) / n
    above = float((torch.round(u) > qmax).sum()) / n
    return half, below, above, float(cap['passed'].sum()) / n


def check_range_preconditions(cap32, cap64, bits, what=''):
    """the issue's preconditions on the oracle pair; returns (margins fp32, margins fp64)"""
    assert cap32['codes'].shape == cap64['codes'].shape
    differ = int((cap32['codes'].double() != cap64['codes'].double()).sum())
    assert differ == 0, '%s: %d codes differ between the fp32 and the fp64 oracle' % (what, differ)
    differ = int((cap32['passed'] != cap64['passed']).sum())
    assert differ == 0, '%s: %d pass decisions differ between the fp32 and the fp64 oracle' % (what, differ)
    assert cap32['zero_point'] == cap64['zero_point'], (what, cap32['zero_point'], cap64['zero_point'])
    out = []
    for cap in (cap32, cap64):
        half, below, above, passing = range_margins(cap, bits)
        assert half >= QU.MARGIN, '%s (%s): a value lies %.3e from a half-integer' % (what, cap['dtype'], half)
        assert below >= 0.01 and above >= 0.01, '%s (%s): clipped %.4f below, %.4f above' % (what, cap['dtype'], below, above)
        assert passing >= 0.5, '%s (%s): only %.4f pass' % (what, cap['dtype'], passing)
        out.append((half, below, above, passing))
    return out
