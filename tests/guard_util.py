"""Guard-band arena: every buffer a launch touches is a view into ONE allocation, with owned guard bytes around it.

include/hnd_hip.h promises caller-owned buffers of stated sizes.  A test that hands a kernel separate torch.empty tensors
cannot see a store one row past an output (it lands in the caching allocator's slack or in another tensor) nor a load past
an input (the neighbour's bytes are benign).  Here the neighbours are guards filled with 0xFF:
  as fp32 it is a NaN -- an over-read that reaches a result poisons it;
  as int32 / int64 it is -1; as a mask byte every bit is set;
and any byte of a guard that is no longer 0xFF after the launch is an out-of-bounds write, reported by Arena.check().

A plain module: no fixtures, no pytest settings.  Works on any torch device (the self-test uses 'cpu').
"""
import math

import torch

FILL = 0xFF
ALIGN = 256                       # every view starts on a 256-byte boundary (what torch's allocator gives a tensor)
# Guard width G = max(MIN_GUARD, GUARD_ROWS * row pitch), from the code: 256 rows is the tallest block tile of any GEMM
# here (the 256 x 64 build of the B-streamed kernels), 256 KiB is two relay accumulator sets (2 * RELAY_SET * 4 bytes,
# csrc/stream_k_relay.h) -- a tail tile or a parked set that is off by one whole unit still lands in owned memory.
MIN_GUARD = 256 * 1024
GUARD_ROWS = 256


class GuardDamage(AssertionError):
    """raised by Arena.check(); .reports = [dict(name, side, first, last, count)]"""

    def __init__(self, reports):
        self.reports = reports
        AssertionError.__init__(self, 'guard bytes damaged: ' + '; '.join(
            '%(count)d byte(s) %(side)s view %(name)r, offsets %(first)d..%(last)d from its edge' % r for r in reports))


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def guard_bytes(shape, dtype, guard_rows=None):
    """G of a view: its row pitch is the extent of its last dimension (one NHWC pixel, one GEMM row); a flat buffer has
    rows of one element"""
    shape = tuple(shape) if not isinstance(shape, int) else (shape,)
    pitch = _itemsize(dtype) * (shape[-1] if len(shape) > 1 else 1)
    return max(MIN_GUARD, (GUARD_ROWS if guard_rows is None else guard_rows) * pitch)


def view_bytes(shape, dtype):
    shape = tuple(shape) if not isinstance(shape, int) else (shape,)
    return _itemsize(dtype) * int(math.prod(shape))


def arena_bytes(specs):
    """bytes an Arena needs for views of these (shape, dtype) pairs, in any order (an upper bound)"""
    total = ALIGN
    for shape, dtype in specs:
        total += 2 * guard_bytes(shape, dtype) + view_bytes(shape, dtype) + ALIGN
    return total


class Arena(object):
    def __init__(self, device, nbytes):
        self.base = torch.full((int(nbytes),), FILL, dtype=torch.uint8, device=device)
        self.views = []           # (name, start, end, guard): the view owns base[start:end]

    def take(self, name, shape, dtype=torch.float32, fill=None, guard_rows=None):
        """a contiguous view of `shape` / `dtype`: starts on a 256-byte boundary, ends exactly at its last byte (no rounding),
        at least G guard bytes on either side.  The interior starts as 0xFF (fp32 NaN) unless `fill` is given -- the
        workspaces the header wants zero-filled once (relay workspace, loss outputs) are taken with fill=0."""
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        assert name not in [v[0] for v in self.views], name
        nbytes, g = view_bytes(shape, dtype), guard_bytes(shape, dtype, guard_rows)
        assert nbytes > 0, (name, shape)
        if self.views:
            _, _, prev_end, prev_g = self.views[-1]
            lo = prev_end + max(prev_g, g)            # neighbours share one band, as wide as the wider of the two asks
        else:
            lo = g
        addr = self.base.data_ptr() + lo
        start = lo + (-addr) % ALIGN
        end = start + nbytes
        if end + g > self.base.numel():
            raise ValueError('arena of %d bytes is too small for view %r: needs %d' % (self.base.numel(), name, end + g))
        self.views.append((name, start, end, g))
        v = self.base[start:end].view(dtype).view(shape)
        assert v.is_contiguous() and v.data_ptr() % ALIGN == 0 and v.data_ptr() == self.base.data_ptr() + start
        if fill is not None:
            v.fill_(fill)
        return v

    def load(self, name, tensor, guard_rows=None):
        """take + copy, for inputs"""
        v = self.take(name, tuple(tensor.shape), tensor.dtype, guard_rows=guard_rows)
        v.copy_(tensor)
        return v

    def guard_of(self, name):
        return [v[3] for v in self.views if v[0] == name][0]

    def _gaps(self):
        edges = [0]
        for _, start, end, _ in self.views:
            edges += [start, end]
        edges.append(self.base.numel())
        return [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2) if edges[i + 1] > edges[i]]

    def check(self):
        """one device-side reduction over every byte no view owns; raises GuardDamage naming, per damaged band, the view,
        the side ('before' / 'after'), the offsets of the first and the last damaged byte from the view's edge (0 = the
        byte that touches the view) and how many bytes are damaged"""
        gaps = self._gaps()
        counts = torch.stack([(self.base[lo:hi] != FILL).sum() for lo, hi in gaps]).cpu().tolist()
        if not any(counts):
            return
        reports = []

        def report(name, side, offsets):
            if offsets.numel():
                reports.append(dict(name=name, side=side, first=int(offsets.min()), last=int(offsets.max()),
                                    count=int(offsets.numel())))
        for (lo, hi), cnt in zip(gaps, counts):
            if not cnt:
                continue
            idx = torch.nonzero(self.base[lo:hi] != FILL).flatten() + lo
            # a gap lies after the view that ends at `lo` and before the view that starts at `hi`; the nearer edge owns
            # the byte (a shared band is split where the two distances meet, the tie going to the view before it)
            prev = [v for v in self.views if v[2] == lo]
            nxt = [v for v in self.views if v[1] == hi]
            if not prev and not nxt:
                report('<empty arena>', 'after', idx)
                continue
            after = idx - lo <= hi - 1 - idx if (prev and nxt) else torch.full_like(idx, bool(prev), dtype=torch.bool)
            if prev:
                report(prev[0][0], 'after', (idx - lo)[after])
            if nxt:
                report(nxt[0][0], 'before', (hi - 1 - idx)[~after])
        order = {v[0]: k for k, v in enumerate(self.views)}
        reports.sort(key=lambda r: (order.get(r['name'], -1), r['side']))
        raise GuardDamage(reports)
