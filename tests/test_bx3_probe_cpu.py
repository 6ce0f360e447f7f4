"""CPU: the exact plane-product probes of tests/bx3_probe_util.py are valid and see every single fault -- with the reference
alone, for every shape tests/test_bx3_probe_gpu.py launches.

  * Split: hi + mid + lo == x, at most 8 significant bits a plane, every class occupies exactly its planes, the three dropped
    pairs contribute exactly 0.0.
  * Exact in any order: all plane products of an output element are multiples of one unit and their magnitudes sum to less
    than 2^24 units (a proof for every order); and the fp32 accumulation of the single products in four orders gives the fp64
    result bit for bit.
  * Sensitivity: each of the 36 single faults (a kept pair dropped, taken twice, taken with the wrong B plane or the wrong A
    plane), planted in one k block, in the rows of one residue mod 3, or everywhere, changes at least one element of every k
    block it touches, somewhere in the probe set (cross layout at three phases + the mm launch).  Column j of a probe is zero
    outside k block j % nblocks (checked here), so a fault planted in ONE k block changes exactly the columns of that block
    that the fault planted everywhere changes: one table [fault, row scope, k block] answers all three placements."""
import functools
import random

import pytest
import torch

from tests import bx3_probe_util as U

GEMM_SHAPES = [('gemm', k, c, m) for k in U.GEMM_KS for c in U.GEMM_COUTS for m in U.GEMM_MS]
# (the data-gradient, rider and native 1x1 cases reuse operands of GEMM_SHAPES)
assert all(('gemm',) + c in GEMM_SHAPES for c in (U.DGRAD_CASE, U.RIDER_CASE, U.RES_UP_CASE))
assert all(('gemm', k, U.NATIVE_COUT, U.NATIVE_M) in GEMM_SHAPES for k in U.NATIVE_KS)
OTHER_SHAPES = ([('gemm_s2',) + U.STRIDE2_CASE] + [('tap', i) for i in range(len(U.TAP_CASES))]
                + [('relay',)] + [('bres', i) for i in range(len(U.BRES_CASES))])
SHAPES = GEMM_SHAPES + OTHER_SHAPES


@functools.lru_cache(maxsize=2)
def probes_of(shape):
    kind = shape[0]
    if kind in ('gemm', 'gemm_s2'):
        return U.gemm_probe_set(U.GEMM_MS[shape[3]], shape[1], shape[2], 2 if kind == 'gemm_s2' else 1)
    if kind == 'tap':
        return U.conv_probe_set(*U.TAP_CASES[shape[1]][1:])
    if kind == 'relay':
        _, n, cin, h, w, cout = U.RELAY_CASE
        return U.gemm_probe_set((n, h, w), cin, cout)
    _, kdim, cout, m_shape, _ = U.BRES_CASES[shape[1]]
    return U.gemm_probe_set(m_shape, kdim, cout)


def _id(shape):
    return '-'.join(str(v) for v in shape)


def test_split3_is_the_split_of_bf16x3_h():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4096, generator=g) * torch.exp2(torch.randn(4096, generator=g) * 6)
    x = torch.cat([x, torch.tensor([0.0, 1.0, -1.0, 1 + 2.0 ** -8 + 2.0 ** -16, 1 + 2.0 ** -18, 3.0 + 3 * 2.0 ** -9 + 3 * 2.0 ** -18])])
    hi, mid, lo = U.split3(x)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    for p in (hi, mid, lo):
        assert U.significant_bits(p) <= 8 and torch.equal(p.view(torch.int32) & 0xffff, torch.zeros_like(p, dtype=torch.int32))
    # truncation: hi and the remainders keep x's sign, |hi| <= |x|
    assert bool((hi.abs() <= x.abs()).all()) and bool((hi * x >= 0).all()) and bool((mid * x >= 0).all())
    one = U.split3(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -16, 1 + 2.0 ** -18]))
    assert [float(p[0]) for p in one] == [1.0, 2.0 ** -8, 2.0 ** -16]
    assert [float(p[1]) for p in one] == [1.0, 2.0 ** -18, 0.0]          # the remainder renormalises into MID


@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_probe_planes_are_where_the_classes_say(shape):
    for p in probes_of(shape):
        nb = p.nblocks
        for t in (p.A, p.B):
            planes = U.split3(t)
            assert torch.equal(sum(q.double() for q in planes), t.double())
            assert all(1 <= U.significant_bits(q) <= 3 or not bool(q.any()) for q in planes)
        # column j is zero outside k block j % nblocks, and has something in it
        kb = torch.arange(p.K)[:, None] // U.KSTEP
        own = kb == (torch.arange(p.N)[None, :] % nb)
        assert not bool((p.B != 0)[~own].any()) and bool((p.B != 0).any(0).all())
        # the class belongs to the GEMM row of a 1x1 probe and to the input pixel of a tap probe
        a_planes = U.split3(p.A if p.k == 1 else p.x.reshape(-1, p.x.shape[3]))
        b_planes = [q.t() for q in U.split3(p.B)]
        rows = torch.arange(a_planes[0].shape[0])
        for c in range(3):
            rsel = (torch.ones_like(rows) if p.layout == 'mm' else U.row_class(rows, p.phase)).eq(c)
            csel = torch.tensor([U.col_class(j, nb, p.phase, p.layout) == c for j in range(p.N)])
            for sel, planes in ((rsel, a_planes), (csel, b_planes)):
                if not bool(sel.any()):
                    # (64 columns at K = 1024: two B classes a launch, the third comes with the next phase)
                    assert (p.layout == 'mm' and c != 1) or (sel is csel and p.N < 3 * nb)
                    continue
                hi_, mid_, lo_ = (q[sel] for q in planes)
                assert bool(hi_.ne(0).any(-1).all())
                assert bool(mid_.ne(0).any(-1).eq(c >= 1).all()) and bool(lo_.ne(0).any(-1).eq(c >= 2).all())
        prod = U.plane_products(p.A, p.B)
        for pair in U.DROPPED:
            assert not bool(prod[pair].any()), (p.name(), pair)
        assert not bool(U.model_gemm(p.A, p.B, U.DROPPED, prod).any())
        if p.layout == 'cross':
            assert not bool(prod[(U.MID, U.MID)].any())
        else:
            assert bool(prod[(U.MID, U.MID)].any())


def _orders(nterms, npairs, seed):
    """term index = k position * npairs + pair (pairs in the kernels' order, smallest first)"""
    natural = list(range(nterms))
    shuffled = natural[:]
    random.Random(seed).shuffle(shuffled)
    by_pair = [t * npairs + q for q in range(npairs) for t in range(nterms // npairs)]
    return {'natural': natural, 'reversed': natural[::-1], 'shuffled': shuffled, 'pair by pair': by_pair}


KERNEL_ORDER = ((U.LO, U.HI), (U.HI, U.LO), (U.MID, U.MID), (U.MID, U.HI), (U.HI, U.MID), (U.HI, U.HI))


@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_probes_are_exact_in_any_order(shape):
    assert sorted(KERNEL_ORDER) == sorted(U.KEPT)
    for p in probes_of(shape):
        # (p.want is the plain fp64 matmul cast to fp32; the sum again without B's zero parts, and plane by plane)
        ref64 = U._matmul64(p.A.double(), p.B.double())
        assert torch.equal(p.want.double(), ref64), 'the fp64 result is no fp32 number'
        assert torch.equal(U.model_gemm(p.A[:BIG_M_ROWS], p.B, U.KEPT), ref64[:BIG_M_ROWS])
        # the proof: multiples of u whose magnitudes sum to s < 2^24 u.  (All nine pairs: the dropped ones are zero.)
        u, s = U.bit_budget(p.A, p.B)
        assert u >= 2.0 ** -18 and s < 2.0 ** 24 * u, (p.name(), u, s)
        # ... and four orders of fp32 accumulation, term by term.  Only the 32 k of the column's own block have non-zero
        # terms.  (More than 384 rows: the first and the last 192, the rows come from one generator.)
        rows = torch.arange(p.M) if p.M <= BIG_M_ROWS else torch.cat([torch.arange(192), torch.arange(p.M - 192, p.M)])
        pa, pb = [q[rows] for q in U.split3(p.A)], U.split3(p.B)
        orders = _orders(U.KSTEP * 6, 6, 7 + p.K)
        for b in range(p.nblocks):
            cols = torch.arange(b, p.N, p.nblocks)
            ks = slice(b * U.KSTEP, (b + 1) * U.KSTEP)
            terms = torch.stack([pa[i][:, None, ks] * pb[j][ks][:, cols].t()[None] for i, j in KERNEL_ORDER], 3)
            terms = terms.reshape(rows.numel(), cols.numel(), -1)                     # fp32 products, exact
            want = p.want[rows][:, cols]
            for name, order in orders.items():
                acc = torch.zeros_like(want)
                for t in order:
                    acc = acc + terms[:, :, t]
                assert torch.equal(acc, want), (p.name(), 'k block', b, name)


BIG_M_ROWS = 384
ROW_SCOPES = ('every row',) + tuple('rows = %d mod 3' % c for c in range(U.ROW_PERIOD))


def detection_table(probes):
    """bool [fault, row scope, k block]: some element of the k block's columns, in the scope's rows, differs from the expected
    output in some probe of the set"""
    muts = U.mutations()
    nb = probes[0].nblocks
    table = torch.zeros(len(muts), len(ROW_SCOPES), nb, dtype=torch.bool)
    for p in probes:
        # (the first 384 rows are enough: a fault seen in some rows of a scope is seen in the scope)
        A, want = p.A[:BIG_M_ROWS], p.want[:BIG_M_ROWS]
        prod = U.plane_products(A, p.B)
        blk = torch.arange(p.N) % nb
        for mi, (_, pairs) in enumerate(muts):
            diff = U.model_gemm(A, p.B, pairs, prod).float() != want
            for si in range(len(ROW_SCOPES)):
                d = (diff if si == 0 else diff[si - 1::U.ROW_PERIOD]).any(0)
                table[mi, si] |= torch.zeros(nb).index_add_(0, blk, d.float()) > 0
    return muts, table


@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_every_single_fault_is_seen_in_every_k_block_it_touches(shape):
    muts, table = detection_table(probes_of(shape))
    assert len(muts) == 6 * (1 + 1 + 2 + 2)
    missed = [(muts[m][0], ROW_SCOPES[s], 'k block %d' % b) for m, s, b in (~table).nonzero().tolist()]
    assert not missed, '%d of %d (fault, rows, k block) go unseen, e.g. %s' % (len(missed), table.numel(), missed[:5])


def test_a_probe_names_the_wrong_element():
    p = U.gemm_probe(U.GEMM_MS[240], 512, 64, 'cross', 1)
    assert p.first_wrong(p.want.clone()) is None
    y = p.want.clone()
    y[200, 37] += 2.0 ** -10
    msg = p.first_wrong(y)
    assert 'row 200' in msg and 'chunk 3, in the tail' in msg and 'k block 5' in msg and '256-k pass 0' in msg, msg
    y[3, 1] = float('nan')
    assert 'row 3' in p.first_wrong(y)
