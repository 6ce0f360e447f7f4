"""GPU: the fixed quantisation range of the bottleneck (include/hnd_qrange.h and the layers above it).

 (1) hnd_fake_quantize_range against the numpy fp32 restatement of the header (tests/qrange_util.py): y bit for bit, the
     clip mask byte for byte, in place and out of place, garbage in the pad channels of the source, values beyond both
     ends, exact ties and the two pass boundaries; its BatchNorm partial sums against the fp64 sums of what it stored;
 (2) anchored to the merged code: on the qparams hnd_fake_quantize_bits made it returns that call's bits with every mask
     bit set, and the one-launch codec exports return the bytes / payload of hnd_quantize_bits / hnd_quantize_pack_bits;
 (3) hnd_qrange_observe over three batches and hnd_qrange_qparams against the numpy sequence, bit for bit;
 (4) hnd_qrange_mask_grad;
 (5) the host classes, and 'trained' resolved from a checkpoint the runner wrote;
 (6) one distillation step on a frozen literal range against the fp64 / fp32 oracle with the CLIPPED straight-through
     estimator, every code and every mask bit included;
 (7) plan isolation: with the range off, the launches and the loss bits of a student that never heard of it."""
import numpy as np
import pytest
import torch

from oracle import hnd_oracle as O
from tests import golden_util as G
from tests import model_util as MU
from tests import qat_util as QU
from tests import qrange_util as R
from tests import test_model_gpu as TM

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROWS = R.ROWS
PAD_GARBAGE = 1.0e6

# (c, cs, npix): one pixel; one row short of a tile, a tile, a tile and a row; 36 tiles, the last of 71 rows (3 * 37 * 41);
# 3 real channels of 4, 5 of 8 (a pad-only tail in the second group), 12 of 12 (no padding); 65 groups = one more than the
# 64 a wave covers in a pass, 258 of 260 real, over two tiles
SHAPES = [(c, cs, npix) for c, cs in ((3, 4), (5, 8), (12, 12)) for npix in (1, 127, 128, 129, 3 * 37 * 41)] + [(258, 260, 130)]
WIDTHS = [1, 2, 4, 8]


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


@pytest.fixture(scope='module', autouse=True)
def leave_nothing_behind():
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def literal_range(bits, exact):
    """exact: scale = 0.5 and an integral zero point, so that ties and the pass boundaries are exact fp32 inputs"""
    qmax = 2 ** bits - 1
    return (-1.0, -1.0 + 0.5 * qmax) if exact else (-0.73, 1.91)


_INPUTS = {}


def make_input(c, cs, npix, bits, exact):
    """host [npix, cs] buffer: normal values scaled so that a good share lies beyond both ends of literal_range, with -- as
    far as the buffer has room -- exact ties u = k + 0.5, u = -0.5, u = qmax + 0.5, the two ends themselves, 0 and values
    far outside planted at fixed positions; garbage in the pad channels"""
    key = (c, cs, npix, bits, exact)
    if key not in _INPUTS:
        lo, hi = literal_range(bits, exact)
        qp = R.qparams_np(lo, hi, bits)
        scale, zp, qmax = float(qp[2]), float(qp[3]), 2 ** bits - 1
        g = torch.Generator().manual_seed(11 * c + npix + bits)
        x = (torch.randn(npix, c, generator=g) * (hi - lo) * 0.6 + 0.5 * (lo + hi)).numpy().astype(np.float32)
        special = [(-0.5 - zp) * scale, (qmax + 0.5 - zp) * scale, lo, hi, 0.0, lo - 100.0, hi + 100.0]
        special += [(k + 0.5 - zp) * scale for k in range(min(qmax, 6))]
        special += [np.nextafter(np.float32(s), np.float32(np.inf)) for s in special[:2]]
        special += [np.nextafter(np.float32(s), np.float32(-np.inf)) for s in special[:2]]
        flat = x.reshape(-1)
        for i, s in enumerate(special[:flat.size]):                      # evenly spread; the first ones when room is short
            flat[i * flat.size // len(special) if flat.size >= len(special) else i] = np.float32(s)
        buf = np.full((npix, cs), PAD_GARBAGE, dtype=np.float32)
        buf[:, :c] = x
        _INPUTS[key] = buf
    return _INPUTS[key]


def bits_of(t):
    t = t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------ (1) the numpy restatement
@pytest.mark.parametrize('bits', WIDTHS)
@pytest.mark.parametrize('c,cs,npix', SHAPES)
def test_fake_quantize_range_is_the_header_arithmetic_bit_for_bit(ops, c, cs, npix, bits):
    for exact in (True, False):
        src = make_input(c, cs, npix, bits, exact)
        lo, hi = literal_range(bits, exact)
        qp_ref = R.qparams_np(lo, hi, bits)
        y_ref, mask_ref, u = R.fake_quantize_range_np(src, c, bits, qp_ref)
        if exact and npix * c >= 20:                                      # the planted boundaries are really there
            assert (u == -0.5).any() and (u == 2 ** bits - 0.5).any() and (np.rint(u) < 0).any() and (np.rint(u) > 2 ** bits - 1).any()
        qp = torch.full((4,), float('nan'), device=DEV)
        ops.qrange_qparams(lo, hi, bits, qp)
        x = dev(src).view(1, 1, npix, cs)
        nt = ops.fake_quantize_tiles(npix)
        # out of place, with the mask, no statistics
        out = torch.full_like(x, float('nan'))
        mask = torch.full(ops.qrange_mask_shape(x), 0xFF, dtype=torch.uint8, device=DEV)
        assert ops.fake_quantize_range(x, c, bits, qp, out=out, mask=mask) is out
        ops.sync_check()
        assert torch.equal(bits_of(qp), bits_of(qp_ref))
        assert torch.equal(bits_of(x.view(npix, cs)), bits_of(src))                      # the source is read only
        assert torch.equal(bits_of(out.view(npix, cs)), bits_of(y_ref))
        assert np.array_equal(mask.view(npix, cs // 4).cpu().numpy(), mask_ref)
        # in place, with statistics, without the mask
        y = x.clone()
        stats = torch.full((nt, 2, cs), float('nan'), device=DEV)
        assert ops.fake_quantize_range(y, c, bits, qp, stats=stats) is y
        ops.sync_check()
        assert torch.equal(bits_of(y.view(npix, cs)), bits_of(y_ref))
        # in place with both; the statistics against fp64 sums of the stored values (the bound of
        # tests/test_fake_quant_gpu.py::test_partial_sums_are_those_of_the_stored_values)
        y2 = x.clone()
        mask2 = torch.full_like(mask, 0xFF)
        stats2 = torch.full((nt, 2, cs), float('nan'), device=DEV)
        ops.fake_quantize_range(y2, c, bits, qp, mask=mask2, stats=stats2)
        ops.sync_check()
        assert torch.equal(bits_of(y2.view(npix, cs)), bits_of(y_ref)) and torch.equal(mask2, mask)
        assert torch.equal(bits_of(stats2), bits_of(stats)) and not bool(torch.isnan(stats).any())
        stored = torch.from_numpy(y_ref).double()
        got = stats.cpu().double()
        for t in range(nt):
            blk = stored[t * ROWS:(t + 1) * ROWS]
            for k, vals in enumerate((blk, blk * blk)):
                err = (got[t, k] - vals.sum(0)).abs()
                assert bool((err <= ROWS * 2.0 ** -24 * vals.abs().sum(0)).all()), (t, k)
        if cs != c:
            assert float(stats[:, :, c:].abs().max()) == 0.0 and float(y[..., c:].abs().max()) == 0.0


def test_a_nan_stays_a_nan_and_does_not_pass(ops):
    c, cs, npix, bits = 5, 8, 129, 4
    src = make_input(c, cs, npix, bits, True).copy()
    src[7, 2] = src[128, 4] = np.nan
    lo, hi = literal_range(bits, True)
    y_ref, mask_ref, _ = R.fake_quantize_range_np(src, c, bits, R.qparams_np(lo, hi, bits))
    qp = torch.empty(4, device=DEV)
    ops.qrange_qparams(lo, hi, bits, qp)
    x = dev(src).view(1, 1, npix, cs)
    mask = torch.empty(ops.qrange_mask_shape(x), dtype=torch.uint8, device=DEV)
    ops.fake_quantize_range(x, c, bits, qp, mask=mask)
    ops.sync_check()
    got = x.view(npix, cs).cpu().numpy()
    assert np.isnan(got[7, 2]) and np.isnan(got[128, 4]) and int(np.isnan(got).sum()) == 2
    assert np.array_equal(np.isnan(got), np.isnan(y_ref)) and np.array_equal(mask.view(npix, -1).cpu().numpy(), mask_ref)
    assert not R.mask_bits(mask_ref, c)[7, 2] and not R.mask_bits(mask_ref, c)[128, 4]


# ------------------------------------------------------------------------------------------ (2) anchors to merged code
ANCHOR_SHAPES = [(3, 4, (2, 5, 7)), (6, 8, (3, 37, 41)), (12, 12, (1, 9, 15))]


def anchor_input(c, cs, nhw):
    """values whose batch range quantises without clipping: min and max are planted so that -min / scale is an integer at
    every width in use ((max - min) = 255 * 2^-5, min = -85 * 2^-5: the zero point is 85 * qmax / 255, integral for qmax in
    {1 (85 -> clamped), 3, 15, 255}), which the test asserts on the numpy restatement before it asks the kernel"""
    n, h, w = nhw
    npix = n * h * w
    g = torch.Generator().manual_seed(5 * c + npix)
    lo, hi = -85.0 / 32.0, 170.0 / 32.0
    x = (torch.rand(npix, c, generator=g) * (hi - lo) * 0.98 + lo + 0.01 * (hi - lo)).numpy().astype(np.float32)
    x[0, 0], x[npix - 1, c - 1] = lo, hi
    buf = np.full((npix, cs), PAD_GARBAGE, dtype=np.float32)
    buf[:, :c] = x
    return buf.reshape(n, h, w, cs)


@pytest.mark.parametrize('bits', [2, 4, 8])
@pytest.mark.parametrize('c,cs,nhw', ANCHOR_SHAPES)
def test_on_the_batch_qparams_it_is_the_merged_fake_quantiser_and_the_merged_codec(ops, c, cs, nhw, bits):
    src = anchor_input(c, cs, nhw)
    npix = src.size // cs
    flat = src.reshape(npix, cs)
    # precondition, on the numpy restatement alone: with the batch's own range nothing is clipped
    qp_np = R.qparams_np(flat[:, :c].min(), flat[:, :c].max(), bits)
    _, mask_np, _ = R.fake_quantize_range_np(flat, c, bits, qp_np)
    assert R.mask_bits(mask_np, c).all()
    x = dev(src)
    scratch = torch.empty(ops.minmax_scratch_elems(), device=DEV)
    qp = torch.empty(4, device=DEV)
    ref = torch.empty_like(x)
    ops.fake_quantize_bits(x, c, bits, qp, scratch, out=ref)
    out = torch.full_like(x, float('nan'))
    mask = torch.zeros(ops.qrange_mask_shape(x), dtype=torch.uint8, device=DEV)
    ops.fake_quantize_range(x, c, bits, qp, out=out, mask=mask)
    ops.sync_check()
    assert torch.equal(bits_of(qp), bits_of(qp_np))
    assert torch.equal(bits_of(out), bits_of(ref))
    assert np.array_equal(mask.view(npix, -1).cpu().numpy(), mask_np) and R.mask_bits(mask.view(npix, -1).cpu().numpy(), c).all()
    # the one-launch codec: the bytes of quantize_bits and the payload of quantize_pack_bits, qparams untouched
    q_ref = torch.empty(x.shape, dtype=torch.uint8, device=DEV)
    qp2 = torch.empty(4, device=DEV)
    ops.quantize_bits(x, c, bits, q_ref, qp2, scratch)
    q = torch.full(x.shape, 0xFF, dtype=torch.uint8, device=DEV)
    ops.quantize_range_bits(x, c, bits, q, qp)
    n, h, w = nhw
    nbytes = ops.codec_packed_bytes(n * c * h * w, bits)
    p_ref = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ops.quantize_pack_bits(x, c, bits, p_ref, qp2, scratch)
    payload = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    ops.quantize_pack_range_bits(x, c, bits, payload, qp)
    ops.sync_check()
    assert torch.equal(q, q_ref) and torch.equal(payload, p_ref) and torch.equal(bits_of(qp), bits_of(qp2))
    assert np.array_equal(q.view(npix, cs).cpu().numpy(), R.quantize_range_np(flat, c, bits, qp_np))
    # ... and they invert as they are: unpack_dequantize / dequantize_u8 give the fake quantiser's tensor
    back = torch.full_like(x, float('nan'))
    ops.unpack_dequantize_bits(payload, qp, back, c, bits)
    back2 = torch.full_like(x, float('nan'))
    ops.dequantize_u8(q, qp, back2, c)
    ops.sync_check()
    assert torch.equal(bits_of(back), bits_of(ref)) and torch.equal(bits_of(back2), bits_of(ref))


@pytest.mark.parametrize('bits', [1, 3])
def test_one_launch_codec_clips_to_a_literal_range(ops, bits):
    c, cs, npix = 5, 8, 3 * 37 * 41
    src = make_input(c, cs, npix, bits, False)
    lo, hi = literal_range(bits, False)
    qp = torch.empty(4, device=DEV)
    ops.qrange_qparams(lo, hi, bits, qp)
    x = dev(src).view(3, 37, 41, cs)
    q = torch.full(x.shape, 0xFF, dtype=torch.uint8, device=DEV)
    ops.quantize_range_bits(x, c, bits, q, qp)
    ops.sync_check()
    ref = R.quantize_range_np(src, c, bits, R.qparams_np(lo, hi, bits))
    assert np.array_equal(q.view(npix, cs).cpu().numpy(), ref) and (ref[:, :c] == 0).any() and (ref[:, :c] == 2 ** bits - 1).any()


# ------------------------------------------------------------------------------------------ (3) the observer
@pytest.mark.parametrize('c,cs,npix,bits,momentum', [(3, 4, 129, 2, 0.01), (5, 8, 3 * 37 * 41, 4, 0.3), (258, 260, 130, 8, 1.0)])
def test_observer_follows_the_numpy_sequence_bit_for_bit(ops, c, cs, npix, bits, momentum):
    g = torch.Generator().manual_seed(npix + c)
    state = torch.zeros(4, device=DEV)
    state_np = np.zeros(4, dtype=np.float32)
    qp = torch.full((4,), float('nan'), device=DEV)
    scratch = torch.empty(ops.minmax_scratch_elems(), device=DEV)
    for step, (gain, shift) in enumerate(((1.0, 0.0), (2.5, 0.7), (0.4, -1.3))):
        src = np.full((npix, cs), PAD_GARBAGE, dtype=np.float32)
        src[:, :c] = (torch.randn(npix, c, generator=g) * gain + shift).numpy()
        src[:, c:] *= -1.0 if step == 1 else 1.0                          # (pad channels: never counted, either sign)
        x = dev(src).view(1, 1, npix, cs)
        ops.qrange_observe(x, c, bits, momentum, state, qp, scratch)
        ops.sync_check()
        state_np, qp_np = R.observe_np(state_np, src, c, momentum, bits)
        assert torch.equal(bits_of(state), bits_of(state_np)), (step, state.cpu(), state_np)
        assert torch.equal(bits_of(qp), bits_of(qp_np)), (step, qp.cpu(), qp_np)
        assert torch.equal(bits_of(x.view(npix, cs)), bits_of(src))                      # read only
        if step == 0:                                                     # the first call initialises
            assert state_np[0] == src[:, :c].min() and state_np[1] == src[:, :c].max() and state_np[2] == 1.0
    assert state_np[2] == 3.0 and state_np[3] == 0.0


@pytest.mark.parametrize('bits', WIDTHS)
def test_qparams_of_a_literal_range_are_the_numpy_ones(ops, bits):
    for lo, hi in ((-1.0, 2.0), (-0.73, 1.91), (0.25, 7.0), (-9.0, -1.0), (-9.4, 10.34), (-8.29, 6.17)):
        qp = torch.full((4,), float('nan'), device=DEV)
        ops.qrange_qparams(lo, hi, bits, qp)
        ops.sync_check()
        assert torch.equal(bits_of(qp), bits_of(R.qparams_np(lo, hi, bits))), (lo, hi, qp.cpu())


# ------------------------------------------------------------------------------------------ (4) the mask's backward
@pytest.mark.parametrize('c,cs,npix', SHAPES)
def test_mask_grad_zeroes_the_clipped_and_keeps_every_other_bit(ops, c, cs, npix):
    g = torch.Generator().manual_seed(3 * c + npix)
    grad = torch.randn(npix, cs, generator=g)
    grad[0, 0] = -0.0
    grad[:, c:] = -PAD_GARBAGE                                            # pads keep their bits, whatever the mask says
    mask = torch.randint(0, 256, (npix, cs // 4), generator=g, dtype=torch.uint8)      # (high nibbles and pad bits set too)
    keep = torch.from_numpy(R.mask_bits(mask.numpy(), c))
    want = grad.clone()
    want[:, :c] = torch.where(keep, grad[:, :c], torch.zeros(()))
    gd = grad.to(DEV).view(1, 1, npix, cs)
    assert ops.qrange_mask_grad(gd, mask.to(DEV), c) is gd
    ops.sync_check()
    assert torch.equal(bits_of(gd.view(npix, cs)), bits_of(want))
    assert int((~keep).sum()) > 0 or npix == 1
    assert int((bits_of(gd.view(npix, cs))[:, :c][~keep] != 0).sum()) == 0          # +0, not -0


# ------------------------------------------------------------------------------------------ (5) host classes
def _attached(buf, c):
    from hnd_ghnd_object_detectors_amd.hipnn import attach
    return attach(buf[..., :c].permute(0, 3, 1, 2), buf)


@pytest.mark.parametrize('packed', [False, True])
@pytest.mark.parametrize('bits', [1, 4, 8])
def test_static_quantizer_dequantizer_pair_is_the_static_fake_quantizer(ops, bits, packed, monkeypatch):
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    c, cs, nhw = 6, 8, (3, 37, 41)
    lo, hi = literal_range(bits, False)
    src = make_input(5, cs, nhw[0] * nhw[1] * nhw[2], bits, False).copy()
    src[:, 5] = src[:, 0] * 0.5
    src[:, c:] = 0.0                                                      # a HIP-path tensor: pad channels are 0
    src = src.reshape(nhw + (cs,))
    buf_a, buf_b = dev(src), dev(src)
    fq = T.FakeQuantizer(bits, static_range=[lo, hi])
    quant = T.Quantizer(bits, packed=packed, static_range=[lo, hi])
    calls = []
    for name in ('qrange_qparams', 'fake_quantize_range', 'quantize_range_bits', 'quantize_pack_range_bits',
                 'fake_quantize_bits', 'quantize_bits', 'quantize_u8', 'quantize_pack_bits'):
        def spy(*a, _f=getattr(ops, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        monkeypatch.setattr(T.ops, name, spy)
    for _ in range(2):                                                    # the second call makes no qparams launch
        out_a, tgt = fq(_attached(buf_a, c), 'target')
        qz, _ = quant(_attached(buf_b, c), None)
        out_b, _ = T.Dequantizer(bits)(qz, None)
    quant.set_static_range(lo, hi + 1.0)                                  # rebinding: one more qparams launch
    quant(_attached(dev(src), c), None)
    ops.sync_check()
    one = 'quantize_pack_range_bits' if packed else 'quantize_range_bits'
    assert calls == ['qrange_qparams', 'fake_quantize_range', 'qrange_qparams', one, 'fake_quantize_range', one,
                     'qrange_qparams', one], calls
    assert tgt == 'target' and out_a._hnd is buf_a and isinstance(qz, T.PackedBottleneck if packed else T.QuantizedTensor)
    assert torch.equal(bits_of(out_a), bits_of(out_b)) and torch.equal(bits_of(buf_a), bits_of(buf_b))
    assert torch.equal(bits_of(fq.qparams), bits_of(R.qparams_np(lo, hi, bits)))
    y_ref, _, _ = R.fake_quantize_range_np(src.reshape(-1, cs), c, bits, R.qparams_np(lo, hi, bits))
    # (applied twice: the second pass quantises already-quantised values, which are fixed points of the quantiser)
    y_ref2, _, _ = R.fake_quantize_range_np(y_ref, c, bits, R.qparams_np(lo, hi, bits))
    assert torch.equal(bits_of(buf_a.view(-1, cs)), bits_of(y_ref2))


def test_trained_range_resolves_from_a_checkpoint_the_runner_wrote(ops, tmp_path, capsys):
    import json
    import os
    from hnd_ghnd_object_detectors_amd import mimic_runner
    from hnd_ghnd_object_detectors_amd.models import get_model, load_ckpt
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg_path = os.path.join(root, 'config', 'ghnd', 'faster_rcnn-backbone_resnet50-b3ch.yaml')
    ckpt = str(tmp_path / 'student.pt')
    tiny = {'pretrained': False, 'min_size': 64, 'max_size': 128}
    override = {'teacher_model': {'backbone': {'params': {'pretrained': False}}, 'params': tiny, 'ckpt': str(tmp_path / 'none.pt')},
                'student_model': {'backbone': {'params': {'pretrained': False}}, 'params': tiny, 'ckpt': ckpt},
                'train': {'batch_size': 2, 'log_freq': 1,
                          'fake_quantize': {'num_bits': 3, 'range': {'type': 'ema', 'momentum': 0.25}}}}
    argv = ['--config', cfg_path, '--json', json.dumps(override), '-distill', '--synthetic_batches', '2',
            '--image_size', '64x96', '--num_epochs', '1', '--loader_workers', '0', '-no_prefetch']
    mimic_runner.main(mimic_runner.get_argparser().parse_args(argv))
    assert 'Updating ckpt' in capsys.readouterr().out
    saved = torch.load(ckpt, weights_only=False)
    info = saved['bottleneck_range']
    assert sorted(info) == ['max', 'min', 'momentum', 'num_bits', 'steps'] and all(type(v) in (float, int) for v in info.values())
    assert info['steps'] == 2.0 and info['num_bits'] == 3 and info['momentum'] == 0.25 and info['min'] < info['max']
    assert 'backbone.body.layer1.qrange_state' not in saved['model']     # the checkpoint's state dict did not change
    assert saved['config']['train']['fake_quantize'] == override['train']['fake_quantize']
    student = get_model(saved['config']['student_model'], torch.device(DEV))
    layer1 = student.backbone.body.layer1
    quant, fake = T.Quantizer(3, static_range='trained'), T.FakeQuantizer(3, static_range='trained')
    layer1.bottleneck_transformer = T.Compose([quant, T.Dequantizer(3)])
    with pytest.raises(RuntimeError, match="Quantizer.*'trained'.*before its range was resolved"):
        quant(torch.zeros(1, 3, 2, 2, device=DEV), None)
    load_ckpt(ckpt, model=student)
    assert quant.static_range == (info['min'], info['max'])
    layer1.bottleneck_transformer = fake
    load_ckpt(ckpt, model=student)
    assert fake.static_range == (info['min'], info['max'])
    z = torch.linspace(info['min'] - 1.0, info['max'] + 1.0, 3 * 4 * 5, device=DEV).view(1, 3, 4, 5)
    out, _ = fake(z.clone(), None)
    ops.sync_check()
    flat = z.permute(0, 2, 3, 1).reshape(-1, 3).cpu().numpy()
    want, _, _ = R.fake_quantize_range_np(np.concatenate([flat, np.zeros((flat.shape[0], 1), dtype=np.float32)], 1), 3, 3,
                                          R.qparams_np(info['min'], info['max'], 3))
    assert torch.equal(bits_of(out.permute(0, 2, 3, 1).reshape(-1, 3)), bits_of(want[:, :3])) and 2 < len(torch.unique(out)) <= 8
    # a checkpoint without the key is refused by name; one trained at another width as well
    del saved['bottleneck_range']
    bare = str(tmp_path / 'bare.pt')
    torch.save(saved, bare)
    layer1.bottleneck_transformer = T.Compose([T.Quantizer(3, static_range='trained')])
    with pytest.raises(ValueError, match=r"Quantizer\(static_range='trained'\): no bottleneck_range.*bare.pt"):
        load_ckpt(bare, model=student)
    layer1.bottleneck_transformer = T.Compose([T.Quantizer(4, static_range='trained')])
    with pytest.raises(ValueError, match='trained at 3 bits'):
        load_ckpt(ckpt, model=student)


# ------------------------------------------------------------------------------------------ (6) one step vs the oracle
@pytest.mark.parametrize('name,bits,lo,hi', R.ONE_STEP_RANGE_CASES)
def test_one_step_on_a_frozen_literal_range_matches_the_clipped_straight_through_oracle(ops, name, bits, lo, hi, monkeypatch):
    """The bars and the method are those of
    tests/test_fake_quant_gpu.py::test_one_step_with_the_fake_quantiser_matches_the_straight_through_oracle: LOSS_TOL,
    _grad_check against fp64, 0 differing codes -- and 0 differing mask bits.  Without the qrange_mask_grad launch the
    encoder's gradients miss the bar (the clipped elements then carry the decoder's gradient).  Achieved on MI355X: 0 of
    4320 / 3360 codes and mask bits differ, 349 / 276 values clipped, loss 7.6e-08 / 7.7e-07, gradients 1.7e-04 / 2.2e-05
    from fp64 (bar 2e-03); with qrange_mask_grad replaced by a no-op: 2.2e-01 / 3.8e-01 on backbone.body.conv1.weight."""
    z, meta = G.load(name)
    cfg, t_sd, s_sd, teacher, student, box, opt, warm = TM._setup(meta)
    layer1 = student.backbone.body.layer1
    layer1.train_fake_quant_bits = bits
    layer1.train_fake_quant_range = {'momentum': 0.01, 'frozen': True, 'range': [lo, hi]}
    state_before = bits_of(layer1.qrange_state)
    terms = MU.terms_of(cfg)
    images, targets = G.case_inputs(meta)
    ms = meta['min_size'] if isinstance(meta['min_size'], list) else [meta['min_size']]
    capture = {}
    monkeypatch.setattr(O, 'student_layer1', QU.make_student_layer1(bits, fake_quant=R.clipped_ste(bits, lo, hi, capture)))
    kw = dict(terms=terms, min_size=tuple(ms), max_size=meta['max_size'])
    orc64 = O.DistillOracle(t_sd, s_sd, dtype=torch.float64, **kw)
    orc32 = O.DistillOracle(t_sd, s_sd, **kw)
    TM._sync_oracle(orc64, student)
    TM._sync_oracle(orc32, student)
    loss64, terms64, g64, _ = orc64.step(images)
    _, _, g32, _ = orc32.step(images)
    cap32, cap64 = capture[torch.float32], capture[torch.float64]
    R.check_range_preconditions(cap32, cap64, bits, '%s at %d bits on [%g, %g]' % (name, bits, lo, hi))

    ims, tgs = TM._to_dev(images, targets)
    loss = box(ims, tgs)
    worst = {'loss': abs(loss.item() - loss64) / abs(loss64), 'grad': 0.0, 'buffer': 0.0}
    per_term = loss.per_term.cpu()
    for i, k in enumerate(terms):
        worst['loss'] = max(worst['loss'], abs(float(per_term[i]) - terms64[k]) / abs(terms64[k]))
    opt.zero_grad()
    loss.backward()
    ops.sync_check()
    eng = layer1.head_engine()
    c = eng.layers[3].cout
    assert eng.fq_range is not None and eng.fq_range['frozen'] and eng.fq_mask is not None
    assert torch.equal(bits_of(layer1.qrange_state), state_before)       # frozen: the state is left alone
    assert torch.equal(bits_of(eng.fq[0]), bits_of(R.qparams_np(lo, hi, bits)))
    qp = eng.fq[0].cpu().double()
    zq = eng.bottleneck().cpu()[..., :c].permute(0, 3, 1, 2).double()
    recovered = zq / qp[2] + qp[3]
    codes = torch.round(recovered)
    assert float((recovered - codes).abs().max()) < 1e-3 and float(qp[3]) == cap64['zero_point']
    differ = int((codes != cap64['codes'].double()).sum())
    npix = eng.count[3]
    passed = torch.from_numpy(R.mask_bits(eng.fq_mask.view(npix, -1).cpu().numpy(), c)).view(zq.shape[0], zq.shape[2], zq.shape[3], c)
    mask_differ = int((passed.permute(0, 3, 1, 2) != cap64['passed']).sum())
    print('\n[%s, %d bits, [%g, %g]] loss %.2e; codes differing from the oracle: %d, mask bits differing: %d of %d; clipped %d'
          % (name, bits, lo, hi, worst['loss'], differ, mask_differ, codes.numel(), int((~passed).sum())))
    assert differ == 0 and mask_differ == 0
    assert worst['loss'] < TM.LOSS_TOL, worst
    for n, p in student.named_parameters():
        if p.requires_grad and not n.endswith(G.ZERO_GRAD_SUFFIXES):
            worst['grad'] = max(worst['grad'], TM._grad_check(n, p.grad, g32[n], g64[n]))
    sd = student.state_dict()
    for stat in ('running_mean', 'running_var'):
        key = 'backbone.body.layer1.decoder.0.' + stat
        ref = orc64.s[key].double()
        err = float((sd[key].cpu().double() - ref).abs().max())
        worst['buffer'] = max(worst['buffer'], err / (1 + float(ref.abs().max())))
        assert err <= 1e-4 * (1 + float(ref.abs().max())), (key, err)
    print('[%s, %d bits] worst: loss %.2e (tol %.0e), grads vs fp64 %.2e (%.0e or 2x torch-fp32), decoder.0 buffers %.2e '
          '(1e-4)' % (name, bits, worst['loss'], TM.LOSS_TOL, worst['grad'], TM.GRAD_TOL, worst['buffer']))


def test_unfrozen_step_observes_then_quantises_on_the_running_range(ops):
    """the engine's own sequence on two steps: the first observation initialises the state to the batch's range (so the
    step is the per-batch quantiser's, bit for bit, with nothing clipped beyond rounding), the second folds with momentum"""
    z, meta = G.load('tiny_ghnd_faster')
    cfg, t_sd, s_sd, teacher, student, box, opt, warm = TM._setup(meta)
    layer1 = student.backbone.body.layer1
    layer1.train_fake_quant_bits = 4
    layer1.train_fake_quant_range = {'momentum': 0.5, 'frozen': False}
    images, targets = G.case_inputs(meta)
    ims, tgs = TM._to_dev(images, targets)
    twin = TM._setup(meta)
    twin[4].backbone.body.layer1.train_fake_quant_bits = 4
    loss = box(ims, tgs)
    loss_twin = twin[5](ims, tgs)
    ops.sync_check()
    eng, eng_twin = layer1.head_engine(), twin[4].backbone.body.layer1.head_engine()
    state = layer1.qrange_state.cpu()
    assert float(state[2]) == 1.0 and torch.equal(bits_of(state[:2]), bits_of(eng_twin.fq[0][:2]))
    assert torch.equal(bits_of(eng.fq[0]), bits_of(eng_twin.fq[0]))
    assert torch.equal(bits_of(eng.bottleneck()), bits_of(eng_twin.bottleneck()))
    assert loss.item() == loss_twin.item()
    opt.zero_grad()
    loss.backward()
    opt.step()
    box(ims, tgs)
    ops.sync_check()
    state2 = layer1.qrange_state.cpu()
    assert float(state2[2]) == 2.0 and float(state2[3]) == 0.0
    assert torch.equal(bits_of(eng.fq[0][:2]), bits_of(state2[:2]))
    assert torch.equal(bits_of(eng.fq[0]), bits_of(R.qparams_np(state2[0].numpy(), state2[1].numpy(), 4)))


# ------------------------------------------------------------------------------------------ (7) plan isolation
QUANT_OPS = ('fake_quantize_bits', 'fake_quantize_range', 'qrange_observe', 'qrange_mask_grad', 'qrange_qparams',
             'bn_finalize', 'bn_bwd_apply', 'bn_bwd_reduce', 'bn_bwd_finalize', 'affine_relu', 'add_inplace')


def _traced_step(ops, monkeypatch, meta, prepare):
    from hnd_ghnd_object_detectors_amd import engine as E
    cfg, t_sd, s_sd, teacher, student, box, opt, warm = TM._setup(meta)
    prepare(student.backbone.body.layer1)
    images, targets = G.case_inputs(meta)
    ims, tgs = TM._to_dev(images, targets)
    trace = []
    run = E._run
    with monkeypatch.context() as mp:
        mp.setattr(E, '_run', lambda l, tag=None: (trace.append(tag or type(l).__name__), run(l, tag))[1])
        for name in QUANT_OPS:
            def spy(*a, _f=getattr(ops, name), _n=name, **k):
                trace.append('ops.' + _n)
                return _f(*a, **k)
            mp.setattr(E.ops, name, spy)
        loss = box(ims, tgs)
        opt.zero_grad()
        loss.backward()
        ops.sync_check()
    grads = {n: p.grad.detach().clone() for n, p in student.named_parameters() if p.requires_grad and p.grad is not None}
    return trace, loss.item(), grads, student


def test_with_the_range_off_the_step_launches_and_computes_what_it_did_before(ops, monkeypatch):
    z, meta = G.load('tiny_ghnd_faster')

    def toggled(layer1):
        layer1.train_fake_quant_bits = 4
        layer1.train_fake_quant_range = {'momentum': 0.1, 'frozen': False}      # on ... and off again before the step
        layer1.train_fake_quant_range = None

    def batch_only(layer1):
        layer1.train_fake_quant_bits = 4

    def range_without_width(layer1):
        layer1.train_fake_quant_range = {'momentum': 0.1, 'frozen': False}      # inert without a width

    def ranged(layer1):
        layer1.train_fake_quant_bits = 4
        layer1.train_fake_quant_range = {'momentum': 0.1, 'frozen': False}

    t_plain, l_plain, g_plain, _ = _traced_step(ops, monkeypatch, meta, lambda layer1: None)
    t_inert, l_inert, g_inert, _ = _traced_step(ops, monkeypatch, meta, range_without_width)
    t_batch, l_batch, g_batch, _ = _traced_step(ops, monkeypatch, meta, batch_only)
    t_off, l_off, g_off, s_off = _traced_step(ops, monkeypatch, meta, toggled)
    t_on, l_on, g_on, _ = _traced_step(ops, monkeypatch, meta, ranged)
    new = {'ops.fake_quantize_range', 'ops.qrange_observe', 'ops.qrange_mask_grad', 'ops.qrange_qparams'}
    assert len(t_plain) > 20 and not new & set(t_plain) and 'ops.fake_quantize_bits' not in t_plain
    assert t_inert == t_plain and l_inert == l_plain
    assert t_off == t_batch and l_off == l_batch and not new & set(t_batch) and t_batch.count('ops.fake_quantize_bits') == 1
    assert [t for t in t_batch if t != 'ops.fake_quantize_bits'] == t_plain     # (what the merged QAT plan adds: one call)
    for a, b in ((g_inert, g_plain), (g_off, g_batch)):
        assert sorted(a) == sorted(b) and all(torch.equal(bits_of(a[k]), bits_of(b[k])) for k in a)
    # on: the per-batch call is replaced by observe + the one-launch quantiser, and the backward gains exactly one launch
    assert [t for t in t_on if t not in new] == t_plain
    assert [t for t in t_on if t in new] == ['ops.qrange_observe', 'ops.fake_quantize_range', 'ops.qrange_mask_grad']
    i = t_on.index('ops.qrange_mask_grad')
    assert t_on[i - 1] == 'ops.bn_bwd_apply' and 'layer1.conv3' in str(t_on[i + 1])
    # the first observation is the batch's own range: the forward is the per-batch quantiser's
    assert l_on == l_batch
    assert 'qrange_state' in dict(s_off.backbone.body.layer1.named_buffers())
    assert 'backbone.body.layer1.qrange_state' not in s_off.state_dict()
