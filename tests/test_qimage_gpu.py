"""GPU: per-image scales for the bottleneck codec and the fake quantiser (include/hnd_qimage.h and the layers above it).

 (1) every export against the numpy restatement of tests/qimage_util.py (which tests/test_qimage_cpu.py pins to the
     reference's quantize_tensor / dequantize_tensor applied to each image alone): torch.equal on bytes, payloads, qparams,
     dequantised floats and the stats recomputed on the host, on the smallest shapes at which each mechanism can go wrong;
 (2) batch invariance and the n = 1 anchor on the per-tensor kernels: image i of a batched call is hnd_quantize_bits /
     hnd_fake_quantize_bits on x[i:i+1] alone, and with n = 1 every export gives its per-tensor twin's bits, stats and
     payload included;
 (3) the fake quantiser in place, out of place and without stats; constant images beside live ones; the refusals;
 (4) the host classes, batch 1, the split model, the engine with the flag absent, off and on, and one training step against
     the fp64 / fp32 oracle with a per-image straight-through estimator."""
import pytest
import torch

from oracle import hnd_oracle as O
from tests import codec_util as CU
from tests import golden_util as G
from tests import model_util as MU
from tests import qat_util as QU
from tests import qimage_util as QI
from tests import test_model_gpu as TM

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAD_GARBAGE = 1.0e6             # what the pad channels of the SOURCE hold: never counted, never copied


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


@pytest.fixture(scope='module', autouse=True)
def leave_nothing_behind():
    """the students, oracles and plans of this file are garbage once it is done: collect them and hand their device memory
    back, so the files that run after it meet the process as they did before"""
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def source(z, cs):
    """device NHWC buffer of stride cs: the real channels of z, garbage in the pad channels"""
    n, c, h, w = z.shape
    buf = torch.full((n, h, w, cs), PAD_GARBAGE)
    buf[..., :c] = z.permute(0, 2, 3, 1)
    return buf.to(DEV)


def nan_like(shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), device=DEV) if dtype == torch.float32 else \
        torch.full(shape, 0xAB, dtype=dtype, device=DEV)


def run_all(ops, z, cs, bits, stats=False):
    """every export on z: dict(q, qp, deq, payload, qp_packed, unpacked, fake, qp_fake[, stats])"""
    n, c, h, w = z.shape
    x = source(z, cs)
    scratch = torch.empty(ops.qimage_scratch_elems(n), device=DEV)
    r = {'x': x}
    r['q'], r['qp'] = nan_like(x.shape, torch.uint8), nan_like((n, 4))
    ops.qimage_quantize_bits(x, c, bits, r['q'], r['qp'], scratch)
    r['deq'] = ops.qimage_dequantize_u8(r['q'], r['qp'], nan_like(x.shape), c)
    r['payload'] = nan_like((ops.codec_packed_bytes(n * c * h * w, bits),), torch.uint8)
    r['qp_packed'] = nan_like((n, 4))
    ops.qimage_quantize_pack_bits(x, c, bits, r['payload'], r['qp_packed'], scratch)
    r['unpacked'] = ops.qimage_unpack_dequantize_bits(r['payload'], r['qp_packed'], nan_like(x.shape), c, bits)
    r['qp_fake'] = nan_like((n, 4))
    r['stats'] = nan_like((ops.fake_quantize_tiles(n * h * w), 2, cs)) if stats else None
    r['fake'] = ops.qimage_fake_quantize_bits(x, c, bits, r['qp_fake'], scratch, out=nan_like(x.shape), stats=r['stats'])
    ops.sync_check()
    assert torch.equal(x.cpu()[..., :c], z.permute(0, 2, 3, 1))           # the source is read only
    return r


def check_against(r, ref, shape, cs, bits):
    n, c, h, w = shape
    assert torch.equal(CU.logical(r['q'], c), ref.codes)
    for k in ('qp', 'qp_packed', 'qp_fake'):
        assert torch.equal(bits_of(r[k]), bits_of(ref.qparams)), k
    assert torch.equal(r['payload'].cpu(), torch.from_numpy(ref.payload))
    # the unpacked and the packed path give the same codes (host_unpack also asserts the unused high bits are 0)
    assert torch.equal(CU.host_unpack(r['payload'].cpu().numpy(), shape, bits), CU.logical(r['q'], c))
    for k in ('deq', 'unpacked', 'fake'):
        assert torch.equal(bits_of(CU.logical(r[k], c)), bits_of(ref.dequantized)), k
        assert not bool(torch.isnan(r[k]).any())
        if cs > c:
            assert float(r[k][..., c:].abs().max()) == 0.0, k                 # pad channels are 0
    if cs > c:
        assert int(r['q'][..., c:].max()) == 0
    if r['stats'] is not None:
        want = QI.restate_stats(r['fake'].cpu().view(n * h * w, cs), cs)
        assert tuple(r['stats'].shape) == tuple(want.shape) == ((n * h * w + QI.ROWS - 1) // QI.ROWS, 2, cs)
        assert torch.equal(bits_of(r['stats']), bits_of(want))
        if cs > c:
            assert float(r['stats'][:, :, c:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ (1) bit identity
@pytest.mark.parametrize('shape,cs,bits', QI.CASES)
def test_every_export_is_the_restatement_bit_for_bit(ops, shape, cs, bits):
    r = run_all(ops, QI.make_input(shape), cs, bits, stats=True)
    check_against(r, QI.restated(shape, bits), shape, cs, bits)
    assert len(torch.unique(r['q'][..., :shape[1]])) <= 2 ** bits


# ------------------------------------------------------------------------------------------ (2) invariance and the anchor
@pytest.mark.parametrize('shape,cs,bits', QI.CASES)
def test_image_i_of_a_batched_call_is_the_per_tensor_kernel_on_that_image_alone(ops, shape, cs, bits):
    n, c, h, w = shape
    z = QI.make_input(shape)
    r = run_all(ops, z, cs, bits)
    scratch = torch.empty(ops.minmax_scratch_elems(), device=DEV)
    for i in range(n):
        x1 = source(z[i:i + 1], cs)
        q1, qp1 = nan_like(x1.shape, torch.uint8), nan_like((4,))
        ops.quantize_bits(x1, c, bits, q1, qp1, scratch)
        fake1 = ops.fake_quantize_bits(x1, c, bits, nan_like((4,)), scratch, out=nan_like(x1.shape))
        ops.sync_check()
        assert torch.equal(r['q'][i:i + 1], q1), i
        assert torch.equal(bits_of(r['qp'][i]), bits_of(qp1)), i
        assert torch.equal(bits_of(r['fake'][i:i + 1]), bits_of(fake1)), i


@pytest.mark.parametrize('bits', QI.ALL_WIDTHS)
@pytest.mark.parametrize('shape,cs', [QI.SHAPES_ALL_WIDTHS[0], ((1, 3, 13, 10), 4), ((1, 6, 9, 11), 32)])
def test_one_image_gives_the_per_tensor_twins_bits(ops, shape, cs, bits):
    """bytes, qparams, payload, floats and stats; beside the issue's (1, 3, 1, 2) two shapes with more than one stats tile and
    a wide stride"""
    n, c, h, w = shape
    assert n == 1
    z = QI.make_input(shape)
    r = run_all(ops, z, cs, bits, stats=True)
    x = r['x']
    scratch = torch.empty(ops.minmax_scratch_elems(), device=DEV)
    q, qp = nan_like(x.shape, torch.uint8), nan_like((4,))
    ops.quantize_bits(x, c, bits, q, qp, scratch)
    deq = nan_like(x.shape)
    ops.dequantize_u8(q, qp, deq, c)
    payload, qp_p = nan_like((r['payload'].numel(),), torch.uint8), nan_like((4,))
    ops.quantize_pack_bits(x, c, bits, payload, qp_p, scratch)
    unpacked = nan_like(x.shape)
    ops.unpack_dequantize_bits(payload, qp_p, unpacked, c, bits)
    qp_f, stats = nan_like((4,)), nan_like(tuple(r['stats'].shape))
    fake = ops.fake_quantize_bits(x, c, bits, qp_f, scratch, out=nan_like(x.shape), stats=stats)
    ops.sync_check()
    assert torch.equal(r['q'], q) and torch.equal(bits_of(r['qp']).view(-1), bits_of(qp))
    assert torch.equal(r['payload'], payload) and torch.equal(bits_of(r['qp_packed']).view(-1), bits_of(qp_p))
    assert torch.equal(bits_of(r['deq']), bits_of(deq)) and torch.equal(bits_of(r['unpacked']), bits_of(unpacked))
    assert torch.equal(bits_of(r['fake']), bits_of(fake)) and torch.equal(bits_of(r['qp_fake']).view(-1), bits_of(qp_f))
    assert torch.equal(bits_of(r['stats']), bits_of(stats))


# ------------------------------------------------------------------------------------------ (3) the fake quantiser
@pytest.mark.parametrize('shape,cs,bits', [(s, cs, b) for s, cs, b in QI.CASES if b in (2, 8)])
def test_fake_quantize_in_place_out_of_place_and_without_stats(ops, shape, cs, bits):
    n, c, h, w = shape
    z = QI.make_input(shape)
    ref = QI.restated(shape, bits)
    r = run_all(ops, z, cs, bits, stats=True)
    assert torch.equal(bits_of(r['fake']), bits_of(r['deq']))                 # y = quantise then dequantise
    # in place, and the sums identical across two runs
    scratch = torch.empty(ops.qimage_scratch_elems(n), device=DEV)
    y, qp, stats = source(z, cs), nan_like((n, 4)), nan_like(tuple(r['stats'].shape))
    assert ops.qimage_fake_quantize_bits(y, c, bits, qp, scratch, stats=stats) is y
    # stats = NULL, in place
    y2, qp2 = source(z, cs), nan_like((n, 4))
    assert ops.qimage_fake_quantize_bits(y2, c, bits, qp2, scratch) is y2
    ops.sync_check()
    for got, got_qp in ((y, qp), (y2, qp2)):
        assert torch.equal(bits_of(got), bits_of(r['fake'])) and torch.equal(bits_of(got_qp), bits_of(ref.qparams))
    assert torch.equal(bits_of(stats), bits_of(r['stats']))


@pytest.mark.parametrize('bits', [1, 4, 8])
def test_constant_images_reconstruct_exactly_beside_live_ones(ops, bits):
    shape, cs = (5, 3, 2, 3), 4
    z = QI.with_constants(shape)
    r = run_all(ops, z, cs, bits, stats=True)
    check_against(r, QI.restate(z, bits), shape, cs, bits)
    for k in ('deq', 'unpacked', 'fake'):
        got = CU.logical(r[k], shape[1])
        for i in (0, 1, 4):
            assert torch.equal(bits_of(got[i]), bits_of(z[i])), (k, i)
    assert not bool(torch.isnan(r['stats']).any())


@pytest.mark.parametrize('bits', QI.RMS_WIDTHS)
def test_per_image_reconstruction_beats_per_tensor_on_the_scaled_input(ops, bits):
    shape, cs = QI.RMS_SHAPE, 4
    z = QI.make_input(shape)
    c = shape[1]
    r = run_all(ops, z, cs, bits)
    x = r['x']
    q, qp = nan_like(x.shape, torch.uint8), nan_like((4,))
    ops.quantize_bits(x, c, bits, q, qp, torch.empty(ops.minmax_scratch_elems(), device=DEV))
    flat = nan_like(x.shape)
    ops.dequantize_u8(q, qp, flat, c)
    ops.sync_check()
    per_image, per_tensor = QI.rms_error(z, CU.logical(r['deq'], c)), QI.rms_error(z, CU.logical(flat, c))
    print('\n[%d bits] RMS error per image %.4e, per tensor %.4e, ratio %.3f' % (bits, per_image, per_tensor,
                                                                               per_image / per_tensor))
    assert per_image < per_tensor


def test_every_refusal_names_its_export(ops):
    from hnd_ghnd_object_detectors_amd import _lib
    from tests.test_qimage_cpu import check_every_refusal
    check_every_refusal(_lib.load())
    ops.sync_check()                                                       # nothing was launched, nothing is pending


# ------------------------------------------------------------------------------------------ (4) host classes
@pytest.mark.parametrize('bits', [1, 3, 8])
def test_quantizer_dequantizer_and_fake_quantizer_round_trip_to_the_restatement(ops, bits):
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    shape = (2, 6, 9, 11)
    z = QI.make_input(shape)
    ref = QI.restated(shape, bits)
    qz, tgt = T.Quantizer(bits, per_image=True)(z.to(DEV), 'target')
    assert tgt == 'target' and isinstance(qz, T.QuantizedTensor) and qz.per_image and qz.num_bits == bits
    assert not qz.per_channel
    assert tuple(qz.qparams.shape) == (2, 4) and tuple(qz.scale.shape) == tuple(qz.zero_point.shape) == (2,)
    assert qz.scale.device.type == 'cuda' and qz.scale.data_ptr() == qz.qparams.data_ptr() + 8
    assert torch.equal(qz.tensor.cpu(), ref.codes) and torch.equal(bits_of(qz.qparams), bits_of(ref.qparams))
    deq, _ = T.Dequantizer(bits)(qz, None)
    assert torch.equal(bits_of(deq), bits_of(ref.dequantized))
    with pytest.raises(ValueError, match='per-image tensor quantised at %d bits' % bits):
        T.Dequantizer(4 if bits != 4 else 5)(qz, None)
    pz, _ = T.Quantizer(bits, packed=True, per_image=True)(z.to(DEV), None)
    assert isinstance(pz, T.PackedBottleneck) and pz.per_image and pz.shape == shape
    assert pz.nbytes == ref.payload.size and pz.link_bytes == pz.nbytes + 8 * 2
    assert torch.equal(pz.payload.cpu(), torch.from_numpy(ref.payload))
    # across the link: the payload, its shape and width, and the qparams; nothing of the head's buffers
    linked = T.PackedBottleneck(pz.payload.clone(), pz.shape, pz.num_bits, pz.qparams.clone(), per_image=True)
    deq, _ = T.Dequantizer(bits)(linked, None)
    assert torch.equal(bits_of(deq), bits_of(ref.dequantized))
    fq = T.FakeQuantizer(bits, per_image=True)
    out, _ = fq(z.to(DEV), None)
    assert torch.equal(bits_of(out), bits_of(ref.dequantized)) and torch.equal(bits_of(fq.qparams), bits_of(ref.qparams))
    assert float(out._hnd[..., 6:].abs().max()) == 0.0
    ops.sync_check()


@pytest.mark.parametrize('bits', [2, 5, 8])
def test_at_batch_one_the_keyword_gives_the_bytes_of_the_plain_quantizer(ops, bits):
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    z = QI.make_input((2, 6, 9, 11))[1:2].contiguous()
    plain, _ = T.Quantizer(bits)(z.to(DEV), None)
    keyed, _ = T.Quantizer(bits, per_image=True)(z.to(DEV), None)
    assert torch.equal(keyed.tensor, plain.tensor) and torch.equal(bits_of(keyed.qparams).view(-1), bits_of(plain.qparams))
    plain_p, _ = T.Quantizer(bits, packed=True)(z.to(DEV), None)
    keyed_p, _ = T.Quantizer(bits, packed=True, per_image=True)(z.to(DEV), None)
    assert torch.equal(keyed_p.payload, plain_p.payload) and keyed_p.link_bytes == plain_p.link_bytes
    # ... and inside a batch image 1 keeps those bytes
    both, _ = T.Quantizer(bits, per_image=True)(QI.make_input((2, 6, 9, 11)).to(DEV), None)
    assert torch.equal(both.tensor[1:2], plain.tensor) and torch.equal(bits_of(both.qparams[1]), bits_of(plain.qparams))
    ops.sync_check()


@pytest.fixture(scope='module')
def tiny_student():
    """the tiny student of tiny_eval_quantized, as tests/test_codec_bits_gpu.py builds it"""
    _, meta = G.load('tiny_eval_quantized')
    cfg = MU.config_for(meta)
    t_sd, s_sd = MU.oracle_states(meta['seed'])
    _, student = MU.build_pair(cfg, t_sd, s_sd, DEV)
    student.eval()
    images, _ = G.case_inputs(meta)
    return student, [im.to(DEV) for im in images]


@pytest.mark.parametrize('bits', [2, 4])
def test_per_image_split_gives_the_tail_the_floats_of_the_pair(tiny_student, bits):
    from hnd_ghnd_object_detectors_amd.models.mimic.split_rcnn import split_rcnn_model, split_rcnn_model_per_image
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    student, ims = tiny_student
    layer1 = student.backbone.body.layer1
    saved = layer1.bottleneck_transformer, layer1.use_bottleneck_transformer
    try:
        layer1.bottleneck_transformer = T.Compose([T.Quantizer(bits, per_image=True), T.Dequantizer(bits)])
        layer1.use_bottleneck_transformer = True
        with torch.no_grad():
            whole = {k: v.clone() for k, v in student(ims).items()}
    finally:
        layer1.bottleneck_transformer, layer1.use_bottleneck_transformer = saved
    with torch.no_grad():
        head, _ = split_rcnn_model(student, None)
        head.eval()
        z_plain = head(ims)[0].cpu().clone()              # the head's own unquantised z
    want = QI.restate(z_plain, bits)
    n = z_plain.shape[0]
    feats = {}
    for packed in (False, True):
        head, tail = split_rcnn_model_per_image(student, bits, packed=packed)
        head.eval()
        tail.eval()
        tail.features_only = True
        with torch.no_grad():
            zq, tensors_shape, image_sizes, original_sizes = head(ims)
            assert zq.per_image and tuple(zq.qparams.shape) == (n, 4)
            assert torch.equal(bits_of(zq.qparams), bits_of(want.qparams))
            if packed:
                assert isinstance(zq, T.PackedBottleneck) and zq.link_bytes == zq.nbytes + 8 * n
                emitted = CU.host_unpack(zq.payload.cpu().numpy(), zq.shape, bits)
                zq = T.PackedBottleneck(zq.payload.clone(), zq.shape, zq.num_bits, zq.qparams.clone(), per_image=True)
            else:
                assert isinstance(zq, T.QuantizedTensor)
                emitted = zq.tensor.cpu()
            assert torch.equal(emitted, want.codes)
            feats[packed] = {k: v.clone() for k, v in tail(zq, tensors_shape, image_sizes, original_sizes).items()}
    assert list(feats[True]) == list(feats[False]) == list(whole)
    for k in whole:
        assert torch.equal(feats[True][k], feats[False][k]) and torch.equal(feats[False][k], whole[k]), k


# ------------------------------------------------------------------------------------------ the engine
def _student(cfg, s_sd):
    from hnd_ghnd_object_detectors_amd import mimic_runner
    from hnd_ghnd_object_detectors_amd.models import get_model
    student = get_model(cfg['student_model'], torch.device(DEV))
    student.load_state_dict(s_sd, strict=True)
    mimic_runner.freeze_modules(student, cfg['student_model'])
    student.train()
    student.distill_backbone_only = True
    student.backbone.body.layer1.use_bottleneck_transformer = False
    return student


def test_flag_absent_leaves_the_plan_the_launches_and_the_bottleneck_alone(ops, monkeypatch):
    """three students at 4 bits: one that never heard of the flag (its engine is called without the keyword), one with the
    flag switched on and off again, one with it on"""
    from hnd_ghnd_object_detectors_amd import engine as E
    z, meta = G.load('tiny_ghnd_faster')
    cfg = MU.config_for(meta)
    _, s_sd = MU.oracle_states(meta['seed'], meta['model'], meta.get('bch', 3), meta.get('num_classes', 91))
    images, targets = G.case_inputs(meta)
    ims, tgs = TM._to_dev(images, targets)
    bits = 4
    launches, keywords = [], []
    run, forward = E._run, E.HeadEngine.forward

    def spy_run(l, tag):
        launches.append(tag)
        return run(l, tag)

    def spy_forward(self, x, training, **kw):
        keywords.append(sorted(kw))
        return forward(self, x, training, **kw)
    monkeypatch.setattr(E, '_run', spy_run)
    monkeypatch.setattr(E.HeadEngine, 'forward', spy_forward)
    for name in ('fake_quantize_bits', 'qchannel_fake_quantize_bits', 'qimage_fake_quantize_bits'):
        def spy(*a, _fn=getattr(ops, name), _name=name, **k):
            launches.append(_name)
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    seen = {}
    for which in ('never', 'off', 'on'):
        student = _student(cfg, s_sd)
        layer1 = student.backbone.body.layer1
        layer1.train_fake_quant_bits = bits
        if which != 'never':
            layer1.train_fake_quant_per_image = True
        if which == 'off':
            layer1.train_fake_quant_per_image = False
        del launches[:], keywords[:]
        student(ims, tgs)
        ops.sync_check()
        eng = layer1.head_engine()
        zi = eng.encoder_len - 1
        assert zi == 3
        seen[which] = dict(launches=list(launches), keywords=list(keywords), key=eng.plan_key, z=eng.y[zi].clone(),
                           out=eng.out.clone(), qp=eng.fq[0].clone(), c=eng.layers[zi].cout, per_image=eng.fq_per_image)
    never, off, on = seen['never'], seen['off'], seen['on']
    assert all('fake_quant_per_image' not in kw for kw in never['keywords'] + off['keywords'])
    assert any('fake_quant_per_image' in kw for kw in on['keywords'])
    assert not never['per_image'] and not off['per_image'] and on['per_image']
    # the same launches, the same shape of plan key (its pointers belong to each student), the same y[3] and output
    assert never['launches'] == off['launches'] and 'fake_quantize_bits' in never['launches']
    assert 'qimage_fake_quantize_bits' not in never['launches'] and 'qchannel_fake_quantize_bits' not in never['launches']
    def strip(key):                        # (input pointer, shape, training, parameter pointers, output pointer, width, ...)
        return len(key), key[1], key[2], key[5:]
    assert strip(never['key']) == strip(off['key']) and never['key'][-1] == bits
    assert torch.equal(bits_of(never['z']), bits_of(off['z'])) and torch.equal(bits_of(never['out']), bits_of(off['out']))
    assert tuple(never['qp'].shape) == (4,)
    # on: the per-image launch in the per-tensor one's place, a key that says so, and the pair's bits
    assert on['launches'] == [t if t != 'fake_quantize_bits' else 'qimage_fake_quantize_bits' for t in never['launches']]
    assert on['key'][-1] == 'per_image' and len(on['key']) == len(never['key']) + 1
    c, n = on['c'], on['z'].shape[0]
    assert n == 2 and tuple(on['qp'].shape) == (n, 4)
    assert not torch.equal(bits_of(on['z']), bits_of(never['z']))
    # the unquantised z of the same step: a student with the quantiser off
    plain = _student(cfg, s_sd)
    plain(ims, tgs)
    ops.sync_check()
    z_plain = plain.backbone.body.layer1.head_engine().y[3]
    want = QI.restate(CU.logical(z_plain, c).contiguous().cpu(), bits)
    assert torch.equal(bits_of(CU.logical(on['z'], c)), bits_of(want.dequantized))
    assert torch.equal(bits_of(on['qp']), bits_of(want.qparams))
    assert float(on['z'][..., c:].abs().max()) == 0.0


def test_engine_refuses_the_flag_with_a_fixed_range_per_channel_and_a_non_bool(ops):
    from hnd_ghnd_object_detectors_amd import engine as E
    z, meta = G.load('tiny_ghnd_faster')
    cfg = MU.config_for(meta)
    _, s_sd = MU.oracle_states(meta['seed'], meta['model'], meta.get('bch', 3), meta.get('num_classes', 91))
    eng = _student(cfg, s_sd).backbone.body.layer1.head_engine()
    x = torch.zeros(1, 4, 4, 64, device=DEV)
    with pytest.raises(ValueError, match='HeadEngine.forward: fake_quant_per_image=1 must be a bool'):
        eng.forward(x, True, fake_quant_bits=4, fake_quant_per_image=1)
    rng = {'state': torch.zeros(4, device=DEV), 'momentum': 0.1, 'frozen': False, 'range': None}
    with pytest.raises(ValueError, match='fake_quant_per_image together with fake_quant_range'):
        eng.forward(x, True, fake_quant_bits=4, fake_quant_range=rng, fake_quant_per_image=True)
    with pytest.raises(ValueError, match='fake_quant_per_image together with fake_quant_per_channel'):
        eng.forward(x, True, fake_quant_bits=4, fake_quant_per_channel=True, fake_quant_per_image=True)
    assert isinstance(eng, E.HeadEngine) and eng.plan_key is None          # refused before a plan was built


# ------------------------------------------------------------------------------------------ one step vs the oracle
@pytest.mark.parametrize('name,bits', QI.ONE_STEP_CASES)
def test_one_step_with_the_per_image_fake_quantiser_matches_the_straight_through_oracle(ops, name, bits, monkeypatch):
    """The bars are those tests/test_fake_quant_gpu.py applies to the per-tensor step (LOSS_TOL, _grad_check, its buffer
    bar), the reference being the fp64 oracle with a per-image straight-through estimator (tests/qimage_util.py).  The
    quantiser's rounding decisions are NOT masked out: per image the oracle pair agrees on every one and keeps 1e-4 code
    units from every tie (also held on the CPU, tests/test_qimage_cpu.py), and then the HIP path's codes must equal the
    oracle's everywhere.  Figures achieved on MI355X are printed."""
    z, meta = G.load(name)
    cfg, t_sd, s_sd, teacher, student, box, opt, warm = TM._setup(meta)
    layer1 = student.backbone.body.layer1
    layer1.train_fake_quant_bits = bits
    layer1.train_fake_quant_per_image = True
    terms = MU.terms_of(cfg)
    images, targets = G.case_inputs(meta)
    ms = meta['min_size'] if isinstance(meta['min_size'], list) else [meta['min_size']]
    capture = {}

    def fq(zz):
        capture[zz.dtype] = QI.decide_codes_per_image(zz.detach(), bits)
        return QI.ste_per_image(zz, bits)
    monkeypatch.setattr(O, 'student_layer1', QU.make_student_layer1(bits, fake_quant=fq))
    kw = dict(terms=terms, min_size=tuple(ms), max_size=meta['max_size'])
    orc64 = O.DistillOracle(t_sd, s_sd, dtype=torch.float64, **kw)
    orc32 = O.DistillOracle(t_sd, s_sd, **kw)
    TM._sync_oracle(orc64, student)
    TM._sync_oracle(orc32, student)
    loss64, terms64, g64, _ = orc64.step(images)
    _, _, g32, _ = orc32.step(images)
    caps32, caps64 = capture[torch.float32], capture[torch.float64]
    QI.check_preconditions_per_image(caps32, caps64, '%s at %d bits' % (name, bits))
    assert QI.qparams_differ(caps64)

    ims, tgs = TM._to_dev(images, targets)
    loss = box(ims, tgs)
    worst = {'loss': abs(loss.item() - loss64) / abs(loss64), 'grad': 0.0, 'buffer': 0.0}
    per_term = loss.per_term.cpu()
    for i, k in enumerate(terms):
        worst['loss'] = max(worst['loss'], abs(float(per_term[i]) - terms64[k]) / abs(terms64[k]))
    opt.zero_grad()
    loss.backward()
    ops.sync_check()
    # the quantiser's decisions, recovered per image from the stored values: q = z' / scale + zero_point
    eng = layer1.head_engine()
    assert eng.fq_per_image
    c = eng.layers[3].cout
    qp = eng.fq[0].cpu().double()
    zq = eng.bottleneck().cpu()[..., :c].permute(0, 3, 1, 2).double()
    assert tuple(qp.shape) == (zq.shape[0], 4) == (len(caps64), 4)
    differ = total = 0
    for i in range(zq.shape[0]):
        recovered = zq[i:i + 1] / qp[i, 2] + qp[i, 3]
        codes = torch.round(recovered)
        assert float((recovered - codes).abs().max()) < 1e-3 and float(qp[i, 3]) == caps64[i]['zero_point'], i
        differ += int((codes != caps64[i]['codes'].double()).sum())
        total += codes.numel()
    print('\n[%s, %d bits, per image] loss %.2e; codes differing from the oracle: %d of %d' % (name, bits, worst['loss'],
                                                                                             differ, total))
    assert differ == 0
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
    print('[%s, %d bits, per image] worst: loss %.2e (tol %.0e), grads vs fp64 %.2e (%.0e or 2x torch-fp32), decoder.0 '
          'buffers %.2e (1e-4)' % (name, bits, worst['loss'], TM.LOSS_TOL, worst['grad'], TM.GRAD_TOL, worst['buffer']))
