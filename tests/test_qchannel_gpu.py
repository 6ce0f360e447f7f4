"""GPU: per-channel scales for the bottleneck codec and the fake quantiser (include/hnd_qchannel.h and the layers above it).

 (1) every export against the numpy restatement of tests/qchannel_util.py (which tests/test_qchannel_cpu.py pins to the
     reference's quantize_tensor / dequantize_tensor applied to each channel alone): torch.equal on bytes, payloads, qparams
     and dequantised floats, on the smallest shapes at which each mechanism can go wrong; pad channels, payload tail bits;
 (2) anchors on the per-tensor kernels: with c = 1 the bytes and qparams of hnd_quantize_bits / hnd_quantize_pack_bits /
     hnd_fake_quantize_bits, and each channel's codes those of hnd_quantize_bits on that channel alone;
 (3) the fake quantiser: the pair's bits in place and out of place, its partial sums in the header's order, twice;
 (4) constant channels beside live ones, the RMS property on the disparate-range input, the refusals;
 (5) the host classes, the split model, the engine with the flag absent, and one training step against the fp64 / fp32
     oracle with a per-channel straight-through estimator."""
import pytest
import torch

from oracle import hnd_oracle as O
from tests import codec_util as CU
from tests import golden_util as G
from tests import model_util as MU
from tests import qat_util as QU
from tests import qchannel_util as QC
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
    scratch = torch.empty(ops.qchannel_scratch_elems(cs), device=DEV)
    r = {'x': x}
    r['q'], r['qp'] = nan_like(x.shape, torch.uint8), nan_like((c, 4))
    ops.qchannel_quantize_bits(x, c, bits, r['q'], r['qp'], scratch)
    r['deq'] = ops.qchannel_dequantize_u8(r['q'], r['qp'], nan_like(x.shape), c)
    r['payload'] = nan_like((ops.codec_packed_bytes(n * c * h * w, bits),), torch.uint8)
    r['qp_packed'] = nan_like((c, 4))
    ops.qchannel_quantize_pack_bits(x, c, bits, r['payload'], r['qp_packed'], scratch)
    r['unpacked'] = ops.qchannel_unpack_dequantize_bits(r['payload'], r['qp_packed'], nan_like(x.shape), c, bits)
    r['qp_fake'] = nan_like((c, 4))
    r['stats'] = nan_like((ops.fake_quantize_tiles(n * h * w), 2, cs)) if stats else None
    r['fake'] = ops.qchannel_fake_quantize_bits(x, c, bits, r['qp_fake'], scratch, out=nan_like(x.shape), stats=r['stats'])
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


# ------------------------------------------------------------------------------------------ (1) bit identity
@pytest.mark.parametrize('shape,cs,bits', QC.CASES)
def test_every_export_is_the_restatement_bit_for_bit(ops, shape, cs, bits):
    r = run_all(ops, QC.make_input(shape), cs, bits)
    check_against(r, QC.restated(shape, bits), shape, cs, bits)
    assert len(torch.unique(r['q'][..., :shape[1]])) <= 2 ** bits


# ------------------------------------------------------------------------------------------ (2) anchors
@pytest.mark.parametrize('bits', QC.ALL_WIDTHS)
def test_one_channel_gives_the_per_tensor_kernels_bytes_and_qparams(ops, bits):
    shape, cs = QC.SHAPES_ALL_WIDTHS[0]
    assert shape[1] == 1
    n, c, h, w = shape
    r = run_all(ops, QC.make_input(shape), cs, bits)
    x = r['x']
    scratch = torch.empty(ops.minmax_scratch_elems(), device=DEV)
    q, qp = nan_like(x.shape, torch.uint8), nan_like((4,))
    ops.quantize_bits(x, c, bits, q, qp, scratch)
    payload, qp_p = nan_like((r['payload'].numel(),), torch.uint8), nan_like((4,))
    ops.quantize_pack_bits(x, c, bits, payload, qp_p, scratch)
    qp_f = nan_like((4,))
    fake = ops.fake_quantize_bits(x, c, bits, qp_f, scratch, out=nan_like(x.shape))
    ops.sync_check()
    assert torch.equal(r['q'], q) and torch.equal(bits_of(r['qp']).view(-1), bits_of(qp))
    assert torch.equal(r['payload'], payload) and torch.equal(bits_of(r['qp_packed']).view(-1), bits_of(qp_p))
    assert torch.equal(bits_of(r['fake']), bits_of(fake)) and torch.equal(bits_of(r['qp_fake']).view(-1), bits_of(qp_f))


@pytest.mark.parametrize('bits', QC.ALL_WIDTHS)
def test_each_channels_codes_are_the_per_tensor_kernels_on_that_channel_alone(ops, bits):
    shape, cs = QC.SHAPES_ALL_WIDTHS[2]
    assert shape == (2, 3, 5, 7)
    z = QC.make_input(shape)
    r = run_all(ops, z, cs, bits)
    scratch = torch.empty(ops.minmax_scratch_elems(), device=DEV)
    for ch in range(shape[1]):
        x1 = source(z[:, ch:ch + 1], 4)
        q1, qp1 = nan_like(x1.shape, torch.uint8), nan_like((4,))
        ops.quantize_bits(x1, 1, bits, q1, qp1, scratch)
        ops.sync_check()
        assert torch.equal(r['q'][..., ch], q1[..., 0]), ch
        assert torch.equal(bits_of(r['qp'][ch]), bits_of(qp1)), ch


# ------------------------------------------------------------------------------------------ (3) the fake quantiser
@pytest.mark.parametrize('shape,cs,bits', [(s, cs, b) for s, cs, b in QC.CASES if b in (2, 8)])
def test_fake_quantize_in_place_and_its_partial_sums(ops, shape, cs, bits):
    n, c, h, w = shape
    npix = n * h * w
    z = QC.make_input(shape)
    ref = QC.restated(shape, bits)
    r = run_all(ops, z, cs, bits, stats=True)
    assert torch.equal(bits_of(r['fake']), bits_of(r['deq']))                 # y = quantise then dequantise
    want = QC.restate_stats(r['fake'].cpu().view(npix, cs), cs)
    assert tuple(r['stats'].shape) == tuple(want.shape) == ((npix + QC.ROWS - 1) // QC.ROWS, 2, cs)
    assert torch.equal(bits_of(r['stats']), bits_of(want))
    # in place, and the sums identical across two runs
    scratch = torch.empty(ops.qchannel_scratch_elems(cs), device=DEV)
    y, qp, stats = source(z, cs), nan_like((c, 4)), nan_like(tuple(want.shape))
    assert ops.qchannel_fake_quantize_bits(y, c, bits, qp, scratch, stats=stats) is y
    ops.sync_check()
    assert torch.equal(bits_of(y), bits_of(r['deq'])) and torch.equal(bits_of(qp), bits_of(ref.qparams))
    assert torch.equal(bits_of(stats), bits_of(r['stats']))
    if cs > c:
        assert float(stats[:, :, c:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ (4) constants, RMS, refusals
@pytest.mark.parametrize('bits', [1, 4, 8])
def test_constant_channels_reconstruct_exactly_beside_live_ones(ops, bits):
    shape, cs = (2, 15, 3, 5), 16
    z = QC.with_constants(shape)
    r = run_all(ops, z, cs, bits, stats=True)
    check_against(r, QC.restate(z, bits), shape, cs, bits)
    for k in ('deq', 'unpacked', 'fake'):
        got = CU.logical(r[k], shape[1])
        for ch in (0, 1, 14):
            assert torch.equal(bits_of(got[:, ch]), bits_of(z[:, ch])), (k, ch)
    assert not bool(torch.isnan(r['stats']).any())


@pytest.mark.parametrize('bits', QC.RMS_WIDTHS)
def test_per_channel_reconstruction_beats_per_tensor_on_disparate_ranges(ops, bits):
    shape, cs = QC.RMS_SHAPE
    z = QC.make_input(shape)
    c = shape[1]
    r = run_all(ops, z, cs, bits)
    x = r['x']
    q, qp = nan_like(x.shape, torch.uint8), nan_like((4,))
    ops.quantize_bits(x, c, bits, q, qp, torch.empty(ops.minmax_scratch_elems(), device=DEV))
    flat = nan_like(x.shape)
    ops.dequantize_u8(q, qp, flat, c)
    ops.sync_check()
    per_channel, per_tensor = QC.rms_error(z, CU.logical(r['deq'], c)), QC.rms_error(z, CU.logical(flat, c))
    print('\n[%d bits] RMS error per channel %.4e, per tensor %.4e, ratio %.3f' % (bits, per_channel, per_tensor,
                                                                                 per_channel / per_tensor))
    assert per_channel < per_tensor


def test_every_refusal_names_its_export(ops):
    from hnd_ghnd_object_detectors_amd import _lib
    from tests.test_qchannel_cpu import check_every_refusal
    check_every_refusal(_lib.load())
    ops.sync_check()                                                       # nothing was launched, nothing is pending


# ------------------------------------------------------------------------------------------ (5) host classes
@pytest.mark.parametrize('bits', [1, 3, 8])
def test_quantizer_dequantizer_and_fake_quantizer_round_trip_to_the_restatement(ops, bits):
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    shape = (1, 6, 9, 11)
    z = QC.make_input(shape)
    ref = QC.restated(shape, bits)
    qz, tgt = T.Quantizer(bits, per_channel=True)(z.to(DEV), 'target')
    assert tgt == 'target' and isinstance(qz, T.QuantizedTensor) and qz.per_channel and qz.num_bits == bits
    assert tuple(qz.qparams.shape) == (6, 4) and tuple(qz.scale.shape) == tuple(qz.zero_point.shape) == (6,)
    assert qz.scale.device.type == 'cuda' and qz.scale.data_ptr() == qz.qparams.data_ptr() + 8
    assert torch.equal(qz.tensor.cpu(), ref.codes) and torch.equal(bits_of(qz.qparams), bits_of(ref.qparams))
    deq, _ = T.Dequantizer(bits)(qz, None)
    assert torch.equal(bits_of(deq), bits_of(ref.dequantized))
    with pytest.raises(ValueError, match='per-channel tensor quantised at %d bits' % bits):
        T.Dequantizer(4 if bits != 4 else 5)(qz, None)
    pz, _ = T.Quantizer(bits, packed=True, per_channel=True)(z.to(DEV), None)
    assert isinstance(pz, T.PackedBottleneck) and pz.per_channel and pz.shape == shape
    assert pz.nbytes == ref.payload.size and pz.link_bytes == pz.nbytes + 8 * 6
    assert torch.equal(pz.payload.cpu(), torch.from_numpy(ref.payload))
    # across the link: the payload, its shape and width, and the qparams; nothing of the head's buffers
    linked = T.PackedBottleneck(pz.payload.clone(), pz.shape, pz.num_bits, pz.qparams.clone(), per_channel=True)
    deq, _ = T.Dequantizer(bits)(linked, None)
    assert torch.equal(bits_of(deq), bits_of(ref.dequantized))
    fq = T.FakeQuantizer(bits, per_channel=True)
    out, _ = fq(z.to(DEV), None)
    assert torch.equal(bits_of(out), bits_of(ref.dequantized)) and torch.equal(bits_of(fq.qparams), bits_of(ref.qparams))
    assert float(out._hnd[..., 6:].abs().max()) == 0.0
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
def test_per_channel_split_gives_the_tail_the_floats_of_the_pair(tiny_student, bits):
    from hnd_ghnd_object_detectors_amd.models.mimic.split_rcnn import split_rcnn_model, split_rcnn_model_per_channel
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    student, ims = tiny_student
    layer1 = student.backbone.body.layer1
    saved = layer1.bottleneck_transformer, layer1.use_bottleneck_transformer
    try:
        layer1.bottleneck_transformer = T.Compose([T.Quantizer(bits, per_channel=True), T.Dequantizer(bits)])
        layer1.use_bottleneck_transformer = True
        with torch.no_grad():
            whole = {k: v.clone() for k, v in student(ims).items()}
    finally:
        layer1.bottleneck_transformer, layer1.use_bottleneck_transformer = saved
    with torch.no_grad():
        head, _ = split_rcnn_model(student, None)
        head.eval()
        z_plain = head(ims)[0].cpu().clone()              # the head's own unquantised z
    want = QC.restate(z_plain, bits)
    feats = {}
    for packed in (False, True):
        head, tail = split_rcnn_model_per_channel(student, bits, packed=packed)
        head.eval()
        tail.eval()
        tail.features_only = True
        with torch.no_grad():
            zq, tensors_shape, image_sizes, original_sizes = head(ims)
            assert zq.per_channel and torch.equal(bits_of(zq.qparams), bits_of(want.qparams))
            if packed:
                assert isinstance(zq, T.PackedBottleneck) and zq.link_bytes == zq.nbytes + 8 * z_plain.shape[1]
                emitted = CU.host_unpack(zq.payload.cpu().numpy(), zq.shape, bits)
                zq = T.PackedBottleneck(zq.payload.clone(), zq.shape, zq.num_bits, zq.qparams.clone(), per_channel=True)
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
    for name in ('fake_quantize_bits', 'qchannel_fake_quantize_bits'):
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
            layer1.train_fake_quant_per_channel = True
        if which == 'off':
            layer1.train_fake_quant_per_channel = False
        del launches[:], keywords[:]
        student(ims, tgs)
        ops.sync_check()
        eng = layer1.head_engine()
        zi = eng.encoder_len - 1
        assert zi == 3
        seen[which] = dict(launches=list(launches), keywords=list(keywords), key=eng.plan_key, z=eng.y[zi].clone(),
                           out=eng.out.clone(), qp=eng.fq[0].clone(), c=eng.layers[zi].cout)
    never, off, on = seen['never'], seen['off'], seen['on']
    assert all('fake_quant_per_channel' not in kw for kw in never['keywords'] + off['keywords'])
    assert any('fake_quant_per_channel' in kw for kw in on['keywords'])
    # the same launches, the same shape of plan key (its pointers belong to each student), the same y[3] and output
    assert never['launches'] == off['launches'] and 'fake_quantize_bits' in never['launches']
    assert 'qchannel_fake_quantize_bits' not in never['launches']
    def strip(key):                        # (input pointer, shape, training, parameter pointers, output pointer, width, ...)
        return len(key), key[1], key[2], key[5:]
    assert strip(never['key']) == strip(off['key']) and never['key'][-1] == bits
    assert torch.equal(bits_of(never['z']), bits_of(off['z'])) and torch.equal(bits_of(never['out']), bits_of(off['out']))
    assert tuple(never['qp'].shape) == (4,)
    # on: the per-channel launch in the per-tensor one's place, a key that says so, and the pair's bits
    assert on['launches'] == [t if t != 'fake_quantize_bits' else 'qchannel_fake_quantize_bits' for t in never['launches']]
    assert on['key'][-1] == 'per_channel' and len(on['key']) == len(never['key']) + 1
    c = on['c']
    assert tuple(on['qp'].shape) == (c, 4)
    assert not torch.equal(bits_of(on['z']), bits_of(never['z']))
    # the unquantised z of the same step: a student with the quantiser off
    plain = _student(cfg, s_sd)
    plain(ims, tgs)
    ops.sync_check()
    z_plain = plain.backbone.body.layer1.head_engine().y[3]
    want = QC.restate(CU.logical(z_plain, c).contiguous(), bits)
    assert torch.equal(bits_of(CU.logical(on['z'], c)), bits_of(want.dequantized))
    assert torch.equal(bits_of(on['qp']), bits_of(want.qparams))
    assert float(on['z'][..., c:].abs().max()) == 0.0


def test_engine_refuses_the_flag_with_a_fixed_range_and_a_non_bool(ops):
    from hnd_ghnd_object_detectors_amd import engine as E
    z, meta = G.load('tiny_ghnd_faster')
    cfg = MU.config_for(meta)
    _, s_sd = MU.oracle_states(meta['seed'], meta['model'], meta.get('bch', 3), meta.get('num_classes', 91))
    eng = _student(cfg, s_sd).backbone.body.layer1.head_engine()
    x = torch.zeros(1, 4, 4, 64, device=DEV)
    with pytest.raises(ValueError, match='HeadEngine.forward: fake_quant_per_channel=1 must be a bool'):
        eng.forward(x, True, fake_quant_bits=4, fake_quant_per_channel=1)
    rng = {'state': torch.zeros(4, device=DEV), 'momentum': 0.1, 'frozen': False, 'range': None}
    with pytest.raises(ValueError, match='fake_quant_per_channel together with fake_quant_range'):
        eng.forward(x, True, fake_quant_bits=4, fake_quant_range=rng, fake_quant_per_channel=True)
    assert isinstance(eng, E.HeadEngine) and eng.plan_key is None          # refused before a plan was built


# ------------------------------------------------------------------------------------------ one step vs the oracle
@pytest.mark.parametrize('name,bits', QC.ONE_STEP_CASES)
def test_one_step_with_the_per_channel_fake_quantiser_matches_the_straight_through_oracle(ops, name, bits, monkeypatch):
    """The bars are those tests/test_fake_quant_gpu.py applies to the per-tensor step (LOSS_TOL, _grad_check, its buffer
    bar), the reference being the fp64 oracle with a per-channel straight-through estimator (tests/qchannel_util.py).  The
    quantiser's rounding decisions are NOT masked out: per channel the oracle pair agrees on every one and keeps 1e-4 code
    units from every tie (also held on the CPU, tests/test_qchannel_cpu.py), and then the HIP path's codes must equal the
    oracle's everywhere.  Figures achieved on MI355X are printed."""
    z, meta = G.load(name)
    cfg, t_sd, s_sd, teacher, student, box, opt, warm = TM._setup(meta)
    layer1 = student.backbone.body.layer1
    layer1.train_fake_quant_bits = bits
    layer1.train_fake_quant_per_channel = True
    terms = MU.terms_of(cfg)
    images, targets = G.case_inputs(meta)
    ms = meta['min_size'] if isinstance(meta['min_size'], list) else [meta['min_size']]
    capture = {}

    def fq(zz):
        capture[zz.dtype] = QC.decide_codes_per_channel(zz.detach(), bits)
        return QC.ste_per_channel(zz, bits)
    monkeypatch.setattr(O, 'student_layer1', QU.make_student_layer1(bits, fake_quant=fq))
    kw = dict(terms=terms, min_size=tuple(ms), max_size=meta['max_size'])
    orc64 = O.DistillOracle(t_sd, s_sd, dtype=torch.float64, **kw)
    orc32 = O.DistillOracle(t_sd, s_sd, **kw)
    TM._sync_oracle(orc64, student)
    TM._sync_oracle(orc32, student)
    loss64, terms64, g64, _ = orc64.step(images)
    _, _, g32, _ = orc32.step(images)
    caps32, caps64 = capture[torch.float32], capture[torch.float64]
    QC.check_preconditions_per_channel(caps32, caps64, '%s at %d bits' % (name, bits))

    ims, tgs = TM._to_dev(images, targets)
    loss = box(ims, tgs)
    worst = {'loss': abs(loss.item() - loss64) / abs(loss64), 'grad': 0.0, 'buffer': 0.0}
    per_term = loss.per_term.cpu()
    for i, k in enumerate(terms):
        worst['loss'] = max(worst['loss'], abs(float(per_term[i]) - terms64[k]) / abs(terms64[k]))
    opt.zero_grad()
    loss.backward()
    ops.sync_check()
    # the quantiser's decisions, recovered per channel from the stored values: q = z' / scale + zero_point
    eng = layer1.head_engine()
    assert eng.fq_per_channel
    c = eng.layers[3].cout
    qp = eng.fq[0].cpu().double()
    assert tuple(qp.shape) == (c, 4) == (len(caps64), 4)
    zq = eng.bottleneck().cpu()[..., :c].permute(0, 3, 1, 2).double()
    differ = total = 0
    for ch in range(c):
        recovered = zq[:, ch:ch + 1] / qp[ch, 2] + qp[ch, 3]
        codes = torch.round(recovered)
        assert float((recovered - codes).abs().max()) < 1e-3 and float(qp[ch, 3]) == caps64[ch]['zero_point'], ch
        differ += int((codes != caps64[ch]['codes'].double()).sum())
        total += codes.numel()
    print('\n[%s, %d bits, per channel] loss %.2e; codes differing from the oracle: %d of %d' % (name, bits, worst['loss'],
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
    print('[%s, %d bits, per channel] worst: loss %.2e (tol %.0e), grads vs fp64 %.2e (%.0e or 2x torch-fp32), decoder.0 '
          'buffers %.2e (1e-4)' % (name, bits, worst['loss'], TM.LOSS_TOL, worst['grad'], TM.GRAD_TOL, worst['buffer']))
