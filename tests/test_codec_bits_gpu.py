"""GPU: the bottleneck codec at 1 ... 8 bits and its bit-packed link payload (include/hnd_codec.h) against the restated
myutils tensor_util (oracle/myutils_r.py), the reference-made fixture tests/golden/tiny_codec_bits.npz, and the payload
format of the header restated with numpy.packbits (tests/codec_util.py).

Byte work: every comparison is torch.equal or ==, no tolerance anywhere -- the bar of
tests/test_ops_gpu.py::test_bottleneck_codec_matches_myutils_semantics (identical correctly rounded fp32 operations in the
reference's order).  Inputs have max > min (a constant tensor divides by a zero scale in the reference too)."""
import pytest
import torch

from tests import codec_util as CU
from tests import golden_util as G
from tests import model_util as MU

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# (n, c, h, w): 3 values, only a tail group | 105 values, a tail of one | 1326 values, a tail of six, a pad channel |
# 96 values, no tail, cs = 8 | 151 200 values, c = 12 | the b3ch extent at batch 4: several passes of the grid-stride loop
SMALL = [(1, 3, 1, 1), (1, 3, 5, 7), (2, 3, 13, 17), (1, 6, 4, 4), (3, 12, 50, 84)]
B3CH = (4, 3, 204, 340)
SHIFTS = [0.3, 5.0]
CASES = [(shape, shift, bits) for shape in SMALL for shift in SHIFTS for bits in range(1, 9)] + \
        [(B3CH, shift, bits) for shift in SHIFTS for bits in (1, 4, 7)]
IDS = ['%s-shift%s-b%d' % ('x'.join(map(str, s)), sh, b) for s, sh, b in CASES]


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


def _stride(ops, shape):
    """the engine's pixel stride for c channels, except cs = 8 for the 6-channel case: a stride the engine does not lay out
    but the ABI takes (any cs >= c), with two pad channels that are no multiple of the group of eight"""
    return 8 if shape[1] == 6 else ops.chan_pad_of(shape[1])


def _buffers(ops, shape):
    return _stride(ops, shape), torch.empty(4, device=DEV), torch.empty(ops.minmax_scratch_elems(), device=DEV)


def _check_qparams(qp, z, ref):
    lo, hi, scale, zp = [float(v) for v in qp.cpu()]
    assert lo == float(z.min()) and hi == float(z.max())
    assert scale == ref.scale and zp == ref.zero_point


# ------------------------------------------------------------------------------------------ the three exports
@pytest.mark.parametrize('shape,shift,bits', CASES, ids=IDS)
def test_quantize_bits_matches_myutils_at_every_width(ops, shape, shift, bits):
    n, c, h, w = shape
    z, ref = CU.make_input(shape, shift), CU.reference(shape, shift, bits)
    cs, qp, scratch = _buffers(ops, shape)
    buf = CU.nhwc_buffer(z, cs, DEV)
    q = torch.full(buf.shape, 0xAA, dtype=torch.uint8, device=DEV)
    ops.quantize_bits(buf, c, bits, q, qp, scratch)
    out = torch.full(buf.shape, float('nan'), device=DEV)
    ops.dequantize_u8(q, qp, out, c)                     # the 8-bit export inverts every width: the width is in the scale
    ops.sync_check()
    _check_qparams(qp, z, ref)
    got = CU.logical(q, c)
    assert torch.equal(got, ref.bytes), 'quantised bytes differ in %d places' % int((got != ref.bytes).sum())
    if cs != c:
        assert int(q[..., c:].max()) == 0
    assert torch.equal(CU.logical(out, c), ref.dequantized)
    if bits == 8:                                         # the bytes and qparams of hnd_quantize_u8
        q8, qp8 = torch.empty_like(q), torch.empty_like(qp)
        ops.quantize_u8(buf, c, q8, qp8, scratch)
        ops.sync_check()
        assert torch.equal(q8, q) and torch.equal(qp8, qp)


@pytest.mark.parametrize('shape,shift,bits', CASES, ids=IDS)
def test_quantize_pack_bits_writes_the_payload_format_of_the_header(ops, shape, shift, bits):
    n, c, h, w = shape
    z, ref = CU.make_input(shape, shift), CU.reference(shape, shift, bits)
    cs, qp, scratch = _buffers(ops, shape)
    buf = CU.nhwc_buffer(z, cs, DEV)
    nbytes = ops.codec_packed_bytes(z.numel(), bits)
    assert nbytes == (z.numel() * bits + 7) // 8 == ref.payload.size
    payload = torch.full((nbytes,), 0xAA, dtype=torch.uint8, device=DEV)
    ops.quantize_pack_bits(buf, c, bits, payload, qp, scratch)
    ops.sync_check()
    _check_qparams(qp, z, ref)
    got = payload.cpu().numpy()
    assert got.tobytes() == ref.payload.tobytes(), 'payload differs in %d of %d bytes' % (
        int((got != ref.payload).sum()), nbytes)


@pytest.mark.parametrize('shape,shift,bits', CASES, ids=IDS)
def test_unpack_dequantize_bits_restores_the_oracle_floats_and_clears_the_pad(ops, shape, shift, bits):
    n, c, h, w = shape
    ref = CU.reference(shape, shift, bits)
    cs = _stride(ops, shape)
    payload = torch.from_numpy(ref.payload.copy()).to(DEV)
    qp = torch.tensor([ref.lo, ref.hi, ref.scale, ref.zero_point], dtype=torch.float32, device=DEV)
    out = torch.full((n, h, w, cs), float('nan'), device=DEV)
    ops.unpack_dequantize_bits(payload, qp, out, c, bits)
    ops.sync_check()
    assert not bool(torch.isnan(out).any())
    assert torch.equal(CU.logical(out, c), ref.dequantized)
    if cs != c:
        assert float(out[..., c:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ the reference-made fixture
@pytest.mark.parametrize('bits', range(1, 8))
def test_quantizer_reproduces_the_reference_at_every_width(ops, bits):
    """Quantizer(b) / Quantizer(b, packed=True) fed the REFERENCE's own bottleneck tensor emit exactly the bytes (packed:
    after a host unpack), scale, zero point and dequantised floats the reference's Quantizer(b) / Dequantizer(b) emitted"""
    from hnd_ghnd_object_detectors_amd.structure.transformer import Dequantizer, PackedBottleneck, QuantizedTensor, \
        Quantizer
    fix = G.load_raw('tiny_codec_bits')
    z_ref = torch.from_numpy(G.load_raw('tiny_eval_quantized')['quantized/z'])
    want = {k: torch.from_numpy(fix['b%d/%s' % (bits, k)]) for k in ('bytes', 'dequantized')}
    scale, zero_point = float(fix['b%d/scale' % bits]), float(fix['b%d/zero_point' % bits])
    qz, _ = Quantizer(bits)(z_ref.to(DEV), None)
    assert isinstance(qz, QuantizedTensor) and qz.tensor.dtype == torch.uint8
    assert torch.equal(qz.tensor.cpu(), want['bytes'])
    assert float(qz.scale) == scale and float(qz.zero_point) == zero_point
    deq, _ = Dequantizer(bits)(qz, None)
    assert torch.equal(deq.cpu(), want['dequantized'])
    pz, _ = Quantizer(bits, packed=True)(z_ref.to(DEV), None)
    assert isinstance(pz, PackedBottleneck) and pz.payload.dtype == torch.uint8 and pz.payload.dim() == 1
    assert pz.shape == tuple(z_ref.shape) and pz.num_bits == bits
    assert pz.nbytes == pz.payload.numel() == (z_ref.numel() * bits + 7) // 8
    assert torch.equal(CU.host_unpack(pz.payload.cpu().numpy(), pz.shape, bits), want['bytes'])
    assert float(pz.scale) == scale and float(pz.zero_point) == zero_point
    assert pz.scale.dim() == 0 and pz.scale.device.type == 'cuda'
    # across the link: the payload, its shape and width, and the qparams; nothing of the head's buffers
    linked = PackedBottleneck(pz.payload.clone(), pz.shape, pz.num_bits, pz.qparams.clone(), origin=None)
    deq, _ = Dequantizer(bits)(linked, None)
    assert torch.equal(deq.cpu(), want['dequantized'])
    with pytest.raises(ValueError, match='packed at %d bits' % bits):
        Dequantizer(8 if bits != 8 else 4)(linked, None)


# ------------------------------------------------------------------------------------------ classes and the split
@pytest.fixture(scope='module')
def tiny_student():
    """the tiny student of tiny_eval_quantized (tests/test_model_gpu.py::test_head_tail_split_matches_reference_golden)"""
    _, meta = G.load('tiny_eval_quantized')
    cfg = MU.config_for(meta)
    t_sd, s_sd = MU.oracle_states(meta['seed'])
    for k in list(s_sd):
        if 'layer1' in k and k.endswith('running_var'):
            s_sd[k] = s_sd[k] * 1.7 + 0.1
        if 'layer1' in k and k.endswith('running_mean'):
            s_sd[k] = s_sd[k] + 0.05
    _, student = MU.build_pair(cfg, t_sd, s_sd, DEV)
    student.eval()
    images, _ = G.case_inputs(meta)
    return student, [im.to(DEV) for im in images]


@pytest.mark.parametrize('bits', [2, 4, 8])
def test_packed_split_unpacked_split_and_unsplit_model_agree_bit_for_bit(tiny_student, bits):
    from oracle.myutils_r import quantize_tensor
    from hnd_ghnd_object_detectors_amd.models.mimic.split_rcnn import split_rcnn_model
    from hnd_ghnd_object_detectors_amd.structure.transformer import Compose, Dequantizer, PackedBottleneck, \
        QuantizedTensor, Quantizer
    student, ims = tiny_student
    layer1 = student.backbone.body.layer1
    saved = layer1.bottleneck_transformer, layer1.use_bottleneck_transformer
    try:
        layer1.bottleneck_transformer = Compose([Quantizer(bits), Dequantizer(bits)])
        layer1.use_bottleneck_transformer = True
        with torch.no_grad():
            whole = {k: v.clone() for k, v in student(ims).items()}
    finally:
        layer1.bottleneck_transformer, layer1.use_bottleneck_transformer = saved
    with torch.no_grad():
        head, _ = split_rcnn_model(student, None)
        head.eval()
        z_plain = head(ims)[0].cpu().clone()              # the head's own unquantised z
    want = quantize_tensor(z_plain.clone(), bits)
    feats = {}
    for packed in (False, True):
        head, tail = split_rcnn_model(student, bits, packed=packed)
        head.eval()
        tail.eval()
        tail.features_only = True
        with torch.no_grad():
            zq, tensors_shape, image_sizes, original_sizes = head(ims)
            if packed:
                assert isinstance(zq, PackedBottleneck) and zq.shape == tuple(z_plain.shape)
                assert zq.nbytes == (z_plain.numel() * bits + 7) // 8 == zq.payload.numel()
                emitted = CU.host_unpack(zq.payload.cpu().numpy(), zq.shape, bits)
                zq = PackedBottleneck(zq.payload.clone(), zq.shape, zq.num_bits, zq.qparams.clone(), origin=None)
            else:
                assert isinstance(zq, QuantizedTensor) and zq.tensor.dtype == torch.uint8
                emitted = zq.tensor.cpu()
                zq = QuantizedTensor(zq.tensor, zq.scale, zq.zero_point, zq.qparams.clone(), origin=None,
                                     channels=zq.channels)
            assert torch.equal(emitted, want.tensor)
            assert float(zq.scale) == float(want.scale) and float(zq.zero_point) == float(want.zero_point)
            feats[packed] = {k: v.clone() for k, v in tail(zq, tensors_shape, image_sizes, original_sizes).items()}
    assert list(feats[True]) == list(feats[False]) == list(whole)
    for k in whole:
        assert torch.equal(feats[True][k], feats[False][k]) and torch.equal(feats[False][k], whole[k]), k


def test_data_logger_at_four_bits_records_the_byte_tensor_not_a_half_tensor():
    """reference :84-85: the quantised size is that of quantize_tensor(z, num_bits)'s pickle, a uint8 tensor at any width"""
    from oracle import myutils_r as MR
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    z = torch.randn(1, 3, 51, 68, generator=torch.Generator().manual_seed(3)) * 2.0 + 0.3
    log = T.DataLogger(4)
    same, _ = log(z.to(DEV), None)
    sizes, fp16, quant, shapes = log.get_data()
    assert torch.equal(same.cpu(), z) and shapes == [[3, 51, 68]]
    kb = z.numel() / 1024                                 # one byte per value + the pickle's header
    assert kb < quant[0] < kb + 1.5 and quant[0] < MR.get_binary_object_size(z.half()) / 1.5
    assert abs(quant[0] - MR.get_binary_object_size(MR.quantize_tensor(z.clone(), 4))) < 0.5
