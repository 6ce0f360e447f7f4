"""GPU: the entropy-coded link payload (include/hnd_entropy.h) against the numpy restatement of the header
(tests/entropy_util.py) and against the existing codec.

Byte work: the histogram equals numpy.bincount, offsets and payload[0 : nbytes] equal the numpy encoder byte for byte, and
what the decoder returns has the bits Dequantizer returns on the plain Quantizer(b) of the same tensor, zeros in the pad
channels included.  No tolerance anywhere.  Only valid streams reach a kernel."""
import numpy as np
import pytest
import torch

from tests import entropy_util as EU
from tests import golden_util as G
from tests import model_util as MU

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
WIDTHS = [1, 2, 4, 8]
CASES = [(shape, bits) for shape in EU.SHAPES for bits in WIDTHS]
IDS = ['%s-b%d' % ('x'.join(map(str, s)), b) for s, b in CASES]


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need a device'
    from hnd_ghnd_object_detectors_amd import ops as o
    assert 'gfx950' in o.device_arch(), o.device_arch()
    return o


def bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def device_input(shape):
    """the logical tensor on the device, attached to an NHWC buffer of the stride the case asks for"""
    from hnd_ghnd_object_detectors_amd.hipnn import attach
    from tests.codec_util import nhwc_buffer
    z = shape if torch.is_tensor(shape) else EU.make_input(shape)
    buf = nhwc_buffer(z, EU.stride_of(z.shape), DEV)
    return attach(buf[..., :z.shape[1]].permute(0, 3, 1, 2), buf)


def plain_round_trip(z, bits, static_range=None):
    """(codes one per byte NHWC, dequantised NHWC buffer incl. pad channels) of the existing Quantizer(b) / Dequantizer(b)"""
    from hnd_ghnd_object_detectors_amd.structure.transformer import Dequantizer, Quantizer
    qz, _ = Quantizer(bits, static_range=static_range)(device_input(z), None)
    codes = qz.tensor._hnd.clone()
    deq, _ = Dequantizer(bits)(qz, None)
    return codes, deq._hnd.clone()


def check_stream(eb, codes, c):
    """the EntropyBottleneck against the numpy encoder of the same codes and table; returns the stream's byte count"""
    symbols = EU.logical_codes(codes, c)
    payload, offsets = EU.encode(symbols, eb.lengths)
    got_offsets = eb.offsets.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_offsets, offsets), (got_offsets.tolist()[:8], offsets.tolist()[:8])
    assert eb.nbytes == int(offsets[-1]) == payload.size
    got = eb.payload[:eb.nbytes].cpu().numpy()
    assert got.tobytes() == payload.tobytes(), 'payload differs in %d of %d bytes' % (int((got != payload).sum()), payload.size)
    assert eb.payload.numel() == EU.capacity(symbols.size)
    assert eb.link_bytes == EU.link_bytes(eb.nbytes, symbols.size, eb.num_bits)
    assert np.array_equal(EU.decode(got, got_offsets, eb.lengths, symbols.size), symbols)
    return eb.nbytes


def across_the_link(eb):
    """what the tail receives: the stream's bytes alone, the offsets, the table, the qparams; nothing of the head's buffers"""
    from hnd_ghnd_object_detectors_amd.structure.transformer import EntropyBottleneck
    return EntropyBottleneck(eb.payload[:eb.nbytes].clone(), eb.offsets.clone(), bytes(eb.lengths), eb.shape, eb.num_bits,
                             eb.qparams.clone(), origin=None)


def decoded(eb, cs):
    """the decoder's NHWC buffer, pad channels included, pre-filled with NaN"""
    from hnd_ghnd_object_detectors_amd import ops as o
    n, c, h, w = eb.shape
    out = torch.full((n, h, w, cs), float('nan'), device=DEV)
    o.entropy_decode_dequantize(eb.payload, eb.offsets, eb.lengths, eb.qparams, out, c, eb.num_bits)
    o.sync_check()
    return out


# ------------------------------------------------------------------------------------------ the exports
@pytest.mark.parametrize('shape,bits', CASES, ids=IDS)
def test_histogram_equals_bincount(ops, shape, bits):
    codes, _ = plain_round_trip(shape, bits)
    hist = torch.full((256,), -1, dtype=torch.int32, device=DEV)
    ops.code_histogram(codes, shape[1], bits, hist)
    ops.sync_check()
    want = np.bincount(EU.logical_codes(codes, shape[1]), minlength=256)
    assert np.array_equal(hist.cpu().numpy(), want) and not want[1 << bits:].any()


@pytest.mark.parametrize('shape,bits', CASES, ids=IDS)
def test_stream_is_the_header_s_and_decodes_to_the_plain_codec_s_bits(ops, shape, bits):
    from hnd_ghnd_object_detectors_amd.structure.transformer import Dequantizer, EntropyBottleneck, Quantizer
    c, cs = shape[1], EU.stride_of(shape)
    codes, want = plain_round_trip(shape, bits)
    eb, _ = Quantizer(bits, entropy=True)(device_input(shape), None)
    assert isinstance(eb, EntropyBottleneck) and eb.shape == tuple(shape) and eb.num_bits == bits
    assert eb.scale.dim() == 0 and eb.scale.device.type == 'cuda'
    check_stream(eb, codes, c)
    linked = across_the_link(eb)
    assert torch.equal(bits_of(decoded(linked, cs)), bits_of(want))              # zeros in the pad channels included
    deq, _ = Dequantizer(bits)(linked, None)
    assert torch.equal(bits_of(deq), bits_of(want[..., :c].permute(0, 3, 1, 2)))
    with pytest.raises(ValueError, match='entropy-coded at %d bits' % bits):
        Dequantizer(8 if bits != 8 else 4)(linked, None)


@pytest.mark.parametrize('shape,bits', CASES, ids=IDS)
def test_the_same_holds_on_a_static_range_and_with_a_fixed_table(ops, shape, bits):
    from hnd_ghnd_object_detectors_amd.structure.transformer import Quantizer
    c, cs = shape[1], EU.stride_of(shape)
    rng = [-1.5, 2.75]                                                           # clips both tails of the normal input
    codes, want = plain_round_trip(shape, bits, static_range=rng)
    eb, _ = Quantizer(bits, static_range=rng, entropy=True)(device_input(shape), None)
    check_stream(eb, codes, c)
    assert torch.equal(bits_of(decoded(across_the_link(eb), cs)), bits_of(want))
    # a complete fixed table: no histogram, no read-back; Kraft sum 1 at every width, lengths not monotone in the symbol at 4
    table = {1: [1, 1], 2: [1, 2, 3, 3], 4: [5] * 4 + [3] * 4 + [4] * 4 + [5] * 4, 8: [9] * 64 + [7] * 32 + [8] * 160}[bits]
    assert EU.kraft(table) == 1 << 12
    codes, want = plain_round_trip(shape, bits)
    eb, _ = Quantizer(bits, entropy=True, code_lengths=table)(device_input(shape), None)
    assert eb.lengths == bytes(table)
    check_stream(eb, codes, c)
    assert torch.equal(bits_of(decoded(across_the_link(eb), cs)), bits_of(want))


@pytest.mark.parametrize('code,rng', [(0, [100.0, 1.0e6]), (15, [-1.0e6, -100.0])], ids=['low', 'high'])
def test_one_symbol_tensor_gets_one_bit_per_value(ops, code, rng):
    """a static_range far to one side of the values clips everything to one end (max == min is undefined in the codec): the
    zero point is that end and no value moves the code by half a step of 66 660: one code of length 1"""
    from hnd_ghnd_object_detectors_amd.structure.transformer import Quantizer
    shape, bits = (2, 3, 7, 13), 4
    codes, want = plain_round_trip(shape, bits, static_range=rng)
    assert set(EU.logical_codes(codes, 3).tolist()) == {code}
    eb, _ = Quantizer(bits, static_range=rng, entropy=True)(device_input(shape), None)
    assert sum(eb.lengths) == 1 and eb.lengths[code] == 1
    assert check_stream(eb, codes, 3) == 32 + 32 + 5                             # 256, 256 and 34 symbols of one bit
    assert torch.equal(bits_of(decoded(across_the_link(eb), 4)), bits_of(want))


def test_geometric_histogram_exercises_the_longest_codes(ops):
    from hnd_ghnd_object_detectors_amd.structure.transformer import Quantizer
    z, bits, rng = EU.geometric_input(), 4, [0.0, 15.0]
    codes, want = plain_round_trip(z, bits, static_range=rng)
    assert np.bincount(EU.logical_codes(codes, 2), minlength=16).tolist() == EU.GEOMETRIC_HIST
    eb, _ = Quantizer(bits, static_range=rng, entropy=True)(device_input(z), None)
    assert max(eb.lengths) == 12 and min(eb.lengths) == 1
    check_stream(eb, codes, 2)
    sizes = np.diff(eb.offsets.cpu().numpy().view(np.uint32).astype(np.int64))
    assert sizes.min() >= 32 and sizes.max() <= 384 and sizes.max() > 2 * sizes.min()
    assert torch.equal(bits_of(decoded(across_the_link(eb), 4)), bits_of(want))


# ------------------------------------------------------------------------------------------ the split model
@pytest.fixture(scope='module')
def tiny_student():
    """the tiny student of tiny_eval_quantized, as tests/test_codec_bits_gpu.py builds it"""
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
def test_entropy_split_gives_the_detections_of_the_plain_split(tiny_student, bits):
    from hnd_ghnd_object_detectors_amd.models.mimic.split_rcnn import split_rcnn_model, split_rcnn_model_entropy
    from hnd_ghnd_object_detectors_amd.structure.transformer import EntropyBottleneck
    student, ims = tiny_student
    results = {}
    for name, split in (('plain', split_rcnn_model), ('entropy', split_rcnn_model_entropy)):
        head, tail = split(student, bits)
        head.eval()
        tail.eval()
        with torch.no_grad():
            zq, tensors_shape, image_sizes, original_sizes = head(ims)
            if name == 'entropy':
                assert isinstance(zq, EntropyBottleneck)
                assert 0 < zq.nbytes <= zq.payload.numel() and zq.link_bytes > zq.nbytes
                zq = across_the_link(zq)
            results[name] = [{k: v.clone() for k, v in det.items()} for det in
                             tail(zq, tensors_shape, image_sizes, original_sizes)]
    assert len(results['plain']) == len(results['entropy']) == len(ims)
    for a, b in zip(results['plain'], results['entropy']):
        assert list(a) == list(b)
        for k in a:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
