"""GPU: per-image entropy streams (include/hnd_istream.h and the layers above it).  Every comparison is bit-exact: the
histograms against numpy.bincount, the device-built tables against transformer.huffman_lengths, every image's stream against
the numpy encoder of tests/entropy_util.py AND against the merged per-tensor export on that image alone, the decoder against
ops.qimage_dequantize_u8 on the same codes, image(i) through the existing Dequantizer, batch invariance, repeatability, the
fixed table and the split model.  Each case runs the exports once (run_case) and the tests compare; well-formed inputs only."""
import numpy as np
import pytest
import torch

from tests import entropy_util as EU
from tests import golden_util as G
from tests import istream_util as IU
from tests import model_util as MU

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U8, I32, F32 = torch.uint8, torch.int32, torch.float32
CLASS_CASES = [((3, 3, 5, 7), 3), ((2, 5, 9, 31), 8), (IU.SPECIAL[0], 8), (IU.SPECIAL[0], 2)]


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
    _RUNS.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def source(z, cs):
    """device NHWC buffer of stride cs: the real channels of z, garbage in the pad channels"""
    n, c, h, w = z.shape
    buf = torch.full((n, h, w, cs), 1.0e6)
    buf[..., :c] = z.permute(0, 2, 3, 1)
    return buf.to(DEV)


def filled(shape, dtype, byte=0xAB):
    return torch.full(shape, float('nan'), device=DEV) if dtype == F32 else \
        torch.full((int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size(),), byte, dtype=U8,
                   device=DEV).view(dtype).view(shape)


_RUNS = {}


def run_case(ops, shape, cs, bits):
    """the four exports on the case's input, once: dict of host copies (q, qp, hist, lengths, payload, offsets, x) and the
    per-image symbols; the device buffers start poisoned"""
    key = (tuple(shape), cs, bits)
    if key in _RUNS:
        return _RUNS[key]
    n, c, h, w = shape
    chw = c * h * w
    cpi = ops.istream_chunks_per_image(chw)
    x = source(IU.make_input(shape), cs)
    q, qp = filled(x.shape, U8), filled((n, 4), F32)
    ops.qimage_quantize_bits(x, c, bits, q, qp, torch.empty(ops.qimage_scratch_elems(n), device=DEV))
    hist, lengths = filled((n, 256), I32), filled((n, 256), U8)
    payload = filled((ops.istream_capacity(n, chw),), U8)
    offsets, scratch = filled((n * cpi + 1,), I32), filled((n * cpi,), I32)
    ops.istream_histogram(q, c, bits, hist)
    ops.istream_build_tables(hist, bits, lengths)
    ops.istream_encode(q, c, bits, lengths, payload, offsets, scratch)
    out = ops.istream_decode_dequantize(payload, offsets, lengths, qp, filled(x.shape, F32), c, bits)
    want = ops.qimage_dequantize_u8(q, qp, filled(x.shape, F32), c)
    ops.sync_check()
    r = dict(n=n, c=c, chw=chw, cpi=cpi, q_dev=q, qp_dev=qp, lengths_dev=lengths,
             q=q.cpu().numpy(), qp=qp.cpu(), hist=hist.cpu().numpy(), lengths=lengths.cpu().numpy(),
             payload=payload.cpu().numpy(), offsets=offsets.cpu().numpy().view(np.uint32), sizes=scratch.cpu().numpy(),
             x=out.cpu(), want_x=want.cpu())
    r['symbols'] = IU.image_symbols(r['q'], c)
    _RUNS[key] = r
    return r


def segment(r, i):
    """(payload bytes, rebased offsets) of image i"""
    offs = r['offsets'][i * r['cpi']:(i + 1) * r['cpi'] + 1].astype(np.int64)
    return r['payload'][offs[0]:offs[-1]], (offs - offs[0]).astype(np.uint32)


# ------------------------------------------------------------------------------------------ (1) the exports
@pytest.mark.parametrize('shape,cs,bits', IU.CASES, ids=IU.CASE_IDS)
def test_histogram_counts_every_image_s_real_codes_and_nothing_else(ops, shape, cs, bits):
    r = run_case(ops, shape, cs, bits)
    n, c, nsym = r['n'], r['c'], 1 << bits
    for i in range(n):
        assert np.array_equal(r['hist'][i], np.bincount(r['symbols'][i], minlength=256)), i
    # garbage in the pad bytes and, in the real channels, some bytes at or above 2^bits: counted nowhere
    rng = np.random.RandomState(5)
    q = r['q'].copy()
    q[..., c:] = rng.randint(0, 256, size=q[..., c:].shape)
    if bits < 8:
        flat = q[..., :c].reshape(n, -1).copy()
        for i in range(n):
            where = rng.permutation(flat.shape[1])[:max(1, flat.shape[1] // 7)]
            flat[i, where] = rng.randint(nsym, 256, size=where.size)
        q[..., :c] = flat.reshape(q[..., :c].shape)
    hist = filled((n, 256), I32)
    ops.istream_histogram(torch.from_numpy(q).to(DEV), c, bits, hist)
    ops.sync_check()
    for i, sym in enumerate(IU.image_symbols(q, c)):
        assert np.array_equal(hist[i].cpu().numpy(), np.bincount(sym[sym < nsym], minlength=256)), i


@pytest.mark.parametrize('shape,cs,bits', IU.CASES, ids=IU.CASE_IDS)
def test_device_built_tables_are_the_host_routine_s_byte_for_byte(ops, shape, cs, bits):
    from hnd_ghnd_object_detectors_amd.structure.transformer import huffman_lengths
    r = run_case(ops, shape, cs, bits)
    for i in range(r['n']):
        want = huffman_lengths(r['hist'][i].tolist(), bits)
        assert r['lengths'][i, :1 << bits].tobytes() == want, (i, r['lengths'][i, :1 << bits].tolist(), list(want))
        assert not r['lengths'][i, 1 << bits:].any()
    if tuple(shape) == IU.SPECIAL[0]:
        assert sorted(np.flatnonzero(r['hist'][1])) in ([0], [1]) and r['lengths'][1].sum() == 1         # the constant image
        assert np.count_nonzero(r['hist'][2]) == 2 and sorted(r['lengths'][2][r['lengths'][2] > 0]) == [1, 1]
        if bits == 8:       # the skewed image: the unconstrained tree is deeper than 12, so the limit binds
            assert r['hist'][3].tolist() == IU.skewed_histogram()
            assert max(EU.heap_huffman_depths(r['hist'][3].tolist()).values()) > 12 and r['lengths'][3].max() == 12


@pytest.mark.parametrize('shape,cs,bits', IU.CASES, ids=IU.CASE_IDS)
def test_every_image_s_stream_is_the_numpy_encoder_s_and_the_merged_export_s(ops, shape, cs, bits):
    r = run_case(ops, shape, cs, bits)
    n, c, chw, cpi = r['n'], r['c'], r['chw'], r['cpi']
    assert int(r['offsets'][0]) == 0 and cpi == EU.chunks(chw)
    assert np.array_equal(np.diff(r['offsets'].astype(np.int64)), r['sizes'])
    assert (r['payload'][int(r['offsets'][-1]):] == 0xAB).all()                   # nothing at or beyond the end is written
    cap, words = ops.entropy_capacity(chw), ops.entropy_chunks(chw)
    for i in range(n):
        table = r['lengths'][i, :1 << bits].tobytes()
        got_payload, got_offsets = segment(r, i)
        want_payload, want_offsets = EU.encode(r['symbols'][i], table)
        assert np.array_equal(got_offsets, want_offsets), i
        assert got_payload.tobytes() == want_payload.tobytes(), i
        assert np.array_equal(EU.decode(got_payload, got_offsets, table, chw), r['symbols'][i]), i
        # the merged coder on q[i:i+1] under the same table
        payload, offsets, scratch = filled((cap,), U8), filled((words + 1,), I32), filled((words,), I32)
        alone = r['q_dev'][i:i + 1].clone()                 # a buffer of its own: the image may begin off the 16-byte grid
        ops.entropy_encode(alone, c, bits, table, payload, offsets, scratch)
        ops.sync_check()
        assert np.array_equal(offsets.cpu().numpy().view(np.uint32), got_offsets), i
        assert payload.cpu().numpy()[:got_payload.size].tobytes() == got_payload.tobytes(), i
        if n == 1:          # the whole output, unwritten bytes included
            assert np.array_equal(payload.cpu().numpy(), r['payload']) and np.array_equal(scratch.cpu().numpy(), r['sizes'])


@pytest.mark.parametrize('shape,cs,bits', IU.CASES, ids=IU.CASE_IDS)
def test_decoder_gives_the_floats_of_the_per_image_dequantiser(ops, shape, cs, bits):
    r = run_case(ops, shape, cs, bits)
    assert torch.equal(bits_of(r['x']), bits_of(r['want_x']))
    assert not torch.isnan(r['x']).any() and float(r['x'][..., r['c']:].abs().max() if cs > r['c'] else 0.0) == 0.0
    # payload cut to its stream: the decoder reads nothing beyond payload_bytes
    n, c = r['n'], r['c']
    cut = torch.from_numpy(r['payload'][:max(int(r['offsets'][-1]), 1)].copy()).to(DEV)
    out = ops.istream_decode_dequantize(cut, torch.from_numpy(r['offsets'].view(np.int32)).to(DEV), r['lengths_dev'],
                                        r['qp_dev'], filled(r['x'].shape, F32), c, bits)
    ops.sync_check()
    assert torch.equal(bits_of(out), bits_of(r['want_x']))


# ------------------------------------------------------------------------------------------ (2) the classes
@pytest.mark.parametrize('shape,bits', CLASS_CASES)
def test_quantizer_emits_self_contained_messages_the_existing_dequantizer_takes(ops, shape, bits):
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    z = IU.make_input(shape)
    n, c, h, w = shape
    chw = c * h * w
    per_image, _ = T.Quantizer(bits, per_image=True)(z.to(DEV), None)
    want, _ = T.Dequantizer(bits)(per_image, None)
    want, want_qp = want.cpu().clone(), per_image.qparams.cpu().clone()
    sb, tgt = T.ImageStreamQuantizer(bits)(z.to(DEV), 'target')
    assert tgt == 'target' and isinstance(sb, T.ImageStreamBottleneck) and sb.shape == shape and sb.num_bits == bits
    assert sb.lengths.device.type == 'cuda' and tuple(sb.lengths.shape) == (n, 256) and sb.lengths.dtype == U8
    assert sb.chunks_per_image == EU.chunks(chw) and sb.offsets.numel() == n * sb.chunks_per_image + 1
    assert torch.equal(bits_of(sb.qparams), bits_of(want_qp)) and sb.scale.data_ptr() == sb.qparams.data_ptr() + 8
    assert sb.payload.numel() == n * EU.capacity(chw) and sum(sb.image_nbytes) == sb.nbytes
    assert sb.link_bytes == sum(IU.image_link_bytes(b, chw, bits) for b in sb.image_nbytes)
    messages = [sb.image(i) for i in range(n)]
    deq, _ = T.Dequantizer(bits)(T.ImageStreamBottleneck(sb.payload.clone(), sb.offsets.clone(), sb.lengths.clone(), sb.shape,
                                                         bits, sb.qparams.clone()), None)
    assert torch.equal(bits_of(deq), bits_of(want))
    with pytest.raises(ValueError, match='per-image streams entropy-coded at %d bits' % bits):
        T.Dequantizer(4 if bits != 4 else 5)(sb, None)
    for i, eb in enumerate(messages):                       # each alone, through the per-tensor path
        assert isinstance(eb, T.EntropyBottleneck) and eb.shape == (1, c, h, w) and eb.payload.data_ptr() % 16 == 0
        assert eb.link_bytes == sb.image_link_bytes[i] and isinstance(eb.lengths, bytes)
        one, _ = T.Dequantizer(bits)(eb, None)
        assert torch.equal(bits_of(one), bits_of(want[i:i + 1])), i
    ops.sync_check()


@pytest.mark.parametrize('shape,bits', CLASS_CASES)
def test_an_image_alone_gives_the_bytes_of_its_segment_in_any_batch_and_calls_repeat(ops, shape, bits):
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    z = IU.make_input(shape)
    n = shape[0]
    quantizer = T.ImageStreamQuantizer(bits)

    def host(sb):
        cpi, offs = sb.chunks_per_image, sb.offsets.cpu().numpy().view(np.uint32).astype(np.int64)
        payload, lengths, qp = sb.payload.cpu().numpy(), sb.lengths.cpu().numpy(), bits_of(sb.qparams)
        return [(payload[offs[i * cpi]:offs[(i + 1) * cpi]].tobytes(), (offs[i * cpi:(i + 1) * cpi + 1] - offs[i * cpi]).tolist(),
                 lengths[i].tobytes(), qp[i].tolist()) for i in range(sb.shape[0])]

    batch = host(quantizer(z.to(DEV), None)[0])
    assert host(quantizer(z.to(DEV), None)[0]) == batch                           # the same call again: identical bytes
    for i in range(n):
        assert host(quantizer(z[i:i + 1].contiguous().to(DEV), None)[0]) == [batch[i]], i
    if n > 1:                                                                     # other neighbours, another position
        order = list(range(n - 1, -1, -1))
        flipped = host(quantizer(z[order].contiguous().to(DEV), None)[0])
        assert [flipped[order.index(i)] for i in range(n)] == batch
    ops.sync_check()


@pytest.mark.parametrize('bits', [2, 8])
def test_a_fixed_table_skips_the_histogram_and_the_table_launch(ops, bits):
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    shape = (3, 3, 5, 7)
    n, c, h, w = shape
    z = IU.make_input(shape)
    table = EU.valid_lengths([1 + (s % 5) for s in range(1 << bits)], bits)       # complete, not flat
    assert all(table) and len(set(table)) > 1
    quantizer = T.ImageStreamQuantizer(bits, code_lengths=list(table))
    sb, _ = quantizer(z.to(DEV), None)
    hist, lengths = [b for b in quantizer._bufs[next(iter(quantizer._bufs))] if tuple(b.shape) == (n, 256)]
    hist.fill_(0x5A5A5A5A)
    lengths.fill_(0x5A)
    sb, _ = quantizer(z.to(DEV), None)
    ops.sync_check()
    assert (hist == 0x5A5A5A5A).all() and (lengths == 0x5A).all()                # neither launch ran
    assert sb.lengths is quantizer._tables[(n, sb.payload.device)] and len(quantizer._tables) == 1
    assert torch.equal(sb.lengths.cpu(), torch.tensor(list(table) + [0] * (256 - len(table)), dtype=U8).repeat(n, 1))
    codes, _ = T.Quantizer(bits, per_image=True)(z.to(DEV), None)
    symbols = IU.image_symbols(codes.tensor.permute(0, 2, 3, 1).cpu().numpy(), c)
    cpi, offs = sb.chunks_per_image, sb.offsets.cpu().numpy().view(np.uint32).astype(np.int64)
    payload = sb.payload.cpu().numpy()
    for i in range(n):
        want_payload, want_offsets = EU.encode(symbols[i], table)
        assert np.array_equal(offs[i * cpi:(i + 1) * cpi + 1] - offs[i * cpi], want_offsets), i
        assert payload[offs[i * cpi]:offs[(i + 1) * cpi]].tobytes() == want_payload.tobytes(), i
    deq, _ = T.Dequantizer(bits)(sb, None)
    want, _ = T.Dequantizer(bits)(codes, None)
    assert torch.equal(bits_of(deq), bits_of(want))


# ------------------------------------------------------------------------------------------ (3) the split model
@pytest.fixture(scope='module')
def tiny_student():
    """the tiny student of tiny_eval_quantized, as tests/test_qimage_gpu.py builds it: a batch of 2"""
    _, meta = G.load('tiny_eval_quantized')
    cfg = MU.config_for(meta)
    t_sd, s_sd = MU.oracle_states(meta['seed'])
    _, student = MU.build_pair(cfg, t_sd, s_sd, DEV)
    student.eval()
    images, _ = G.case_inputs(meta)
    return student, [im.to(DEV) for im in images]


@pytest.mark.parametrize('bits', [2, 8])
def test_image_stream_split_gives_the_tail_the_floats_of_the_per_image_split(tiny_student, bits):
    from hnd_ghnd_object_detectors_amd.models.mimic.split_rcnn import split_rcnn_model_image_streams, split_rcnn_model_per_image
    from hnd_ghnd_object_detectors_amd.structure import transformer as T
    student, ims = tiny_student
    assert len(ims) == 2
    feats = {}
    for name, split in (('per_image', split_rcnn_model_per_image), ('streams', split_rcnn_model_image_streams)):
        head, tail = split(student, bits)
        head.eval()
        tail.eval()
        tail.features_only = True
        with torch.no_grad():
            zq, tensors_shape, image_sizes, original_sizes = head(ims)
            if name == 'streams':
                assert isinstance(zq, T.ImageStreamBottleneck) and zq.shape[0] == 2
                assert torch.equal(bits_of(zq.qparams), qparams)
                # across the link: the streams, the offsets, the tables and the qparams; nothing of the head's buffers
                zq = T.ImageStreamBottleneck(zq.payload[:max(zq.nbytes, 1)].clone(), zq.offsets.clone(), zq.lengths.clone(),
                                             zq.shape, zq.num_bits, zq.qparams.clone())
            else:
                qparams = bits_of(zq.qparams)
            feats[name] = {k: v.clone() for k, v in tail(zq, tensors_shape, image_sizes, original_sizes).items()}
    assert list(feats['streams']) == list(feats['per_image']) and feats['streams']
    for k in feats['per_image']:
        assert torch.equal(feats['streams'][k], feats['per_image'][k]), k
