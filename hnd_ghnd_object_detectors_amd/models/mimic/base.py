"""Encoder/decoder container of the bottleneck-injected layer1 (mirror of src/models/mimic/base.py).

``BottleneckBase4Ext.forward`` (reference :50-58) = decoder(encoder(x)), with the eval-only bottleneck
transformer (:54-57: quantise / dequantise the bottleneck tensor) applied between the two when
``use_bottleneck_transformer`` is set.  With a neural filter (``ext_config``; :13-19, :38-48) the
layer returns ``(features or None, ext_z)``: the filter runs first on the stem output and, for batch-1 inference
below ``threshold``, the encoder/decoder are skipped (early exit).
"""
from torch import nn

from ... import engine as E
from ...hipnn import attach, to_nhwc


class ExtEncoder(nn.Module):
    """container that keeps the reference's ``encoder.encoder.N`` / ``encoder.ext_classifier.*`` state-dict
    prefixes; the convolutions execute inside the parent's HeadEngine, the classifier through its FilterEngine."""

    def __init__(self, encoder, ext_classifier=None, ext_config=None):
        super().__init__()
        self.encoder, self.ext_classifier = encoder, ext_classifier
        self.threshold = None if ext_config is None else ext_config['threshold']

    def get_ext_classifier(self):
        return self.ext_classifier

    def filter(self, x):
        """reference forward_with_ext (:13-19) up to the gate: (run the encoder?, ext_z)."""
        ext_z = self.ext_classifier(x)
        if not self.training and ext_z.shape[0] == 1 and float(ext_z[0][1]) < self.threshold:
            return False, ext_z
        return True, ext_z

    def forward(self, x):
        raise RuntimeError('ExtEncoder executes fused inside Bottleneck4LargeResNet on the HIP path')


class BottleneckBase4Ext(nn.Module):
    """encoder -> [eval-only bottleneck transformer] -> decoder, executed as one HeadEngine plan."""

    def __init__(self, encoder, decoder, bottleneck_transformer=None):
        super().__init__()
        self.encoder, self.decoder = encoder, decoder
        self.bottleneck_transformer = bottleneck_transformer
        self.use_bottleneck_transformer = False
        # quantisation-aware distillation (an extension; yaml train.fake_quantize.num_bits, set by mimic_runner.distill):
        # 1 ... 8 = in TRAIN mode the bottleneck tensor is quantised and dequantised at that width between encoder and
        # decoder, straight-through in the backward (HeadEngine.forward); None = off, the reference's training
        self.train_fake_quant_bits = None
        # ... with a scale and a zero point per channel (an extension; yaml train.fake_quantize.per_channel; include/
        # hnd_qchannel.h).  Read with train_fake_quant_bits; not together with train_fake_quant_range
        self.train_fake_quant_per_channel = False
        # ... or per image of the batch (an extension; yaml train.fake_quantize.per_image; include/hnd_qimage.h): the
        # quantiser the reference deploys at batch 1.  Not together with per_channel or train_fake_quant_range
        self.train_fake_quant_per_image = False
        # ... on a FIXED range (an extension; yaml train.fake_quantize.range: {type: ema}; include/hnd_qrange.h): see the
        # property train_fake_quant_range.  None = the range of each batch
        self._fq_range = None
        self.uses_ext_encoder = isinstance(encoder, ExtEncoder) and encoder.ext_classifier is not None
        from ...structure.transformer import DataLogger
        self.data_logging = isinstance(bottleneck_transformer, DataLogger)       # reference :34
        self._engine = None

    def head_layers(self):
        """[(conv, pad, following BatchNorm2d, relu_after)] in execution order."""
        raise NotImplementedError

    def head_engine(self):
        if self._engine is None:
            self._engine = E.HeadEngine(self.head_layers())
        return self._engine

    @property
    def train_fake_quant_range(self):
        """None, or {'momentum': m, 'frozen': bool}: with train_fake_quant_bits set, the training-time fake quantiser clips
        to a fixed range -- the exponential moving average (momentum m) of the batch min / max, kept in the buffer
        ``qrange_state`` = {running_min, running_max, steps, 0} -- and the gradient of a clipped value is zero.  ``frozen``
        stops the observation; the range is then whatever the buffer holds, or the literal pair of the optional key
        ``'range': [lo, hi]``, which is written into the buffer.  Turning the mode on registers ``qrange_state`` as a
        NON-persistent buffer (zeros), so state_dict() and the reference's checkpoint format do not change; it does not
        exist before that."""
        return self._fq_range

    @train_fake_quant_range.setter
    def train_fake_quant_range(self, value):
        import math
        import torch
        if value is None:
            self._fq_range = None
            return
        m = value.get('momentum') if isinstance(value, dict) else None
        pair = value.get('range') if isinstance(value, dict) else None
        if not isinstance(value, dict) or not set(value) <= {'momentum', 'frozen', 'range'} or isinstance(m, bool) or \
                not isinstance(m, (int, float)) or not 0 < m <= 1 or not isinstance(value.get('frozen', False), bool):
            raise ValueError('train_fake_quant_range=%r must be None or {\'momentum\': m, \'frozen\': bool} with '
                             '0 < m <= 1' % (value,))
        if pair is not None:
            if not value.get('frozen', False):
                raise ValueError('train_fake_quant_range: a literal \'range\' needs \'frozen\': True')
            if len(pair) != 2 or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in pair) or \
                    not pair[0] < pair[1]:
                raise ValueError('train_fake_quant_range: \'range\'=%r needs finite lo < hi' % (pair,))
        if 'qrange_state' not in self._buffers:
            device = next(self.parameters()).device
            self.register_buffer('qrange_state', torch.zeros(4, dtype=torch.float32, device=device), persistent=False)
        if pair is not None:
            self.qrange_state.copy_(torch.tensor([float(pair[0]), float(pair[1]), 1.0, 0.0]))
        self._fq_range = {'momentum': float(m), 'frozen': bool(value.get('frozen', False)),
                          'range': None if pair is None else (float(pair[0]), float(pair[1]))}

    def fake_quant_range_host(self):
        """{'min', 'max', 'steps'} of qrange_state as host floats (ONE synchronisation), or None while the mode is off"""
        if 'qrange_state' not in self._buffers:
            return None
        lo, hi, steps, _ = self.qrange_state.detach().cpu().tolist()
        return {'min': lo, 'max': hi, 'steps': steps}

    def _fake_quant_range_arg(self):
        """what HeadEngine.forward takes as fake_quant_range.  A frozen range is handed over as a host pair (the engine's
        plan makes its qparams once): the literal one, or the buffer's, read when the plan's key changes"""
        r = self._fq_range
        if r is None or self.train_fake_quant_bits is None:
            return None
        pair = r['range']
        if r['frozen'] and pair is None:
            pair = r.get('host_pair')
        if r['frozen'] and pair is None:            # (once per setting of the attribute: one synchronisation)
            host = self.fake_quant_range_host()
            if not host['steps'] > 0 or not host['min'] < host['max']:
                raise RuntimeError('train_fake_quant_range is frozen but qrange_state holds no range yet '
                                   '(running_min %r, running_max %r, steps %r)' % (host['min'], host['max'], host['steps']))
            pair = r['host_pair'] = (host['min'], host['max'])
        return {'state': self.qrange_state, 'momentum': r['momentum'], 'frozen': r['frozen'], 'range': pair}

    def fake_quant_bits_checked(self):
        """train_fake_quant_bits, or the refusals that go with it (by name, before any launch of this layer): a width
        outside 1 ... 8; a forward hook on ``layer1.encoder`` (a loss term on the bottleneck tensor -- the reference's hook
        would see the unquantised z, which no longer exists once the buffer is quantised in place); the shared trunk
        (HND_MERGE_TRUNK=1), a combination no test runs."""
        bits = self.train_fake_quant_bits
        if bits is None:
            return None
        from ...structure.transformer import check_fake_quant_bits
        check_fake_quant_bits('train_fake_quant_bits (train.fake_quantize.num_bits)', bits)
        if not isinstance(self.train_fake_quant_per_channel, bool):
            raise ValueError('train_fake_quant_per_channel (train.fake_quantize.per_channel)=%r must be a bool'
                             % (self.train_fake_quant_per_channel,))
        if self.train_fake_quant_per_channel and self._fq_range is not None:
            raise ValueError('train_fake_quant_per_channel together with train_fake_quant_range (train.fake_quantize.range: '
                             '{type: ema}) is not built: the fixed range has no per-channel form')
        if not isinstance(self.train_fake_quant_per_image, bool):
            raise ValueError('train_fake_quant_per_image (train.fake_quantize.per_image)=%r must be a bool'
                             % (self.train_fake_quant_per_image,))
        if self.train_fake_quant_per_image and self.train_fake_quant_per_channel:
            raise ValueError('train_fake_quant_per_image together with train_fake_quant_per_channel is not built: the scales '
                             'are per image or per channel')
        if self.train_fake_quant_per_image and self._fq_range is not None:
            raise ValueError('train_fake_quant_per_image together with train_fake_quant_range (train.fake_quantize.range: '
                             '{type: ema}) is not built: the fixed range has no per-image form')
        if self.encoder._forward_hooks:
            raise NotImplementedError(
                'fake quantisation (train.fake_quantize) together with a hook / loss term on backbone.body.layer1.encoder '
                'is not built: the bottleneck tensor is quantised in place, so the unquantised tensor the reference\'s hook '
                'would see does not exist')
        if E.MERGE_TRUNK:
            raise NotImplementedError('fake quantisation (train.fake_quantize) with the shared trunk on '
                                      '(HND_MERGE_TRUNK=1) is not built')
        return bits

    def forward(self, x):
        ext_z = None
        if self.uses_ext_encoder:                       # reference :38-48 via ExtEncoder.forward_with_ext
            go_on, ext_z = self.encoder.filter(x)
            if not go_on:
                if self.data_logging:                   # reference :40-42: a rejected image logs an empty bottleneck
                    self.bottleneck_transformer(None, target=None)
                return None, ext_z
        use_codec = self.use_bottleneck_transformer and not self.training and self.bottleneck_transformer is not None
        fq_bits = self.fake_quant_bits_checked() if self.training else None
        eng = self.head_engine()
        out = eng.forward(to_nhwc(x), self.training,
                          codec=self.bottleneck_transformer if use_codec else None,   # base.py:54-57
                          fake_quant_bits=fq_bits,
                          **({} if fq_bits is None or self._fq_range is None
                             else {'fake_quant_range': self._fake_quant_range_arg()}),
                          **({} if fq_bits is None or not self.train_fake_quant_per_channel
                             else {'fake_quant_per_channel': True}),
                          **({} if fq_bits is None or not self.train_fake_quant_per_image
                             else {'fake_quant_per_image': True}))
        body = self.__dict__.get('_body')
        z = None
        if self.encoder._forward_hooks or self.decoder._forward_hooks:
            # hooks on ``...layer1.encoder`` / ``...layer1.decoder`` (src/distillation/tool.py:22-35 takes any path): the
            # encoder's output is the bottleneck tensor z (raw output of its last conv; the BatchNorm that follows is
            # decoder.0), the decoder's output is the layer's
            from ...hipnn import fire_forward_hooks
            zi = eng.encoder_len - 1
            zbuf = eng.y[zi]
            z = attach(E.logical(zbuf, eng.layers[zi].cout), zbuf, (body, 'layer1', 'encoder'))
            fire_forward_hooks(self.encoder, x, z)
            fire_forward_hooks(self.decoder, z, attach(E.logical(out), out, (body, 'layer1', 'decoder')))
        out = attach(E.logical(out), out)
        return (out, ext_z) if self.uses_ext_encoder else out

    def get_ext_classifier(self):
        raise NotImplementedError('get_ext_classifier function is not implemented')
