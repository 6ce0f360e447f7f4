"""Programmatic builders for the hnd/ghnd YAML schema (reference config/{hnd,ghnd}/*.yaml).

The reference's own YAML files load unchanged through myutils.common.yaml_util (``!join`` supported); this module
produces the same dictionaries for tests, bench.py and smoke(), and tools/gen_configs.py dumps them to config/.
"""
from collections import OrderedDict

MODELS = ('faster_rcnn', 'mask_rcnn', 'keypoint_rcnn')
FROZEN = ['backbone.body.layer2', 'backbone.body.layer3', 'backbone.body.layer4', 'backbone.fpn', 'rpn', 'roi_heads']


def _term(layer):
    path = 'backbone.body.' + layer
    return {'ts_modules': [path, path], 'criterion': {'type': 'MSELoss', 'params': {'reduction': 'sum'}},
            'factor': 1.0}


ENCODER_PATH = 'backbone.body.layer1.encoder'


FAKE_QUANTIZE_MOMENTUM = 0.01       # default of train.fake_quantize.range.momentum


def _fake_quantize_section(config):
    """(section or None, bits, range dict or None) of ``train.fake_quantize``, with every refusal of its shape"""
    train = config.get('train') or {}
    section = train.get('fake_quantize')
    if section is None:
        return None, None, None
    shape = '{num_bits: b} or {num_bits: b, range: {type: batch}} or {num_bits: b, range: {type: ema, momentum: m}}' \
            ' (each optionally with per_channel: true | false or per_image: true | false, not both and neither with range: ' \
            '{type: ema})'
    if not isinstance(section, dict) or 'num_bits' not in section or \
            not set(section) <= {'num_bits', 'range', 'per_channel', 'per_image'}:
        raise ValueError('train.fake_quantize must be %s, got %r' % (shape, section))
    if not isinstance(section.get('per_channel', False), bool):
        raise ValueError('train.fake_quantize.per_channel=%r must be a bool' % (section['per_channel'],))
    if not isinstance(section.get('per_image', False), bool):
        raise ValueError('train.fake_quantize.per_image=%r must be a bool' % (section['per_image'],))
    if section.get('per_image', False) and section.get('per_channel', False):
        raise ValueError('train.fake_quantize: per_image together with per_channel is not built: the scales are per image or '
                         'per channel')
    bits = section['num_bits']
    if isinstance(bits, bool) or not isinstance(bits, int) or not 1 <= bits <= 8:
        raise ValueError('train.fake_quantize.num_bits=%r is outside 1 ... 8, the widths the fake-quantised bottleneck '
                         'implements' % (bits,))
    rng = None
    if 'range' in section:
        r = section['range']
        if not isinstance(r, dict) or r.get('type') not in ('batch', 'ema') or \
                not set(r) <= ({'type', 'momentum'} if r.get('type') == 'ema' else {'type'}):
            raise ValueError('train.fake_quantize must be %s, got %r' % (shape, section))
        if r['type'] == 'ema':
            m = r.get('momentum', FAKE_QUANTIZE_MOMENTUM)
            if isinstance(m, bool) or not isinstance(m, (int, float)) or not 0 < m <= 1:
                raise ValueError('train.fake_quantize must be %s with 0 < momentum <= 1, got momentum=%r' % (shape, m))
            if section.get('per_channel', False):
                raise ValueError('train.fake_quantize: per_channel together with range: {type: ema} is not built: the fixed '
                                 'range has no per-channel form (per-channel scales come from the min / max of each batch)')
            if section.get('per_image', False):
                raise ValueError('train.fake_quantize: per_image together with range: {type: ema} is not built: the fixed '
                                 'range has no per-image form (per-image scales come from the min / max of each image)')
            rng = {'momentum': float(m), 'frozen': False}
    return section, bits, rng


def fake_quantize_bits_of(config):
    """the width of the optional section ``train.fake_quantize: {num_bits: b}`` (quantisation-aware distillation, an
    extension: the reference has no such key), or None when the section is absent.  Refused by name here, at config time:
    a width outside 1 ... 8, a malformed section (``range``: see fake_quantize_range_of), and a criterion term whose student
    module is the bottleneck tensor's (layer1.encoder)."""
    section, bits, _ = _fake_quantize_section(config)
    if section is None:
        return None
    terms = (((config.get('train') or {}).get('criterion') or {}).get('terms') or {})
    for name, term in terms.items():
        if list(term.get('ts_modules', ()))[1:2] == [ENCODER_PATH]:
            raise NotImplementedError('train.fake_quantize together with the loss term `%s` on %s is not built: the '
                                      'bottleneck tensor is quantised in place, so the unquantised tensor the reference\'s '
                                      'hook would see does not exist' % (name, ENCODER_PATH))
    return bits


def fake_quantize_range_of(config):
    """``train.fake_quantize.range``: None for no section, no ``range`` key or ``{type: batch}`` (min / max of each batch,
    include/hnd_qat.h), or ``{'momentum': m, 'frozen': False}`` for ``{type: ema, momentum: m}`` (0 < m <= 1, default
    0.01): the fixed range of include/hnd_qrange.h, an exponential moving average of the batch min / max"""
    fake_quantize_bits_of(config)
    return _fake_quantize_section(config)[2]


def fake_quantize_per_channel_of(config):
    """``train.fake_quantize.per_channel`` (a bool, default False; include/hnd_qchannel.h): the training-time fake quantiser
    takes min / max, scale and zero point per channel of the bottleneck.  Refused by name: a non-bool, and the key together
    with ``range: {type: ema}``"""
    fake_quantize_bits_of(config)
    section = _fake_quantize_section(config)[0]
    return bool(section.get('per_channel', False)) if section is not None else False


def fake_quantize_per_image_of(config):
    """``train.fake_quantize.per_image`` (a bool, default False; include/hnd_qimage.h): the training-time fake quantiser
    takes min / max, scale and zero point per image of the batch, which is the quantiser the reference deploys at batch 1.
    Refused by name: a non-bool, and the key together with ``per_channel`` or ``range: {type: ema}``"""
    fake_quantize_bits_of(config)
    section = _fake_quantize_section(config)[0]
    return bool(section.get('per_image', False)) if section is not None else False


def make_config(model='faster_rcnn', method='ghnd', bch=3, batch_size=4, pretrained=True, min_size=None,
                max_size=None, ckpt_root='./resource/ckpt', fake_quantize_bits=None, fake_quantize_range=None,
                fake_quantize_per_channel=None, fake_quantize_per_image=None):
    """fake_quantize_range: None, or the ``range`` section itself ({'type': 'ema', 'momentum': m} / {'type': 'batch'});
    fake_quantize_per_channel / fake_quantize_per_image: None (no key) or the bool of ``per_channel`` / ``per_image``; all
    three need fake_quantize_bits"""
    config = _make_config(model, method, bch, batch_size, pretrained, min_size, max_size, ckpt_root)
    if fake_quantize_per_image is not None and fake_quantize_bits is None:
        raise ValueError('train.fake_quantize must be given num_bits (fake_quantize_bits) for per_image %r'
                         % (fake_quantize_per_image,))
    if fake_quantize_per_channel is not None and fake_quantize_bits is None:
        raise ValueError('train.fake_quantize must be given num_bits (fake_quantize_bits) for per_channel %r'
                         % (fake_quantize_per_channel,))
    if fake_quantize_range is not None and fake_quantize_bits is None:
        raise ValueError('train.fake_quantize must be given num_bits (fake_quantize_bits) for a range %r'
                         % (fake_quantize_range,))
    if fake_quantize_bits is not None:
        config['train']['fake_quantize'] = {'num_bits': fake_quantize_bits}
        if fake_quantize_range is not None:
            config['train']['fake_quantize']['range'] = dict(fake_quantize_range) \
                if isinstance(fake_quantize_range, dict) else fake_quantize_range
        if fake_quantize_per_channel is not None:
            config['train']['fake_quantize']['per_channel'] = fake_quantize_per_channel
        if fake_quantize_per_image is not None:
            config['train']['fake_quantize']['per_image'] = fake_quantize_per_image
        fake_quantize_range_of(config)
    return config


def _make_config(model, method, bch, batch_size, pretrained, min_size, max_size, ckpt_root):
    assert model in MODELS and method in ('hnd', 'ghnd')
    keypoint = model == 'keypoint_rcnn'
    dataset = 'coco2017'
    root = './resource/dataset/' + dataset
    ann = 'person_keypoints' if keypoint else 'instances'
    splits = {}
    for split, sub, rm in (('train', 'train2017', True), ('val', 'val2017', False), ('test', 'val2017', False)):
        splits[split] = {'images': '%s/%s' % (root, sub), 'annotations': '%s/annotations/%s_%s.json' % (root, ann, sub),
                         'remove_non_annotated_imgs': rm, 'jpeg_quality': None}
    params = {'num_classes': 2 if keypoint else 91, 'pretrained': pretrained}
    if keypoint:
        params['num_keypoints'] = 17
    if min_size is not None:
        params['min_size'] = min_size
    if max_size is not None:
        params['max_size'] = max_size
    t_exp = '%s-%s-backbone_resnet50' % (dataset, model)
    s_exp = '%s-%s-backbone_custom_resnet50_from_%s-backbone_resnet50-b%dch' % (dataset, model, model, bch)
    layers = ['layer1'] if method == 'hnd' else ['layer1', 'layer2', 'layer3', 'layer4']
    return {
        'dataset': {'name': dataset, 'root': root, 'num_workers': 4, 'aspect_ratio_group_factor': 3,
                    'splits': splits},
        'teacher_model': {'name': model,
                          'backbone': {'name': 'resnet50', 'params': {'pretrained': pretrained,
                                                                      'freeze_layers': True}},
                          'params': dict(params), 'experiment': t_exp,
                          'ckpt': '%s/org/%s.pt' % (ckpt_root, t_exp)},
        'student_model': {'name': model,
                          'backbone': {'name': 'custom_resnet50',
                                       'params': {'pretrained': pretrained, 'freeze_layers': False,
                                                  'layer1': {'name': 'Bottleneck4LargeResNet',
                                                             'bottleneck_channel': bch}}},
                          'bottleneck_transformer': {'order': ['quantizer', 'dequantizer'],
                                                     'components': {'quantizer': {'params': {'num_bits': 8}},
                                                                    'dequantizer': {'params': {'num_bits': 8}}}},
                          'params': dict(params), 'distill_backbone_only': True, 'frozen_modules': list(FROZEN),
                          'experiment': s_exp, 'ckpt': '%s/%s/%s.pt' % (ckpt_root, method, s_exp)},
        'train': {'num_epochs': 35 if keypoint else 20, 'batch_size': batch_size, 'log_freq': 1000,
                  'optimizer': {'type': 'Adam', 'params': {'lr': 0.001}},
                  'criterion': {'type': 'general', 'params': {'org_loss_factor': 0.0},
                                'terms': OrderedDict((l, _term(l)) for l in layers)},
                  'scheduler': {'type': 'MultiStepLR',
                                'params': {'milestones': [9, 27] if keypoint else [5, 15], 'gamma': 0.1}}},
        'test': {'batch_size': 1},
    }


def make_ext_config(bch=3, batch_size=2, pretrained=True, min_size=None, max_size=None, threshold=0.01,
                    ckpt_root='./resource/ckpt'):
    """the neural-filter schema of the reference's config/ext/keypoint_rcnn-backbone_ext_resnet50-b3ch.yaml"""
    base = make_config('keypoint_rcnn', 'ghnd', bch, batch_size, pretrained, min_size, max_size, ckpt_root)
    for split in base['dataset']['splits'].values():
        split['remove_non_annotated_imgs'] = False          # the filter needs the person-free images
    model = base['student_model']
    for key in ('distill_backbone_only', 'frozen_modules'):
        del model[key]
    model['backbone']['params']['freeze_layers'] = True
    model['backbone']['ext_config'] = {
        'backbone_frozen': True, 'threshold': threshold,
        'ckpt': '%s/ext/coco2017-keypoint_rcnn-backbone_ext_custom_resnet50-b%dch.pt' % (ckpt_root, bch)}
    return {'dataset': base['dataset'], 'model': model,
            'train': {'num_epochs': 30, 'batch_size': batch_size, 'log_freq': 10000,
                      'optimizer': {'type': 'SGD', 'params': {'lr': 0.001, 'momentum': 0.9, 'weight_decay': 0.0001}},
                      'scheduler': {'type': 'MultiStepLR', 'params': {'milestones': [15, 25], 'gamma': 0.1}}},
            'test': {'batch_size': 1}}


def make_org_config(model='faster_rcnn', pretrained=True, min_size=None, max_size=None, ckpt_root='./resource/ckpt'):
    """the schema of the reference's config/org/<model>-backbone_resnet50.yaml (the original detectors: what
    src/coco_runner.py trains / evaluates and the hnd/ghnd teachers are loaded from)"""
    base = make_config(model, 'ghnd', 3, 2, pretrained, min_size, max_size, ckpt_root)
    keypoint = model == 'keypoint_rcnn'
    return {'dataset': base['dataset'], 'model': base['teacher_model'],
            'train': {'num_epochs': 46 if keypoint else 26, 'batch_size': 2, 'log_freq': 1000,
                      'optimizer': {'type': 'SGD', 'params': {'lr': 0.0075, 'momentum': 0.9, 'weight_decay': 0.0001}},
                      'scheduler': {'type': 'MultiStepLR',
                                    'params': {'milestones': [36, 43] if keypoint else [16, 22], 'gamma': 0.1}}},
            'test': {'batch_size': 1}}
