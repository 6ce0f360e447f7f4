"""CPU: the conv kernel pickers decide what tests/golden/conv_picker_table.npz recorded (tests/golden/make_picker_table.py:
the sample, the environment settings and the commit the table was taken from).  hnd_conv2d_igemm and its tile / build /
workspace queries share one decision (csrc/conv_igemm.hip: pick_conv), hnd_conv2d_wgrad and its variant query another
(csrc/conv_wgrad.hip: pick_wgrad); a change to any kernel's rule, to the order they are asked in or to a switch's accepted
spellings shows here as a changed answer.  No GPU: the pickers read pointer VALUES only and take 256 compute units when no
device answers, which is also what an MI355X has."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELAY_TILE_CODES = (11, 12, 14, 15)


def _generator():
    spec = importlib.util.spec_from_file_location('make_picker_table', os.path.join(ROOT, 'tests', 'golden', 'make_picker_table.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def replay():
    """{setting: answers} of THIS build for every recorded setting, with the table and the generator module"""
    import __graft_entry__ as g
    g.build()
    from hnd_ghnd_object_detectors_amd import _lib
    gen = _generator()
    table = np.load(gen.TABLE)
    assert list(table['conv_fields']) == gen.field_names(_lib.ConvDesc)
    assert list(table['wgrad_fields']) == gen.field_names(_lib.WgradDesc)
    saved = {s: os.environ.get(s) for s in gen.SWITCHES}
    try:
        got = {}
        for setting in table['settings']:
            gen.set_env(str(setting))
            got[str(setting)] = gen.evaluate(_lib.load(), _lib, table['conv'], table['wgrad'], table['rec'])
    finally:
        gen.set_env('')
        os.environ.update({s: v for s, v in saved.items() if v is not None})
    return got, table, gen


def test_the_table_covers_every_setting_and_every_answer(replay):
    got, table, gen = replay
    assert tuple(str(s) for s in table['settings']) == gen.SETTINGS
    assert len(table['conv']) > 3000 and len(table['wgrad']) > 500 and len(table['rec']) > 1000
    base = table['conv_tile'][0]
    assert all((base == c).sum() >= 5 for c in gen.TILE_CODES)
    assert set(np.unique(table['wgrad_variant'][0])) == {0, 1, 2, 3}


@pytest.mark.parametrize('answer', ['conv_tile', 'conv_build', 'conv_workspace', 'wgrad_variant', 'wgrad_workspace', 'rec_bx3',
                                    'rec_bxs'])
def test_every_recorded_answer_is_given_again_under_every_setting(replay, answer):
    got, table, gen = replay
    for i, setting in enumerate(gen.SETTINGS):
        want, have = table[answer][i], got[setting][answer]
        bad = np.nonzero(want != have)[0]
        assert bad.size == 0, '%s under %r: %d rows differ, first row %d: recorded %d, now %d' % (
            answer, setting, bad.size, bad[0], want[bad[0]], have[bad[0]])


def test_only_the_relay_kernels_ask_for_a_workspace_and_only_the_emulation_has_a_second_build(replay):
    got, table, gen = replay
    for setting in gen.SETTINGS:
        a = got[setting]
        assert np.isin(a['conv_tile'][a['conv_workspace'] > 0], RELAY_TILE_CODES).all(), setting
        assert (a['conv_tile'][a['conv_build'] != 0] == 13).all(), setting
        assert set(np.unique(a['conv_tile'])) <= set(gen.TILE_CODES), setting
