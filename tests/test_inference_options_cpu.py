"""CPU tests of the single statements of the inference and evaluation host path: the evaluators' shared loop restores the target's
training state when a prediction raises, evaluate.py / demo.py / train.py declare the same test-time augmentation flags
(chainer_maskrcnn/inference_options.py), and evaluate.py / demo.py do not import the training script."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from chainer_maskrcnn import evaluator as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the evaluators' loop ---------------------------------------------------------------------------------------------------------------------
class _FailsOnTheSecondImage(object):
    """A target whose forward leaves the flags a real one leaves (train off everywhere), finds nothing in the first image - so that no
    kernel is needed - and raises in the second."""

    def __init__(self):
        self.device = torch.device('cpu')
        self.train = 'target-train'
        self.rpn, self.head = types.SimpleNamespace(train='rpn-train'), types.SimpleNamespace(train='head-train', n_keypoints=17)
        self.calls = 0

    def _forward(self):
        from chainer_maskrcnn.nn import core
        self.calls += 1
        self.train = core.TRAIN = self.rpn.train = self.head.train = False
        if self.calls == 2:
            raise RuntimeError('the second image')

    def predict(self, imgs):
        self._forward()
        self.last_bboxes = [torch.zeros((0, 4))]
        return [torch.zeros((0,) + tuple(imgs[0].shape[1:]), dtype=torch.bool)], [torch.zeros((0,), dtype=torch.int32)], [torch.zeros((0,))]

    def predict_keypoints(self, imgs):
        self._forward()
        self.last_bboxes = [torch.zeros((0, 4))]
        return [torch.zeros((0, 17, 4))], [torch.zeros((0,), dtype=torch.int32)], [torch.zeros((0,))]


EVALUATORS = {'voc': lambda t: ev.InstanceSegmentationVOCEvaluator(ev.SyntheticEvalDataset(3, 32, 40, n_fg_class=5, G=2), t),
              'keypoint': lambda t: ev.KeypointCOCOEvaluator(ev.SyntheticKeypointEvalDataset(3, 32, 40, G=2), t),
              'coco': lambda t: ev.InstanceSegmentationCOCOEvaluator(ev.SyntheticCOCOEvalDataset(3, 32, 40, n_fg_class=5, G=2), t, results=[])}


@pytest.mark.parametrize('kind', sorted(EVALUATORS))
def test_a_failing_prediction_leaves_the_training_state_as_it_was(kind, monkeypatch):
    from chainer_maskrcnn.nn import core
    monkeypatch.setattr(core, 'TRAIN', 'core-train')
    target = _FailsOnTheSecondImage()
    with pytest.raises(RuntimeError, match='the second image'):
        EVALUATORS[kind](target).evaluate()
    assert target.calls == 2                                            # the first image went through, the third was never asked for
    assert (target.train, core.TRAIN, target.rpn.train, target.head.train) == ('target-train', 'core-train', 'rpn-train', 'head-train')


def test_copy_to_host_splits_what_it_concatenated():
    parts = (torch.arange(3, dtype=torch.int32), torch.tensor([[0.5, -1.25], [3.0, float('inf')]]), torch.zeros((0, 4)),
             torch.arange(6, dtype=torch.int32).reshape(2, 3))
    got = ev.copy_to_host(*parts)
    assert [g.dtype for g in got] == [np.int32, np.float32, np.float32, np.int32]
    for g, p in zip(got, parts):
        np.testing.assert_array_equal(g, p.numpy())
    empty = ev.copy_to_host(torch.zeros((0,), dtype=torch.int32), torch.zeros((0, 4)))
    assert [(e.shape, e.dtype) for e in empty] == [((0,), np.int32), ((0, 4), np.float32)]
    with pytest.raises(TypeError):
        ev.copy_to_host(torch.zeros(2, dtype=torch.int64))


# ---- the flags ----------------------------------------------------------------------------------------------------------------------------------
TTA_CASES = [([], None),
             (['--tta-hflip', '1'], {'sizes': [600], 'hflip': True, 'max_size': None}),
             (['--tta-sizes', '700'], {'sizes': [700], 'hflip': False, 'max_size': None}),
             (['--tta-sizes', '640', '800', '1000', '--tta-hflip', '1', '--tta-max-size', '1333'],
              {'sizes': [640, 800, 1000], 'hflip': True, 'max_size': 1333})]


@pytest.mark.parametrize('argv,want', TTA_CASES)
def test_the_three_scripts_declare_the_same_tta_flags(argv, want):
    import demo
    import evaluate
    import train
    from chainer_maskrcnn.inference_options import tta_settings
    got = []
    for parser in (evaluate.build_parser(), demo.build_parser()):
        a = parser.parse_args(argv)
        got.append(tta_settings(a.tta_sizes, a.tta_hflip, a.tta_max_size, 600))
    for keypoints in (False, True):
        a = train.build_parser(keypoints).parse_args([w.replace('--tta-', '--eval-tta-') for w in argv])
        got.append(tta_settings(a.eval_tta_sizes, a.eval_tta_hflip, a.eval_tta_max_size, 600))
    assert got == [want] * 4


def test_every_script_refuses_a_tta_hflip_of_two():
    import demo
    import evaluate
    import train
    for parser, flag in ((evaluate.build_parser(), '--tta-hflip'), (demo.build_parser(), '--tta-hflip'),
                         (train.build_parser(False), '--eval-tta-hflip'), (train.build_parser(True), '--eval-tta-hflip')):
        with pytest.raises(SystemExit):
            parser.parse_args([flag, '2'])


def test_use_tta_resolves_the_keypoint_flip_map():
    from chainer_maskrcnn.dataset import augment
    from chainer_maskrcnn.inference_options import use_tta

    class Model(object):
        def __init__(self, head_arch, K=17):
            self.head_arch, self.head, self.calls = head_arch, types.SimpleNamespace(n_keypoints=K), []

        def use_test_augmentation(self, sizes, hflip=False, max_size=None, keypoint_flip_perm=None):
            self.calls.append((sizes, hflip, max_size, keypoint_flip_perm))
    on = {'sizes': [600, 800], 'hflip': True, 'max_size': 1000}
    m = Model('fpn')
    use_tta(m, None)
    assert m.calls == []
    use_tta(m, on)
    assert m.calls == [([600, 800], True, 1000, None)]
    k = Model('fpn_keypoint')
    use_tta(k, dict(on, hflip=False))
    assert k.calls[-1] == ([600, 800], False, 1000, None)              # no mirror: no flip map
    use_tta(k, on)
    np.testing.assert_array_equal(k.calls[-1][3], augment.flip_permutation(augment.COCO_KEYPOINT_NAMES))
    names = list(augment.COCO_KEYPOINT_NAMES)[::-1]
    use_tta(k, on, names)
    np.testing.assert_array_equal(k.calls[-1][3], augment.flip_permutation(names))
    with pytest.raises(ValueError, match='--tta-hflip 1: 17 keypoint names for 20 keypoints'):
        use_tta(Model('fpn_keypoint', 20), on)
    with pytest.raises(ValueError, match='--eval-tta-hflip 1: 17 keypoint names for 20 keypoints'):       # train.py's text
        use_tta(Model('fpn_keypoint', 20), on, None, '--eval-')
    with pytest.raises(ValueError, match='flip map'):
        use_tta(k, on, ['k%d' % i for i in range(17)])


def test_read_labels(tmp_path):
    from chainer_maskrcnn.inference_options import read_labels
    assert read_labels(str(tmp_path / 'missing.txt')) is None
    (tmp_path / 'l.txt').write_text('person\nbicycle\ncar\n')
    assert read_labels(str(tmp_path / 'l.txt')) == ['person', 'bicycle', 'car']
    assert len(read_labels(os.path.join(ROOT, 'data', 'label_coco.txt'))) == 80


# ---- the table of model extensions ------------------------------------------------------------------------------------------------------------
def _extension_names():
    from chainer_maskrcnn.inference_options import EXTENSIONS
    return [e.name for e in EXTENSIONS]


def _parsers():
    import demo
    import evaluate
    import train
    return {'train': train.build_parser(), 'train_keypoints': train.build_parser(keypoints=True), 'evaluate': evaluate.build_parser(),
            'demo': demo.build_parser()}


def test_the_table_lists_the_extensions_in_model_order():
    assert _extension_names() == ['head_norm', 'fpn_norm', 'cascade', 'mask_iou', 'point_rend']


@pytest.mark.parametrize('name', _extension_names())
def test_every_extension_is_wired_into_the_four_scripts(name, tmp_path):
    """What the scripts owe every record of inference_options.EXTENSIONS, asked of the record: a new extension is checked without new test code."""
    import argparse
    import re
    import demo
    import evaluate
    import train
    from chainer_maskrcnn import inference_options as io
    e = {x.name: x for x in io.EXTENSIONS}[name]
    parsers = _parsers()
    own = argparse.ArgumentParser()
    io.add_extension_flags(own, training=True)
    e_only = argparse.ArgumentParser()
    e.add_flags(e_only, **({'weight': True} if e.weight_flag else {}))
    flags = ['--' + dest.replace('_', '-') for dest in vars(e_only.parse_args([]))]
    assert e.switch.split()[0] in flags and set(vars(e_only.parse_args([]))) <= set(vars(own.parse_args([])))
    # the flags: every parser takes them, the weight flag is a training flag, train_keypoints.py takes both spellings
    for script, p in parsers.items():
        for flag in flags:
            training_only = flag == e.weight_flag and script in ('evaluate', 'demo')
            assert (flag in p._option_string_actions) == (not training_only), (script, flag)
        assert e.is_on(e.settings(p.parse_args(['--head-arch' if script != 'train_keypoints' else '--head_arch', 'fpn'] + e.switch.split()),
                                  script.startswith('train')))
    if e.weight_flag:
        assert train.build_parser().parse_args(e.switch.split() + [e.weight_flag, '0.5']) is not None
        for script in ('evaluate', 'demo'):
            with pytest.raises(SystemExit):
                parsers[script].parse_args(e.switch.split() + [e.weight_flag, '0.5'])
    for flag in flags:
        assert '--' + flag[2:].replace('-', '_') in parsers['train_keypoints']._option_string_actions, flag
    # all flags off: the 'off' record, and nothing is on
    for script, p in parsers.items():
        training = script.startswith('train')
        s = io.extension_settings(p.parse_args([]), '--eval-tta-' if training else '--tta-', training=training,
                                  keypoints=script == 'train_keypoints')[e.name]
        assert not e.is_on(s) and (e.off is None or s == e.off), script
    p = train.build_parser()
    on, off = p.parse_args(e.switch.split()), p.parse_args([])
    # the trainer state: a round trip through the file resumes, a missing key means off, another setting is refused by its noun
    assert (e.state_key is None) == (e.off is None) == (e.settings_noun is None)
    if e.state_key:
        assert [c for c in train.RESUME_CHECKS if c[0] == e.state_key] == [(e.state_key, e.off, e.settings_noun)]
        now = io.extension_settings(on, '--eval-tta-', training=True)[e.name]
        assert io.state_records(io.extension_settings(on, '--eval-tta-', training=True))[e.state_key] == now != e.off
        ck, old = str(tmp_path / 'trainer_5.pt'), str(tmp_path / 'trainer_old.pt')
        torch.save({'iteration': 5, e.state_key: now}, ck)
        torch.save({'iteration': 3}, old)
        state = torch.load(ck, map_location='cpu', weights_only=False)
        io.check_resume(state, e.state_key, e.off, now, e.settings_noun, ck)
        io.check_resume({'iteration': 3}, e.state_key, e.off, io.extension_settings(off, '--eval-tta-', training=True)[e.name], e.settings_noun, old)
        refusal = '--resume .*%s' % re.escape(e.settings_noun)
        with pytest.raises(ValueError, match=refusal):
            io.check_resume(state, e.state_key, e.off, e.off, e.settings_noun, ck)
        with pytest.raises(ValueError, match=refusal):          # through run(): refused before any device work
            train.run(p.parse_args(['--resume', old] + e.switch.split()))
        with pytest.raises(ValueError, match=refusal):
            train.run(p.parse_args(['--resume', ck]))
    # test-time augmentation: each script refuses it in its own flags' name
    if e.refuses_tta:
        for tta in (['--tta-hflip', '1'], ['--tta-sizes', '160', '200']):
            for mod, argv in ((evaluate, []), (demo, ['--synthetic', '1'])):
                with pytest.raises(ValueError, match=re.escape(e.switch) + ' does not go with --tta-sizes / --tta-hflip.*' + re.escape(e.model_noun)):
                    mod.check_args(mod.build_parser().parse_args(argv + e.switch.split() + tta))
            with pytest.raises(ValueError, match=re.escape(e.switch) + ' does not go with --eval-tta-.*' + re.escape(e.model_noun)):
                train.run(p.parse_args(e.switch.split() + [w.replace('--tta-', '--eval-tta-') for w in tta]))
    # mask heads only: keypoint training refuses it with its own sentence
    if e.mask_heads_only:
        with pytest.raises(ValueError) as err:
            train.run(parsers['train_keypoints'].parse_args(e.switch.split()), keypoints=True)
        assert str(err.value) == e.mask_heads_only[1] and 'mask heads' in str(err.value) and 'train_keypoints.py' in str(err.value)


# ---- the behaviour of the entry scripts, pinned ---------------------------------------------------------------------------------------------------
class _Built(Exception):
    pass


def _replay(script, argv, monkeypatch):
    """What ``script`` makes of ``argv`` before any device work, as tests/golden/entry_script_settings.json records it: the keyword arguments
    it builds MaskRCNN (and, training, FPNMaskRCNNTrainChain) with and the records it writes into trainer_<it>.pt, or the exception it refuses
    with.  The two classes are replaced by recorders that stop the script where it would build them."""
    import demo
    import evaluate
    import train
    from chainer_maskrcnn import inference_options as io
    from chainer_maskrcnn.model import fpn_maskrcnn_train_chain, maskrcnn
    got = {}

    def plain(kw):
        return {k: v.__name__ if callable(v) else v for k, v in kw.items() if k != 'device'}

    class Model(object):
        def __init__(self, **kw):
            got['model'] = plain(kw)
            if not script.startswith('train'):
                raise _Built()

    class Chain(object):
        def __init__(self, model, **kw):
            got['chain'] = plain(kw)
            raise _Built()
    monkeypatch.setattr(maskrcnn, 'MaskRCNN', Model)
    monkeypatch.setattr(fpn_maskrcnn_train_chain, 'FPNMaskRCNNTrainChain', Chain)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda dev: None)
    try:
        if script.startswith('train'):
            keypoints = script == 'train_keypoints'
            args = train.build_parser(keypoints).parse_args(argv)
            with pytest.raises(_Built):
                train.run(args, keypoints=keypoints)
            state = io.state_records(io.extension_settings(args, '--eval-tta-', training=True, keypoints=keypoints))
            got['state'] = dict(state, freeze=train.freeze_settings(args), optim=train.optim_settings(args)[0], augment=train.augment_settings(args))
        else:
            mod = {'evaluate': evaluate, 'demo': demo}[script]
            args = mod.build_parser().parse_args(argv)
            mod.check_args(args)
            with pytest.raises(_Built):
                mod.build_model(args)
    except (ValueError, SystemExit) as e:
        return {'error': [type(e).__name__, str(e)]}
    return got


def test_the_entry_scripts_derive_what_they_derived_before_the_table(monkeypatch):
    """tests/golden/entry_script_settings.json holds, for 143 argument vectors of train.py, train_keypoints.py, evaluate.py and demo.py (every
    extension alone, in pairs, with test-time augmentation, under keypoint training, with every --head-arch, with another --backbone, shape and
    weight flags without their switch), what the scripts derived at the commit before the extensions were declared in one table.  The
    scripts must derive the same: equal keyword arguments, equal trainer-state records, the same exception type and the same full message.
    Tuples and lists compare as JSON does (the file cannot tell them apart): the result goes through json before it is compared."""
    import json
    monkeypatch.chdir(ROOT)             # the default --label_file is relative to the repository
    rows = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'entry_script_settings.json')))
    assert len(rows) == 143 and {r['script'] for r in rows} == {'train', 'train_keypoints', 'evaluate', 'demo'}
    different = []
    for r in rows:
        got = json.loads(json.dumps(_replay(r['script'], r['argv'], monkeypatch)))
        if got != r['result']:
            different.append((r['script'], r['argv'], got, r['result']))
    assert not different, different[:3]


# ---- the import chain ---------------------------------------------------------------------------------------------------------------------------
def test_demo_and_evaluate_do_not_import_the_training_script():
    code = ('import sys; sys.path.insert(0, %r); import demo; '
            'assert "evaluate" not in sys.modules, "demo imported evaluate"; assert "train" not in sys.modules, "demo imported train"; '
            'import evaluate; assert "train" not in sys.modules, "evaluate imported train"; '
            'assert callable(demo.build_model) and callable(evaluate.build_model)' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], cwd=str(ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
