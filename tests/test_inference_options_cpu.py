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


# ---- the import chain ---------------------------------------------------------------------------------------------------------------------------
def test_demo_and_evaluate_do_not_import_the_training_script():
    code = ('import sys; sys.path.insert(0, %r); import demo; '
            'assert "evaluate" not in sys.modules, "demo imported evaluate"; assert "train" not in sys.modules, "demo imported train"; '
            'import evaluate; assert "train" not in sys.modules, "evaluate imported train"; '
            'assert callable(demo.build_model) and callable(evaluate.build_model)' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], cwd=str(ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
