"""The seeded training step on the shrunk model that the GPU tests of the step and of the model extensions share: one model and chain
builder, one batch, one seeded forward / step, the inference model, and the two judges.  A helper of the tests, not a test."""
import numpy as np
import torch

from chainer_maskrcnn.model.fpn_maskrcnn_train_chain import FPNMaskRCNNTrainChain, calc_mask_loss
from chainer_maskrcnn.model.maskrcnn import MaskRCNN
from chainer_maskrcnn.nn import core
from chainer_maskrcnn.utils.synthetic import make_batch

DEV = 'cuda:0'


def build(shrink, seed=7, chain_kw=None, mask_rows='all', **model_kw):
    m = MaskRCNN(n_fg_class=80, device=DEV, seed=seed, _test_shrink=shrink, **model_kw)
    return m, FPNMaskRCNNTrainChain(m, mask_loss_fun=calc_mask_loss, mask_rows=mask_rows, **(chain_kw or {}))


def batch(N=2, H=128, W=160, G=3):
    b = make_batch(3, N, H, W, G=G)
    b['bboxes'][:, :, 2:] = np.minimum(b['bboxes'][:, :, 2:], [H, W])
    return {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}


def seed(chain):
    chain.sampler_keys = None
    chain.proposal_target_creator.set_seed(5)
    chain.anchor_target_creator.set_seed(9)


def forward(chain, b):
    seed(chain)
    return chain(b['imgs'], b['bboxes'], b['labels'], b['masks'], 1.0)


def step(chain, b):
    forward(chain, b).backward()
    core.join_side_stream(torch.device(DEV))
    torch.cuda.synchronize()


def predict_model(shrink, seed, **model_kw):
    m = MaskRCNN(n_fg_class=80, device=DEV, seed=seed, _test_shrink=shrink, min_size=160, max_size=260, **model_kw)
    m.use_preset('evaluate')
    m.score_thresh = 0.0125                         # random weights: ~uniform class probabilities (1/81 = 0.0123)
    return m


def _f64(x):
    return x.detach().cpu().to(torch.float64) if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, np.float64))


def check(name, got, want64, want32, bad):
    """got (torch or NumPy) against the float64 reference, both errors relative to the reference's largest magnitude.
    bar = max(1e-3, 3 x floor): 1e-3 the BASELINE north_star gradient bar, floor the same CPU computation in float32."""
    want64 = _f64(want64)
    scale = max(float(want64.abs().max()), 1e-30)
    err = float((_f64(got) - want64).abs().max()) / scale
    floor = float((_f64(want32) - want64).abs().max()) / scale
    print('%-28s err %.3e floor %.3e' % (name, err, floor))
    if not err <= max(1e-3, 3 * floor):
        bad.append((name, err, floor))


def grad_ok(got, want, err, floor, tol):
    """err = max |got - want| / tensor scale, floor = the same for the float32 oracle.  Pass: err < max(tol, 3 x floor) - or
    the deviation is ONE flipped ReLU decision: a pre-activation of fc1 / fc2 / a head convolution within rounding of zero
    toggles a whole (RoI, unit) term, i.e. a few entries of the gradient move by up to ~5e-3 of its scale while the tensor
    as a whole does not (relative L2 error < tol).  Measured: head/fc1/W differs by 4.4e-3 in max norm between two DEVICE
    evaluations whose BatchNorm statistics differ by 1e-7 (features by 2e-6) - no float32 implementation is stable there."""
    if err < max(tol, 3 * floor):
        return True
    l2 = float((got - want).norm()) / max(float(want.norm()), 1e-30)
    return l2 < tol and err < 10 * tol
