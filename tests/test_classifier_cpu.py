"""CPU: the classifier head's model surface (generate_model(classifier=True): modules, state_dict keys, initialisation, the 512-width
rule), the checkpoint hand-off from a contrastive model, the new C-ABI entry points' argument checks, and the no-device errors of the
loss / accuracy functions.  Nothing here computes on a device."""
import contextlib
import ctypes
import io
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

KW = dict(hidden_layer=64, out_dim=32, n_input_channels=3, shortcut_type='B', conv1_t_size=7, conv1_t_stride=1, no_max_pool=True,
          widen_factor=1.0, predict_temporal_ds=False, spatio_temporal_attention=False)


def _model(depth=10, **kw):
    from video_similarity_search_amd.models import generate_model
    with contextlib.redirect_stdout(io.StringIO()):
        return generate_model(depth, **dict(KW, **kw))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "classifier.npz"))


@pytest.mark.parametrize("tag,proj,dropout", [("plain", False, None), ("proj", True, None), ("drop", False, 0.5)])
def test_state_dict_keys_match_the_reference(golden, tag, proj, dropout):
    m = _model(classifier=True, num_classes=11, projection_head=proj, dropout=dropout)
    assert sorted(m.state_dict()) == [str(k) for k in golden[f"{tag}/keys"]]
    if dropout:
        assert isinstance(m.linear, nn.Sequential) and isinstance(m.linear[0], nn.Dropout) and m.linear[0].p == dropout
        assert isinstance(m.linear[1], nn.Linear)
    else:
        assert isinstance(m.linear, nn.Linear)
    assert hasattr(m, "fc1") == proj and hasattr(m, "bn_proj") == proj and hasattr(m, "fc2") == proj


def test_dropout_zero_or_none_builds_a_bare_linear():
    for d in (None, 0.0):
        assert isinstance(_model(classifier=True, num_classes=7, dropout=d, projection_head=False).linear, nn.Linear)


@pytest.mark.parametrize("C,dropout", [(101, None), (400, 0.5)])
def test_linear_initialisation(C, dropout):
    """weights normal(0, 0.01), biases exactly 0 (models/resnet.py:247-252).  The sample standard deviation s of n = 512 C normal draws
    has standard error sigma / sqrt(2 n) (the variance of a chi-square with n - 1 degrees of freedom, delta method), so
    |s - 0.01| <= 6 * 0.01 / sqrt(2 n); the sample mean has standard error sigma / sqrt(n)."""
    torch.manual_seed(1234)
    m = _model(classifier=True, num_classes=C, dropout=dropout, projection_head=False)
    lin = m.linear[1] if dropout else m.linear
    assert lin.weight.shape == (C, 512) and lin.bias.shape == (C,)
    assert torch.count_nonzero(lin.bias) == 0
    n = 512 * C
    w = lin.weight.detach().double()
    assert abs(w.std().item() - 0.01) <= 6 * 0.01 / math.sqrt(2 * n)
    assert abs(w.mean().item()) <= 6 * 0.01 / math.sqrt(n)
    # ... and the conv / BatchNorm rules still hold behind it (kaiming fan_out: std = sqrt(2 / (cout * k^3)); 64 * 27 * 64 samples)
    c = m.layer1[0].conv1.weight.detach().double()
    sig = math.sqrt(2.0 / (64 * 27))
    assert abs(c.std().item() - sig) <= 6 * sig / math.sqrt(2 * c.numel())
    assert torch.all(m.bn1.weight == 1) and torch.all(m.bn1.bias == 0)


def test_pooled_width_other_than_512_raises_value_error():
    with pytest.raises(ValueError, match="512"):
        _model(classifier=True, widen_factor=0.5)
    with pytest.raises(ValueError, match="512"):
        _model(50, classifier=True)
    _model(classifier=False, widen_factor=0.5)            # the rule belongs to the classifier head alone


def test_attention_and_temporal_ds_still_raise():
    for kw in (dict(spatio_temporal_attention=True), dict(predict_temporal_ds=True)):
        with pytest.raises(NotImplementedError):
            _model(classifier=True, **kw)
        with pytest.raises(NotImplementedError):
            _model(**kw)


def test_contrastive_checkpoint_loads_into_classifier(tmp_path):
    """models/model_utils.py load_checkpoint(classifier=True): trunk from the contrastive model, fc* / bn_proj* dropped, linear.* untouched"""
    from video_similarity_search_amd.models.model_utils import load_checkpoint
    torch.manual_seed(5)
    src = _model(classifier=False, projection_head=True)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(0.01 * torch.randn_like(p))
        src.bn1.running_mean.add_(0.3)
    path = os.path.join(tmp_path, "contrastive.pth.tar")
    torch.save({"epoch": 3, "best_prec1": 0.5, "state_dict": src.state_dict()}, path)
    dst = _model(classifier=True, num_classes=51, dropout=0.5, projection_head=False)
    w0, b0 = dst.linear[1].weight.detach().clone(), dst.linear[1].bias.detach().clone()
    with contextlib.redirect_stdout(io.StringIO()):
        load_checkpoint(dst, path, classifier=True, is_master_proc=False)
    sd_src, sd_dst = src.state_dict(), dst.state_dict()
    trunk = [k for k in sd_src if not k.startswith(("fc1.", "fc2.", "bn_proj."))]
    assert trunk and all(torch.equal(sd_src[k], sd_dst[k]) for k in trunk)
    assert torch.equal(dst.linear[1].weight, w0) and torch.equal(dst.linear[1].bias, b0)


def test_new_entry_points_reject_null_arguments():
    """the header / ctypes-table match is tests/test_abi.py's; here each new symbol is called with NULL and must answer non-zero with a message"""
    from video_similarity_search_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slic_hip.h")).read()
    calls = {
        "slic_softmax_ce_fwd": (None, 8, 2, 8, None, None, None, None, None, None),
        "slic_softmax_ce_bwd": (None, 8, None, None, 2, 8, None, None, None),
        "slic_dropout_fwd": (None, 16, 0.5, 1, 0, None, None),
        "slic_dropout_bwd": (None, 16, 0.5, 1, 0, None, None),
    }
    for name, args in calls.items():
        assert name in _lib.SIGNATURES and f"int {name}(" in header
        assert getattr(lib, name)(*args) != 0
        assert name.encode() in lib.slic_last_error(), name
    # host-side argument rules that need no device: ld < C, p outside [0, 1]
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.slic_softmax_ce_fwd(p, 4, 2, 8, p, p, p, p, p, None) != 0
    assert lib.slic_dropout_fwd(p, 16, 1.5, 1, 0, p, None) != 0 and lib.slic_dropout_bwd(p, 16, -0.1, 1, 0, p, None) != 0


def test_loss_and_accuracy_fail_loudly_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from video_similarity_search_amd._lib import SlicError
    from video_similarity_search_amd.loss import CrossEntropyLoss, calc_topk_accuracy
    x, t = torch.randn(4, 7), torch.tensor([0, 1, 2, 6])
    with pytest.raises(SlicError):
        CrossEntropyLoss()(x, t)
    with pytest.raises(SlicError):
        calc_topk_accuracy(x, t, (1, 5))
    with pytest.raises(SlicError):
        _model(classifier=True, projection_head=False)(torch.randn(1, 3, 8, 32, 32))
