"""ResNet's batch-statistics training mode, what needs no device: the keyword of the mode setters, the
plan-cache key, the refusals, and tests/resnet_bn_train_restated.py's backward-from-the-saved-forward against plain autograd."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_bn_train_restated as R  # noqa: E402


def test_modes_keyword_and_plan_key():
    from two_stage_object_detection_amd.models.resnet import resnet50
    m = resnet50(include_top=False).requires_grad_(False).eval()
    keys = list(m.state_dict())
    assert m.train_from("layer4", batch_stats=True) is m and m._batch_stats and m.train_mode == "layer4"
    assert m._plan_variant() == ()                                        # nothing of the section requires grad
    for p in m.trainable_parameters():
        p.requires_grad_(True)
    assert m._plan_variant() == m.train_from("layer4")._plan_variant() == ("train_from", "layer4")        # eval(): the key is unchanged
    assert not m._batch_stats and not m._trains_in_plan()
    assert m.train_from("layer4", batch_stats=True).train()._plan_variant() == ("train_from", "layer4", "batch_stats")
    assert m._trains_in_plan()
    with torch.no_grad():
        assert m._plan_variant() == () and not m._trains_in_plan()
    assert m.train_blocks(2, batch_stats=True)._plan_variant() == ("train_blocks", 2, "batch_stats")
    assert m.train_full(batch_stats=True)._plan_variant() == ("train_from", "stem", "batch_stats")
    assert m.set_train_mode("layer2", True)._batch_stats and not m.set_train_mode(None, True)._batch_stats
    assert not m.train_full()._batch_stats and list(m.state_dict()) == keys
    names = [k for k, _ in m._section_norms("stem")]
    assert len(names) == 53 and names[0] == "bn1" and names[1:5] == ["layer1.0.bn1", "layer1.0.bn2", "layer1.0.bn3", "layer1.0.downsample.1"]
    assert [k for k, _ in m._section_norms(1)] == ["layer4.2.bn1", "layer4.2.bn2", "layer4.2.bn3"]


def test_batchnorms_the_kernels_do_not_cover_are_refused():
    from two_stage_object_detection_amd.models.resnet import resnet50
    m = resnet50(include_top=False).eval()
    m.layer4[0].downsample[1].momentum = None
    m.train_from("layer4")                                                # folded: nothing to refuse
    m.train_blocks(2, batch_stats=True)                                   # layer4.0 is not reached
    with pytest.raises(NotImplementedError, match="layer4.0.downsample.1"):
        m.train_from("layer4", batch_stats=True)
    m.layer4[0].downsample[1].momentum = 0.1
    m.bn1.track_running_stats = False
    m.train_from("layer2", batch_stats=True)                              # the stem is not reached
    with pytest.raises(NotImplementedError, match="bn1"):
        m.train_full(batch_stats=True)
    m.bn1.track_running_stats = True
    m.layer3[1].bn2.affine = False
    with pytest.raises(NotImplementedError, match="layer3.1.bn2"):
        m.train_from("layer3", batch_stats=True)


def test_train_without_batch_stats_still_raises():
    from two_stage_object_detection_amd._ffi import TsodError
    from two_stage_object_detection_amd.models.resnet import resnet50
    m = resnet50(include_top=False).train_from("layer4").train()
    with pytest.raises(TsodError, match="call .eval"):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(TsodError, match="call .eval"):
        m.forward_nhwc(torch.zeros(1, 3, 32, 32))


def test_trainer_keyword_is_still_refused_for_resnet():
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    with pytest.raises(ValueError):
        FasterRCNNTrainer("train", 20, backbone="resnet50", bn_batch_stats=True)
    assert "train_from(\"layer4\", batch_stats=True)" in FasterRCNNTrainer.__doc__


def test_saved_forward_restatement_against_plain_autograd():
    """section_reference, fed the plain float64 forward's own z / outputs as the 'saved' ones, is plain autograd of the modules
    in .train() (the stem, a projection Bottleneck at stride 2, an identity Bottleneck), and T bounds every gradient."""
    from two_stage_object_detection_amd.models.resnet import Bottleneck, _conv
    torch.manual_seed(7)
    owner = types.SimpleNamespace(conv1=_conv(3, 64, 7, 2, 3).double(), bn1=torch.nn.BatchNorm2d(64).double(),
                                  relu=torch.nn.PReLU().double())
    down = torch.nn.Sequential(_conv(64, 32, 1, 2), torch.nn.BatchNorm2d(32))
    b0, b1 = Bottleneck(64, 8, stride=2, downsample=down).double().train(), Bottleneck(32, 8).double().train()
    mods = dict(owner.__dict__, **{"layer1.0": b0, "layer1.1": b1})
    for mod in list(b0.modules()) + list(b1.modules()) + [owner.bn1]:
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.3)
    with torch.no_grad():
        b1.relu.weight.fill_(0.1)
    x = torch.randn(2, 3, 20, 28, dtype=torch.float64)
    z0 = torch.nn.functional.conv2d(x, owner.conv1.weight, None, 2, 3)
    y0 = torch.nn.functional.prelu(torch.nn.functional.batch_norm(z0, None, None, owner.bn1.weight, owner.bn1.bias, True, 0.0,
                                                                  owner.bn1.eps), owner.relu.weight)
    s0 = R.block_forward_plain(b0, torch.nn.functional.max_pool2d(y0, 3, 2, 1))
    s1 = R.block_forward_plain(b1, s0["y3"])
    out = s1["y3"]
    assert tuple(out.shape) == (2, 32, 3, 4)
    gy = torch.randn_like(out)
    params = {}
    for prefix, mod in mods.items():
        for k, p in mod.named_parameters():
            params[f"{prefix}.{k}"] = p
    plain = torch.autograd.grad(out, list(params.values()), gy)
    det = lambda d: {k: v.detach() for k, v in d.items()}
    ref = R.section_reference((owner, dict(x=x, y=y0.detach(), z=z0.detach())),
                              [("layer1.0", b0, det(s0)), ("layer1.1", b1, det(s1))], gy)
    assert set(ref) == set(params) and len(ref) == 4 + 13 + 10
    for (name, p), g in zip(params.items(), plain):
        got, T, n = ref[name]
        assert got.shape == p.shape and n > 0 and bool((T >= got.abs() * (1 - 1e-9)).all()), name
        assert float((got - g).abs().max()) <= 1e-10 * max(float(g.abs().max()), float(T.max()) * 1e-3), name
    assert ref["layer1.1.bn3.bias"][2] < ref["layer1.0.bn3.bias"][2] < ref["conv1.weight"][2]      # (more BatchNorms above the stem)
