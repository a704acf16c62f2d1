"""ResNet.train_from: the gradients of every Bottleneck from the first block of a stage to the end of
layer4, projection blocks included, against tests/resnet_stage_grads_restated.py's float64 section, fed every block's input and
stage outputs read back from the HIP run (``f.grad_fn.saved``), so that only the backward is under test.  The bar:
|err| <= (n + 8) 2^-24 T elementwise."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resnet_stage_grads_restated import assert_within, section_reference  # noqa: E402

IDENTITY_KEYS = {"name", "x", "y1", "y2", "y3", "w", "scale", "rot", "slope", "bn"}
PROJECTION_KEYS = IDENTITY_KEYS | {"wd", "scaled", "stride", "s2d", "bn_d"}
DEPTH = {"layer2": 4, "layer3": 6, "layer4": 3}


def seeded_backbone(dev, seed=0):
    """Seeded resnet50 with non-trivial BatchNorm statistics and affine terms (the folding rule needs a mean); the helper of
    tests/test_resnet_block_grads.py."""
    from two_stage_object_detection_amd.models.resnet import resnet50
    torch.manual_seed(seed)
    m = resnet50(include_top=False)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                C = mod.num_features
                mod.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(C, generator=g) + 0.5)
                mod.weight.copy_(torch.rand(C, generator=g) * 0.5 + 0.5)
                mod.bias.copy_(torch.randn(C, generator=g) * 0.1)
    m.requires_grad_(False)
    return m.to(dev).eval()


def unfreeze(m, stage):
    m.train_from(stage)
    for p in m.trainable_parameters():
        p.requires_grad_(True)
    return m


def block_names(stage):
    stages = ("layer2", "layer3", "layer4")
    return [f"{st}.{i}" for st in stages[stages.index(stage):] for i in range(DEPTH[st])]


def images(seed, dev, shape=(2, 3, 64, 96)):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def reference_for(m, f, gy):
    """{name: (gradient, T, n)} of the section that produced ``f``, from the node's saved tensors."""
    blocks = []
    for b in f.grad_fn.saved["blocks"]:
        blk = copy.deepcopy(m.get_submodule(b["name"])).cpu().double()
        assert float(blk.relu.weight.detach()) == b["slope"]
        blocks.append((b["name"], blk, {k: nchw(b[k]) for k in ("x", "y1", "y2", "y3")}))
    return section_reference(blocks, gy.cpu())


def clear(m):
    for p in m.parameters():
        p.grad = None


@pytest.mark.gpu
@pytest.mark.parametrize("stage,shape,hw", [("layer4", (2, 3, 64, 96), (2, 3)), ("layer4", (2, 3, 80, 112), (3, 4)),
                                            ("layer2", (2, 3, 64, 96), (2, 3))])
def test_train_from_output_unchanged_and_gradients_match_f64(dev, stage, shape, hw):
    m = seeded_backbone(dev)
    x = images(1, dev, shape)
    with torch.no_grad():
        plain = m(x).clone()
    assert tuple(plain.shape[2:]) == hw
    gy = torch.randn(plain.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    m.train_from(stage)
    assert not m(x).requires_grad                                  # nothing of the section requires grad: the plain map
    unfreeze(m, stage)
    names = [k for k, _ in m._trainable_named()]
    f = m(x)
    assert f.requires_grad and torch.equal(f.detach(), plain)
    with torch.no_grad():
        assert not m(x).requires_grad
    saved = f.grad_fn.saved["blocks"]
    assert [b["name"] for b in saved] == block_names(stage)        # forward order
    for b in saved:
        if b["name"].endswith(".0"):
            assert set(b) == PROJECTION_KEYS and b["stride"] == 2 and b["rot"] is None and len(b["w"]) == 3
            C, Cout = b["w"][1].shape[3], b["w"][1].shape[0]
            assert tuple(b["s2d"].shape) == (4 * C, 2, 2, Cout) and tuple(b["wd"].shape) == (b["y3"].shape[3], 1, 1, b["x"].shape[3])
            assert b["y1"].shape[1:3] == b["x"].shape[1:3] and b["y2"].shape[1] == (b["x"].shape[1] - 1) // 2 + 1
        else:
            assert set(b) == IDENTITY_KEYS and b["rot"] is not None
    f.backward(gy)
    ref = reference_for(m, f, gy)
    assert set(ref) == set(names) and len(names) == {"layer4": 33, "layer2": 139}[stage]
    worst = {}
    for name, p in zip(names, m.trainable_parameters()):
        assert p.grad is not None and p.grad.shape == p.shape, name
        g, T, cnt = ref[name]
        assert_within(p.grad, g, T, cnt, name)
        kind = ".".join(name.split(".")[2:])
        ratio = float(((p.grad.double().cpu() - g).abs() / ((cnt + 8) * 2.0 ** -24 * T).clamp_min(1e-300)).max())
        worst[kind] = max(worst.get(kind, 0.0), ratio)
    print(f"train_from({stage!r}) {shape}: largest err / bar per tensor kind: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    ours = {id(p) for p in m.trainable_parameters()}
    assert all(p.grad is None for p in m.parameters() if id(p) not in ours)
    assert {k[3:] for k in m._plans} == {(), ("train_from", stage)}
    # the NHWC entry point carries the same node
    got = [p.grad.clone() for p in m.trainable_parameters()]
    clear(m)
    f2 = m.forward_nhwc(x)
    assert f2.requires_grad and torch.equal(f2.detach().permute(0, 3, 1, 2), plain)
    f2.backward(gy.permute(0, 2, 3, 1).contiguous())
    assert all(torch.equal(p.grad, g) for p, g in zip(m.trainable_parameters(), got))       # and the same bits, run to run
    m.set_train_mode(None)
    assert not m(x).requires_grad


@pytest.mark.gpu
def test_two_forwards_then_their_backwards_in_reverse_order(dev):
    m = unfreeze(seeded_backbone(dev), "layer4")
    xa, xb = images(5, dev), images(6, dev)
    gen = torch.Generator().manual_seed(7)
    ga, gb = torch.randn(2, 2048, 2, 3, generator=gen).to(dev), torch.randn(2, 2048, 2, 3, generator=gen).to(dev)
    singles = []
    for x, gy in ((xa, ga), (xb, gb)):
        clear(m)
        m(x).backward(gy)
        singles.append([p.grad.clone() for p in m.trainable_parameters()])
    clear(m)
    fa = m(xa)
    fb = m(xb)
    fb.backward(gb)
    fa.backward(ga)
    for (name, _), p, s1, s2 in zip(m._trainable_named(), m.trainable_parameters(), *singles):
        assert torch.equal(p.grad, s2 + s1), name


@pytest.mark.gpu
def test_train_blocks_2_after_a_stage_mode_gives_todays_records(dev):
    m = unfreeze(seeded_backbone(dev), "layer4")
    x = images(3, dev)
    gy = torch.randn(2, 2048, 2, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    m(x).backward(gy)
    stage = {k: p.grad.clone() for k, p in m._trainable_named()}
    clear(m)
    m.train_blocks(2)
    f = m(x)
    saved = f.grad_fn.saved["blocks"]
    assert [b["name"] for b in saved] == ["layer4.1", "layer4.2"] and all(set(b) == IDENTITY_KEYS for b in saved)
    f.backward(gy)
    assert all(p.grad is None for p in m.layer4[0].parameters())
    assert len(m._trainable_named()) == 20
    for k, p in m._trainable_named():
        assert torch.equal(p.grad, stage[k]), k                   # the identity blocks' gradients do not depend on the mode
    assert {k[3:] for k in m._plans} == {("train_from", "layer4"), ("train_blocks", 2)}


@pytest.mark.gpu
def test_forward_follows_an_optimizer_step(dev):
    from two_stage_object_detection_amd import optim
    from two_stage_object_detection_amd.models.resnet import resnet50
    m = unfreeze(seeded_backbone(dev), "layer4")
    x = images(8, dev)
    with torch.no_grad():
        stale = m(x).clone()
    f = m(x)
    f.backward(torch.ones_like(f))
    version = m.weights_version
    frozen_pack = m._packed_cache[("layer3.5.conv1", x.device)]
    for key in ("layer4.0.conv3.grad", "layer4.0.downsample.grad", "layer4.0.conv2.s2d", "layer4.0.conv3+downsample"):
        assert (key, x.device) in m._packed_cache, key
    optim.AdamW(m.trainable_parameters(), lr=1e-3).step()
    assert m.refresh_packs().weights_version > version
    assert not [k for k in m._packed_cache if isinstance(k[0], str) and k[0].startswith("layer4.")]
    assert m._packed_cache[("layer3.5.conv1", x.device)] is frozen_pack      # a frozen block keeps its packs
    after = m(x).detach().clone()
    fresh = resnet50(include_top=False)
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = fresh(x)
    assert not torch.equal(after, stale) and torch.equal(after, want)


@pytest.mark.gpu
def test_a_slope_that_is_not_positive_is_refused_in_a_projection_block(dev):
    from two_stage_object_detection_amd._ffi import TsodError
    m = unfreeze(seeded_backbone(dev), "layer4")
    x = images(9, dev)
    with torch.no_grad():
        m.layer4[0].relu.weight.fill_(0.0)
    with pytest.raises(TsodError, match=r"layer4\.0"):
        m(x)


# the size tests/golden/trainer_ref.npz uses: ProposalTargetCreator keeps its n_sample samples there with these weights
TRAINER_HW = (320, 448)


@pytest.mark.gpu
def test_trainer_backbone_grads_layer4(dev, golden_dir):
    """``backbone_grads="layer4"``: every one of the 33 backbone tensors and the eight head tensors gets a finite gradient, and
    the four losses are those of the same trainer on the ``features=tr.feat_extra(x)`` recipe."""
    from two_stage_object_detection_amd._ffi import TsodError
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    from two_stage_object_detection_amd.testing import synthetic_detector
    z = np.load(os.path.join(golden_dir, "trainer_ref.npz"))
    img = torch.from_numpy(z["img_u8"]).float() / 255
    assert tuple(img.shape[1:]) == TRAINER_HW
    x = img[None].to(dev)
    bbox, label = torch.from_numpy(z["bbox"]).to(dev), torch.from_numpy(z["label"]).to(dev)
    _, sd = synthetic_detector("resnet50", num_classes=80, seed=0)
    sd = {("feat_extra." + k[len("extractor."):] if k.startswith("extractor.") else k): v for k, v in sd.items()}
    tr = FasterRCNNTrainer("train", 80, backbone="resnet50", head_grads=True, backbone_grads="layer4")
    tr.load_state_dict(sd, strict=True)
    tr = tr.to(dev).eval()
    with pytest.raises(TsodError, match="layer4"):                 # the frozen-backbone check names the stage
        tr(x, [bbox], [label])
    tr.feat_extra.requires_grad_(False)
    ours = unfreeze(tr.feat_extra, "layer4").trainable_parameters()
    tr.feat_extra.set_train_mode(None)                             # (forward sets the mode itself)
    assert len(ours) == 33
    losses = tr(x, [bbox], [label])[0]
    assert tr.feat_extra.train_mode == "layer4"
    (losses[-1] / 32).backward()
    heads = tr._head_params()
    assert len(heads) == 8
    for p in list(ours) + list(heads):
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all())
    assert all(bool(p.grad.any()) for p in ours)
    assert all(p.grad is None for k, p in tr.feat_extra.named_parameters() if not k.startswith("layer4."))
    got = [p.grad.clone() for p in ours]
    # the documented recipe on the same trainer: the same forward, the same bits
    clear(tr)
    recipe = tr(x, [bbox], [label], features=tr.feat_extra(x))[0]
    assert len(losses) == 5 and all(torch.equal(a.detach(), b.detach()) for a, b in zip(losses[:4], recipe[:4]))
    (recipe[-1] / 32).backward()
    assert all(torch.equal(p.grad, g) for p, g in zip(ours, got))
