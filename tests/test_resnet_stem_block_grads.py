"""ResNet.train_from("stem") / train_full: the gradients of every parameter of the backbone against
tests/resnet_stem_grads_restated.py's float64 section, fed the image, the stem's output and every block's input and stage
outputs read back from the HIP run (``f.grad_fn.saved``), so that only the backward is under test.  The bar:
|err| <= (n + 8) 2^-24 T elementwise."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resnet_stem_grads_restated import assert_within, stem_section_reference  # noqa: E402
from test_resnet_stage_block_grads import (IDENTITY_KEYS, PROJECTION_KEYS, TRAINER_HW, clear, images, nchw,  # noqa: E402
                                           seeded_backbone, unfreeze)

STEM = ["conv1.weight", "bn1.weight", "bn1.bias", "relu.weight"]
STEM_KEYS = {"x4", "y", "w", "scale", "slope", "bn"}
BLOCKS = [f"layer{li}.{i}" for li, n in zip((1, 2, 3, 4), (3, 4, 6, 3)) for i in range(n)]


def reference_for(m, f, gy):
    """{name: (gradient, T, n)} of the whole backbone that produced ``f``, from the node's saved tensors."""
    sv = f.grad_fn.saved
    blocks = []
    for b in sv["blocks"]:
        blk = copy.deepcopy(m.get_submodule(b["name"])).cpu().double()
        assert float(blk.relu.weight.detach()) == b["slope"]
        blocks.append((b["name"], blk, {k: nchw(b[k]) for k in ("x", "y1", "y2", "y3")}))
    owner = types.SimpleNamespace(**{k: copy.deepcopy(getattr(m, k)).cpu().double() for k in ("conv1", "bn1", "relu")})
    assert float(owner.relu.weight.detach()) == sv["stem"]["slope"]
    stem = (owner, dict(x=nchw(sv["stem"]["x4"][..., :3]), y=nchw(sv["stem"]["y"])))
    return stem_section_reference(stem, blocks, gy.cpu())


def check_all(m, ref, label):
    names = [k for k, _ in m._trainable_named()]
    assert set(ref) == set(names) and len(names) == 176
    worst = {}
    for name, p in zip(names, m.trainable_parameters()):
        assert p.grad is not None and p.grad.shape == p.shape, name
        g, T, cnt = ref[name]
        assert_within(p.grad, g, T, cnt, name)
        kind = "stem." + name if name in STEM else ".".join(name.split(".")[2:])
        ratio = float(((p.grad.double().cpu() - g).abs() / ((cnt + 8) * 2.0 ** -24 * T).clamp_min(1e-300)).max())
        worst[kind] = max(worst.get(kind, 0.0), ratio)
    print(f"{label}: largest err / bar per tensor kind: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,hw", [((2, 3, 64, 96), (2, 3)), ((1, 3, 61, 93), (2, 3))])
def test_train_from_stem_output_unchanged_and_gradients_match_f64(dev, shape, hw):
    m = seeded_backbone(dev)
    x = images(1, dev, shape)
    with torch.no_grad():
        plain = m(x).clone()
    assert tuple(plain.shape[2:]) == hw
    gy = torch.randn(plain.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    assert torch.equal(unfreeze(m, "layer2")(x).detach(), plain)
    m.requires_grad_(False)
    m.train_full()
    assert not m(x).requires_grad                                  # nothing of the section requires grad: the plain map
    unfreeze(m, "stem")
    assert len(m.trainable_parameters()) == 176 == len(list(m.parameters()))
    f = m(x)
    assert f.requires_grad and torch.equal(f.detach(), plain)      # the bits of train_from("layer2") and of inference
    sv = f.grad_fn.saved
    N, _, H, W = shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert set(sv["stem"]) == STEM_KEYS and tuple(sv["stem"]["x4"].shape) == (N, H, W, 4)
    assert tuple(sv["stem"]["y"].shape) == (N, OH, OW, 64) and tuple(sv["stem"]["w"].shape) == (64, 7, 8, 4)
    assert torch.equal(sv["stem"]["x4"][..., :3], x.permute(0, 2, 3, 1))
    assert [b["name"] for b in sv["blocks"]] == BLOCKS and sv["names"][:4] == STEM
    first = sv["blocks"][0]
    assert tuple(first["x"].shape) == (N, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1, 64)                # the pooled map
    assert torch.equal(first["x"], torch.nn.functional.max_pool2d(sv["stem"]["y"].permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))
    assert set(first) == PROJECTION_KEYS and first["stride"] == 1 and first["rot"] is not None and first["s2d"] is None
    assert all(set(b) == IDENTITY_KEYS for b in sv["blocks"][1:3])
    f.backward(gy)
    check_all(m, reference_for(m, f, gy), f"train_from('stem') {shape}")
    assert {k[3:] for k in m._plans} == {(), ("train_from", "layer2"), ("train_from", "stem")}
    got = [p.grad.clone() for p in m.trainable_parameters()]
    # the one-launch switches: inference takes its fused plan, the "stem" plan keeps its per-layer launches and its bits
    m.set_fuse_stem(True).set_fuse_bottleneck(True, projection=True)
    clear(m)
    f2 = m.forward_nhwc(x)
    assert f2.requires_grad and torch.equal(f2.detach().permute(0, 3, 1, 2), plain)
    train_plan = m._plan_for(x, 0)
    assert train_plan.stem_step is None and not train_plan.fused_steps
    f2.backward(gy.permute(0, 2, 3, 1).contiguous())
    assert all(torch.equal(p.grad, g) for p, g in zip(m.trainable_parameters(), got))       # and the same bits, run to run
    with torch.no_grad():
        fused = m(x)
        infer_plan = m._plan_for(x, 0)
    assert infer_plan.stem_step is not None and len(infer_plan.fused_steps) > 1 and fused.shape == plain.shape
    # "stem" is saved in this mode only
    m.train_from("layer2")
    assert "stem" not in m(x).grad_fn.saved
    m.set_train_mode(None)
    assert not m(x).requires_grad


@pytest.mark.gpu
def test_frozen_stem_tensors_leave_the_other_gradients_bit_equal(dev):
    m = unfreeze(seeded_backbone(dev), "stem")
    x = images(3, dev)
    gy = torch.randn(2, 2048, 2, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    m(x).backward(gy)
    full = {k: p.grad.clone() for k, p in m._trainable_named()}
    assert all(bool(full[k].any()) for k in STEM)
    clear(m)
    for k, p in m._trainable_named():
        p.requires_grad_(k not in STEM)
    f = m(x)
    assert set(f.grad_fn.saved["stem"]) == STEM_KEYS              # the plan is the same; the backward runs no stem launch
    f.backward(gy)
    for k, p in m._trainable_named():
        if k in STEM:
            assert p.grad is None, k
        else:
            assert torch.equal(p.grad, full[k]), k
    # any one of the four brings the stem's launches back, with the bits of the unfrozen run
    clear(m)
    m.bn1.bias.requires_grad_(True)
    m(x).backward(gy)
    assert torch.equal(m.bn1.bias.grad, full["bn1.bias"]) and m.conv1.weight.grad is None
    assert torch.equal(m.layer1[0].conv1.weight.grad, full["layer1.0.conv1.weight"])


@pytest.mark.gpu
def test_forward_follows_an_optimizer_step_over_all_176_tensors(dev):
    from two_stage_object_detection_amd import optim
    from two_stage_object_detection_amd.models.resnet import resnet50
    m = unfreeze(seeded_backbone(dev), "stem")
    x = images(8, dev)
    with torch.no_grad():
        stale = m(x).clone()
    f = m(x)
    f.backward(torch.ones_like(f))
    version = m.weights_version
    assert ("conv1", x.device) in m._packed_cache
    optim.AdamW(m.trainable_parameters(), lr=1e-3).step()
    assert m.refresh_packs().weights_version > version
    assert not [k for k in m._packed_cache if isinstance(k[0], str) and k[0].startswith(("conv1", "layer"))]   # every pack dropped
    after = m(x).detach().clone()
    fresh = resnet50(include_top=False)
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = fresh(x)
    assert not torch.equal(after, stale) and torch.equal(after, want)
    # a change of the stem alone drops the stem's packs and nothing else
    block_pack = m._packed_cache[("layer1.0.conv1", x.device)]
    version = m.weights_version
    with torch.no_grad():
        m.relu.weight.mul_(1.5)
    assert m.refresh_packs().weights_version > version and ("conv1", x.device) not in m._packed_cache
    assert m._packed_cache[("layer1.0.conv1", x.device)] is block_pack
    # a narrower mode after "stem": it works, and the stem stays watched
    clear(m)
    m.train_from("layer4")
    f4 = m(x)
    assert "stem" not in f4.grad_fn.saved and {"conv1", "bn1", "relu"} <= set(m.__dict__["_watched"])
    f4.backward(torch.ones_like(f4))
    assert m.conv1.weight.grad is None and m.layer4[0].conv1.weight.grad is not None
    version = m.weights_version
    with torch.no_grad():
        m.bn1.weight.mul_(1.1)
    with torch.no_grad():
        moved = m(x)
    assert m.weights_version > version and not torch.equal(moved, f4.detach())


@pytest.mark.gpu
def test_a_stem_slope_that_is_not_positive_is_refused(dev):
    from two_stage_object_detection_amd._ffi import TsodError
    m = unfreeze(seeded_backbone(dev), "stem")
    with torch.no_grad():
        m.relu.weight.fill_(0.0)
    with pytest.raises(TsodError, match="stem's PReLU slope"):
        m(images(9, dev))


@pytest.mark.gpu
def test_trainer_backbone_grads_stem(dev, golden_dir):
    """``backbone_grads="stem"``: the four losses are those of ``backbone_grads="layer2"`` bit for bit, all 176 backbone tensors get a
    finite gradient, and the four stem tensors meet the bar against the float64 section fed the gradient of the feature map."""
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
    losses = {}
    for mode in ("layer2", "stem"):
        tr = FasterRCNNTrainer("train", 80, backbone="resnet50", head_grads=True, backbone_grads=mode)
        tr.load_state_dict(sd, strict=True)
        tr = tr.to(dev).eval()
        if mode == "layer2":
            with pytest.raises(TsodError, match="layer2"):
                tr(x, [bbox], [label])
        tr.feat_extra.requires_grad_(False)
        ours = unfreeze(tr.feat_extra, mode).trainable_parameters()
        tr.feat_extra.set_train_mode(None)                         # (forward sets the mode itself)
        losses[mode] = [v.detach().clone() for v in tr(x, [bbox], [label])[0]]
        assert tr.feat_extra.train_mode == mode
    assert len(ours) == 176
    assert all(torch.equal(a, b) for a, b in zip(losses["stem"], losses["layer2"]))
    out = tr(x, [bbox], [label])[0]
    (out[-1] / 32).backward()
    for p in list(ours) + list(tr._head_params()):
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all())
    assert all(bool(p.grad.any()) for p in ours)
    got = {k: p.grad.clone() for k, p in tr.feat_extra._trainable_named()}
    # the documented recipe on the same trainer gives the same bits, and the gradient of the map for the reference
    clear(tr)
    f = tr.feat_extra(x)
    f.retain_grad()
    recipe = tr(x, [bbox], [label], features=f)[0]
    assert all(torch.equal(a.detach(), b) for a, b in zip(recipe[:4], losses["stem"][:4]))
    (recipe[-1] / 32).backward()
    assert all(torch.equal(p.grad, got[k]) for k, p in tr.feat_extra._trainable_named())
    ref = reference_for(tr.feat_extra, f, f.grad)
    for k in STEM:
        assert_within(got[k], *ref[k], "trainer " + k)
