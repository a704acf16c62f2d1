"""ResNet's one training mode (DESIGN.md sections 4.21 - 4.24): what each mode reaches, what the refresh watches, and the one
backward walk's two variants - BatchNorm folded, BatchNorm on batch statistics - side by side on one module.  The counterpart of
tests/test_hardnet_train_modes.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def _backbones():
    from two_stage_object_detection_amd.models.resnet import Bottleneck, ResNet, resnet50
    return {"resnet50": lambda: resnet50(include_top=False),
            "one_block_per_stage": lambda: ResNet(Bottleneck, [1, 1, 1, 1], include_top=False)}


@pytest.mark.parametrize("which", ["resnet50", "one_block_per_stage"])
def test_every_mode_reaches_its_modules_parameters_and_norms_and_the_watch_only_grows(which):
    """What makes the refresh sound: in every mode ``trainable_parameters()`` is exactly the parameters of the mode's modules
    (``_stem_modules(mode) + _section(mode)``) in module order, ``_section_norms(mode)`` names each of their BatchNorms once, and
    ``_watched`` covers the widest mode set so far - nothing trainable is left unwatched after an optimizer step."""
    m = _backbones()[which]()
    order = {id(p): i for i, p in enumerate(m.parameters())}
    assert m.train_mode is None and m.trainable_parameters() == [] and "_watched" not in m.__dict__
    assert m.n_blocks == {"resnet50": 2, "one_block_per_stage": 0}[which]
    assert m.trainable_sections == ("layer4", "layer3", "layer2", "stem")
    widest = set()
    for mode in [None] + list(range(1, m.n_blocks + 1)) + list(m.trainable_sections):
        assert m.set_train_mode(mode) is m and m.train_mode == mode
        modules = [] if mode is None else m._stem_modules(mode) + m._section(mode)
        assert all(m.get_submodule(name) is mod for name, mod in modules)
        want = [p for _, mod in modules for p in mod.parameters()]
        got = m.trainable_parameters()
        assert [id(p) for p in got] == [id(p) for p in want], mode
        assert [order[id(p)] for p in got] == sorted(order[id(p)] for p in got) and len(set(map(id, got))) == len(got), mode
        if mode == "stem":
            assert [id(p) for p in got] == [id(p) for p in m.parameters()]
        if mode is not None:
            norms = m._section_norms(mode)
            bns = {".".join(k for k in (name, sub) if k): bn for name, mod in modules for sub, bn in mod.named_modules()
                   if isinstance(bn, torch.nn.BatchNorm2d)}
            assert len(norms) == len(bns) and {k: id(bn) for k, bn in norms} == {k: id(bn) for k, bn in bns.items()}, mode
        # the modes came in widening order: the watch is what the widest one so far reaches, and nothing before any
        now = set(m.__dict__.get("_watched", {}))
        assert now >= widest and now == {name for name, _ in modules}, mode
        widest = now
    assert widest == {"conv1", "bn1", "relu"} | {name for name, _ in m._section("stem")}
    for narrower in ("layer4", None):                                   # narrowing or switching off keeps the watch
        m.set_train_mode(narrower)
        assert set(m._watched) == widest


@pytest.mark.gpu
def test_the_folded_and_the_batch_statistics_walk_share_no_state_through_the_module(dev):
    """One module, mode "layer4": a folded forward + backward under .eval(), one on batch statistics under .train(), then - with
    the BatchNorm buffers put back and ``refresh_packs()`` called - the folded one again gives the first run's bits."""
    from test_resnet_stage_block_grads import IDENTITY_KEYS, PROJECTION_KEYS, clear, images, seeded_backbone
    m = seeded_backbone(dev)
    x = images(1, dev)
    gy = torch.randn(2, 2048, 2, 3, generator=torch.Generator().manual_seed(2)).to(dev)

    def step(batch_stats):
        m.set_train_mode("layer4", batch_stats).train(batch_stats)
        for p in m.trainable_parameters():
            p.requires_grad_(True)
        clear(m)
        f = m(x)
        f.backward(gy)
        return f.detach().clone(), [p.grad.clone() for p in m.trainable_parameters()], f.grad_fn.saved

    buffers = {k: v.detach().clone() for k, v in m.state_dict().items() if k.endswith(BUFFERS)}
    f0, g0, folded = step(False)
    assert "batch_stats" not in folded and "stem" not in folded and len(g0) == 33
    assert [set(b) for b in folded["blocks"]] == [PROJECTION_KEYS, IDENTITY_KEYS, IDENTITY_KEYS]

    f1, g1, batch = step(True)
    assert batch["batch_stats"] is True and batch["names"] == folded["names"]
    identity = (IDENTITY_KEYS - {"bn"}) | {"bnt", "stride", "s2d"}
    assert [set(b) for b in batch["blocks"]] == [identity | {"wd", "bnt_d"}, identity, identity]
    for b in batch["blocks"]:
        assert all(set(t) == {"z", "mean", "invstd", "gamma", "C"} for t in b["bnt"])
        assert all(torch.equal(s, torch.ones_like(s)) for s in b["scale"])
    assert not torch.equal(f1, f0)                                      # (the batch's statistics are not the running ones)
    moved = {k: v for k, v in m.state_dict().items() if k.endswith(BUFFERS)}
    assert all(torch.equal(moved[k], buffers[k]) != k.startswith("layer4.") for k in buffers)

    with torch.no_grad():
        for k, v in moved.items():
            v.copy_(buffers[k])
    m.refresh_packs()
    f2, g2, again = step(False)
    assert "batch_stats" not in again and [set(b) for b in again["blocks"]] == [PROJECTION_KEYS, IDENTITY_KEYS, IDENTITY_KEYS]
    assert torch.equal(f2, f0)
    for name, a, b in zip(folded["names"], g0, g2):
        assert torch.equal(a, b), name
