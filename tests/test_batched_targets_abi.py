"""The batched target assignment without a GPU: the four symbols are exported and bound, the workspace formulas are the
ones include/tsod.h states (0 for refused arguments), every refusal comes back before anything is launched, the creators'
``batch`` validates gt_counts on the host, and a trainer whose creators were replaced by plain callables stays on the
per-image route."""
import os
import re

import pytest
import torch

from two_stage_object_detection_amd import _ffi, hip_ops
from two_stage_object_detection_amd.nets import frcnn_training as ft
from two_stage_object_detection_amd.utils import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, ALIGNMENT, WORKSPACE = 0, -1, -3, -4
P = 0x10000          # a fake, 16-byte aligned "device pointer": validation must fail before it is ever dereferenced
ODD = P + 4
BIG = 1 << 30
SYMBOLS = ("tsod_anchor_targets_batch_workspace_bytes", "tsod_anchor_targets_batch_f32",
           "tsod_proposal_targets_batch_workspace_bytes", "tsod_proposal_targets_batch_f32")


def _a16(n):
    return (n + 15) // 16 * 16


def _header():
    with open(os.path.join(ROOT, "include", "tsod.h")) as f:
        return f.read()


def test_symbols_are_declared_bound_and_exported():
    L = _ffi.lib()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in SYMBOLS:
        assert name in _ffi.EXPORTED_SYMBOLS and hasattr(L, name)
        assert len(re.findall(rf"\b{name}\s*\(", code)) == 1
    decl = {n: re.search(rf"\b{n}\s*\(([^;]*)\);", code).group(1) for n in SYMBOLS}
    for name in SYMBOLS:                                             # as many parameters bound as declared
        assert len(decl[name].split(",")) == len(_ffi._SIGNATURES[name][1]), name
    assert "const int32_t *gt_counts" in decl["tsod_anchor_targets_batch_f32"]
    assert "int32_t *sample_src" in decl["tsod_proposal_targets_batch_f32"]
    assert L.tsod_version() == 242                                   # the change only adds exports


def test_workspace_formulas_are_the_headers():
    L, text = _ffi.lib(), " ".join(_header().split())
    assert "tsod_anchor_targets_batch_workspace_bytes(B, A, Gmax) = B * (align16(4 A) + align16(4 max(Gmax, 1)) + 16)" in text
    assert ("tsod_proposal_targets_batch_workspace_bytes(B, R, Gmax, n_sample) = B * (2 align16(4 (R + Gmax)) + "
            "align16(4 n_sample))") in text
    for B, A, G in ((1, 1, 0), (5, 2049, 513), (3, 37800, 20), (2, 7, 1), (65535, 3, 2)):
        want = B * (_a16(4 * A) + _a16(4 * max(G, 1)) + 16)
        assert L.tsod_anchor_targets_batch_workspace_bytes(B, A, G) == want
        assert want == B * L.tsod_anchor_targets_workspace_bytes(A, G)
    for B, R, G, n in ((1, 1, 0, 5), (4, 1023, 513, 128), (16, 600, 8, 128), (2, 0, 1, 1)):
        want = B * (2 * _a16(4 * (R + G)) + _a16(4 * n))
        assert L.tsod_proposal_targets_batch_workspace_bytes(B, R, G, n) == want
        assert want == B * L.tsod_proposal_targets_workspace_bytes(R, G, n)
    for B, A, G in ((0, 8, 2), (-1, 8, 2), (65536, 8, 2), (2, 0, 2), (2, -3, 2), (2, 8, -1)):
        assert L.tsod_anchor_targets_batch_workspace_bytes(B, A, G) == 0
    for B, R, G, n in ((0, 8, 2, 4), (-2, 8, 2, 4), (65536, 8, 2, 4), (2, -1, 2, 4), (2, 8, -1, 4), (2, 0, 0, 4), (2, 8, 2, 0),
                       (2, 8, 2, -4)):
        assert L.tsod_proposal_targets_batch_workspace_bytes(B, R, G, n) == 0


def _anchor(L, anchor=P, A=10, bbox=P, counts=P, B=2, G=3, pos=0.7, neg=0.3, n_pos=128, n_sample=256, loc=P, label=P,
            argmax=P, ws=P, ws_bytes=BIG):
    return L.tsod_anchor_targets_batch_f32(anchor, A, bbox, counts, B, G, pos, neg, n_pos, n_sample, loc, label, argmax, ws,
                                           ws_bytes, None)


def _proposal(L, roi=P, R=10, bbox=P, gt_label=P, counts=P, B=2, G=3, n_sample=128, ppi=64, s_roi=P, s_loc=P, s_lab=P, cnt=P,
              src=None, ws=P, ws_bytes=BIG):
    return L.tsod_proposal_targets_batch_f32(roi, R, bbox, gt_label, counts, B, G, n_sample, ppi, 0.5, 0.5, 0.0, s_roi, s_loc,
                                             s_lab, cnt, src, ws, ws_bytes, None)


def test_every_refusal_comes_before_a_launch():
    """Fake pointers: a call that got as far as a launch would not return one of these codes."""
    L = _ffi.lib()
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(A=0), dict(G=-1), dict(anchor=None), dict(loc=None), dict(label=None),
               dict(argmax=None), dict(bbox=None), dict(counts=None), dict(n_pos=-1), dict(n_sample=-1),
               dict(n_pos=129, n_sample=128), dict(pos=0.0)):
        assert _anchor(L, **kw) == INVALID, kw
    for kw in (dict(anchor=ODD), dict(loc=ODD), dict(bbox=ODD)):
        assert _anchor(L, **kw) == ALIGNMENT, kw
    need = L.tsod_anchor_targets_batch_workspace_bytes(2, 10, 3)
    for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=ODD),
               dict(ws_bytes=L.tsod_anchor_targets_workspace_bytes(10, 3))):         # one image's share is not enough for two
        assert _anchor(L, **kw) == WORKSPACE, kw
    for kw in (dict(B=0), dict(B=-3), dict(B=65536), dict(R=-1), dict(G=-1), dict(R=0, G=0), dict(n_sample=0), dict(ppi=-1),
               dict(ppi=129), dict(roi=None), dict(bbox=None), dict(gt_label=None), dict(counts=None), dict(s_roi=None),
               dict(s_loc=None), dict(s_lab=None), dict(cnt=None)):
        assert _proposal(L, **kw) == INVALID, kw
    for kw in (dict(roi=ODD), dict(bbox=ODD), dict(s_roi=ODD), dict(s_loc=ODD)):
        assert _proposal(L, **kw) == ALIGNMENT, kw
    need = L.tsod_proposal_targets_batch_workspace_bytes(2, 10, 3, 128)
    for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws=ODD), dict(ws_bytes=L.tsod_proposal_targets_workspace_bytes(10, 3, 128))):
        assert _proposal(L, **kw) == WORKSPACE, kw
    for src in (None, P):                                            # sample_src is optional: both forms pass the argument checks
        assert _proposal(L, src=src, ws_bytes=need - 1) == WORKSPACE


# ------------------------------------------------------------------------------------------------ the creators, on the host
@pytest.fixture
def no_device(monkeypatch):
    """CPU tensors pass for GPU tensors and the two batched hip_ops record their arguments instead of launching."""
    calls = []
    for mod in (ft, metrics, hip_ops):
        monkeypatch.setattr(mod, "require_cuda", lambda t, what: None)

    def anchor_targets_batch(bbox, gt_counts, anchor, n_pos, n_sample, pos, neg):
        calls.append(("anchor_batch", bbox, gt_counts))
        B, A = bbox.shape[0], anchor.shape[0]
        return torch.zeros(B, A, 4), torch.zeros(B, A, dtype=torch.int64), torch.zeros(B, A, dtype=torch.int32)

    def proposal_targets_batch(roi, bbox, label, gt_counts, n_sample, ppi, pos, hi, lo, want_src=False):
        calls.append(("proposal_batch", bbox, label, gt_counts, want_src))
        B = roi.shape[0]
        counts = torch.tensor([[n_sample, 1, n_sample - 1, 0]] * B, dtype=torch.int32)
        return (torch.zeros(B, n_sample, 4), torch.zeros(B, n_sample, 4), torch.zeros(B, n_sample, dtype=torch.int64), counts,
                torch.zeros(B, n_sample, dtype=torch.int32) if want_src else None)

    def single(name):
        def fn(*a, **k):
            calls.append((name,))
            raise AssertionError(f"hip_ops.{name} must not be reached")
        return fn
    monkeypatch.setattr(hip_ops, "anchor_targets_batch", anchor_targets_batch)
    monkeypatch.setattr(hip_ops, "proposal_targets_batch", proposal_targets_batch)
    for name in ("anchor_targets", "proposal_targets", "proposal_targets_src"):
        monkeypatch.setattr(hip_ops, name, single(name))
    return calls


def test_batch_validates_gt_counts_on_the_host(no_device):
    anchor, rois = torch.zeros(12, 4), torch.zeros(2, 6, 4)
    bb, lb = torch.rand(2, 3, 4), torch.zeros(2, 3, dtype=torch.int64)
    a, p = ft.AnchorTargetCreator(), ft.ProposalTargetCreator()
    for bad in ([4, 1], [-1, 2], torch.tensor([0, 7]), (3, 3, 3), [1]):
        with pytest.raises(ValueError, match="gt_counts"):
            a.batch(bb, anchor, gt_counts=bad)
        with pytest.raises(ValueError, match="gt_counts"):
            p.batch(rois, bb, lb, gt_counts=bad)
    with pytest.raises(ValueError, match="gt_counts"):               # lists carry their own counts
        a.batch([bb[0], bb[1]], anchor, gt_counts=[3, 3])
    assert no_device == []                                           # ... all of it before any launch
    loc, label = a.batch(bb, anchor, gt_counts=[0, 3])
    assert loc.shape == (2, 12, 4) and label.shape == (2, 12)
    out = p.batch(rois, bb, lb, gt_counts=torch.tensor([3, 0]), with_sources=True)
    assert [tuple(o.shape) for o in out] == [(2, 128, 4), (2, 128, 4), (2, 128), (2, 4), (2, 128)]
    assert p.batch(rois, bb, lb)[4] is None
    kinds = [c[0] for c in no_device]
    assert kinds == ["anchor_batch", "proposal_batch", "proposal_batch"]
    assert no_device[0][2].tolist() == [0, 3] and no_device[0][2].dtype == torch.int32
    assert no_device[1][3].tolist() == [3, 0] and no_device[1][4] is True
    assert no_device[2][3].tolist() == [3, 3]                        # no gt_counts: every row counts


def test_lists_are_packed_like_the_evaluators(no_device):
    boxes = [torch.rand(2, 4), torch.rand(0, 4), torch.rand(3, 4)]
    labels = [torch.tensor([4, 5]), torch.zeros(0, dtype=torch.int64), torch.tensor([1, 2, 3])]
    ft.ProposalTargetCreator().batch(torch.zeros(3, 6, 4), boxes, labels)
    _, pb, pl, gc, _ = no_device[0]
    ev = metrics.DetectionEvaluator(8)._ground_truth(boxes, labels, 3, torch.device("cpu"), None)
    assert torch.equal(pb, ev[0]) and torch.equal(pl, ev[1]) and torch.equal(gc, ev[2])
    assert pb.shape == (3, 3, 4) and gc.tolist() == [2, 0, 3]
    gt = ft.pack_targets(boxes, labels, None, torch.device("cpu"), "test")
    assert gt.host_counts == (2, 0, 3) and torch.equal(gt.boxes, pb)
    ft.AnchorTargetCreator().batch(gt, torch.zeros(5, 4))            # packed once, handed to both creators
    assert no_device[1][1] is gt.boxes and no_device[1][2] is gt.counts
    same = ft.pack_targets([boxes[0], boxes[0] + 1], [labels[0], labels[0] + 1], None, torch.device("cpu"), "test")
    assert torch.equal(same.boxes, torch.stack([boxes[0], boxes[0] + 1])) and same.counts.tolist() == [2, 2]      # equal lengths: stacked
    assert torch.equal(same.labels, torch.stack([labels[0], labels[0] + 1])) and same.counts.dtype == torch.int32


def test_raise_for_counts_speaks_like_the_single_image_path():
    ft.raise_for_counts([[128, 3, 125, 0], [128, 64, 64, 0]], 128)
    ft.raise_for_counts([[5, 3, 2, 0]])                              # without n_sample (the creators): only the status counts
    with pytest.raises(IndexError, match="nets/frcnn_training.py:175"):
        ft.raise_for_counts([[128, 3, 125, 0], [25, 3, 22, 1]], 128)
    with pytest.raises(RuntimeError, match=r"kept 25 samples for image 1, fewer than n_sample = 128"):
        ft.raise_for_counts([[128, 3, 125, 0], [25, 3, 22, 0], [9, 9, 0, 1]], 128)        # image order: image 1 comes first
    with pytest.raises(IndexError):
        ft.raise_for_counts([[25, 3, 22, 1]], 128)                   # per image the T2 error before the Q5 one


def _trainer():
    tr = ft.FasterRCNNTrainer(mode="train", num_classes=80).eval()
    tr.proposal_target_creator.n_sample = 4
    return tr


def test_real_creators_take_the_batched_route(no_device):
    tr = _trainer()
    boxes, labels = [torch.rand(2, 4), torch.rand(1, 4)], [torch.tensor([1, 2]), torch.tensor([3])]
    out = tr._targets(boxes, labels, None, torch.zeros(9, 4), torch.zeros(2, 6, 4), torch.device("cpu"), True)
    assert [c[0] for c in no_device] == ["anchor_batch", "proposal_batch"]
    assert no_device[0][1] is no_device[1][1] and no_device[0][2] is no_device[1][3]      # packed and uploaded once
    assert out[0].shape == (2, 9, 4) and out[2].shape == (2, 4, 4) and out[5].shape == (2, 4) and out[6].shape == (2, 4)


def test_plain_callables_take_the_per_image_route(no_device):
    tr = _trainer()
    seen = []

    def a(bbox, anchor):
        seen.append(("a", bbox.shape[0]))
        return torch.zeros(anchor.shape[0], 4), torch.zeros(anchor.shape[0], dtype=torch.int64)

    def p(roi, bbox, label, std):
        seen.append(("p", bbox.shape[0], label.shape[0]))
        return torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4, dtype=torch.int64)
    a.n_sample, p.n_sample = 256, 4
    bb, lb = torch.rand(3, 5, 4), torch.zeros(3, 5, dtype=torch.int64)
    for swap in ("both", "anchor", "proposal"):                      # one plain callable is enough: the route is chosen per call
        tr = _trainer()
        if swap in ("both", "anchor"):
            tr.anchor_target_creator = a
        if swap == "both":
            tr.proposal_target_creator = p
        del seen[:], no_device[:]
        if swap == "both":
            out = tr._targets(bb, lb, [5, 0, 2], torch.zeros(9, 4), torch.zeros(3, 6, 4), torch.device("cpu"), False)
            assert seen == [("a", 5), ("p", 5, 5), ("a", 0), ("p", 0, 0), ("a", 2), ("p", 2, 2)]     # gt_counts cut each image
            assert no_device == [] and out[6] is None and out[5] is None and out[2].shape == (3, 4, 4)
        else:                                                        # the real creator of the pair goes through its single-image op
            if swap == "proposal":
                tr.proposal_target_creator = p
                with pytest.raises(AssertionError, match="anchor_targets must not be reached"):
                    tr._targets(bb, lb, None, torch.zeros(9, 4), torch.zeros(3, 6, 4), torch.device("cpu"), False)
            else:
                with pytest.raises(AssertionError, match="proposal_targets must not be reached"):
                    tr._targets(bb, lb, None, torch.zeros(9, 4), torch.zeros(3, 6, 4), torch.device("cpu"), False)
            assert all(c[0] in ("anchor_targets", "proposal_targets") for c in no_device) and len(no_device) == 1
