"""tsod_anchor_targets_batch_f32 / tsod_proposal_targets_batch_f32 (hip_ops.anchor_targets_batch / proposal_targets_batch):
a whole batch in one pass, every image with its own number of ground-truth boxes inside one launch.

References: tests/targets_restated.py per image (the CPU restatement test_targets_restated.py ties to the oracle and to the
reference's recordings) and the single-image entry points on the same device.  Bars, the project's existing ones: labels,
argmax, gt_roi_label, the count words and sample_src exact; gathered sample_roi rows bit-exact; loc / gt_roi_loc with the same
finiteness pattern and a relative error <= LOC_REL_BAR against the restatement; against the single-image calls everything is
torch.equal, locs included (they are the same kernels: a single image is a batch of one).  The facts that make the inputs worth running (which images are
cut by the cap, where T1 and T2 fire, how many LDS trips and which chunk each image takes) are asserted from the restatement
before the GPU is looked at."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import targets_restated as T  # noqa: E402

pytestmark = pytest.mark.gpu

F_SENT, I_SENT, L_SENT = -777.25, -123456789, -987654321
PAD = 16                                 # sentinel rows / words behind every output and behind the workspace

A_N, A_G = 2049, (0, 1, 256, 257, 513)
ANCHOR_SETS = {"cap500": dict(n_sample=1000, pos_ratio=0.5, **T.ANCHOR_THR), "t1": dict(n_sample=500, pos_ratio=1.0, **T.ANCHOR_THR)}
P_R, P_G = 1023, (0, 2, 257, 513)
P_KW = dict(n_sample=128, pos_ratio=0.5, pos_iou_thresh=T.PROPOSAL_THR[0], neg_iou_thresh_high=T.PROPOSAL_THR[1],
            neg_iou_thresh_low=T.PROPOSAL_THR[2])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _a16(n):
    return (n + 15) // 16 * 16


def _bits(t):
    return t.view(torch.int32) if t.is_floating_point() else t


def _pad(rows, Gmax, fill, dtype):
    """A list of [G_i, ...] tensors as one [B, Gmax, ...] tensor, ``fill`` in the pad rows."""
    out = torch.full((len(rows), Gmax) + tuple(rows[0].shape[1:]), fill, dtype=dtype)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out


# ================================================================================================ inputs and references, once
@pytest.fixture(scope="module")
def anchors():
    anchor = T.grid_boxes(_gen(101), A_N, 30)
    boxes = [T.grid_boxes(_gen(200 + i), g, 30) for i, g in enumerate(A_G)]
    want = {name: [T.anchor_stages(b, anchor, **kw) for b in boxes] for name, kw in ANCHOR_SETS.items()}
    # ---- what these inputs are for, from the restatement alone
    assert [w["total_pos"] for w in want["cap500"]] == [0, 3, 496, 524, 824]
    assert [w["total_pos"] > w["n_pos"] for w in want["cap500"]] == [False, False, False, True, True]        # the cap of 500 cuts 3 and 4
    assert [w["n_pos"] for w in want["cap500"]] == [500] * 5
    t1 = want["t1"]
    assert [w["n_neg"] for w in t1] == [500, 497, 4, 0, 0]
    assert all(bool((w["label_cap"] == 0).any()) for w in t1[2:])                  # there are negatives to lose ...
    assert not (t1[3]["label"] == 0).any() and not (t1[4]["label"] == 0).any()     # ... T1 takes them all in images 3 and 4
    assert (t1[2]["label"] == 0).any()                                             # ... and spares image 2 (n_neg = 4)
    assert [-(-g // T.ROW_BLOCK) for g in A_G] == [0, 1, 1, 2, 3]                  # trips of the 256-box LDS loop, one launch
    assert [w["flag"] for w in want["cap500"]] == [0, 1, 1, 1, 1]
    return dict(anchor=anchor, boxes=boxes, want=want)


@pytest.fixture(scope="module")
def proposals():
    imgs = []
    for i, G in enumerate(P_G):
        g = _gen(300 + i)
        bbox = T.grid_boxes(g, G, 24)
        label = torch.randint(0, 20, (G,), generator=g)
        roi = T.grid_boxes(g, P_R, 24)
        imgs.append(dict(roi=roi, bbox=bbox, label=label))
    want = [T.proposal_stages(c["roi"], c["bbox"], c["label"], **P_KW) for c in imgs]
    assert [(w["S"], w["status"]) for w in want] == [(0, 0), (25, 1), (128, 0), (128, 1)]     # S = 0, 0 < S < n, S = n; T2 on and off
    assert [T.chunk_of(w["N"]) for w in want] == [1, 2, 2, 2]                      # chunk differs per image within one launch
    return dict(imgs=imgs, want=want)


@pytest.fixture(scope="module")
def ops():
    from two_stage_object_detection_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def ffi():
    from two_stage_object_detection_amd import _ffi
    return _ffi


def _n_pos(kw):
    return int(kw["pos_ratio"] * kw["n_sample"])


def _check_loc(got, ref):
    same, rel = T.loc_error(got.cpu(), ref)
    assert same, "finiteness pattern differs"
    assert rel <= T.LOC_REL_BAR, rel


def check_anchor_image(loc, label, argmax, want):
    assert torch.equal(label.cpu(), want["label"])
    assert torch.equal(argmax.cpu().long(), want["argmax"])
    _check_loc(loc, want["loc"])


def check_proposal_image(s_roi, s_loc, s_lab, counts, src, want, case):
    """One image's rows of a batched call: the first S as check_proposal of test_target_kernels_gpu.py has them, the rest zeros."""
    S = want["S"]
    assert counts.tolist() == [S, want["pos_len"], want["neg_len"], want["status"]]
    s_roi, s_loc, s_lab = s_roi.cpu(), s_loc.cpu(), s_lab.cpu()
    assert torch.equal(s_roi[:S], want["sample_roi"])                                # gathered: bit-exact
    _check_loc(s_loc[:S], want["loc"])
    if want["status"]:                                                               # the reference raises: outside the T2 positions
        outside = torch.ones(S, dtype=torch.bool)
        outside[want["t2"]] = False
        assert torch.equal(s_lab[:S][outside], want["label_before"][outside])
    else:
        assert torch.equal(s_lab[:S], want["label_after"])
    assert (_bits(s_roi[S:]) == 0).all() and (_bits(s_loc[S:]) == 0).all() and (s_lab[S:] == 0).all()      # +0.0, not -0.0
    if src is not None:
        src = src.cpu().long()
        assert torch.equal(src[:S], want["keep"]) and (src[S:] == -1).all()
        assert torch.equal(torch.cat((case["roi"], case["bbox"]))[src[:S]], s_roi[:S])


# ================================================================================================ through the C ABI
def abi_anchor_batch(ffi, dev, anchor, pb, gc, kw, ws=None):
    """Sentinel-filled outputs with PAD rows behind them, a workspace of exactly the size asked for with PAD sentinel words
    behind it (or ``ws``: the tensor an earlier call of the same size left its data in)."""
    B, Gmax = pb.shape[:2]
    A = anchor.shape[0]
    L = ffi.lib()
    need = L.tsod_anchor_targets_batch_workspace_bytes(B, A, Gmax)
    assert need == B * (_a16(4 * A) + _a16(4 * max(Gmax, 1)) + 16)
    if ws is None:
        ws = torch.full((need // 4 + PAD,), I_SENT, dtype=torch.int32, device=dev)
    loc = torch.full((B * A + PAD, 4), F_SENT, dtype=torch.float32, device=dev)
    label = torch.full((B * A + PAD,), L_SENT, dtype=torch.int64, device=dev)
    argmax = torch.full((B * A + PAD,), I_SENT, dtype=torch.int32, device=dev)
    before = (anchor.clone(), None if pb is None else pb.clone(), None if gc is None else gc.clone())
    ffi.check(L.tsod_anchor_targets_batch_f32(ffi.ptr(anchor), A, ffi.ptr(pb) if Gmax else None, ffi.ptr(gc) if Gmax else None, B,
                                              Gmax, kw["pos_iou_thresh"], kw["neg_iou_thresh"], _n_pos(kw), kw["n_sample"],
                                              ffi.ptr(loc), ffi.ptr(label), ffi.ptr(argmax), ffi.ptr(ws), need, ffi.stream_ptr()),
              "anchor_targets_batch")
    assert (loc[B * A:] == F_SENT).all() and (label[B * A:] == L_SENT).all() and (argmax[B * A:] == I_SENT).all()
    assert (ws[need // 4:] == I_SENT).all()
    for x, y in zip((anchor, pb, gc), before):                                       # the inputs are inputs (NaN pad rows included)
        assert y is None or torch.equal(_bits(x), _bits(y))
    return dict(loc=loc[:B * A].view(B, A, 4), label=label[:B * A].view(B, A), argmax=argmax[:B * A].view(B, A), ws=ws)


def abi_proposal_batch(ffi, dev, roi, pb, pl, gc, kw, with_src, ws=None):
    B, R = roi.shape[:2]
    Gmax, n = pb.shape[1], kw["n_sample"]
    L = ffi.lib()
    need = L.tsod_proposal_targets_batch_workspace_bytes(B, R, Gmax, n)
    assert need == B * (2 * _a16(4 * (R + Gmax)) + _a16(4 * n))
    if ws is None:
        ws = torch.full((need // 4 + PAD,), I_SENT, dtype=torch.int32, device=dev)
    s_roi = torch.full((B * n + PAD, 4), F_SENT, dtype=torch.float32, device=dev)
    s_loc = torch.full((B * n + PAD, 4), F_SENT, dtype=torch.float32, device=dev)
    s_lab = torch.full((B * n + PAD,), L_SENT, dtype=torch.int64, device=dev)
    src = torch.full((B * n + PAD,), I_SENT, dtype=torch.int32, device=dev)
    counts = torch.full((4 * B + PAD,), I_SENT, dtype=torch.int32, device=dev)
    gt = [ffi.ptr(t) if Gmax else None for t in (pb, pl, gc)]
    ffi.check(L.tsod_proposal_targets_batch_f32(ffi.ptr(roi), R, *gt, B, Gmax, n, int(n * kw["pos_ratio"]), kw["pos_iou_thresh"],
                                                kw["neg_iou_thresh_high"], kw["neg_iou_thresh_low"], ffi.ptr(s_roi), ffi.ptr(s_loc),
                                                ffi.ptr(s_lab), ffi.ptr(counts), ffi.ptr(src) if with_src else None, ffi.ptr(ws),
                                                need, ffi.stream_ptr()), "proposal_targets_batch")
    assert (s_roi[B * n:] == F_SENT).all() and (s_loc[B * n:] == F_SENT).all() and (s_lab[B * n:] == L_SENT).all()
    assert (counts[4 * B:] == I_SENT).all() and (src[B * n if with_src else 0:] == I_SENT).all()
    assert (ws[need // 4:] == I_SENT).all()
    return dict(sample_roi=s_roi[:B * n].view(B, n, 4), loc=s_loc[:B * n].view(B, n, 4), label=s_lab[:B * n].view(B, n),
                counts=counts[:4 * B].view(B, 4).cpu(), src=src[:B * n].view(B, n) if with_src else None, ws=ws)


def _same_outputs(a, b, keys):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None
        else:
            assert torch.equal(_bits(a[k]), _bits(b[k])), k


def _anchor_inputs(anchors, dev, Gmax=None, fill=0.0):
    Gmax = max(A_G) if Gmax is None else Gmax
    pb = _pad(anchors["boxes"], Gmax, fill, torch.float32).to(dev)
    gc = torch.tensor(A_G, dtype=torch.int32, device=dev)
    return anchors["anchor"].to(dev), pb, gc


def _proposal_inputs(proposals, dev, Gmax=None, fill=0.0, label_fill=-1):
    Gmax = max(P_G) if Gmax is None else Gmax
    imgs = proposals["imgs"]
    roi = torch.stack([c["roi"] for c in imgs]).to(dev)
    pb = _pad([c["bbox"] for c in imgs], Gmax, fill, torch.float32).to(dev)
    pl = _pad([c["label"] for c in imgs], Gmax, label_fill, torch.int64).to(dev)
    gc = torch.tensor(P_G, dtype=torch.int32, device=dev)
    return roi, pb, pl, gc


@pytest.mark.parametrize("name", list(ANCHOR_SETS))
def test_anchor_batch_abi_with_canaries(ffi, dev, anchors, name):
    kw = ANCHOR_SETS[name]
    anchor, pb, gc = _anchor_inputs(anchors, dev)
    got = abi_anchor_batch(ffi, dev, anchor, pb, gc, kw)
    for b, want in enumerate(anchors["want"][name]):
        check_anchor_image(got["loc"][b], got["label"][b], got["argmax"][b], want)
    again = abi_anchor_batch(ffi, dev, anchor, pb, gc, kw, ws=got["ws"])                  # on its own leftovers: the same bits
    _same_outputs(got, again, ("loc", "label", "argmax"))
    other = next(k for k in ANCHOR_SETS if k != name)                                 # ... and on another call's leftovers
    stale = abi_anchor_batch(ffi, dev, anchor, pb, gc, ANCHOR_SETS[other])["ws"]
    _same_outputs(got, abi_anchor_batch(ffi, dev, anchor, pb, gc, kw, ws=stale), ("loc", "label", "argmax"))


@pytest.mark.parametrize("with_src", [True, False])
def test_proposal_batch_abi_with_canaries(ffi, dev, proposals, with_src):
    roi, pb, pl, gc = _proposal_inputs(proposals, dev)
    got = abi_proposal_batch(ffi, dev, roi, pb, pl, gc, P_KW, with_src)
    for b, (want, case) in enumerate(zip(proposals["want"], proposals["imgs"])):
        check_proposal_image(got["sample_roi"][b], got["loc"][b], got["label"][b], got["counts"][b],
                             got["src"][b] if with_src else None, want, case)
    keys = ("sample_roi", "loc", "label", "counts", "src")
    again = abi_proposal_batch(ffi, dev, roi, pb, pl, gc, P_KW, with_src, ws=got["ws"])   # on its own leftovers: the same bits
    _same_outputs(got, again, keys)
    # ... and on the leftovers of a call that kept other rows (reversed image order, same sizes)
    stale = abi_proposal_batch(ffi, dev, roi.flip(0).contiguous(), pb.flip(0).contiguous(), pl.flip(0).contiguous(),
                               gc.flip(0).contiguous(), P_KW, with_src)["ws"]
    _same_outputs(got, abi_proposal_batch(ffi, dev, roi, pb, pl, gc, P_KW, with_src, ws=stale), keys)
    if not with_src:                                                                  # NULL and non-NULL: the same rows
        _same_outputs(got, abi_proposal_batch(ffi, dev, roi, pb, pl, gc, P_KW, True), keys[:4])


# ================================================================================================ through hip_ops: layouts and sizes
@pytest.mark.parametrize("name", list(ANCHOR_SETS))
def test_anchor_batch_images_are_their_single_image_calls(ops, dev, anchors, name):
    kw = ANCHOR_SETS[name]
    anchor, pb, gc = _anchor_inputs(anchors, dev)
    tail = (_n_pos(kw), kw["n_sample"], kw["pos_iou_thresh"], kw["neg_iou_thresh"])
    loc, label, argmax = ops.anchor_targets_batch(pb, gc, anchor, *tail)
    assert loc.shape == (5, A_N, 4) and label.shape == (5, A_N) and label.dtype == torch.int64 and argmax.dtype == torch.int32
    for b, box in enumerate(anchors["boxes"]):
        check_anchor_image(loc[b], label[b], argmax[b], anchors["want"][name][b])
        one = ops.anchor_targets(box.to(dev), anchor, *tail)
        for x, y in zip((loc[b], label[b], argmax[b]), one):
            assert torch.equal(_bits(x), _bits(y))
        solo = ops.anchor_targets_batch(pb[b:b + 1, :max(A_G[b], 1)].contiguous(), gc[b:b + 1], anchor, *tail)      # B = 1
        for x, y in zip(solo, one):
            assert torch.equal(_bits(x[0]), _bits(y))
    # Gmax above every count, NaN in the pad rows (and a count above Gmax is clamped, a negative one is 0)
    wide = ops.anchor_targets_batch(_anchor_inputs(anchors, dev, Gmax=600, fill=float("nan"))[1], gc, anchor, *tail)
    for x, y in zip(wide, (loc, label, argmax)):
        assert torch.equal(_bits(x), _bits(y))
    odd = torch.tensor([-3, 1, 256, 257, 9999], dtype=torch.int32, device=dev)
    clamped = ops.anchor_targets_batch(pb, odd, anchor, *tail)
    for x, y in zip(clamped, (loc, label, argmax)):
        assert torch.equal(_bits(x), _bits(y))


def test_proposal_batch_images_are_their_single_image_calls(ops, dev, proposals):
    roi, pb, pl, gc = _proposal_inputs(proposals, dev)
    tail = (P_KW["n_sample"], int(P_KW["n_sample"] * P_KW["pos_ratio"]), *T.PROPOSAL_THR)
    got = ops.proposal_targets_batch(roi, pb, pl, gc, *tail, want_src=True)
    assert got[3].shape == (4, 4) and got[3].is_cuda and got[4].dtype == torch.int32
    plain = ops.proposal_targets_batch(roi, pb, pl, gc, *tail)
    assert plain[4] is None
    for x, y in zip(plain[:4], got[:4]):
        assert torch.equal(_bits(x), _bits(y))
    counts = got[3].cpu()
    for b, (want, case) in enumerate(zip(proposals["want"], proposals["imgs"])):
        check_proposal_image(got[0][b], got[1][b], got[2][b], counts[b], got[4][b], want, case)
        one = ops.proposal_targets_src(case["roi"].to(dev), case["bbox"].to(dev), case["label"].to(dev), *tail)
        S = want["S"]
        assert one[3].tolist() == counts[b].tolist()
        for x, y in zip((got[0][b], got[1][b], got[2][b], got[4][b]), (one[0], one[1], one[2], one[4])):
            assert torch.equal(_bits(x[:S]), _bits(y[:S]))
        g1 = max(P_G[b], 1)
        solo = ops.proposal_targets_batch(roi[b:b + 1], pb[b:b + 1, :g1].contiguous(), pl[b:b + 1, :g1].contiguous(), gc[b:b + 1],
                                          *tail, want_src=True)                     # B = 1
        for x, y in zip(solo, got):
            assert torch.equal(_bits(x[0]), _bits(y[b]))
    _, wb, wl, _ = _proposal_inputs(proposals, dev, Gmax=700, fill=float("nan"), label_fill=1 << 40)
    wide = ops.proposal_targets_batch(roi, wb, wl, gc, *tail, want_src=True)           # garbage in the pad rows: never read
    for x, y in zip(wide, got):
        assert torch.equal(_bits(x), _bits(y))


def test_no_ground_truth_at_all(ops, ffi, dev, anchors, proposals):
    """Gmax == 0: bbox, gt_label and gt_counts are NULL; every image is the single-image call with G = 0."""
    kw = ANCHOR_SETS["cap500"]
    anchor = anchors["anchor"].to(dev)
    got = abi_anchor_batch(ffi, dev, anchor, torch.zeros((2, 0, 4), device=dev), None, kw)
    one = ops.anchor_targets(torch.zeros((0, 4), device=dev), anchor, _n_pos(kw), kw["n_sample"], kw["pos_iou_thresh"],
                             kw["neg_iou_thresh"])
    for b in range(2):
        for k, y in zip(("loc", "label", "argmax"), one):
            assert torch.equal(_bits(got[k][b]), _bits(y))
    assert (got["label"] == 0).all() and (got["loc"] == 0).all()
    roi = torch.stack([proposals["imgs"][0]["roi"], proposals["imgs"][1]["roi"]]).to(dev)
    kw0 = dict(P_KW, neg_iou_thresh_low=0.0)                                          # the all-zero IoU is then a negative: S = 128
    none = torch.zeros((2, 0, 4), device=dev)
    p = abi_proposal_batch(ffi, dev, roi, none, None, None, kw0, True)
    assert p["counts"].tolist() == [[128, 0, 128, 0]] * 2
    for b in range(2):
        s = ops.proposal_targets_src(roi[b], none[0], torch.zeros(0, dtype=torch.int64, device=dev), 128, 64, 0.5, 0.5, 0.0)
        for k, y in zip(("sample_roi", "loc", "label", "src"), (s[0], s[1], s[2], s[4])):
            assert torch.equal(_bits(p[k][b]), _bits(y))
    empty = abi_proposal_batch(ffi, dev, roi, none, None, None, P_KW, True)           # neg_iou_thresh_low 0.25: nothing is kept
    assert empty["counts"].tolist() == [[0, 0, 0, 0]] * 2 and (empty["src"] == -1).all() and (_bits(empty["sample_roi"]) == 0).all()


def test_creators_batch_on_lists_and_padded_tensors(dev, anchors, proposals):
    from two_stage_object_detection_amd.nets.frcnn_training import AnchorTargetCreator, ProposalTargetCreator, raise_for_counts
    kw = ANCHOR_SETS["cap500"]
    a = AnchorTargetCreator(**kw)
    anchor, pb, _ = _anchor_inputs(anchors, dev, Gmax=520, fill=float("nan"))
    loc, label = a.batch([b.to(dev) for b in anchors["boxes"]], anchor)
    loc2, label2 = a.batch(pb, anchor, gt_counts=list(A_G))
    assert torch.equal(_bits(loc), _bits(loc2)) and torch.equal(label, label2)
    for b, box in enumerate(anchors["boxes"]):
        one = a(box.to(dev), anchor)
        assert torch.equal(_bits(loc[b]), _bits(one[0])) and torch.equal(label[b], one[1])
    p = ProposalTargetCreator(**P_KW)
    roi, wb, wl, _ = _proposal_inputs(proposals, dev, Gmax=520, fill=float("nan"), label_fill=7)
    imgs = proposals["imgs"]
    out = p.batch(roi, [c["bbox"].to(dev) for c in imgs], [c["label"].to(dev) for c in imgs], with_sources=True)
    out2 = p.batch(roi, wb, wl, gt_counts=torch.tensor(P_G), with_sources=True)
    for x, y in zip(out, out2):
        assert torch.equal(_bits(x), _bits(y))
    assert out[3].is_cuda and out[2].dtype == imgs[0]["label"].dtype
    with pytest.raises(IndexError):                                                   # image 1 has status 1: the caller's read says so
        raise_for_counts(out[3].tolist())
    with pytest.raises(ValueError, match="gt_counts"):
        p.batch(roi, wb, wl, gt_counts=[0, 2, 257, 521])
