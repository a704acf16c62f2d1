"""The kernels of csrc/targets.hip at every chunk, tie and cap switch: hip_ops.anchor_targets / proposal_targets /
proposal_targets_src / bbox2loc and the C ABI behind them, on the designed cases of tests/targets_restated.py, against
that restatement (which tests/test_targets_restated.py ties to oracle/targets.py and to the reference's recordings, and
whose cases it shows to reach every switch).

Bars, all the project's existing ones: label, argmax (override included), gt_roi_label, the four count words and
sample_src exact; the gathered sample_roi rows bit-exact; loc / gt_roi_loc with the same finiteness pattern and a relative
error <= 2e-6 with the denominator floored at 1 (test_utils_bbox2loc_surface's bar: one division and one logf, a few ulp).
Canaries: outputs and workspace are filled with a sentinel before the call, the workspace is exactly *_workspace_bytes
long with sentinel words behind it, and nothing outside what the call owns may change."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import targets_restated as T  # noqa: E402

pytestmark = pytest.mark.gpu

F_SENT, I_SENT, L_SENT = -777.25, -123456789, -987654321
PAD = 16                                 # sentinel rows / words behind every output
ANCHORS, PROPOSALS = list(T.ANCHOR_CASES), list(T.PROPOSAL_CASES)


@pytest.fixture(scope="module")
def ops():
    from two_stage_object_detection_amd import hip_ops
    return hip_ops


@pytest.fixture(scope="module")
def ffi():
    from two_stage_object_detection_amd import _ffi
    return _ffi


def _align16(n):
    return (n + 15) // 16 * 16


def _check_loc(got, ref):
    same, rel = T.loc_error(got.cpu(), ref)
    assert same, "finiteness pattern differs"
    assert rel <= T.LOC_REL_BAR, rel


def _n_pos(kw):
    return int(kw["pos_ratio"] * kw["n_sample"])


# ================================================================================================ through the C ABI
def abi_anchor(ffi, dev, case, ws=None):
    """tsod_anchor_targets_f32 into sentinel-filled outputs with PAD rows behind them, on a workspace of exactly the size asked
    for with PAD sentinel words behind it (or on ``ws``, a (tensor, bytes) of an earlier, larger call)."""
    anchor, bbox, kw = case["anchor"].to(dev), case["bbox"].to(dev), case["kw"]
    A, G = anchor.shape[0], bbox.shape[0]
    L = ffi.lib()
    need = L.tsod_anchor_targets_workspace_bytes(A, G)
    assert need == _align16(4 * A) + _align16(4 * max(G, 1)) + 16
    if ws is None:
        ws = (torch.full((need // 4 + PAD,), I_SENT, dtype=torch.int32, device=dev), need)
    loc = torch.full((A + PAD, 4), F_SENT, dtype=torch.float32, device=dev)
    label = torch.full((A + PAD,), L_SENT, dtype=torch.int64, device=dev)
    argmax = torch.full((A + PAD,), I_SENT, dtype=torch.int32, device=dev)
    ffi.check(L.tsod_anchor_targets_f32(ffi.ptr(anchor), A, ffi.ptr(bbox) if G else None, G, kw["pos_iou_thresh"],
                                        kw["neg_iou_thresh"], _n_pos(kw), kw["n_sample"], ffi.ptr(loc), ffi.ptr(label),
                                        ffi.ptr(argmax), ffi.ptr(ws[0]), ws[1], ffi.stream_ptr()), "anchor_targets")
    assert (loc[A:] == F_SENT).all() and (label[A:] == L_SENT).all() and (argmax[A:] == I_SENT).all()
    assert (ws[0][need // 4:need // 4 + PAD] == I_SENT).all() or ws[1] > need           # (a borrowed workspace holds older data there)
    return dict(loc=loc[:A].cpu(), label=label[:A].cpu(), argmax=argmax[:A].cpu(), ws=ws)


def abi_proposal(ffi, dev, case, ws=None, with_src=True):
    roi, bbox, label, kw = case["roi"].to(dev), case["bbox"].to(dev), case["label"].to(dev), case["kw"]
    R, G, n = roi.shape[0], bbox.shape[0], kw["n_sample"]
    L = ffi.lib()
    need = L.tsod_proposal_targets_workspace_bytes(R, G, n)
    assert need == 2 * _align16(4 * (R + G)) + _align16(4 * n)
    if ws is None:
        ws = (torch.full((need // 4 + PAD,), I_SENT, dtype=torch.int32, device=dev), need)
    s_roi = torch.full((n + PAD, 4), F_SENT, dtype=torch.float32, device=dev)
    s_loc = torch.full((n + PAD, 4), F_SENT, dtype=torch.float32, device=dev)
    s_lab = torch.full((n + PAD,), L_SENT, dtype=torch.int64, device=dev)
    src = torch.full((n + PAD,), I_SENT, dtype=torch.int32, device=dev)
    counts = torch.full((4 + PAD,), I_SENT, dtype=torch.int32, device=dev)
    head = (ffi.ptr(roi) if R else None, R, ffi.ptr(bbox) if G else None, G, ffi.ptr(label) if G else None, n,
            int(n * kw["pos_ratio"]), kw["pos_iou_thresh"], kw["neg_iou_thresh_high"], kw["neg_iou_thresh_low"],
            ffi.ptr(s_roi), ffi.ptr(s_loc), ffi.ptr(s_lab), ffi.ptr(counts))
    if with_src:
        ffi.check(L.tsod_proposal_targets_src_f32(*head, ffi.ptr(src), ffi.ptr(ws[0]), ws[1], ffi.stream_ptr()), "proposal_targets_src")
    else:
        ffi.check(L.tsod_proposal_targets_f32(*head, ffi.ptr(ws[0]), ws[1], ffi.stream_ptr()), "proposal_targets")
    c = counts.cpu()
    S = int(c[0])
    assert 0 <= S <= n and (c[4:] == I_SENT).all()
    # rows at and above counts[0], the PAD rows included, are nobody's
    assert (s_roi[S:] == F_SENT).all() and (s_loc[S:] == F_SENT).all() and (s_lab[S:] == L_SENT).all()
    assert (src[S if with_src else 0:] == I_SENT).all()
    assert (ws[0][need // 4:need // 4 + PAD] == I_SENT).all() or ws[1] > need
    return dict(counts=c[:4].tolist(), sample_roi=s_roi[:S].cpu(), loc=s_loc[:S].cpu(), label=s_lab[:S].cpu(), src=src[:S].cpu(),
                ws=ws)


def check_anchor(got, want):
    assert torch.equal(got["label"], want["label"])
    assert torch.equal(got["argmax"].long(), want["argmax"])
    _check_loc(got["loc"], want["loc"])


def check_proposal(got, want, case, with_src=True):
    S = want["S"]
    assert got["counts"] == [S, want["pos_len"], want["neg_len"], want["status"]]
    assert torch.equal(got["sample_roi"], want["sample_roi"])                        # gathered: bit-exact
    _check_loc(got["loc"], want["loc"])
    if want["status"]:                                                               # the reference raises: what T2 leaves alone is still defined
        outside = torch.ones(S, dtype=torch.bool)
        outside[want["t2"]] = False
        assert torch.equal(got["label"][outside], want["label_before"][outside])
    else:
        assert torch.equal(got["label"], want["label_after"])
    if with_src:
        src = got["src"].long()
        assert torch.equal(src, want["keep"])
        assert torch.equal(torch.cat((case["roi"], case["bbox"]))[src], got["sample_roi"])
        for part in (src[:want["pos_len"]], src[want["pos_len"]:]):                  # strictly ascending within each part
            assert (part[1:] > part[:-1]).all()


@pytest.mark.parametrize("name", ANCHORS)
def test_anchor_targets_abi_sweep_with_canaries(ffi, dev, name):
    check_anchor(abi_anchor(ffi, dev, T.anchor_case(name)), T.anchor_want(name))


@pytest.mark.parametrize("name", PROPOSALS)
def test_proposal_targets_abi_sweep_with_canaries(ffi, dev, name):
    case, want = T.proposal_case(name), T.proposal_want(name)
    with_src = abi_proposal(ffi, dev, case)
    check_proposal(with_src, want, case)
    plain = abi_proposal(ffi, dev, case, with_src=False)
    check_proposal(plain, want, case, with_src=False)
    for k in ("sample_roi", "loc", "label"):
        assert torch.equal(plain[k], with_src[k])


def test_workspace_sizes_are_zero_where_the_source_says(ffi):
    L = ffi.lib()
    for A, G in ((0, 3), (-1, 3), (5, -1), (0, 0)):
        assert L.tsod_anchor_targets_workspace_bytes(A, G) == 0
    assert L.tsod_anchor_targets_workspace_bytes(1, 0) == 16 + 16 + 16
    for R, G, n in ((-1, 3, 8), (3, -1, 8), (0, 0, 8), (3, 3, 0), (3, 3, -2)):
        assert L.tsod_proposal_targets_workspace_bytes(R, G, n) == 0
    assert L.tsod_proposal_targets_workspace_bytes(0, 1, 1) == 16 + 16 + 16
    assert L.tsod_proposal_targets_workspace_bytes(1, 0, 5) == 16 + 16 + 32


# ================================================================================================ through hip_ops
@pytest.mark.parametrize("name", ANCHORS)
def test_anchor_targets_sweep(ops, dev, name):
    case, want = T.anchor_case(name), T.anchor_want(name)
    kw = case["kw"]
    args = (case["bbox"].to(dev), case["anchor"].to(dev), _n_pos(kw), kw["n_sample"], kw["pos_iou_thresh"], kw["neg_iou_thresh"])
    loc, label, argmax = ops.anchor_targets(*args)
    check_anchor(dict(loc=loc.cpu(), label=label.cpu(), argmax=argmax.cpu()), want)
    again = ops.anchor_targets(*args)                                                 # two runs: the same bits
    for a, b in zip((loc, label, argmax), again):
        assert torch.equal(a.view(torch.int32) if a.is_floating_point() else a, b.view(torch.int32) if b.is_floating_point() else b)


def _ops_proposal(ops, dev, case, with_src):
    kw = case["kw"]
    fn = ops.proposal_targets_src if with_src else ops.proposal_targets
    out = fn(case["roi"].to(dev), case["bbox"].to(dev), case["label"].to(dev), kw["n_sample"], int(kw["n_sample"] * kw["pos_ratio"]),
             kw["pos_iou_thresh"], kw["neg_iou_thresh_high"], kw["neg_iou_thresh_low"])
    counts = out[3].tolist()
    S = counts[0]
    return dict(counts=counts, sample_roi=out[0][:S].cpu(), loc=out[1][:S].cpu(), label=out[2][:S].cpu(),
                src=out[4][:S].cpu() if with_src else None)


@pytest.mark.parametrize("name", PROPOSALS)
def test_proposal_targets_sweep(ops, dev, name):
    case, want = T.proposal_case(name), T.proposal_want(name)
    got = _ops_proposal(ops, dev, case, True)
    check_proposal(got, want, case)
    check_proposal(_ops_proposal(ops, dev, case, False), want, case, with_src=False)
    again = _ops_proposal(ops, dev, case, True)                                       # two runs: the same bits
    assert again["counts"] == got["counts"]
    for k in ("sample_roi", "loc"):
        assert torch.equal(again[k].view(torch.int32), got[k].view(torch.int32))
    assert torch.equal(again["label"], got["label"]) and torch.equal(again["src"], got["src"])


@pytest.mark.parametrize("name", PROPOSALS)
def test_proposal_creator_raises_exactly_where_the_reference_does(dev, name):
    from two_stage_object_detection_amd.nets.frcnn_training import ProposalTargetCreator
    case, want = T.proposal_case(name), T.proposal_want(name)
    creator = ProposalTargetCreator(**case["kw"])
    args = (case["roi"].to(dev), case["bbox"].to(dev), case["label"].to(dev))
    if want["status"]:
        with pytest.raises(IndexError):
            creator(*args)
        with pytest.raises(IndexError):
            creator.with_sources(*args)
        return
    s_roi, s_loc, s_lab = creator(*args)
    assert torch.equal(s_roi.cpu(), want["sample_roi"]) and torch.equal(s_lab.cpu(), want["label_after"])
    _check_loc(s_loc, want["loc"])
    assert torch.equal(creator.with_sources(*args)[3].cpu().long(), want["keep"])


@pytest.mark.parametrize("name", ["A65-G255", "A1025-G257", "A2049-G257"])
def test_anchor_creator_on_the_sweep(dev, name):
    from two_stage_object_detection_amd.nets.frcnn_training import AnchorTargetCreator
    case, want = T.anchor_case(name), T.anchor_want(name)
    loc, label = AnchorTargetCreator(**case["kw"])(case["bbox"].to(dev), case["anchor"].to(dev))
    assert torch.equal(label.cpu(), want["label"])
    _check_loc(loc, want["loc"])


def test_a_positive_cap_above_n_sample_is_refused(ops, ffi, dev):
    """pos_ratio > 1: the reference drops only the last negatives there (test_targets_restated.py pins it); the kernels do not
    restate that, so the C ABI refuses the arguments and the creators refuse the ratio."""
    a, p = T.anchor_case("A255-G256"), T.proposal_case("R255-G2")
    with pytest.raises(ffi.TsodError):
        ops.anchor_targets(a["bbox"].to(dev), a["anchor"].to(dev), 125, 100, 0.5, 0.25)
    with pytest.raises(ffi.TsodError):
        ops.proposal_targets(p["roi"].to(dev), p["bbox"].to(dev), p["label"].to(dev), 100, 125, 0.5, 0.5, 0.25)
    with pytest.raises(ffi.TsodError):
        ops.proposal_targets_src(p["roi"].to(dev), p["bbox"].to(dev), p["label"].to(dev), 100, 125, 0.5, 0.5, 0.25)
    ops.anchor_targets(a["bbox"].to(dev), a["anchor"].to(dev), 100, 100, 0.5, 0.25)               # the edge itself is served


def test_single_image_anchor_call_serves_a_zero_threshold_with_ground_truth(ffi, dev):
    """pos_iou_thresh = 0.0 with ground truth present: every anchor is positive and every box exists, so the single-image entry
    point serves it (the batched one refuses pos_iou_thresh <= 0 outright; the single-image one only at G == 0, which
    test_abi_errors.py holds).  A = 65, G = 2, n_sample = 256, pos_ratio = 0.5: all 65 anchors are positive and, n_pos being
    128, the cap keeps them all; the second call (n_sample = 64, n_pos = 32) is the one where the cap cuts."""
    g = torch.Generator().manual_seed(65)
    anchor, bbox = T.grid_boxes(g, 65, 8), T.grid_boxes(g, 2, 8)
    for n_sample, cuts in ((256, False), (64, True)):
        kw = dict(n_sample=n_sample, pos_ratio=0.5, pos_iou_thresh=0.0, neg_iou_thresh=T.ANCHOR_THR["neg_iou_thresh"])
        want = T.anchor_stages(bbox, anchor, **kw)
        assert want["total_pos"] == 65 and (want["label_claim"] == 1).all() and want["flag"] == 1    # before the GPU is looked at
        assert (want["total_pos"] > want["n_pos"]) == cuts and int((want["label"] == 1).sum()) == min(65, n_sample // 2)
        assert (want["max_iou"] == 0).any() and (want["max_iou"] > 0).any()                      # at the threshold and above it
        check_anchor(abi_anchor(ffi, dev, dict(anchor=anchor, bbox=bbox, kw=kw)), want)


# ================================================================================================ stale state
def test_anchor_targets_leave_no_state_in_the_workspace(ffi, dev):
    """A large case with ground truth and a flag of 1, then small ones without (G = 0, flag 0) and with ground truth, on the same
    workspace and stream: each equals its run on a fresh workspace."""
    big = abi_anchor(ffi, dev, T.anchor_case("A2049-G513"))
    assert T.anchor_want("A2049-G513")["flag"] == 1
    for name in ("A1024-G0", "A1-G0", "A63-G2", "A1025-G1"):
        fresh = abi_anchor(ffi, dev, T.anchor_case(name))
        reused = abi_anchor(ffi, dev, T.anchor_case(name), ws=big["ws"])
        check_anchor(reused, T.anchor_want(name))
        for k in ("label", "argmax"):
            assert torch.equal(reused[k], fresh[k])
        assert torch.equal(reused["loc"].view(torch.int32), fresh["loc"].view(torch.int32))
    assert T.anchor_want("A1024-G0")["flag"] == 0 and T.anchor_want("A1025-G1")["flag"] == 0


def test_proposal_targets_leave_no_state_in_the_workspace(ffi, dev):
    big = abi_proposal(ffi, dev, T.proposal_case("R2048-G1-both"))
    for name in ("R256-G0", "R256-G0-lo", "R0-G1", "R255-G1", "R1023-G2"):
        case = T.proposal_case(name)
        fresh = abi_proposal(ffi, dev, case)
        reused = abi_proposal(ffi, dev, case, ws=big["ws"])
        check_proposal(reused, T.proposal_want(name), case)
        assert reused["counts"] == fresh["counts"]
        for k in ("sample_roi", "loc"):
            assert torch.equal(reused[k].view(torch.int32), fresh[k].view(torch.int32))
        assert torch.equal(reused["label"], fresh["label"]) and torch.equal(reused["src"], fresh["src"])


# ================================================================================================ bbox2loc
def test_bbox2loc_past_the_grid(ops, ffi, dev):
    """n = 4096 x 256 + 3: the last three boxes are reached only by the grid-stride loop's second trip."""
    n = T.B2L_BLOCKS * T.B2L_THREADS + 3
    src, dst = T.bbox2loc_boxes(n)
    ref = T.oracle_targets.bbox2loc(src, dst)
    got = ops.bbox2loc(src.to(dev), dst.to(dev))
    _check_loc(got, ref)
    _check_loc(got[-3:], ref[-3:])
    out = torch.full((n + PAD, 4), F_SENT, dtype=torch.float32, device=dev)
    s, d = src.to(dev), dst.to(dev)
    ffi.check(ffi.lib().tsod_bbox2loc_f32(ffi.ptr(s), ffi.ptr(d), n, ffi.ptr(out), ffi.stream_ptr()), "bbox2loc")
    assert (out[n:] == F_SENT).all() and torch.equal(out[:n].view(torch.int32), got.view(torch.int32))
    for m in (1, 255, 257):                                                           # one partial block, two blocks
        _check_loc(ops.bbox2loc(s[:m].clone(), d[:m].clone()), ref[:m])
