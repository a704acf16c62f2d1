"""tests/targets_restated.py on the CPU: what makes the sweep of tests/test_target_kernels_gpu.py honest without a GPU.

  * the restatement's final outputs equal oracle/targets.py on every case of the sweep (status 1 exactly where the oracle
    raises IndexError), and equal the reference's own recordings (tests/golden/targets_*.npz), bit for bit;
  * the geometry it restates is the one in csrc/targets.hip (source text);
  * every switch of the kernels is reached by some case - one assertion per switch, from the restatement alone;
  * every deliberately wrong restatement (MUTANTS) differs from the true one on some case: a mutant nothing catches is a
    hole in the case list;
  * pos_ratio outside [0, 1]: what the reference does there is pinned, and the creators refuse it."""
import ast
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import targets_restated as T  # noqa: E402
from oracle import targets as oracle_targets  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "two_stage_object_detection_amd", "csrc", "targets.hip")
ANCHORS, PROPOSALS = list(T.ANCHOR_CASES), list(T.PROPOSAL_CASES)


def _same(a, b):
    """torch.equal that also holds for the -inf / nan a degenerate box leaves in ``loc``."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.numpy(), b.numpy(), equal_nan=a.is_floating_point())


def _some(cases, want, pred):
    return [n for n in cases if pred(want(n))]


# ================================================================================================ agreement
@pytest.mark.parametrize("name", ANCHORS)
def test_anchor_restatement_equals_the_oracle(name):
    c, w = T.anchor_case(name), T.anchor_want(name)
    loc, label, dbg = oracle_targets.anchor_targets(c["bbox"], c["anchor"], return_debug=True, **c["kw"])
    assert _same(label, w["label"]) and _same(loc, w["loc"])
    assert _same(dbg["argmax_ious"].long(), w["argmax"]) and _same(dbg["max_ious"], w["max_iou"])
    assert _same(dbg["gt_argmax_ious"].long(), w["gt_argmax"])
    assert torch.isfinite(w["loc"]).all()                           # grid sides are >= 1: no degenerate box in the sweep


@pytest.mark.parametrize("name", PROPOSALS)
def test_proposal_restatement_equals_the_oracle(name):
    c, w = T.proposal_case(name), T.proposal_want(name)
    try:
        roi, loc, label = oracle_targets.proposal_targets(c["roi"], c["bbox"], c["label"], **c["kw"])
    except IndexError:
        assert w["status"] == 1
        return
    assert w["status"] == 0
    assert _same(roi, w["sample_roi"]) and _same(loc, w["loc"]) and _same(label, w["label_after"])
    assert w["S"] == w["pos_len"] + w["neg_len"] <= c["kw"]["n_sample"]


@pytest.mark.parametrize("name", ["default", "dup", "many_pos", "all_pos_ratio", "no_gt"])
def test_anchor_restatement_equals_the_reference_vectors(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "targets_anchor.npz"))
    kw = ast.literal_eval(str(z[f"{name}.kw"]))
    w = T.anchor_stages(torch.from_numpy(z[f"{name}.bbox"]), torch.from_numpy(z["anchor"]), **kw)
    assert np.array_equal(w["label"].numpy(), z[f"{name}.label"])
    assert np.array_equal(w["loc"].numpy(), z[f"{name}.loc"])


@pytest.mark.parametrize("name", ["default", "few", "no_gt", "thresholds", "thresholds_gap", "index_error"])
def test_proposal_restatement_equals_the_reference_vectors(golden_dir, name):
    z = np.load(os.path.join(golden_dir, "targets_proposal.npz"))
    kw = ast.literal_eval(str(z[f"{name}.kw"]))
    w = T.proposal_stages(*(torch.from_numpy(z[f"{name}.{k}"]) for k in ("roi", "bbox", "label")), **kw)
    assert w["status"] == int(bool(z[f"{name}.raises"]))
    if w["status"]:
        return
    assert np.array_equal(w["sample_roi"].numpy(), z[f"{name}.sample_roi"])
    assert np.array_equal(w["loc"].numpy(), z[f"{name}.gt_roi_loc"])
    assert np.array_equal(w["label_after"].numpy(), z[f"{name}.gt_roi_label"])


def test_planted_iou_values_are_exact():
    a = torch.tensor([[0., 0, 1, 1]])
    assert T.bbox_iou(a, torch.tensor([[0., 0, 2, 1]])).item() == 0.5
    assert T.bbox_iou(a, torch.tensor([[0., 0, 4, 1]])).item() == 0.25


# ================================================================================================ the geometry in the source
def test_restated_geometry_is_the_one_in_the_source():
    with open(SOURCE) as f:
        src = f.read()
    assert f"__shared__ float4 s_gt[{T.ROW_BLOCK}];" in src
    assert f"const int n = blockIdx.x * {T.ROW_BLOCK} + threadIdx.x;" in src
    assert f"for (int g0 = 0; g0 < G; g0 += {T.ROW_BLOCK})" in src
    assert "const float4 box = n < na ? a[n] : (n < N ? b[n - na]" in src
    assert "float best = G > 0 ? -INFINITY : 0.f;" in src
    assert f"for (int n = threadIdx.x; n < A; n += {T.COL_THREADS})" in src
    assert "for (int off = 32; off > 0; off >>= 1)" in src and "for (int w = 1; w < 4; ++w)" in src      # 64 lanes, 4 waves
    assert "gt_argmax[blockIdx.x] = bi == INT_MAX ? 0 : bi;" in src
    assert f"const int chunk = (A + {T.THREADS - 1}) / {T.THREADS};" in src
    assert f"const int chunk = (N + {T.THREADS - 1}) / {T.THREADS};" in src
    assert f"for (int g = tid; g < G; g += {T.THREADS})" in src
    assert f"for (int j = tid; j < neg_len; j += {T.THREADS})" in src
    assert "if (1 > n_neg)" in src
    assert len(re.findall(rf"dim3\(B\), dim3\({T.THREADS}\)", src)) == 2             # both kernels of one workgroup per image
    assert len(re.findall(r"\b__global__\b", src)) == 6 and "_batch_kernel" not in src         # five steps and bbox2loc_kernel
    assert f"(n + 255) / 256 < {T.B2L_BLOCKS} ? (n + 255) / 256 : {T.B2L_BLOCKS}" in src
    # the argument ranges for which the workspace sizes are 0
    assert "if (A <= 0 || G < 0) return 0;" in src
    assert "if (R < 0 || G < 0 || R + G <= 0 || n_sample <= 0) return 0;" in src


def test_sizes_of_the_sweep():
    A = {T.ANCHOR_CASES[n][0] for n in ANCHORS}
    G = {T.ANCHOR_CASES[n][1] for n in ANCHORS}
    assert {1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049} <= A
    assert {0, 1, 2, 255, 256, 257, 513, 1025} <= G
    N = {T.PROPOSAL_CASES[n][0] + T.PROPOSAL_CASES[n][1] for n in PROPOSALS}
    assert {1, 256, 257, 1024, 1025, 2049} <= N


# ================================================================================================ coverage: rowmax_kernel
def test_rowmax_tie_across_the_lds_chunks():
    """A row maximum attained first at g <= 255 and again at g >= 256 - and one at exactly g = 255 and g = 256."""
    def straddles(w, exact):
        if w["ious"].shape[1] <= T.ROW_BLOCK:
            return False
        hit = w["ious"] == w["max_iou"][:, None]
        first = w["argmax_before"] if "argmax_before" in w else w["assign"]
        if exact:
            return bool(((first == 255) & hit[:, 256]).any())
        return bool(((first < T.ROW_BLOCK) & hit[:, T.ROW_BLOCK:].any(dim=1)).any())
    for want, cases in ((T.anchor_want, ANCHORS), (T.proposal_want, PROPOSALS)):
        assert _some(cases, want, lambda w: straddles(w, False))
    assert _some(ANCHORS, T.anchor_want, lambda w: straddles(w, True))


def test_rowmax_candidate_switch_and_partial_blocks():
    RG = {n: T.PROPOSAL_CASES[n][:2] for n in PROPOSALS}
    assert [n for n, (R, G) in RG.items() if G > 0 and R % T.ROW_BLOCK]                     # n == na inside a block
    assert [n for n, (R, G) in RG.items() if G > 0 and R > 0 and R % T.ROW_BLOCK == 0]            # ... on a block edge
    assert [n for n, (R, G) in RG.items() if R == 0] and [n for n, (R, G) in RG.items() if G == 0]
    assert [n for n, (R, G) in RG.items() if (R + G) % T.ROW_BLOCK] and [n for n, (R, G) in RG.items() if (R + G) % T.ROW_BLOCK == 0]
    A = [T.ANCHOR_CASES[n][0] for n in ANCHORS]
    assert [a for a in A if a % T.ROW_BLOCK] and [a for a in A if a % T.ROW_BLOCK == 0] and [a for a in A if a > T.ROW_BLOCK]


def test_rowmax_without_ground_truth():
    for n in ANCHORS:
        if T.ANCHOR_CASES[n][1] == 0:
            w = T.anchor_want(n)
            assert (w["max_iou"] == 0).all() and (w["argmax"] == 0).all() and w["flag"] == 0 and (w["label"] == 0).all()
    assert sum(T.ANCHOR_CASES[n][1] == 0 for n in ANCHORS) >= 2
    kept = [T.proposal_want(n)["S"] for n in PROPOSALS if T.PROPOSAL_CASES[n][1] == 0]
    assert 0 in kept and any(kept)                                   # neg_iou_thresh_low above and at the all-zero IoU


# ================================================================================================ coverage: colargmax_kernel
def _col_ties(w):
    """Per ground-truth box: the anchors that attain its column maximum."""
    hit = w["ious"] == w["ious"].max(dim=0, keepdim=True).values
    return [torch.where(hit[:, g])[0] for g in range(hit.shape[1])]


def test_colargmax_idle_lanes_and_waves():
    withgt = [T.ANCHOR_CASES[n][0] for n in ANCHORS if T.ANCHOR_CASES[n][1] > 0]
    assert [a for a in withgt if a < T.WAVE] and [a for a in withgt if T.WAVE <= a < T.COL_THREADS]
    assert [a for a in withgt if a == T.COL_THREADS] and [a for a in withgt if a > 2 * T.COL_THREADS]


def test_colargmax_ties_between_lanes_waves_and_trips():
    seen = set()
    for n in ANCHORS:
        if T.ANCHOR_CASES[n][1] == 0:
            continue
        for tied in _col_ties(T.anchor_want(n)):
            if tied.numel() < 2:
                continue
            first, rest = int(tied[0]), tied[1:]
            t0, t = first % T.COL_THREADS, rest % T.COL_THREADS
            if (t == t0).any():
                seen.add("same_thread")
            if ((t != t0) & (t // T.WAVE == t0 // T.WAVE)).any():
                seen.add("lanes_of_one_wave")
            if (t // T.WAVE != t0 // T.WAVE).any():
                seen.add("across_waves")
            if (t < t0).any():
                seen.add("first_in_the_higher_thread")
            if (t // T.WAVE < t0 // T.WAVE).any():
                seen.add("first_in_the_higher_wave")
    assert seen == {"same_thread", "lanes_of_one_wave", "across_waves", "first_in_the_higher_thread", "first_in_the_higher_wave"}
    w = T.anchor_want("A257-G513")                                   # the planted one: anchors 250 and 256 tie, 250 is the answer
    assert 250 in w["gt_argmax"].tolist() and 256 not in w["gt_argmax"].tolist()


def test_colargmax_box_that_overlaps_no_anchor():
    def lonely(w):
        return w["ious"].shape[1] > 0 and bool(((w["ious"].max(dim=0).values == 0) & (w["gt_argmax"] == 0)).any())
    assert len(_some(ANCHORS, T.anchor_want, lonely)) >= 3


def test_anchor_claimed_by_three_boxes_and_the_last_wins():
    def triple(w):
        if w["gt_argmax"].numel() == 0:
            return False
        a, count = torch.unique(w["gt_argmax"], return_counts=True)
        for anchor in a[count >= 3].tolist():
            claimers = torch.where(w["gt_argmax"] == anchor)[0]
            assert int(w["argmax"][anchor]) == int(claimers[-1])
        return bool((count >= 3).any())
    assert len(_some(ANCHORS, T.anchor_want, triple)) >= 3


# ================================================================================================ coverage: anchor_label_kernel
def test_anchor_label_chunks():
    A = {T.ANCHOR_CASES[n][0] for n in ANCHORS}
    assert {T.chunk_of(a) for a in A} == {1, 2, 3}
    assert [a for a in A if a < T.THREADS] and T.THREADS in A
    assert T.THREADS + 1 in A and -(-(T.THREADS + 1) // T.chunk_of(T.THREADS + 1)) == 513     # threads from 513 on own nothing


def _cut(pos, keep, n_items):
    """Where the cap's cut falls: ('none' | 'zero' | 'inside' | 'chunk_edge' | 'wave_edge'), total - keep."""
    total = pos.numel()
    if total <= keep:
        return "none", total - keep
    if keep == 0:
        return "zero", total
    chunk = T.chunk_of(n_items)
    kept, dropped = int(pos[keep - 1]) // chunk, int(pos[keep]) // chunk
    where = "inside" if kept == dropped else ("chunk_edge" if kept // T.WAVE == dropped // T.WAVE else "wave_edge")
    return where, total - keep


def test_anchor_positive_cap_cuts():
    cuts = {n: _cut(T.anchor_want(n)["pos"], T.anchor_want(n)["n_pos"], T.ANCHOR_CASES[n][0]) for n in ANCHORS}
    where = {c[0] for c in cuts.values()}
    assert {"inside", "chunk_edge", "wave_edge", "zero", "none"} <= where
    assert [n for n, c in cuts.items() if c[0] == "inside" and T.chunk_of(T.ANCHOR_CASES[n][0]) >= 2 and c[1] > 1]
    assert [n for n, c in cuts.items() if c[1] == 0 and T.anchor_want(n)["total_pos"] > 0]        # total_pos == n_pos
    assert [n for n, c in cuts.items() if c[1] == 1 and T.anchor_want(n)["n_pos"] > 0]            # total_pos == n_pos + 1
    assert [n for n, c in cuts.items() if c[0] == "zero"]                                         # n_pos == 0 with positives
    for n in ANCHORS:
        w = T.anchor_want(n)
        assert int((w["label_cap"] == 1).sum()) == w["pos_length"] == min(w["total_pos"], w["n_pos"])


def test_anchor_override_across_the_1024_stride():
    w = T.anchor_want("A300-G1025")
    assert w["gt_argmax"].numel() > T.THREADS
    a = int(w["gt_argmax"][T.THREADS])
    claimers = torch.where(w["gt_argmax"] == a)[0]
    assert claimers.numel() >= 3 and int(claimers[0]) < T.THREADS and int(w["argmax"][a]) == T.THREADS


def test_anchor_quirk_t1_fires_only_below_one():
    fires = _some(ANCHORS, T.anchor_want, lambda w: w["n_neg"] == 0 and bool((w["label_cap"] == 0).any()))
    spared = _some(ANCHORS, T.anchor_want, lambda w: w["n_neg"] == 1 and int((w["label_cap"] == 0).sum()) >= 2)
    assert fires and spared
    for n in fires:
        assert not (T.anchor_want(n)["label"] == 0).any()
    for n in spared:
        assert _same(T.anchor_want(n)["label"], T.anchor_want(n)["label_cap"])
    assert _some(ANCHORS, T.anchor_want, lambda w: w["n_neg"] > 1 and bool((w["label"] == 0).any()))


def test_anchor_exact_threshold_hits():
    def at(w, v, label):
        unclaimed = torch.ones_like(w["label_thr"], dtype=torch.bool)
        unclaimed[w["gt_argmax"]] = False
        return bool(((w["max_iou"] == v) & unclaimed & (w["label_thr"] == label)).any())
    assert len(_some(ANCHORS, T.anchor_want, lambda w: at(w, 0.5, 1))) >= 3
    assert len(_some(ANCHORS, T.anchor_want, lambda w: at(w, 0.25, -1))) >= 3
    seen = set()
    for n in ANCHORS:
        seen |= set(T.anchor_want(n)["label"].tolist())
    assert seen == {-1, 0, 1}


# ================================================================================================ coverage: proposal_select_kernel
def test_proposal_chunks_and_scans():
    N = {T.proposal_want(n)["N"] for n in PROPOSALS}
    assert {T.chunk_of(n) for n in N} == {1, 2, 3}
    # the two scans share one LDS array back to back: their totals differ, both non-zero
    assert len(_some(PROPOSALS, T.proposal_want, lambda w: 0 < w["pos_all"].numel() != w["neg_all"].numel() > 0)) >= 3


def test_proposal_positive_cap_cuts():
    cuts = {n: _cut(T.proposal_want(n)["pos_all"], T.proposal_want(n)["ppi"], T.proposal_want(n)["N"]) for n in PROPOSALS}
    assert {"inside", "chunk_edge", "wave_edge", "zero", "none"} <= {c[0] for c in cuts.values()}
    assert [n for n, c in cuts.items() if c[1] == 0 and T.proposal_want(n)["ppi"] > 0]
    assert [n for n, c in cuts.items() if c[1] == 1 and T.proposal_want(n)["ppi"] > 0]
    assert [n for n, c in cuts.items() if c[0] == "inside" and T.proposal_want(n)["status"] == 0]


def test_proposal_candidate_kept_as_positive_and_as_negative():
    def twice(w):
        return len(set(w["pos_idx"].tolist()) & set(w["neg_idx"].tolist())) > 0
    names = _some(PROPOSALS, T.proposal_want, twice)
    assert len(names) >= 2
    assert [n for n in names if T.proposal_want(n)["S"] > T.proposal_want(n)["N"]]                # more slots than candidates


def test_proposal_negative_clip():
    assert _some(PROPOSALS, T.proposal_want, lambda w: w["neg_all"].numel() > w["room"] > 0 and w["neg_len"] == w["room"])
    assert _some(PROPOSALS, T.proposal_want, lambda w: w["neg_all"].numel() > 0 and w["room"] == 0 and w["neg_len"] == 0)
    assert _some(PROPOSALS, T.proposal_want, lambda w: 0 < w["neg_all"].numel() < w["room"])


def test_proposal_quirk_t2():
    raising = _some(PROPOSALS, T.proposal_want, lambda w: w["status"] == 1)
    assert len(raising) >= 3
    assert [n for n in raising if T.proposal_want(n)["t2"].numel() > 0]                           # some positions still in range
    # not raising, and T2 lands on a positive's slot (the kept position equals a negative's ORIGINAL index)
    assert len(_some(PROPOSALS, T.proposal_want,
                     lambda w: w["status"] == 0 and bool((w["t2"] < w["pos_len"]).any()) and
                     bool((w["label_before"][w["t2"]] != 0).any()))) >= 3
    # ... and sampled negatives elsewhere keep label + 1
    assert _some(PROPOSALS, T.proposal_want, lambda w: w["status"] == 0 and bool((w["label_after"][w["pos_len"]:] != 0).any()))


def test_proposal_negative_ranked_by_a_late_thread_without_raising():
    def late(w):
        return w["status"] == 0 and w["neg_len"] > 0 and int(w["neg_idx"][-1]) // T.chunk_of(w["N"]) >= T.WAVE
    names = _some(PROPOSALS, T.proposal_want, late)
    assert names and [n for n in names if T.proposal_case(n)["kw"]["n_sample"] >= 2000]


def test_proposal_exact_threshold_hits():
    for v in (0.5, 0.25):
        assert len(_some(PROPOSALS, T.proposal_want, lambda w: bool((w["max_iou"] == v).any()))) >= 3


def test_bbox2loc_size_is_past_the_grid():
    assert 5000 <= T.B2L_BLOCKS * T.B2L_THREADS        # the older test's 5 000 boxes: one trip; the sweep's n is this product + 3


# ================================================================================================ mutants
@pytest.mark.parametrize("mutant", T.ANCHOR_MUTANTS)
def test_every_anchor_mutant_is_caught(mutant):
    keys = ("label", "argmax", "max_iou")
    caught = [n for n in ANCHORS if not all(_same(T.anchor_want(n, mutant)[k], T.anchor_want(n)[k]) for k in keys)]
    assert caught, f"no case of the sweep tells '{mutant}' from the true restatement"


@pytest.mark.parametrize("mutant", T.PROPOSAL_MUTANTS)
def test_every_proposal_mutant_is_caught(mutant):
    def differs(n):
        m, w = T.proposal_want(n, mutant), T.proposal_want(n)
        return not (_same(m["keep"], w["keep"]) and _same(m["label_after"], w["label_after"]) and m["status"] == w["status"] and
                    (m["pos_len"], m["neg_len"]) == (w["pos_len"], w["neg_len"]) and _same(m["assign"], w["assign"]))
    assert [n for n in PROPOSALS if differs(n)], f"no case of the sweep tells '{mutant}' from the true restatement"


# ================================================================================================ pos_ratio outside [0, 1]
def test_reference_with_pos_ratio_above_one_drops_only_the_last_negatives():
    """pos_ratio > 1 gives n_sample - pos_length < 0.  The reference's ``i[n_neg:]`` then disables only the last |n_neg|
    negatives (AnchorTargetCreator) and ``i[:neg_roi_per_this_image]`` drops only the last of them (ProposalTargetCreator);
    the kernels' `1 > n_neg` branch and max(0, ...) clamp do something else.  Pinned here on the oracle and the restatement;
    the creators refuse such a ratio (below), so the kernels are never asked."""
    c = T.anchor_case("A255-G256")
    kw = dict(c["kw"], n_sample=100, pos_ratio=1.25)                                               # n_pos 125, n_neg -25
    loc, label = oracle_targets.anchor_targets(c["bbox"], c["anchor"], **kw)
    w = T.anchor_stages(c["bbox"], c["anchor"], **kw)
    assert w["n_neg"] == -25 and _same(label, w["label"])
    neg = torch.where(w["label_cap"] == 0)[0]
    assert neg.numel() > 25 and (label[neg[:-25]] == 0).all() and (label[neg[-25:]] == -1).all()
    p = T.proposal_case("R767-G257-dense")
    kw = dict(p["kw"], n_sample=100, pos_ratio=1.25)                                               # 125 positives, room -25
    w = T.proposal_stages(p["roi"], p["bbox"], p["label"], **kw)
    assert w["pos_len"] == 125 and w["room"] == -25 and w["neg_len"] == w["neg_all"].numel() - 25 > 0
    try:
        roi, _, _ = oracle_targets.proposal_targets(p["roi"], p["bbox"], p["label"], **kw)
        assert w["status"] == 0 and _same(roi, w["sample_roi"])
    except IndexError:
        assert w["status"] == 1


@pytest.mark.parametrize("ratio", [1.25, -0.25, float("nan")])
def test_creators_refuse_a_pos_ratio_outside_the_unit_interval(ratio):
    from two_stage_object_detection_amd.nets import frcnn_training as ft
    with pytest.raises(ValueError, match="pos_ratio"):
        ft.AnchorTargetCreator(pos_ratio=ratio)
    with pytest.raises(ValueError, match="pos_ratio"):
        ft.ProposalTargetCreator(pos_ratio=ratio)
    late = ft.AnchorTargetCreator()
    late.pos_ratio = ratio                                           # the attribute is read at call time: checked there too
    with pytest.raises(ValueError, match="pos_ratio"):
        late(torch.zeros(1, 4), torch.zeros(4, 4))
    for ok in (0.0, 0.5, 1.0):
        ft.AnchorTargetCreator(pos_ratio=ok), ft.ProposalTargetCreator(pos_ratio=ok)
