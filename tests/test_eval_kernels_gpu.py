"""The kernels of csrc/eval_metrics.hip at every chunk, lane and pass switch, called directly through hip_ops (eval_match,
eval_match_coco, eval_accumulate, eval_accumulate_coco, sort_pairs_u64) on the designed cases of
tests/eval_kernels_restated.py, against coco_eval_restated.match_image / accumulate and test_detection_eval.evaluate_np.

Every integer (records, masks, ranks, npig, TP / FP / FN, n_records, sorted keys and payloads) is compared bit for bit; f64
precision and recall within 1e-12, the evaluator tests' bar; two runs must give identical bits.  The tests without the gpu
mark pin the case tables to the constants in the source text and check that each case is what its name says."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_eval_restated as CR  # noqa: E402
import eval_kernels_restated as K  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "two_stage_object_detection_amd", "csrc", "eval_metrics.hip")
F64_BAR = 1e-12


@pytest.fixture(scope="module")
def ops():
    from two_stage_object_detection_amd import hip_ops
    return hip_ops


# ================================================================================================ the cases, built once
segment_case = functools.lru_cache(maxsize=None)(K.segment_case)
sparse_case = functools.lru_cache(maxsize=None)(K.sparse_case)
odd_scores_case = functools.lru_cache(maxsize=None)(K.odd_scores_case)
pass_case = functools.lru_cache(maxsize=None)(K.pass_case)
cell_case = functools.lru_cache(maxsize=None)(K.cell_case)
live_count_cases = functools.lru_cache(maxsize=None)(K.live_count_cases)


@functools.lru_cache(maxsize=None)
def match_cases():
    cases = {}
    for B in K.OFFSET_BATCHES:
        cases[f"B{B}"] = K.offsets_case(B)
    cases["overflow"] = K.overflow_case()
    for n in K.CLASSES_PER_IMAGE:
        cases[f"classes{n}"] = K.classes_case(n)
    for n, cap in K.DETS_VS_CAP:
        cases[f"n{n}-cap{cap}"] = K.cap_case(n, cap)
    for R in K.ROW_COUNTS:
        cases[f"R{R}"] = K.rows_case(R)
    for n in K.GT_COUNTS:
        cases[f"gt{n}"] = K.gt_case(n)
    cases.update(K.tie_cases())
    cases["keep"] = K.keep_case()
    cases["odd_rows"] = K.odd_rows_case()
    cases["negative_area"] = K.negative_area_case()
    cases["coco_special"] = K.coco_special_case()
    cases["coco_special_derived"] = K.coco_special_case(name="coco_special_derived", derived=True)
    cases["coco_special_A1"] = K.coco_special_case(areas=(K.COCO_RANGES[2],), name="coco_special_A1")
    return cases


@functools.lru_cache(maxsize=None)
def want_match(name, coco):
    return K.want_match(match_cases()[name], coco)


MATCH_FAMILIES = {
    "offsets": [f"B{B}" for B in K.OFFSET_BATCHES],
    "classes": [f"classes{n}" for n in K.CLASSES_PER_IMAGE],
    "cap": [f"n{n}-cap{c}" for n, c in K.DETS_VS_CAP],
    "rows": [f"R{R}" for R in K.ROW_COUNTS],
    "gt": [f"gt{n}" for n in K.GT_COUNTS],
    "ties": ["equal_iou_later_gt", "duplicate_gt", "iou_at_threshold", "equal_scores_cap"],
    "odd": ["keep", "odd_rows", "negative_area"],
}
COCO_ONLY = ["coco_special", "coco_special_derived", "coco_special_A1"]


def image_records(name, b, update=-1):
    """The COCO restatement's records of image b of one update of a match case (rows [n, 11])."""
    case = match_cases()[name]
    lo = [np.float32(a[0]) for a in case["areas"]]
    hi = [np.float32(a[1]) for a in case["areas"]]
    recs, _ = CR.match_image(case["updates"][update]["images"][b], list(case["thr"]), lo, hi, case["C"], case["max_dets"],
                             case["ignore_class"])
    return recs


# ============================================================================================== CPU: tables and conditions
def test_case_tables_straddle_the_constants_in_the_source():
    """The restated constants are the ones in eval_metrics.hip, and the tables have a case on each side of every one of
    them: a changed constant or rule must fail here, or the GPU cases silently stop reaching their switch."""
    with open(SOURCE) as f:
        src = f.read()

    def const(name):
        base, *shift = re.search(rf"constexpr int {name} = ([0-9 <]+);", src).group(1).split("<<")     # "8192" or "1 << 18"
        return int(base) << (int(shift[0]) if shift else 0)

    assert (const("kThreads"), const("kApItems"), const("kRadixItems")) == (K.THREADS, K.AP_ITEMS, K.RADIX_ITEMS)
    assert (const("kMaxR"), const("kMaxG"), const("kMaxT"), const("kMaxClasses")) == (K.MAX_R, K.MAX_G, K.MAX_T, K.MAX_CLASSES)
    assert "constexpr int kRadixTile = kThreads * kRadixItems;" in src
    # the loops whose trips the cases count
    assert len(re.findall(r"for \(int c0 = s; c0 < e; c0 \+= kThreads \* kApItems\)", src)) == 1      # the AP scan
    assert len(re.findall(r"for \(int b0 = 0; b0 < B; b0 \+= kThreads\)", src)) == 1                  # the offsets scan
    assert len(re.findall(r"int NP = 64;\s*while \(NP < R\) NP <<= 1;", src)) == 1                    # the match launcher
    assert "const int per = (NP + kThreads - 1) / kThreads;" in src
    assert re.search(r"int class_bits\(int C\) \{\s*int bits = 1;\s*while \(bits < 31 && \(1ll << bits\) < \(long long\)C\) "
                     r"\+\+bits;\s*return bits;\s*\}", src)
    assert len(re.findall(r"launch_sort\(w\.keys, nullptr, capacity, nd, 0, 32 \+ class_bits\(num_classes\)", src)) == 1
    assert "const int passes = (int)tsod_cdiv(end_bit - begin_bit, 8);" in src
    assert "const bool to_out = ((passes - 1 - i) & 1) == 0;" in src
    assert len(re.findall(r"for \(int base = 0; base < NP; base \+= 64\)", src)) == 1                 # segment starts by ballot
    assert len(re.findall(r"if \(\(seg\+\+ & 3\) != wave\) continue;", src)) == 1                     # four waves, round-robin
    assert len(re.findall(r"for \(int q0 = 0; q0 < max_dets; q0 \+= 64\)", src)) == 1
    assert len(re.findall(r"if \(nv < 64\) break;", src)) == 1
    assert len(re.findall(r"for \(int g0 = 0; g0 < gn; g0 \+= 64\)", src)) == 1
    # one kernel of each kind (every path runs the loops above), instantiated through its launcher for both record types
    assert len(re.findall(r"\neval_match_kernel\(", src)) == len(re.findall(r"\neval_ap_kernel\(", src)) == 1
    for kernel, launcher in (("eval_match_kernel", "launch_match"), ("eval_ap_kernel", "launch_accumulate")):
        assert f"hipLaunchKernelGGL({kernel}<Rec>," in src
        for rec in ("tsod_eval_record", "tsod_eval_record_coco"):
            assert f"return {launcher}<{rec}>(" in src
    assert K.WAVE == 64

    chunk = K.AP_CHUNK
    assert {chunk - 1, chunk, chunk + 1, 2 * chunk} <= set(K.SEGMENT_LENGTHS)
    assert {K.AP_ITEMS - 1, K.AP_ITEMS, K.AP_ITEMS + 1, 1} <= set(K.SEGMENT_LENGTHS)                  # one thread's items
    assert max(K.SEGMENT_LENGTHS) > 3 * chunk and max(K.SEGMENT_LENGTHS) % chunk % K.AP_ITEMS
    assert K.BEFORE % K.THREADS and K.BEFORE > 0
    assert min(K.OFFSET_BATCHES) == K.THREADS + 1 and max(K.OFFSET_BATCHES) > 2 * K.THREADS           # two trips and three
    assert max(K.OFFSET_BATCHES) <= 65535
    assert [K.radix_passes(C) for C in K.CLASS_COUNTS] == [5, 5, 5, 5, 6, 6, 7, 7]
    assert {256, 257, 65536, 65537} <= set(K.CLASS_COUNTS) and max(K.CLASS_COUNTS) == K.MAX_CLASSES
    assert [K.class_bits(C) for C in (1, 2, 3, 4, 5, 256, 257, 1 << 18)] == [1, 1, 2, 2, 3, 8, 9, 18]
    assert [(e - b + 7) // 8 for b, e in K.SORT_WIDTHS] == [5, 6, 7] and all((e - b) % 8 for b, e in K.SORT_WIDTHS)
    assert set(K.SORT_SIZES) == {K.RADIX_TILE - 1, K.RADIX_TILE, K.RADIX_TILE + 1}
    assert {K.WAVE - 1, K.WAVE, K.WAVE + 1, K.THREADS - 1, K.THREADS, K.THREADS + 1} <= set(K.ROW_COUNTS)
    assert [K.np_of(R) for R in K.ROW_COUNTS] == [64, 64, 64, 128, 256, 256, 512, 1024]
    assert [K.cap_chunk(R) for R in K.ROW_COUNTS] == [1, 1, 1, 1, 1, 1, 2, 4] and max(K.ROW_COUNTS) <= K.MAX_R
    assert {0, 1, K.WAVE - 1, K.WAVE, K.WAVE + 1} <= set(K.GT_COUNTS) and 2 * K.WAVE < max(K.GT_COUNTS) <= K.MAX_G - 16
    assert {(K.WAVE - 1, K.WAVE), (K.WAVE, K.WAVE), (K.WAVE + 1, K.WAVE), (2 * K.WAVE + 1, K.WAVE),
            (2 * K.WAVE + 2, 2 * K.WAVE)} <= set(K.DETS_VS_CAP)
    assert any(n == K.WAVE and cap > n for n, cap in K.DETS_VS_CAP)                     # nv == 64, then an empty trip
    assert any(cap % K.WAVE and n > cap > K.WAVE for n, cap in K.DETS_VS_CAP) and any(cap == 1 for _, cap in K.DETS_VS_CAP)
    assert {1, 4, 5, 9} <= set(K.CLASSES_PER_IMAGE) and max(K.CLASSES_PER_IMAGE) > 2 * K.WAVE
    assert cell_case()["T"] == K.MAX_T


def test_sparse_accumulate_is_the_restatement_on_every_class():
    """want_accumulate (classes without records or ground truth filled in with array operations) against the restatement
    looped over every class, and against answers worked out by hand."""
    case = dict(score=np.float32([.9, .8, .7, .6, .5]), cls=np.int32([4, 4, 1, 4, 1]), rank=np.int32([0, 1, 0, 2, 1]),
                tp=np.uint32([[1, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]),
                ig=np.zeros((5, 4), np.uint32), npig=np.int64([[0], [2], [0], [3], [2], [0]]), T=1, caps=(2, 3), max_dets=3,
                n_records=5, C=6)
    got = K.want_accumulate(case, True)
    full = CR.accumulate(case["score"], case["cls"], case["rank"], case["tp"], case["ig"], case["npig"], 1, [2, 3])
    for g, w in zip(got, full):
        assert np.array_equal(g, w)
    precision, recall, TP, FP, FN = got
    assert TP[:, 0, 1, 0].tolist() == [0, 1, 0, 0, 2, 0] and FP[:, 0, 1, 0].tolist() == [0, 1, 0, 0, 1, 0]
    assert FN[:, 0, 1, 0].tolist() == [0, 1, 0, 3, 0, 0] and TP[4, 0, 0, 0] == 1 and FP[4, 0, 0, 0] == 1
    assert precision[:, 0, 1, 0].tolist()[:4] == [-1.0, 51 / 101, -1.0, 0.0]          # class 1: precision 1 up to recall 0.5
    want = 0.0
    for v in [1.0] * 51 + [2 / 3] * 50:                                                # class 4, cap 3: tp 1, 1, 2 of 2
        want += v
    assert precision[4, 0, 1, 0] == want / 101 and precision[4, 0, 0, 0] == 51 / 101
    assert recall[:, 0, 1, 0].tolist() == [-1.0, .5, -1.0, 0.0, 1.0, -1.0]
    plain = K.want_accumulate(case, False)                                             # no cap, no rank
    assert plain[2][:, 0, 0, 0].tolist() == [0, 1, 0, 0, 2, 0] and plain[0][4, 0, 0, 0] == want / 101


def test_accumulate_case_conditions():
    for coco in (False, True):
        for L in K.SEGMENT_LENGTHS:
            for pattern in K.TP_PATTERNS:
                case = segment_case(L, pattern, coco)
                seg = K.sorted_segment(case, 1)
                assert len(seg) == L and len(K.sorted_segment(case, 0)) == K.BEFORE and len(K.sorted_segment(case, 2)) == K.AFTER
                assert (np.diff(case["score"][seg]) < 0).all()                         # distinct scores: positions are fixed
                assert not (np.diff(seg) > 0).all() or L < 3                           # the sort has work to do
                bits = case["tp"][seg, 0]
                assert bits.sum() == case["n_tp"]
                want = {"all": L, "none": 0, "at4095": int(L > 4095), "at4096": int(L > 4096), "alternating": (L + 1) // 2}
                if pattern in want:
                    assert case["n_tp"] == want[pattern]
                if pattern == "at4095" and L > 4095:
                    assert bits[K.AP_CHUNK - 1] == 1                                   # the last position of the first chunk
                if pattern == "at4096" and L > 4096:
                    assert bits[K.AP_CHUNK] == 1                                       # the first position of the second
                if pattern == "random":
                    assert L < 15 or 0 < case["n_tp"] < L
                values = K.npig_values(case["n_tp"])
                assert values[0] == 0 and all(v >= case["n_tp"] for v in values[1:])
                if coco:                                                               # sparse: range 1 and the cap of 10
                    live = (case["ig"][seg, 1] == 0) & (case["rank"][seg] < 10)
                    assert L < 4000 or 0 < live.sum() < L / 4
    assert -(-12293 // K.AP_CHUNK) == 4 and -(-8192 // K.AP_CHUNK) == 2 and -(-4097 // K.AP_CHUNK) == 2

    case = sparse_case("dead_middle")
    live = case["live_sorted"].reshape(-1)
    per_chunk = [int(live[i:i + K.AP_CHUNK].sum()) for i in range(0, len(live), K.AP_CHUNK)]
    assert per_chunk[1] == 0 and per_chunk[0] == K.AP_CHUNK and per_chunk[2] > 0 and len(per_chunk) == 4
    seg = K.sorted_segment(case, 1)
    assert np.array_equal((case["rank"][seg] < 50) & (case["ig"][seg, 0] == 0), live)
    case = sparse_case("carry_n_apart")
    live = case["live_sorted"]
    assert 2 * K.AP_CHUNK - int(live[:2 * K.AP_CHUNK].sum()) > K.AP_CHUNK              # position - live count at chunk 2
    assert live[:2 * K.AP_CHUNK].sum() == 10 and live[2 * K.AP_CHUNK:].all()
    assert (case["tp"][K.sorted_segment(case, 1), 0][2 * K.AP_CHUNK:] == 1).any() and case["npig"][1, 0] > 0

    case = odd_scores_case()
    seg = K.sorted_segment(case, 1)
    s, tp = case["score"][seg], case["tp"][seg, 0]
    a, b = K.AP_CHUNK - 1, K.AP_CHUNK
    assert s[a].view(np.int32) == s[b].view(np.int32) and tp[a] != tp[b] and (s[a - 5:b + 6] == s[a]).all()
    assert np.isposinf(s[:3]).all() and (s < 0).any() and (np.abs(s[s != 0]).min() < np.finfo(np.float32).tiny)
    z = case["zero_at"]
    assert s[z:z + 4].view(np.uint32).tolist() == [0, 0x80000000, 0, 0x80000000] and tp[z:z + 4].tolist() == [1, 0, 0, 1]
    assert len(set(K.desc_score_bits(s[z:z + 4]).tolist())) == 1 and (np.diff(seg[z:z + 4]) > 0).all()
    assert (np.diff(K.desc_score_bits(s).astype(np.int64)) >= 0).all()                 # the key order is the score order
    flipped = {k: (v[::-1].copy() if isinstance(v, np.ndarray) and k != "npig" else v) for k, v in case.items()}
    assert K.want_accumulate(flipped, False)[0][1, 0, 0, 0] != K.want_accumulate(case, False)[0][1, 0, 0, 0]   # order shows

    passes = set()
    for C in K.CLASS_COUNTS:
        case = pass_case(C)
        assert case["classes"] == sorted({0, C // 2, C - 1}) and case["T"] == 1 and case["n_records"] > K.RADIX_TILE
        assert all(len(K.sorted_segment(case, c)) >= 1400 for c in case["classes"])
        passes.add(K.radix_passes(C))
        if C > 256:
            assert (C - 1) << 32 >= 1 << 40                                            # key bits above bit 40
    assert passes == {5, 6, 7}

    (padded, base), (empty, _), (over, base2) = live_count_cases()
    N = base["n_records"]
    assert len(padded["score"]) == N + 500 and padded["n_records"] == N and (padded["cls"][N:] == 1).all()
    assert (padded["tp"][N:] == 1).all() and (padded["score"][N:] > base["score"].max()).all()
    assert empty["n_records"] == 0 and over["n_records"] > len(over["score"]) and base2 is base

    case = cell_case()
    assert case["T"] == 32 and case["npig"].shape == (3, 4) and len(case["caps"]) == 4
    assert (case["tp"] >> np.uint32(31)).any() and (case["ig"] >> np.uint32(31)).any()
    assert len(K.sorted_segment(case, 1)) > K.AP_CHUNK
    precision, recall, TP, FP, FN = K.want_accumulate(case, True)
    cells = {(int(TP[1][i]), int(FP[1][i]), float(precision[1][i])) for i in np.ndindex(4, 4, 32)}
    assert len(cells) == 4 * 4 * 32 and (TP <= case["npig"][:, :, None, None]).all()   # every cell its own value


def class_starts(recs):
    cls = np.array([r[1] for r in recs])
    return np.nonzero(np.diff(cls, prepend=-1))[0]


def test_match_case_conditions():
    cases = match_cases()
    # offsets: two and three trips, images without detections, records before the update
    for B in K.OFFSET_BATCHES:
        case = cases[f"B{B}"]
        first, big = case["updates"]
        assert len(big["images"]) == B and big["det"].shape == (B, 6, 6)
        n = [len(im[0]) for im in big["images"]]
        assert min(n) == 0 and max(n) == 6 and sum(k == 0 for k in n) > 5
        assert sum(len(image_records(f"B{B}", b, 0)) for b in range(5)) > 0
        tail = sum(len(image_records(f"B{B}", b)) for b in range(K.THREADS, B))
        assert tail > 0                                                                 # records behind the first trip
    case = cases["overflow"]
    assert 0 < case["capacity"] < len(want_match("overflow", True)[0])

    # classes per image (the second image of the batch)
    for n in K.CLASSES_PER_IMAGE:
        recs = image_records(f"classes{n}", 1)
        starts = class_starts(recs)
        assert len(starts) == n and len(recs) == sum(1 + c % 3 for c in range(n)) < 512
        sizes = np.diff(np.append(starts, len(recs)))
        assert sizes.min() >= 1 and sizes.max() <= 3
    starts = class_starts(image_records("classes130", 1))
    sizes = np.diff(np.append(starts, 259))
    assert (starts % 64 == 63).any() and (starts[1:] % 64 == 0).any()                   # lane 63, lane 0 of a later block
    assert ((starts % 64) + sizes > 64).any()                                           # a segment across two blocks
    assert len(starts) // 4 >= 32                                                       # every wave owns many segments

    # detections per class against the cap
    for n, cap in K.DETS_VS_CAP:
        case = cases[f"n{n}-cap{cap}"]
        d = case["updates"][0]["images"][1][0]
        assert (d[:, 5] == 1).sum() == n and case["max_dets"] == cap
        recs = image_records(f"n{n}-cap{cap}", 1)
        got = [r for r in recs if r[1] == 1]
        assert len(got) == min(n, cap) and [r[2] for r in got] == list(range(min(n, cap)))
        assert recs[0][1] == 0 and recs[-1][1] == 2                                     # classes before and after
        assert any(any(r[3]) for r in got)
    assert cases["n10-cap20"]["updates"][0]["det"].shape[1] < 20                        # max_dets > R

    # sizes of R and NP
    for R in K.ROW_COUNTS:
        up = cases[f"R{R}"]["updates"][0]
        assert up["det"].shape[1] == R and up["counts"][1] == R and up["counts"][0] < max(R, 2)
    d = cases["R1000"]["updates"][0]["images"][1][0]
    assert (d[:, 5] == 3).sum() > 20 * K.cap_chunk(1000)                                # one class over many thread chunks
    assert (d[:, 5] == 3).sum() > cases["R1000"]["max_dets"]

    # ground truth
    for n in K.GT_COUNTS:
        case = cases[f"gt{n}"]
        up = case["updates"][0]
        gl, gc = up["gl"][1], int(up["gt_counts"][1])
        assert (gl[:gc] == 1).sum() == n and gc < up["gl"].shape[1] and (gl[gc:] == 0).all()
        assert (up["gb"][1, gc:] == K.FILL_GT).all()                                    # padding looks like class 0's boxes
        assert -1 in gl[:gc] and case["C"] in gl[:gc] and case["ignore_class"] == 2
        assert (gl[:gc] == 2).any() and (up["images"][1][0][:, 5] == 2).any()
        recs = image_records(f"gt{n}", 1)
        assert all(r[1] != 2 for r in recs) and want_match(f"gt{n}", True)[1][2].sum() == 0
        assert n == 0 or any(any(r[3]) for r in recs if r[1] == 1)

    # ties: the equalities hold in f32
    gts = [[0, 0, 10, 10], [10, 0, 20, 10]]
    iou = CR.iou_f32([5, 0, 15, 10], gts)
    assert iou[0, 0].view(np.int32) == iou[0, 1].view(np.int32) and iou[0, 0] >= np.float32(.3)
    assert [r[3][0] for r in image_records("equal_iou_later_gt", 0)] == [1, 1]          # the earlier index would give [1, 0]
    assert CR.iou_f32([0, 0, 2, 1], [[0, 0, 1, 1]])[0, 0].view(np.int32) == np.float32(.5).view(np.int32)
    assert np.float32(K.HALF_UP) > np.float32(.5)
    assert [r[3][0] for r in image_records("iou_at_threshold", 0)] == [1]               # bit 0 (0.5) set, bit 1 not
    assert [r[3][0] for r in image_records("duplicate_gt", 0)] == [3, 3, 0]
    recs = image_records("equal_scores_cap", 0)
    d = cases["equal_scores_cap"]["updates"][0]["images"][0][0]
    assert len(set(d[1:7, 4].view(np.int32).tolist())) == 1
    assert [(r[1], r[2], r[3][0]) for r in recs] == [(0, 0, 0), (0, 1, 1), (0, 2, 1), (0, 3, 1), (1, 0, 0)]

    up = cases["keep"]["updates"][0]
    assert up["counts"] is None and (up["keep"][:, 3] == -1).all() and (up["keep"][:, 17] == 40).all()
    assert [len(im[0]) for im in up["images"]] == [28, 38, 0]
    assert all(sorted(k.tolist()) != k.tolist() for k in up["keep"])

    recs = image_records("odd_rows", 0)
    assert [(r[1], float(r[0])) for r in recs] == [(0, np.inf), (0, -0.0), (0, 0.0), (0, 0.0), (2, .5), (2, -1.5)]
    assert np.float32(recs[1][0]).view(np.uint32) == 0x80000000                         # -0.0 == +0.0: the lower row first

    # negative areas: counted by the plain metric, ignored by COCO's "all"; the two restatements must differ here
    plain, coco = want_match("negative_area", False), want_match("negative_area", True)
    assert plain[0].tolist() == [[1063675494, 0, 0], [1061997773, 1, 3]] and plain[1].tolist() == [1, 1]
    assert coco[0].tolist() == [[1063675494, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0], [1061997773, 1, 0, 3, 0, 0, 0, 0, 0, 0, 0]]
    assert coco[1].tolist() == [[0], [1]]
    assert plain[0][0, 2] == 0 and coco[0][0, 7] == 3 and plain[1][0] != coco[1][0, 0]   # an FP against ignored; npig 1 against 0

    # COCO only
    recs = image_records("coco_special", 0)
    im = cases["coco_special"]["updates"][0]["images"][0]
    assert [r[4][0] for r in recs[:3]] == [3, 3, 3] and [r[3][0] for r in recs[:3]] == [0, 0, 0]   # one crowd, three times
    assert im[4][1].view(np.int32) == np.float32(32 ** 2).view(np.int32) == np.float32(K.COCO_RANGES[1][1]).view(np.int32)
    hi_medium, lo_large = np.float32(K.COCO_RANGES[2][1]), np.float32(K.COCO_RANGES[3][0])
    assert im[4][2].view(np.int32) == hi_medium.view(np.int32) == lo_large.view(np.int32)
    npig = want_match("coco_special", True)[1]
    assert npig[1].tolist() == [2, 1, 2, 1] and npig[0].tolist() == [0, 0, 0, 0]
    assert recs[5][1] == 2 and recs[5][3] == [0, 0, 0, 0] and recs[5][4] == [0, 0, 3, 3]           # unmatched, out of range
    derived = image_records("coco_special_derived", 0)
    assert cases["coco_special_derived"]["updates"][0]["area"] is None and cases["coco_special"]["updates"][0]["area"] is not None
    assert [r[3] for r in derived[3:5]] == [r[3] for r in recs[3:5]]
    one = image_records("coco_special_A1", 0)
    assert [(r[3][0], r[4][0]) for r in one] == [(r[3][2], r[4][2]) for r in recs]                  # A = 1 is A = 4's range 2


# ========================================================================================================= GPU: running
def up(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def run_accumulate(ops, dev, case, coco):
    rows = K.coco_rows(case) if coco else K.plain_rows(case)
    records, n = up(rows, dev), torch.tensor([case["n_records"]], dtype=torch.int64, device=dev)
    if coco:
        out = ops.eval_accumulate_coco(records, n, up(case["npig"], dev), case["T"], case["caps"], case["max_dets"])
    else:
        out = ops.eval_accumulate(records, n, up(case["npig"][:, 0], dev), case["T"])
    torch.cuda.synchronize()
    assert torch.equal(records.cpu(), torch.from_numpy(rows)) and int(n) == case["n_records"]          # inputs untouched
    return out.cpu().numpy()


def check_accumulate(ops, dev, case, coco, want=None):
    got = run_accumulate(ops, dev, case, coco)
    want = K.want_accumulate(case, coco) if want is None else want
    shape = want[0].shape if coco else (want[0].shape[0], want[0].shape[3])
    assert got.shape == (5,) + shape
    for i, k in ((2, "TP"), (3, "FP"), (4, "FN")):
        assert np.array_equal(got[i - 1], want[i].reshape(shape)), (case["name"], k)
    for i, j, k in ((0, 0, "precision"), (4, 1, "recall")):
        err = np.abs(got[i].view(np.float64) - want[j].reshape(shape)).max()
        assert err <= F64_BAR, (case["name"], k, err)
    assert np.array_equal(got, run_accumulate(ops, dev, case, coco)), case["name"]                     # two runs: same bits
    return got


def run_match(ops, dev, case, coco):
    ints = K.COCO_INTS if coco else K.PLAIN_INTS
    C, A = case["C"], len(case["areas"])
    bound = sum(u["det"].shape[0] * u["det"].shape[1] for u in case["updates"])
    cap = bound + 8 if case["capacity"] is None else case["capacity"]
    buf = torch.full((cap + 64, ints), K.SENTINEL, dtype=torch.int32, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    npig = torch.zeros((C, A) if coco else (C,), dtype=torch.int64, device=dev)
    thr = torch.tensor(case["thr"], dtype=torch.float32, device=dev)
    lo = torch.tensor([a[0] for a in case["areas"]], dtype=torch.float32, device=dev)
    hi = torch.tensor([a[1] for a in case["areas"]], dtype=torch.float32, device=dev)
    counts_after = []
    for u in case["updates"]:
        kw = {k: None if u[k] is None else up(u[k], dev) for k in ("counts", "keep", "n_kept")}
        args = (up(u["det"], dev), up(u["gb"], dev), up(u["gl"], dev), up(u["gt_counts"], dev), thr)
        if coco:
            ops.eval_match_coco(*args, lo, hi, C, case["max_dets"], case["ignore_class"], buf[:cap], n, npig,
                                gt_crowd=None if u["crowd"] is None else up(u["crowd"], dev),
                                gt_area=None if u["area"] is None else up(u["area"], dev), **kw)
        else:
            ops.eval_match(*args, C, case["max_dets"], case["ignore_class"], buf[:cap], n, npig, **kw)
        counts_after.append(int(n))
    return buf.cpu().numpy(), counts_after, npig.cpu().numpy()


def check_match(ops, dev, name, coco):
    case = match_cases()[name]
    want_rows, want_npig = want_match(name, coco)
    buf, counts_after, npig = run_match(ops, dev, case, coco)
    total, cap = len(want_rows), len(buf) - 64
    assert counts_after[-1] == total, (name, counts_after, total)
    assert np.array_equal(npig, want_npig), name
    live = min(total, cap)
    diff = np.nonzero((buf[:live] != want_rows[:live]).any(1))[0]
    assert len(diff) == 0, (name, "first differing record", int(diff[0]), buf[diff[0]].tolist(), want_rows[diff[0]].tolist())
    assert (buf[live:] == K.SENTINEL).all(), name                                                      # nothing past the records
    again = run_match(ops, dev, case, coco)
    assert np.array_equal(buf, again[0]) and counts_after == again[1] and np.array_equal(npig, again[2]), name
    return buf[:live], counts_after


# ---------------------------------------------------------------------------------------------------------- A. accumulate
@gpu
@pytest.mark.parametrize("coco", [False, True], ids=["plain", "coco"])
@pytest.mark.parametrize("pattern", K.TP_PATTERNS)
@pytest.mark.parametrize("L", K.SEGMENT_LENGTHS)
def test_ap_scan_segment_lengths(dev, ops, L, pattern, coco):
    """One to four chunks of the AP scan, every TP pattern, npig of 0, 1, the TP count and three times it."""
    case = segment_case(L, pattern, coco)
    for value in K.npig_values(case["n_tp"]):
        got = check_accumulate(ops, dev, K.with_npig(case, value), coco)
        ap = got[0].view(np.float64)[1]
        assert (ap == -1).all() if value == 0 else (ap >= 0).all()


@gpu
@pytest.mark.parametrize("kind", ["dead_middle", "carry_n_apart"])
def test_ap_scan_sparse_live_records(dev, ops, kind):
    check_accumulate(ops, dev, sparse_case(kind), True)


@gpu
@pytest.mark.parametrize("coco", [False, True], ids=["plain", "coco"])
def test_ap_scan_ties_and_odd_scores(dev, ops, coco):
    check_accumulate(ops, dev, odd_scores_case(), coco)


@gpu
@pytest.mark.parametrize("coco", [False, True], ids=["plain", "coco"])
@pytest.mark.parametrize("C", K.CLASS_COUNTS)
def test_accumulate_radix_pass_counts(dev, ops, C, coco):
    """5, 6 and 7 radix passes (both ping-pong parities) and class bits above bit 40."""
    case = pass_case(C)
    got = check_accumulate(ops, dev, case, coco)
    tp = got[1].reshape(C)
    assert all(tp[c] > 0 for c in case["classes"]) and tp.sum() == sum(tp[c] for c in case["classes"])


@gpu
@pytest.mark.parametrize("coco", [False, True], ids=["plain", "coco"])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["dead_tail", "no_records", "count_above_capacity"])
def test_accumulate_live_count(dev, ops, which, coco):
    case, same_as = live_count_cases()[which]
    check_accumulate(ops, dev, case, coco, want=K.want_accumulate(same_as, coco))


@gpu
def test_accumulate_cell_addressing(dev, ops):
    check_accumulate(ops, dev, cell_case(), True)


@gpu
@pytest.mark.parametrize("n", K.SORT_SIZES)
@pytest.mark.parametrize("bits", K.SORT_WIDTHS, ids=lambda b: f"bits{b[0]}-{b[1]}")
def test_sort_widths_off_the_byte(dev, ops, bits, n):
    """A last pass of 1 bit: the key bits at and above end_bit must not take part."""
    rng = np.random.default_rng(n + bits[1])
    keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    keys[rng.random(n) < .5] &= np.uint64((1 << 64) - (1 << (bits[1] - 3)))               # many equal sorted fields
    vals = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    field = keys & np.uint64((1 << bits[1]) - 1)
    order = np.argsort(field, kind="stable")
    assert (field[order][1:] == field[order][:-1]).any() and (keys >> np.uint64(bits[1])).any()
    for _ in range(2):
        k_out, v_out = ops.sort_pairs_u64(up(keys.view(np.int64), dev), up(vals, dev), *bits)
        assert np.array_equal(v_out.cpu().numpy(), vals[order])
        assert np.array_equal(k_out.cpu().numpy().view(np.uint64), keys[order])


# ------------------------------------------------------------------------------------------------ B. match and compaction
def both(names):
    return [(n, c) for n in names for c in (False, True)]


def ids(v):
    return {False: "plain", True: "coco"}.get(v, v) if isinstance(v, (bool, str)) else None


@gpu
@pytest.mark.parametrize("name,coco", both(MATCH_FAMILIES["offsets"]), ids=ids)
def test_offsets_scan_trips_and_running_total(dev, ops, name, coco):
    _, counts_after = check_match(ops, dev, name, coco)
    assert 0 < counts_after[0] < counts_after[1]


@gpu
@pytest.mark.parametrize("coco", [False, True], ids=["plain", "coco"])
def test_capacity_overflow(dev, ops, coco):
    rows, counts_after = check_match(ops, dev, "overflow", coco)
    assert len(rows) == match_cases()["overflow"]["capacity"] < counts_after[-1]


@gpu
@pytest.mark.parametrize("name,coco", both(MATCH_FAMILIES["classes"]), ids=ids)
def test_classes_per_image(dev, ops, name, coco):
    check_match(ops, dev, name, coco)


@gpu
@pytest.mark.parametrize("name,coco", both(MATCH_FAMILIES["cap"]), ids=ids)
def test_detections_per_class_against_the_cap(dev, ops, name, coco):
    check_match(ops, dev, name, coco)


@gpu
@pytest.mark.parametrize("name,coco", both(MATCH_FAMILIES["rows"]), ids=ids)
def test_row_counts_and_sort_sizes(dev, ops, name, coco):
    check_match(ops, dev, name, coco)


@gpu
@pytest.mark.parametrize("name,coco", both(MATCH_FAMILIES["gt"]), ids=ids)
def test_ground_truth_counts(dev, ops, name, coco):
    check_match(ops, dev, name, coco)


@gpu
@pytest.mark.parametrize("name,coco", both(MATCH_FAMILIES["ties"]), ids=ids)
def test_tie_rules(dev, ops, name, coco):
    check_match(ops, dev, name, coco)


@gpu
@pytest.mark.parametrize("name,coco", both(MATCH_FAMILIES["odd"]), ids=ids)
def test_keep_indirection_and_odd_rows(dev, ops, name, coco):
    check_match(ops, dev, name, coco)


@gpu
@pytest.mark.parametrize("name", COCO_ONLY)
def test_coco_crowd_area_bounds_and_ranges(dev, ops, name):
    check_match(ops, dev, name, True)
