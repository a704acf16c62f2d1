"""The detection overlay kernel on the GPU: every case is bit-equal to the NumPy painter's restatement
(tests/draw_restated.py) on the WHOLE buffer, the bytes between 3 W and the row pitch included (they must stay as they were).
Everything is integer arithmetic beyond one f32 multiply per coordinate, so there is no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_restated as D  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("boxes", "counts", "keep", "n_kept", "labels")
NAMES = [b"cat", b"dog", b"A-b_c.d:e%(f)/g", b"x" * 31]


@pytest.fixture(scope="module")
def font():
    from two_stage_object_detection_amd import hip_ops
    return hip_ops.draw_font5x7()


def table(names=NAMES):
    t = np.zeros((len(names), 32), dtype=np.uint8)
    for i, s in enumerate(names):
        t[i, :len(s)] = list(s)
    return t


def group(boxes, **kw):
    boxes = np.asarray(boxes, dtype=np.float32)
    if boxes.ndim == 2:
        boxes = boxes[None]
    g = dict(boxes=boxes, color=(255, 0, 0), alpha=255, width=1, tag="none", text_color=(0, 0, 255), tag_bg=(255, 255, 255),
             tag_alpha=255, font_scale=1, padding=0, score_line=False, label_offset=0, scale=(1.0, 1.0))
    g.update(kw)
    for k, dt in (("counts", np.int32), ("keep", np.int32), ("n_kept", np.int32), ("labels", np.int64)):
        if g.get(k) is not None:
            g[k] = np.asarray(g[k], dtype=dt)
    return g


def run(dev, font, H, W, groups, strings=None, B=1, row_pad=0, seed=0, repeat=1):
    """Paint a random pitched buffer on the device and in NumPy; assert that every byte agrees.  -> the painted [B,H,W,3] view."""
    from two_stage_object_detection_amd import hip_ops
    row = 3 * W + row_pad
    buf = np.random.default_rng(seed).integers(0, 256, size=(B, H, row), dtype=np.uint8)
    want = buf.copy()
    view = np.lib.stride_tricks.as_strided(want, shape=(B, H, W, 3), strides=(H * row, row, 3, 1))
    for g in groups:
        g.setdefault("strings", (0, 0 if strings is None else len(strings)))
    D.draw(view, groups, strings, font)
    on_dev = [{k: (torch.from_numpy(v).to(dev) if k in ARRAYS and v is not None else v) for k, v in g.items()} for g in groups]
    st = None if strings is None else torch.from_numpy(strings).to(dev)
    for _ in range(repeat):
        t = torch.from_numpy(buf.copy()).to(dev)
        hip_ops.draw_groups(t.as_strided((B, H, W, 3), (H * row, row, 3, 1)), on_dev, st)
        got = t.cpu().numpy()
        diff = np.argwhere(got != want)
        assert diff.size == 0, f"{len(diff)} bytes differ, first at (b, y, byte) = {diff[0].tolist()}"
    return view


# ---------------------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7)])
def test_tiny_images(dev, font, H, W):
    boxes = [[0, 0, 0, 0], [-3, -2, 2, 2], [1, 1, 20, 20], [-5, -5, 30, 30], [9, 9, 12, 12], [-9, -9, -1, -1], [3, 1, 2, 4],
             [1, 3, 5, 2]]                                           # inside, partly out, covering, wholly out, X2 < X1, Y2 < Y1
    for k, bx in enumerate(boxes):
        run(dev, font, H, W, [group([bx], color=(k, 200, 10))], seed=k)
    out = run(dev, font, H, W, [group(boxes, alpha=100)])
    assert out.shape == (1, H, W, 3)


def test_non_finite_and_huge_coordinates(dev, font):
    nan, inf = float("nan"), float("inf")
    boxes = [[nan, 1, 5, 5], [1, nan, 5, 5], [1, 1, inf, 5], [-inf, 1, 5, 5], [1, 1, 5, -inf], [2, 2, 1e30, 1e30], [-1e30, -1e30, 3, 3],
             [-1e30, 4, 1e30, 6], [0, 0, 3.4e38, 2]]
    before = np.random.default_rng(3).integers(0, 256, size=(1, 9, 3 * 11), dtype=np.uint8)
    for k, bx in enumerate(boxes):
        out = run(dev, font, 9, 11, [group([bx], tag="below", labels=[[1]])], table(), seed=3)
        assert (k < 5) == np.array_equal(out.reshape(1, 9, 33), before), k      # the first five draw nothing, not even a tag
    # a scale that overflows the product: clamped, not dropped; a NaN product (0 * inf) draws nothing
    run(dev, font, 9, 11, [group([[1, 1, 2, 2]], scale=(3e38, 1e38))])
    out = run(dev, font, 9, 11, [group([[0, 0, 2, 2]], scale=(inf, 1.0))], seed=3)
    assert np.array_equal(out.reshape(1, 9, 33), before)


def test_rounding_ties_thickness_and_scale(dev, font):
    halves = [[0.5, 1.5, 6.5, 7.5], [2.5, 2.5, 3.5, 3.5], [-0.5, -1.5, 4.5, 5.5], [1.4999, 1.5001, 8.5, 9.49]]
    for t in (1, 3, 4, 50):                                          # 50: larger than half of any box here, the boxes fill
        run(dev, font, 12, 13, [group(halves, width=t, alpha=90)], seed=t)
    for scale in ((0.5, 0.5), (1.5, 0.25), (600 / 224, 600 / 160), (-1.0, 1.0)):
        run(dev, font, 12, 13, [group([[1, 2, 7, 30], [3, 3, 4, 4], [-9, 5, -1, 11]], scale=scale, width=2)])


# ------------------------------------------------------------------------------------------------------ blending and order
def test_alpha_and_painters_order(dev, font):
    for a in (0, 128, 255):
        run(dev, font, 20, 24, [group([[2, 2, 15, 15]], alpha=a, width=3, tag="below", labels=[[0]], tag_alpha=a)], table(), seed=a)
    # three overlapping items from two groups: the later one wins where they meet, blended over what is there
    g0 = group([[2, 2, 14, 14], [6, 6, 18, 17]], color=(255, 0, 0), alpha=128, width=4)
    g1 = group([[4, 0, 10, 19]], color=(0, 255, 0), alpha=200, width=5)
    run(dev, font, 20, 24, [g0, g1])
    assert not np.array_equal(run(dev, font, 20, 24, [g0, g1]), run(dev, font, 20, 24, [g1, g0]))
    # the first row's tag lies over the second row's outline, which is painted before every tag
    first = group([[2, 2, 30, 9], [1, 11, 34, 16]], labels=[[0, 1]], tag="below", width=2, tag_alpha=255, color=(9, 9, 9))
    out = run(dev, font, 40, 40, [first], table())
    assert (out[0, 11, 4] == 255).all() and not (out[0, 11, 32] == 255).all()       # tag background over the outline's top edge


# -------------------------------------------------------------------------------------------------------------- row selection
def test_row_selection(dev, font):
    rng = np.random.default_rng(5)
    lo = rng.integers(0, 20, size=(2, 6, 2))
    boxes = np.concatenate([lo, lo + rng.integers(1, 12, size=(2, 6, 2))], axis=-1).astype(np.float32)
    run(dev, font, 30, 33, [group(boxes, counts=[2, 5], alpha=180)], B=2)
    run(dev, font, 30, 33, [group(boxes, counts=[-4, 99], alpha=180)], B=2)                        # clamped into [0, R]
    keep = [[4, 6, 0, -1, 2, 2], [1, 2, 3, 4, 5, 0]]                                                # 6 and -1 draw nothing
    run(dev, font, 30, 33, [group(boxes, keep=keep, n_kept=[5, 0], alpha=180)], B=2)
    run(dev, font, 30, 33, [group(boxes, keep=keep, n_kept=[9, -1], alpha=180)], B=2)
    out = run(dev, font, 30, 33, [group(boxes, keep=keep, n_kept=[0, 0])], B=2, seed=8)
    assert np.array_equal(out, run(dev, font, 30, 33, [group(np.zeros((2, 0, 4)))], B=2, seed=8))  # R == 0 is a no-op
    run(dev, font, 30, 33, [group(np.zeros((2, 0, 6)), score_line=True, tag="above"), group(boxes, counts=[6, 1])], B=2)


def test_labels_offsets_and_string_lookup(dev, font):
    b4 = [[2, 14, 40, 30], [50, 40, 90, 60]]
    b6 = [[2, 14, 40, 30, 0.5, 1], [50, 40, 90, 60, 0.25, 12]]
    plain = run(dev, font, 80, 120, [group(b4, width=2)], table())
    assert np.array_equal(run(dev, font, 80, 120, [group(b4, width=2, tag="above")], table()), plain)   # pitch 4, no labels: no tag
    named = run(dev, font, 80, 120, [group(b6, width=2, tag="above")], table())                         # the class column names
    assert not np.array_equal(named, plain)
    assert np.array_equal(run(dev, font, 80, 120, [group(b4, width=2, tag="above", labels=[[1, 12]])], table()), named)
    run(dev, font, 80, 120, [group(b6, tag="below", score_line=True, labels=[[3, 0]])], table())        # labels override column 5
    for off in (-2, -1, 1, 11):                                       # class_-1, class_12, class_23 ... and table rows
        run(dev, font, 80, 120, [group(b6, tag="below", label_offset=off, score_line=True)], table())
    run(dev, font, 80, 120, [group(b6, tag="below")], None)           # no table: every label prints class_<n>
    run(dev, font, 80, 120, [group(b4, tag="below", labels=[[-2 ** 63, 2 ** 63 - 1]])], table())
    run(dev, font, 80, 120, [group([[2, 14, 40, 30, 0.5, float("nan")], [50, 40, 90, 60, 0.5, 3e9]], tag="below")], table())
    # two groups read two windows of one table
    both = table([b"GT: cat", b"GT: dog", b"Pred: cat", b"Pred: dog"])
    run(dev, font, 80, 120, [group(b4, labels=[[0, 1]], tag="above", strings=(0, 2), color=(0, 128, 0)),
                             group(b6, tag="below", strings=(2, 2), score_line=True, label_offset=0)], both)


# ----------------------------------------------------------------------------------------------------------------------- tags
def test_tag_placement(dev, font):
    t = table()
    for tag, bx in (("above", [4, 3, 40, 30]), ("above", [4, 8, 40, 30]), ("above", [4, 20, 40, 30]),       # flips at the top edge
                    ("below", [4, 3, 40, 50]), ("below", [4, 3, 40, 51]), ("below", [4, 3, 40, 30]),        # flips at the bottom
                    ("below", [70, 3, 88, 20]), ("below", [89, 3, 200, 20]), ("above", [-7, 20, 30, 30]),   # shifted left; clipped
                    ("below", [4, 55, 40, 70])):
        for lab in (0, 2):
            run(dev, font, 60, 90, [group([bx], tag=tag, labels=[[lab]], width=1, padding=1)], t)
    # a tag wider than the image starts at 0 and is clipped on the right; the 31-byte string
    run(dev, font, 24, 50, [group([[20, 2, 30, 10]], tag="below", labels=[[3]])], t)
    run(dev, font, 40, 400, [group([[300, 2, 330, 10]], tag="below", labels=[[3]], font_scale=2, padding=3)], t)


@pytest.mark.parametrize("scale,pad", [(1, 0), (2, 3), (3, 1), (1, 3), (2, 0)])
def test_font_scale_padding_and_scores(dev, font, scale, pad):
    scores = [0.0, 1.0, 0.9995, 0.0004, -1.0, 2.0, float("nan"), 0.12345, float("inf")]
    boxes = [[3 + 10 * k, 2 + 28 * k, 30 + 10 * k, 9 + 28 * k, s, k % 3] for k, s in enumerate(scores)]
    run(dev, font, 280, 230, [group(boxes, tag="below", score_line=True, font_scale=scale, padding=pad, tag_alpha=204,
                                    text_color=(255, 0, 0))], table())
    run(dev, font, 60, 200, [group([[3, 30, 30, 40, 0.5, 2]], tag="above", font_scale=scale, padding=pad)], table())


# ----------------------------------------------------------------------------------------------------------- launch switches
def test_tile_edges_with_a_pitched_row(dev, font):
    rng = np.random.default_rng(11)
    lo = rng.integers(-10, 60, size=(2, 12, 2))
    boxes = np.concatenate([lo, lo + rng.integers(1, 40, size=(2, 12, 2)), rng.random((2, 12, 1)), rng.integers(0, 6, size=(2, 12, 1))],
                           axis=-1).astype(np.float32)
    gt = group(boxes[:, :4, :4].copy(), labels=[[0, 1, 2, 0]] * 2, tag="above", color=(0, 128, 0), width=2, padding=2, tag_alpha=204)
    pred = group(boxes, counts=[12, 7], tag="below", score_line=True, width=2, padding=2, tag_alpha=204, label_offset=-1)
    run(dev, font, 45, 70, [gt, pred], table(), B=2, row_pad=5)
    run(dev, font, 70, 45, [gt, pred], table(), B=2, row_pad=1)
    run(dev, font, 17, 130, [gt, pred, gt, pred], table(), B=2, row_pad=3)                          # four groups


def test_list_overflow_takes_further_passes(dev, font):
    from two_stage_object_detection_amd import _ffi
    cap = _ffi.DRAW_LIST_CAPACITY
    rng = np.random.default_rng(13)
    for n in (cap, cap + 1, 2 * cap + 3, 5 * cap):                   # every box meets tile (0, 0); 5 cap > one read of the stream
        lo = rng.integers(0, 10, size=(n, 2))
        boxes = np.concatenate([lo, lo + rng.integers(1, 30, size=(n, 2))], axis=-1)
        g = group(boxes, alpha=77, width=2, labels=[list(rng.integers(0, 3, size=n))], tag="below", tag_alpha=60)
        run(dev, font, 40, 80, [g], table(), seed=n)


def test_bit_identical_from_run_to_run(dev, font):
    rng = np.random.default_rng(17)
    lo = rng.integers(0, 100, size=(1, 90, 2))
    boxes = np.concatenate([lo, lo + rng.integers(1, 60, size=(1, 90, 2)), rng.random((1, 90, 2))], axis=-1)
    run(dev, font, 150, 170, [group(boxes, alpha=128, width=2, tag="below", score_line=True, tag_alpha=128)], table(), repeat=2)


# ------------------------------------------------------------------------------------------------------------------ end to end
def _records_group(det, counts=None, keep=None, n_kept=None, scale=(1.0, 1.0), strings=(0, 0), label_offset=0):
    return group(det, counts=counts, keep=keep, n_kept=n_kept, color=(255, 0, 0), tag="below", score_line=True, width=2, padding=2,
                 tag_alpha=204, text_color=(255, 0, 0), scale=scale, strings=strings, label_offset=label_offset)


def test_draw_detections_on_a_seeded_detector(dev, font):
    from two_stage_object_detection_amd.testing import synthetic_detector
    from two_stage_object_detection_amd.utils import overlay
    names = [f"thing{i}" for i in range(20)]
    model, _ = synthetic_detector("resnet50", num_classes=20, seed=0)
    model = model.to(dev).eval()
    x = torch.rand(2, 3, 160, 224, generator=torch.Generator().manual_seed(1234)).to(dev)
    frames = torch.randint(0, 256, (2, 160, 224, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(dev)
    both = np.concatenate([table([b"GT: " + n.encode() for n in names]), table([b"Pred: " + n.encode() for n in names])])
    with torch.inference_mode():
        rows = model.predict(x)
        det = model.detections(x)
        det_sorted, keep, n_kept = model.postprocess(det)
    got = overlay.draw_detections(frames, rows, class_names=names)
    assert got is not frames and got.shape == frames.shape
    R = max(1, max(r.shape[0] for r in rows))
    padded = np.zeros((2, R, 6), dtype=np.float32)
    for b, r in enumerate(rows):
        padded[b, :r.shape[0]] = r.cpu().numpy()
    want = frames.cpu().numpy().copy()
    D.draw(want, [_records_group(padded, counts=[r.shape[0] for r in rows], strings=(20, 20))], both, font)
    assert sum(r.shape[0] for r in rows) > 0 and not np.array_equal(want, frames.cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), want)
    # the same through postprocess's keep / n_kept, in place, and with ground truth and another output size
    again = frames.clone()
    assert overlay.draw_detections(again, det_sorted, keep=keep, n_kept=n_kept, class_names=names, out=again) is again
    assert np.array_equal(again.cpu().numpy(), want)
    big = torch.randint(0, 256, (2, 200, 300, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(6)).to(dev)
    gtb = [torch.tensor([[10., 20., 100., 120.], [5., 5., 50., 60.]], device=dev), torch.tensor([[30., 40., 200., 150.]], device=dev)]
    gtl = [torch.tensor([3, 25], device=dev), torch.tensor([0], device=dev)]
    scale = (300 / 224, 200 / 160)
    got = overlay.draw_detections(big, det_sorted, gtb, gtl, keep=keep, n_kept=n_kept, class_names=names, box_scale=scale)
    want = big.cpu().numpy().copy()
    gt = group(np.array([[[10, 20, 100, 120], [5, 5, 50, 60]], [[30, 40, 200, 150], [0, 0, 0, 0]]]), labels=[[3, 25], [0, -1]],
               counts=[2, 1], color=(0, 128, 0), text_color=(0, 128, 0), tag="above", width=2, padding=2, tag_alpha=204, scale=scale,
               strings=(0, 20))
    D.draw(want, [gt, _records_group(det_sorted.cpu().numpy(), keep=keep.cpu().numpy(), n_kept=n_kept.cpu().numpy(), scale=scale,
                                     strings=(20, 20))], both, font)
    assert np.array_equal(got.cpu().numpy(), want)
    # draw_bounding_boxes: one style, its own table
    one = overlay.draw_bounding_boxes(frames[0], rows[0][:, :4], labels=rows[0][:, 5].long(), scores=rows[0][:, 4], class_names=names,
                                      prefix="P ", color=(1, 2, 3), width=1, alpha=200, tag="above", font_scale=2)
    want = frames[:1].cpu().numpy().copy()
    g = group(padded[:1, :rows[0].shape[0]], labels=padded[:1, :rows[0].shape[0], 5].astype(np.int64), color=(1, 2, 3), alpha=200,
              text_color=(1, 2, 3), tag="above", font_scale=2, padding=2, tag_alpha=204, score_line=True, strings=(0, 20))
    D.draw(want, [g], table([b"P " + n.encode() for n in names]), font)
    assert np.array_equal(one.cpu().numpy(), want[0])


def test_multi_inference_is_the_trainer_plus_draw_detections(dev, golden_dir):
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd.nets.frcnn_training import FasterRCNNTrainer
    from two_stage_object_detection_amd.testing import synthetic_detector
    from two_stage_object_detection_amd.utils import overlay
    z = np.load(os.path.join(golden_dir, "trainer_ref.npz"))
    _, sd = synthetic_detector("hardnet39", conditioned=True)
    tr = FasterRCNNTrainer(mode="train", num_classes=80)
    tr.load_state_dict({("feat_extra." + k[len("extractor."):] if k.startswith("extractor.") else k): v for k, v in sd.items()}, strict=True)
    tr = tr.to(dev).eval()
    x = (torch.from_numpy(z["img_u8"]).float() / 255)[None].to(dev)
    bbox, label = torch.from_numpy(z["bbox"]).to(dev), torch.from_numpy(z["label"]).to(dev)
    frame = torch.randint(0, 256, (1, 120, 150, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).to(dev)
    names = {i: f"c{i}" for i in range(80)}
    annotated, det, keep, n_kept = overlay.multi_inference(tr, x, [bbox], [label], frame, names)
    with torch.inference_mode():
        _, ap, cp, csp = tr(x, [bbox], [label])[:4]
        rec = torch.cat([ap.float(), csp.float().unsqueeze(-1), cp.float().unsqueeze(-1)], dim=-1)
        want_det, want_keep, want_n = hip_ops.filter_detections(rec, iou_thr=0.1)
    assert torch.equal(det, want_det) and torch.equal(keep, want_keep) and torch.equal(n_kept, want_n) and int(n_kept[0]) > 0
    scale = (150 / x.shape[-1], 120 / x.shape[-2])
    want = overlay.draw_detections(frame, det, [bbox], [label], keep=keep, n_kept=n_kept, class_names=names, box_scale=scale,
                                   label_offset=-1)
    assert annotated.shape == frame.shape and not torch.equal(annotated, frame) and torch.equal(annotated, want)
