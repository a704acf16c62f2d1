"""dataset/transform.py -- the evaluation-time input transform on the GPU.

Reference: ``eval_transform = T.Compose([T.Resize((600, 600)), T.ToTensor()])`` (dataset/transform.py:14-17) applied to
``{"image": tv_tensors.Image(PIL image, dtype=float32), "boxes": ..., "labels": ...}`` (dataset/dataloader.py:35-44,
multi_inference.py:65-76).  On a float tensor torchvision's v2 ``Resize`` is ATen's antialiased bilinear interpolation
(``align_corners=False``); ``ToTensor`` passes tensors through, so the detector sees f32 CHW values in 0..255 (the
reference never divides by 255) and XYXY boxes scaled by (600/W, 600/H).

Here the decoded image stays u8 HWC, goes to the GPU as it is (a third of the f32 bytes), and one HIP kernel
(``tsod_resize_bilinear_aa_u8_f32``) produces the resized f32 image directly in the layout asked for: NCHW like the
reference's tensor (``EvalTransform.__call__``), or the NHWC(4) buffer the first conv reads (``EvalTransform.batch``).
``TrainTransform`` ports the reference's training transform (``transform``, dataset/transform.py:4-12):
the random draws are made on the host in torchvision v2's order, and four HIP kernels apply them (contrast's grayscale
mean, colour ops + flip + ScaleJitter's resize fused, the second resize to 600x600, and the box flip / scale / sanitize
for a whole batch).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import hip_ops
from .._ffi import AUG_MEAN_PARTS, NHWC4Images, TsodError


class EvalTransform:
    """``EvalTransform(size)(sample)`` mirrors ``eval_transform(sample)`` for ``sample["image"]`` = u8 [H,W,3] CUDA tensor.

    ``mul`` scales the output (1.0 = the reference: values stay 0..255; 1/255 gives [0,1])."""

    def __init__(self, size=(600, 600), mul: float = 1.0):
        self.size = (int(size[0]), int(size[1]))
        self.mul = float(mul)

    def __call__(self, sample):
        if isinstance(sample, dict):
            img = sample["image"]
            out = dict(sample)
            out["image"] = self.image(img)
            if sample.get("boxes") is not None:
                H, W = img.shape[0], img.shape[1]
                b = torch.as_tensor(sample["boxes"], dtype=torch.float32)
                # v2 Resize on XYXY boxes: x * (new_w / w), y * (new_h / h)
                ratio = torch.tensor([self.size[1] / W, self.size[0] / H, self.size[1] / W, self.size[0] / H],
                                     dtype=torch.float32, device=b.device)
                out["boxes"] = b * ratio
            return out
        return self.image(sample)

    def image(self, img_u8_hwc: torch.Tensor) -> torch.Tensor:
        """u8 [H,W,3] on the GPU -> f32 [3,OH,OW] (the tensor the reference's transform returns)."""
        return hip_ops.resize_bilinear_aa(img_u8_hwc, self.size[0], self.size[1], layout="nchw", mul=self.mul)

    def batch(self, images, out: NHWC4Images | None = None) -> NHWC4Images:
        """A list of u8 [H_i,W_i,3] CUDA images (sizes may differ) -> one ``NHWC4Images`` [B,OH,OW,4] batch, one launch per
        image.  ``out`` = ``model.extractor.input_buffer(B, OH, OW, device, slot)`` writes straight into the backbone's
        input buffer."""
        if len(images) == 0:
            raise TsodError("EvalTransform.batch: empty image list")
        OH, OW = self.size
        dev = images[0].device
        if out is None:
            out = NHWC4Images(torch.empty((len(images), OH, OW, 4), dtype=torch.float32, device=dev))
        if tuple(out.data.shape) != (len(images), OH, OW, 4):
            raise TsodError(f"EvalTransform.batch: out is {tuple(out.data.shape)}, expected {(len(images), OH, OW, 4)}")
        for b, img in enumerate(images):
            hip_ops.resize_bilinear_aa(img, OH, OW, layout="nhwc4", mul=self.mul, out=out.data[b])
        return out


@dataclass(frozen=True)
class AugmentParams:
    """One image's draws: the four RandomPhotometricDistort factors (None = not drawn), whether contrast runs before
    saturation, the channel permutation (None = not drawn), the flip, and ScaleJitter's (new_h, new_w)."""
    brightness: float | None
    contrast: float | None
    saturation: float | None
    hue: float | None
    contrast_before: bool
    perm: tuple | None
    flip: bool
    size: tuple


class TrainTransform:
    """``TrainTransform()(sample)`` mirrors the reference's ``transform(sample)`` for ``sample["image"]`` = u8 [H,W,3]
    CUDA tensor: RandomPhotometricDistort, RandomHorizontalFlip(flip_p), ScaleJitter(size, scale_range), Resize(size),
    SanitizeBoundingBoxes(min_size) (ToTensor and ConvertImageDtype(float32) pass an f32 image through).

    ``photometric_white=1.0`` reproduces the reference, whose 0..255 image is clamped into [0, 1] by every brightness,
    contrast and saturation op (quirk Q18); ``255.0`` runs the colour ops on x/255 and scales the result back.
    Draws use the global torch CPU RNG, or ``generator``."""

    def __init__(self, size=(600, 600), scale_range=(0.8, 1.2), flip_p: float = 0.5, photometric_p: float = 0.5,
                 min_size: float = 1.0, photometric_white: float = 1.0, generator: torch.Generator | None = None):
        self.size = (int(size[0]), int(size[1]))
        self.scale_range = (float(scale_range[0]), float(scale_range[1]))
        self.flip_p = float(flip_p)
        self.photometric_p = float(photometric_p)
        self.min_size = float(min_size)
        self.photometric_white = float(photometric_white)
        self.generator = generator
        # RandomPhotometricDistort's defaults: brightness, contrast, saturation, hue
        self.ranges = ((0.875, 1.125), (0.5, 1.5), (0.5, 1.5), (-0.05, 0.05))

    def make_params(self, H: int, W: int) -> AugmentParams:
        """The draws for one H x W image, in torchvision v2's order (RandomPhotometricDistort, RandomHorizontalFlip,
        ScaleJitter)."""
        g, p = self.generator, self.photometric_p
        factors = []
        for lo, hi in self.ranges:
            factors.append(torch.empty(1).uniform_(lo, hi, generator=g).item() if torch.rand(1, generator=g) < p else None)
        contrast_before = bool(torch.rand((), generator=g) < 0.5)
        perm = tuple(torch.randperm(3, generator=g).tolist()) if torch.rand(1, generator=g) < p else None
        flip = not bool(torch.rand(1, generator=g) >= self.flip_p)
        lo, hi = self.scale_range
        scale = lo + torch.rand(1, generator=g) * (hi - lo)
        r = min(self.size[1] / H, self.size[0] / W) * scale
        new_w, new_h = int(W * r), int(H * r)
        return AugmentParams(*factors, contrast_before=contrast_before, perm=perm, flip=flip, size=(new_h, new_w))

    def photometric(self, params: AugmentParams):
        return hip_ops.photometric(params.brightness, params.contrast, params.saturation, params.hue,
                                   params.contrast_before, params.perm, self.photometric_white)

    def __call__(self, sample, params: AugmentParams | None = None):
        img = sample["image"] if isinstance(sample, dict) else sample
        if not isinstance(sample, dict):
            return self.batch([img], params=None if params is None else [params])[0][0]
        has_boxes = sample.get("boxes") is not None
        boxes = [sample["boxes"]] if has_boxes else None
        labels = [sample["labels"]] if has_boxes and sample.get("labels") is not None else None
        images, b, lab = self.batch([img], boxes, labels, params=None if params is None else [params])
        out = dict(sample)
        out["image"] = images[0]
        if has_boxes:
            out["boxes"] = b[0]
            if labels is not None:
                out["labels"] = lab[0]
        return out

    def batch(self, images, bboxes=None, labels=None, params=None, out: NHWC4Images | None = None):
        """u8 [H_i,W_i,3] CUDA images (sizes may differ) + per-image XYXY boxes [G_i,4] and labels [G_i] (CPU or GPU
        tensors or lists) -> (images, boxes list, labels list).  images: the stacked f32 [B,3,OH,OW] batch, or ``out``
        (an ``NHWC4Images`` [B,OH,OW,4], e.g. ``model.extractor.input_buffer(B, OH, OW, device)``) written in place.
        ``params``: one ``AugmentParams`` per image, else drawn here image by image.  The kept boxes and labels are on the
        device; their counts are read back once per batch."""
        if len(images) == 0:
            raise TsodError("TrainTransform.batch: empty image list")
        B = len(images)
        OH, OW = self.size
        dev = images[0].device
        if params is None:
            params = [self.make_params(int(i.shape[0]), int(i.shape[1])) for i in images]
        if len(params) != B or (bboxes is not None and len(bboxes) != B) or (labels is not None and len(labels) != B):
            raise TsodError("TrainTransform.batch: images, params, boxes and labels must have one entry per image")
        if out is None:
            data, layout = torch.empty((B, 3, OH, OW), dtype=torch.float32, device=dev), "nchw"
        else:
            if tuple(out.data.shape) != (B, OH, OW, 4):
                raise TsodError(f"TrainTransform.batch: out is {tuple(out.data.shape)}, expected {(B, OH, OW, 4)}")
            data, layout = out.data, "nhwc4"
        for b, (img, p) in enumerate(zip(images, params)):
            self._image(img, p, data[b], layout)
        result = out if out is not None else data
        if bboxes is None:
            return result, None, None
        kept_boxes, kept_labels = self._boxes(images, bboxes, labels, params, dev)
        return result, kept_boxes, (kept_labels if labels is not None else None)

    def _image(self, img, p: AugmentParams, out, layout):
        new_h, new_w = p.size
        if new_h < 1 or new_w < 1:
            raise TsodError(f"TrainTransform: ScaleJitter size {p.size} of a {tuple(img.shape[:2])} image is empty")
        photo = self.photometric(p)
        parts = AUG_MEAN_PARTS * 8                                 # f64 partial sums, then the f32 intermediate
        ws = hip_ops.ARENA.get(img.device, parts + 3 * new_h * new_w * 4)
        partials = None
        if p.contrast is not None:
            partials = hip_ops.augment_gray_mean_partials(img, photo, out=ws[:parts].view(torch.float64))
        mid = ws[parts:parts + 3 * new_h * new_w * 4].view(torch.float32).view(3, new_h, new_w)
        hip_ops.augment_resize(img, new_h, new_w, photo, p.flip, partials, layout="nchw", out=mid)
        hip_ops.resize_bilinear_aa_f32(mid, self.size[0], self.size[1], layout=layout, out=out)

    def _boxes(self, images, bboxes, labels, params, dev):
        OH, OW = self.size
        boxes = [torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4) for b in bboxes]
        counts = [int(b.shape[0]) for b in boxes]
        if labels is None:
            labs = [torch.zeros(n, dtype=torch.int64) for n in counts]
        else:
            labs = [torch.as_tensor(l, dtype=torch.int64).reshape(-1) for l in labels]
            if [int(l.shape[0]) for l in labs] != counts:
                raise TsodError("TrainTransform.batch: every image needs one label per box")
        N = sum(counts)
        if N == 0:
            return ([torch.zeros((0, 4), dtype=torch.float32, device=dev) for _ in boxes],
                    [torch.zeros(0, dtype=torch.int64, device=dev) for _ in boxes])
        ip = np.zeros((len(boxes), 4), np.int32)
        fp = np.zeros((len(boxes), 8), np.float32)
        first = 0
        for b, (img, p, n) in enumerate(zip(images, params, counts)):
            H, W = int(img.shape[0]), int(img.shape[1])
            new_h, new_w = p.size
            ip[b] = (first, n, int(p.flip), 0)
            # v2 resize of boxes: x * fl32(new_w / old_w), y * fl32(new_h / old_h), once per resize
            fp[b] = (W, new_w / W, new_h / H, OW / new_w, OH / new_h, OW, OH, self.min_size)
            first += n
        all_boxes = torch.cat([b.to(dev) for b in boxes]).contiguous()
        all_labels = torch.cat([l.to(dev) for l in labs]).contiguous()
        b_out, l_out, kept = hip_ops.augment_boxes(all_boxes, all_labels, torch.from_numpy(ip).to(dev),
                                                   torch.from_numpy(fp).to(dev))
        kept = kept.tolist()                                          # the one read-back of the batch
        starts = ip[:, 0].tolist()
        return ([b_out[s:s + k] for s, k in zip(starts, kept)], [l_out[s:s + k] for s, k in zip(starts, kept)])


eval_transform = EvalTransform((600, 600))      # the reference's instance (dataset/transform.py:14)
transform = TrainTransform()                    # the reference's instance (dataset/transform.py:4-12)
