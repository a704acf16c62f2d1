"""dataset/image_io.py -- reading JPEG files into u8 [H,W,3] device tensors.

Reference: ``Image.open(path).convert("RGB")`` (dataset/dataloader.py:35, multi_inference.py:65).  Here the file's bit-serial
Huffman pass runs on the host, in the library's C code on a thread pool (ctypes releases the GIL), and everything that is
arithmetic over pixels - dequantisation, the inverse DCT, chroma upsampling, YCbCr -> RGB and the crop - runs on the GPU in two
launches for a whole batch, whatever the sizes and samplings of its images.  With ``entropy="device"`` the Huffman pass runs on
the GPU too: the host only unstuffs the entropy-coded bytes and checks the restart markers, the upload is the files' own bytes
instead of 6 bytes of coefficients per pixel, and one more launch (after a fill launch) decodes every restart interval of the
batch; ``split=`` cuts a long interval - a whole file without restart markers - into chunks for one workgroup each, joined
exactly, in three launches instead of that one.  Damage inside the entropy-coded data is then found on the device: ``batch``
returns without a host wait, the image's
pixels are unspecified (inside its own view), ``decoder.status`` is nonzero for it and ``decoder.raise_if_corrupt()`` raises.  The pixels are bit-equal to Pillow's
(libjpeg-turbo) for every file this decodes: 8-bit baseline or extended-sequential Huffman files, grey or YCbCr with 4:4:4,
4:2:2 or 4:2:0 sampling.  Anything else raises ``UnsupportedJPEG``, a damaged file ``CorruptJPEG``, both before anything is
uploaded or launched; there is no CPU fallback - the caller decides what to do with a progressive file.

The tensors feed ``EvalTransform`` / ``TrainTransform`` (``image`` and ``batch``) and ``utils.overlay.draw_detections`` unchanged.
"""
from __future__ import annotations

import ctypes
import os
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

import numpy as np
import torch

from .. import hip_ops
from .._ffi import JpegImage, TsodError

MAX_THREADS = 16                 # the CPUs a job gets; never derived from os.cpu_count()
ALIGN = 256                      # every image of a batch starts on this boundary of the one output allocation


class UnsupportedJPEG(TsodError):
    """A valid file of a kind that is not built: progressive, lossless, arithmetic-coded, 12-bit, CMYK, RGB-coded, multi-scan,
    or a sampling other than 4:4:4 / 4:2:2 / 4:2:0."""


class CorruptJPEG(TsodError):
    """Not a JPEG file, or one that is cut short or damaged."""


class JPEGInfo(NamedTuple):
    height: int
    width: int
    components: int              # 1 (grey) or 3 (YCbCr)
    sampling: tuple              # the luma sampling (h, v): (1, 1) 4:4:4, (2, 1) 4:2:2, (2, 2) 4:2:0
    restart_interval: int


def _raise(status: int, index: int, name: str, stage: str):
    where = f"item {index}" + (f" ({name})" if name else "")
    if status == -2:
        raise UnsupportedJPEG(f"{where}: a JPEG this decoder is not built for (progressive, lossless, arithmetic, 12-bit, CMYK / "
                              "RGB-coded, multi-scan or a sampling other than 4:4:4 / 4:2:2 / 4:2:0); there is no CPU fallback")
    raise CorruptJPEG(f"{where}: not a JPEG file or a damaged one ({stage})")


def _load(item):
    """(u8 ndarray, name) of one item: the bytes themselves, or the file a path names."""
    if isinstance(item, (str, os.PathLike)):
        with open(item, "rb") as f:
            return hip_ops.jpeg_bytes(f.read()), os.fspath(item)
    return hip_ops.jpeg_bytes(item), ""


def jpeg_info(data) -> JPEGInfo:
    """What the markers of a JPEG file (bytes or a path) say, on the host."""
    raw, name = _load(data)
    status, info = hip_ops.jpeg_parse(raw)
    if status:
        _raise(status, 0, name, "markers")
    return JPEGInfo(info.H, info.W, info.n_comp, (info.hmax, info.vmax), info.restart_interval)


def _staging(nbytes: int) -> torch.Tensor:
    """The pinned host buffer one batch goes up in."""
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)


def _upload(staging: torch.Tensor, device) -> torch.Tensor:
    return staging.to(device, non_blocking=True)


def _empty(nbytes: int, device) -> torch.Tensor:
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _stage(infos, plan, more):
    """ONE staging buffer of byte parts, each on a 256-byte boundary.  The first four - table | idct work | rgb work | quantisers -
    are what both modes send, and are filled here; one part of every size in ``more`` follows.  Returns ``(host, upload)``:
    ``host`` holds those further parts as u8 ndarray views for the caller to fill, and ``upload(device)`` is the one copy,
    returning the four shared parts and the further ones as device tensors."""
    table, idct_work, rgb_work = plan["table"], plan["idct_work"], plan["rgb_work"]
    sizes = (ctypes.sizeof(JpegImage) * len(infos), idct_work.nbytes, rgb_work.nbytes, 2 * plan["quant_count"]) + tuple(more)
    starts = [0]
    for n in sizes:
        starts.append(starts[-1] + (n + ALIGN - 1) // ALIGN * ALIGN)
    spans = [slice(first, first + n) for first, n in zip(starts, sizes)]
    staging = _staging(starts[-1])
    host = [staging.numpy()[span] for span in spans]
    ctypes.memmove(host[0].ctypes.data, table, sizes[0])
    host[1][:] = idct_work.reshape(-1).view(np.uint8)
    host[2][:] = rgb_work.reshape(-1).view(np.uint8)
    quant = host[3].view(np.uint16)
    for i, info in enumerate(infos):
        q = np.ctypeslib.as_array(info.quant)[:info.n_comp].reshape(-1)
        quant[table[i].quant_offset:table[i].quant_offset + q.size] = q

    def upload(device):
        dev = _upload(staging, device)
        parts = [dev[span] for span in spans]
        return parts[:4], parts[4:]

    return host[4:], upload


def _pixels(infos, plan, shared, coef) -> list:
    """``jpeg_idct`` and ``jpeg_to_rgb`` of an uploaded batch (``shared``: the first four parts of ``_stage``) from its
    coefficients: u8 [H_i,W_i,3] views, each starting on a 256-byte boundary, of one allocation."""
    table, (table_dev, idct_dev, rgb_dev, quant_dev) = plan["table"], shared
    planes = _empty(plan["plane_bytes"], coef.device)
    out = _empty(plan["out_bytes"], coef.device)
    hip_ops.jpeg_idct(table, table_dev, plan["idct_work"], idct_dev, coef, quant_dev.view(torch.int16), planes)
    hip_ops.jpeg_to_rgb(table, table_dev, plan["rgb_work"], rgb_dev, planes, out)
    return [out[table[i].out_offset:table[i].out_offset + 3 * info.H * info.W].view(info.H, info.W, 3) for i, info in enumerate(infos)]


def _split_arg(split, entropy):
    """``split`` as ``JPEGDecoder`` keeps it: ``None`` or a checked ``(chunk_subseqs, overlap)`` of ints."""
    if split is True:
        split = JPEGDecoder.SPLIT_DEFAULT
    if split is None:
        return None
    if entropy != "device":
        raise ValueError("JPEGDecoder: split belongs to entropy='device'")
    try:
        chunk, overlap = split
        ok = int(chunk) == chunk and int(overlap) == overlap and 1 <= chunk <= hip_ops.JPEG_SPLIT_MAX and \
            0 <= overlap <= hip_ops.JPEG_SPLIT_MAX - chunk
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"JPEGDecoder: split is None, True or (chunk_subseqs in [1, 256], overlap in [0, 256 - chunk_subseqs]), "
                         f"not {split!r}")
    return int(chunk), int(overlap)


class JPEGDecoder:
    """``JPEGDecoder(device).read(path)`` is the reference's ``Image.open(path).convert("RGB")`` as a u8 [H,W,3] tensor on
    ``device``.  ``threads`` host threads share the host pass of a batch (at most 16).  ``entropy``: ``"host"`` (the Huffman
    pass on those threads) or ``"device"`` (on the GPU, in subsequences of ``subseq_bits`` bits: a multiple of 32 in [32, 2048]).
    ``split`` (``entropy="device"`` only): ``None`` - one workgroup per restart interval - or ``(chunk_subseqs, overlap)``, which
    gives every ``chunk_subseqs`` consecutive subsequences of an interval to a workgroup of their own that warms up over the
    ``overlap`` subsequences before them (``chunk_subseqs`` in [1, 256], ``overlap`` in [0, 256 - ``chunk_subseqs``]); ``True`` is
    ``(224, 32)``.  The pixels and ``status`` do not depend on it.

    ``status`` is the int32 [B] device tensor of the last ``entropy="device"`` batch: nonzero where an image's entropy-coded
    data are damaged (``None`` after an ``entropy="host"`` batch, which raises ``CorruptJPEG`` itself).  ``repaired`` is the
    int32 [n_segments] device tensor of the last ``split`` batch: the chunks of every restart interval whose assumed entry was
    wrong and that were decoded again from the true one (``None`` otherwise)."""

    SPLIT_DEFAULT = (224, 32)

    def __init__(self, device="cuda", threads: int = 4, entropy: str = "host", subseq_bits: int = 1024, split=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TsodError(f"JPEGDecoder: {self.device} is not a CUDA/ROCm device; this package is a HIP-only path (there is no "
                            "CPU fallback)")
        if entropy not in ("host", "device"):
            raise ValueError(f"JPEGDecoder: entropy is 'host' or 'device', not {entropy!r}")
        if int(subseq_bits) != subseq_bits or subseq_bits % 32 or not 32 <= subseq_bits <= 2048:
            raise ValueError(f"JPEGDecoder: subseq_bits is a multiple of 32 in [32, 2048], not {subseq_bits!r}")
        self.threads = min(max(int(threads), 1), MAX_THREADS)
        self.entropy = entropy
        self.subseq_bits = int(subseq_bits)
        self.split = _split_arg(split, entropy)
        self.status = None
        self.repaired = None
        self._names = []
        self._pool = None

    def _map(self, fn, jobs):
        if self.threads == 1 or len(jobs) == 1:
            return [fn(j) for j in jobs]
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.threads, thread_name_prefix="tsod-jpeg")
        return list(self._pool.map(fn, jobs))

    def close(self) -> None:
        """Stop the pool's threads (they are started by the first batch of more than one file)."""
        if self._pool is not None:
            self._pool.shutdown()
            self._pool = None

    def batch(self, items) -> list:
        """Decode ``items`` (each ``bytes`` / ``bytearray`` / ``memoryview`` / a u8 ndarray holding a file, or a path) into a
        list of u8 [H_i,W_i,3] tensors: contiguous views, each starting on a 256-byte boundary, of ONE device allocation.
        One upload and two launches on the current stream (``entropy="device"``: a fill and three launches, with ``split`` a
        fill and five), no host wait."""
        items = list(items)
        if not items:
            return []
        files = [_load(it) for it in items]
        infos = []
        for i, (raw, name) in enumerate(files):
            status, info = hip_ops.jpeg_parse(raw)
            if status:
                _raise(status, i, name, "markers")
            infos.append(info)
        plan = hip_ops.jpeg_plan(infos)
        if self.entropy == "device":
            return self._batch_device(files, infos, plan)
        self.status, self.repaired, self._names = None, None, []
        table = plan["table"]
        (coef,), upload = _stage(infos, plan, (2 * plan["coef_count"],))
        coef = coef.view(np.int16)

        def huffman(i):
            first = table[i].coef_offset[0]
            return hip_ops.jpeg_entropy_decode(files[i][0], coef[first:first + infos[i].coef_total])

        for i, status in enumerate(self._map(huffman, range(len(files)))):
            if status:
                _raise(status, i, files[i][1], "entropy-coded data")
        shared, (coef_dev,) = upload(self.device)
        return _pixels(infos, plan, shared, coef_dev.view(torch.int16))

    def _batch_device(self, files, infos, plan) -> list:
        """``batch`` with the Huffman pass on the device."""
        table = plan["table"]
        n = len(infos)
        caps = [hip_ops.jpeg_scan_sizes(info, files[i][0].size) for i, info in enumerate(infos)]
        seg_first = np.concatenate([[0], np.cumsum([c[1] for c in caps])]).astype(np.int64)
        stream_first = np.concatenate([[0], np.cumsum([c[0] for c in caps])]).astype(np.int64)      # (each a multiple of 4)
        seg_dtype = hip_ops.jpeg_segment_dtype()
        n_seg = int(seg_first[-1])
        words = self.subseq_bits // 32
        n_work = n_seg
        if self.split:
            # the bit lengths come with the sweep: room for the most chunks these streams can hold (a segment of n subsequences
            # has at most 1 + n / chunk_subseqs chunks, and n is at most 1 + bits / subseq_bits)
            n_work = n_seg + (int(stream_first[-1]) * 8 // self.subseq_bits + n_seg) // self.split[0]
        # after the shared parts: code tables | segment records | Huffman work | streams
        (huff, segments, work, stream), upload = _stage(infos, plan, (hip_ops.JPEG_HUFF_BYTES * n, seg_dtype.itemsize * n_seg, 16 * n_work,
                                                                      int(stream_first[-1])))
        segments, work = segments.view(seg_dtype), work.view(np.int32).reshape(-1, 4)

        def sweep(i):
            segs = segments[seg_first[i]:seg_first[i + 1]]
            status, _, count = hip_ops.jpeg_scan_prepare(files[i][0], stream[stream_first[i]:stream_first[i + 1]], segs,
                                                         huff[hip_ops.JPEG_HUFF_BYTES * i:hip_ops.JPEG_HUFF_BYTES * (i + 1)])
            if status == 0 and count != segs.size:               # (a file that parses holds every interval or is refused)
                status = -1
            segs["image"] = i
            segs["stream_offset"] += stream_first[i]
            return status

        for i, status in enumerate(self._map(sweep, range(n))):
            if status:
                _raise(status, i, files[i][1], "restart markers")
        work[:] = 0
        if self.split:
            chunks, n_subseqs = hip_ops.jpeg_split_chunks(segments, words, self.split[0])
            work[:len(chunks)] = chunks
            work = work[:len(chunks)]
        else:
            work[:, 0] = np.arange(n_seg, dtype=np.int32)
        shared, (huff_dev, segments_dev, work_dev, stream_dev) = upload(self.device)
        coef = _empty(2 * plan["coef_count"], self.device).view(torch.int16)
        self.status = _empty(4 * n, self.device).view(torch.int32)
        self._names = [name for _, name in files]
        self.repaired = None
        if self.split:
            workspace = _empty(hip_ops.jpeg_huffman_split_workspace_bytes(n_subseqs, len(work), n_seg), self.device)
            self.repaired = _empty(4 * n_seg, self.device).view(torch.int32)
            hip_ops.jpeg_huffman_split(table, shared[0], segments, segments_dev, work, work_dev[:work.nbytes], stream_dev, huff_dev,
                                       coef, self.status, words, self.split[0], self.split[1], workspace, self.repaired)
        else:
            hip_ops.jpeg_huffman(table, shared[0], segments, segments_dev, work, work_dev, stream_dev, huff_dev, coef, self.status,
                                 words)
        return _pixels(infos, plan, shared, coef)

    def raise_if_corrupt(self) -> None:
        """The one host read of ``status``: raises ``CorruptJPEG`` naming the first image of the last ``entropy="device"``
        batch whose entropy-coded data the device found damaged.  Nothing to do after an ``entropy="host"`` batch."""
        if self.status is None:
            return
        bad = torch.nonzero(self.status.cpu()).reshape(-1)
        if bad.numel():
            i = int(bad[0])
            _raise(-1, i, self._names[i] if i < len(self._names) else "", "entropy-coded data, found on the device")

    def decode(self, data) -> torch.Tensor:
        """One file's bytes -> u8 [H,W,3] on the device."""
        return self.batch([data])[0]

    def read(self, path) -> torch.Tensor:
        """The file at ``path`` -> u8 [H,W,3] on the device: ``Image.open(path).convert("RGB")``."""
        return self.batch([os.fspath(path)])[0]


_DECODERS = {}


def _decoder(device, entropy="host", split=None) -> JPEGDecoder:
    key = (torch.device(device), entropy, _split_arg(split, entropy))
    if key not in _DECODERS:
        _DECODERS[key] = JPEGDecoder(key[0], entropy=entropy, split=key[2])
    return _DECODERS[key]


def decode_jpeg(data, device="cuda", entropy="host", split=None) -> torch.Tensor:
    """``JPEGDecoder(device, entropy=entropy, split=split).decode(data)`` on a decoder kept per device and mode."""
    return _decoder(device, entropy, split).decode(data)


def read_image(path, device="cuda", entropy="host", split=None) -> torch.Tensor:
    """``JPEGDecoder(device, entropy=entropy, split=split).read(path)`` on a decoder kept per device and mode."""
    return _decoder(device, entropy, split).read(path)
