"""dataset/image_io.py -- reading JPEG files into u8 [H,W,3] device tensors.

Reference: ``Image.open(path).convert("RGB")`` (dataset/dataloader.py:35, multi_inference.py:65).  Here the file's bit-serial
Huffman pass runs on the host, in the library's C code on a thread pool (ctypes releases the GIL), and everything that is
arithmetic over pixels - dequantisation, the inverse DCT, chroma upsampling, YCbCr -> RGB and the crop - runs on the GPU in two
launches for a whole batch, whatever the sizes and samplings of its images.  The pixels are bit-equal to Pillow's
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


def _up(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


class JPEGDecoder:
    """``JPEGDecoder(device).read(path)`` is the reference's ``Image.open(path).convert("RGB")`` as a u8 [H,W,3] tensor on
    ``device``.  ``threads`` host threads share the Huffman pass of a batch (at most 16)."""

    def __init__(self, device="cuda", threads: int = 4):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TsodError(f"JPEGDecoder: {self.device} is not a CUDA/ROCm device; this package is a HIP-only path (there is no "
                            "CPU fallback)")
        self.threads = min(max(int(threads), 1), MAX_THREADS)
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
        One upload and two launches on the current stream, no host wait."""
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
        table, idct_work, rgb_work = plan["table"], plan["idct_work"], plan["rgb_work"]
        # one staging buffer: table | idct work | rgb work | quantisers | coefficients, each part on a 256-byte boundary
        sizes = (ctypes.sizeof(JpegImage) * len(infos), idct_work.nbytes, rgb_work.nbytes, 2 * plan["quant_count"], 2 * plan["coef_count"])
        starts = [0]
        for s in sizes:
            starts.append(starts[-1] + _up(s))
        staging = _staging(starts[-1])
        host = staging.numpy()
        ctypes.memmove(host.ctypes.data + starts[0], table, sizes[0])
        host[starts[1]:starts[1] + sizes[1]] = idct_work.reshape(-1).view(np.uint8)
        host[starts[2]:starts[2] + sizes[2]] = rgb_work.reshape(-1).view(np.uint8)
        quant = host[starts[3]:starts[3] + sizes[3]].view(np.uint16)
        coef = host[starts[4]:starts[4] + sizes[4]].view(np.int16)
        for i, info in enumerate(infos):
            q = np.ctypeslib.as_array(info.quant)[:info.n_comp].reshape(-1)
            quant[table[i].quant_offset:table[i].quant_offset + q.size] = q

        def huffman(i):
            first = table[i].coef_offset[0]
            return hip_ops.jpeg_entropy_decode(files[i][0], coef[first:first + infos[i].coef_total])

        for i, status in enumerate(self._map(huffman, range(len(files)))):
            if status:
                _raise(status, i, files[i][1], "entropy-coded data")
        dev = _upload(staging, self.device)
        part = [dev[starts[k]:starts[k] + sizes[k]] for k in range(5)]
        planes = _empty(plan["plane_bytes"], self.device)
        out = _empty(plan["out_bytes"], self.device)
        hip_ops.jpeg_idct(table, part[0], idct_work, part[1], part[4].view(torch.int16), part[3].view(torch.int16), planes)
        hip_ops.jpeg_to_rgb(table, part[0], rgb_work, part[2], planes, out)
        return [out[table[i].out_offset:table[i].out_offset + 3 * info.H * info.W].view(info.H, info.W, 3)
                for i, info in enumerate(infos)]

    def decode(self, data) -> torch.Tensor:
        """One file's bytes -> u8 [H,W,3] on the device."""
        return self.batch([data])[0]

    def read(self, path) -> torch.Tensor:
        """The file at ``path`` -> u8 [H,W,3] on the device: ``Image.open(path).convert("RGB")``."""
        return self.batch([os.fspath(path)])[0]


_DECODERS = {}


def _decoder(device) -> JPEGDecoder:
    device = torch.device(device)
    if device not in _DECODERS:
        _DECODERS[device] = JPEGDecoder(device)
    return _DECODERS[device]


def decode_jpeg(data, device="cuda") -> torch.Tensor:
    """``JPEGDecoder(device).decode(data)`` on a decoder kept per device."""
    return _decoder(device).decode(data)


def read_image(path, device="cuda") -> torch.Tensor:
    """``JPEGDecoder(device).read(path)`` on a decoder kept per device."""
    return _decoder(device).read(path)
