"""ctypes binding of include/tsod.h (libtsod.so, HIP, gfx950).

This is the only way the package reaches compute: there is no CPU or PyTorch-eager fallback.
If the shared library is missing the import of any compute entry point raises immediately.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_uint16, c_uint32, c_uint64,
                    c_void_p)
from typing import NamedTuple

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TSOD_LIB") or os.path.join(_PKG_DIR, "libtsod.so")   # TSOD_LIB: alternate build (experiments)

TSOD_MAX_SEGMENTS = 16
AMAX_WORDS, AMAX_STRIDE = 64, 64                 # range words of one tensor (include/tsod.h): 64 uint32, 64 bytes apart
AMAX_BYTES = AMAX_WORDS * AMAX_STRIDE
ACT_NONE, ACT_PRELU, ACT_RELU6, ACT_RELU = 0, 1, 2, 3
PREC_F32, PREC_BF16X3, PREC_FP16X2 = 0, 1, 2
PREC_NAMES = {0: "f32", 1: "bf16x3", 2: "fp16x2"}
TILE_AUTO, TILE_128x128, TILE_128x64, TILE_64x64, TILE_64x128 = 0, 1, 2, 3, 4


class Tile(NamedTuple):
    name: str
    rows: int                  # output pixels (GEMM rows) per workgroup tile
    precisions: tuple          # the PREC_* it is built in
    dma: bool = False          # fed by LDS-DMA (conv_dma_kernel): the shape limits of include/tsod.h


# The TSOD_TILE_* of include/tsod.h, mirroring the library's tile table (tests/test_abi_errors.py checks it against the resolver)
_F32, _BF16X3, _FP16X2 = (PREC_F32,), (PREC_BF16X3,), (PREC_FP16X2,)
_ALL, _SPLIT = (PREC_F32, PREC_BF16X3, PREC_FP16X2), (PREC_BF16X3, PREC_FP16X2)
TILES = {
     1: Tile("128x128",        128, _F32),
     2: Tile("128x64",         128, _F32),
     3: Tile("64x64",          64,  _ALL),
     4: Tile("64x128",         64,  _F32),
     5: Tile("128x128w8",      128, _F32),
     6: Tile("128x64w8",       128, _F32),
     7: Tile("256x128w8",      256, _F32),
     8: Tile("64x64s1",        64,  _ALL),
     9: Tile("128x64w8s1",     128, _ALL),
    10: Tile("64x64s1k64",     64,  _ALL),
    11: Tile("128x64w8s1k64",  128, _F32),
    12: Tile("64x64w1s1",      64,  _F32),
    13: Tile("128x64w2s1",     128, _F32),
    14: Tile("128x64s1",       128, _ALL),
    15: Tile("64x128s1",       64,  _ALL),
    16: Tile("128x128s1",      128, _ALL),
    17: Tile("d128x128",       128, _SPLIT, dma=True),
    18: Tile("d64x128",        64,  _BF16X3, dma=True),
    19: Tile("d256x128",       256, _SPLIT, dma=True),
    20: Tile("d64x128s2",      64,  _BF16X3, dma=True),
    21: Tile("d128x256",       128, _SPLIT, dma=True),
    22: Tile("d128x128k32",    128, _SPLIT, dma=True),
    23: Tile("d192x128",       192, _FP16X2, dma=True),
    24: Tile("d64x128k64",     64,  _FP16X2, dma=True),
}


def tile_ids(precision: int) -> tuple:
    """The tiles built in arithmetic ``precision``, in id order (the autotuners' candidate order)."""
    return tuple(t for t, row in TILES.items() if precision in row.precisions)


TILE_NAMES = {TILE_AUTO: "auto", **{t: row.name for t, row in TILES.items()}}
TILE_IDS = tile_ids(PREC_F32)
DMA_TILE_IDS = tuple(t for t, row in TILES.items() if row.dma)
BF16X3_TILE_IDS = tile_ids(PREC_BF16X3)
FP16X2_TILE_IDS = tile_ids(PREC_FP16X2)

class TsodError(RuntimeError):
    pass


class ConvDesc(Structure):
    """Mirror of ``tsod_conv2d_desc`` (include/tsod.h)."""
    _fields_ = [
        ("N", c_int32), ("H", c_int32), ("W", c_int32),
        ("in_pitch", c_int32), ("n_seg", c_int32),
        ("seg_off", c_int32 * TSOD_MAX_SEGMENTS), ("seg_len", c_int32 * TSOD_MAX_SEGMENTS),
        ("Cout", c_int32), ("out_pitch", c_int32), ("out_off", c_int32),
        ("KH", c_int32), ("KW", c_int32), ("stride", c_int32), ("pad_h", c_int32), ("pad_w", c_int32),
        ("OH", c_int32), ("OW", c_int32), ("act", c_int32), ("slope", c_float),
        ("res_pitch", c_int32), ("res_off", c_int32), ("tile", c_int32), ("split_k", c_int32), ("precision", c_int32),
        ("c2", c_int32), ("in2_pitch", c_int32), ("in2_off", c_int32), ("stride2", c_int32), ("H2", c_int32), ("W2", c_int32),
        ("a_scale_exp", c_int32), ("w_scale_exp", c_int32), ("range_flag", c_void_p),
        ("amax_in", c_void_p), ("amax_in2", c_void_p), ("amax_out", c_void_p),
    ]


class BottleneckDesc(Structure):
    """Mirror of ``tsod_bottleneck_desc`` (include/tsod.h)."""
    _fields_ = [
        ("N", c_int32), ("H", c_int32), ("W", c_int32), ("Cin", c_int32), ("in_pitch", c_int32), ("Cmid", c_int32),
        ("Cout", c_int32), ("out_pitch", c_int32), ("slope", c_float), ("w_exp", c_int32 * 3), ("a_scale_exp", c_int32),
        ("projection", c_int32), ("range_flag", c_void_p), ("amax_in", c_void_p), ("amax_out", c_void_p),
    ]


class StemDesc(Structure):
    """Mirror of ``tsod_stem_desc`` (include/tsod.h)."""
    _fields_ = [
        ("N", c_int32), ("H", c_int32), ("W", c_int32), ("in_layout", c_int32), ("out_pitch", c_int32), ("slope", c_float),
        ("w_exp", c_int32), ("range_flag", c_void_p), ("amax_out", c_void_p),
    ]


STEM_NCHW, STEM_NHWC4 = 0, 1

AUG_MEAN_PARTS = 256             # TSOD_AUGMENT_MEAN_PARTS
AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE, AUG_CONTRAST_FIRST, AUG_PERMUTE = 1, 2, 4, 8, 16, 32


class Photometric(Structure):
    """Mirror of ``tsod_photometric`` (include/tsod.h)."""
    _fields_ = [("flags", c_int32), ("brightness", c_float), ("contrast", c_float), ("saturation", c_float),
                ("hue", c_float), ("white", c_float), ("perm", c_int32 * 3)]


PW_MAX_SEGMENTS = 16             # TSOD_PW_MAX_SEGMENTS


class PwSegs(Structure):
    """Mirror of ``tsod_pw_segs`` (include/tsod.h): the channel segments a 1x1 ConvLayer gathers its K from."""
    _fields_ = [("n_seg", c_int32), ("off", c_int32 * PW_MAX_SEGMENTS), ("len", c_int32 * PW_MAX_SEGMENTS),
                ("real", c_int32 * PW_MAX_SEGMENTS), ("want", c_int32 * PW_MAX_SEGMENTS)]


ADAMW_CHUNK, ADAMW_MAX_GROUPS = 2048, 32         # TSOD_ADAMW_CHUNK, TSOD_ADAMW_MAX_GROUPS
BN_ROWS_PER_WORKGROUP = 128                      # TSOD_BN_ROWS_PER_WORKGROUP: the rows one workgroup of bn_train.hip reduces
DROPOUT_MAX_SEGMENTS = 16                        # TSOD_DROPOUT_MAX_SEGMENTS


class DropoutSeg(Structure):
    """Mirror of ``tsod_dropout_seg`` (include/tsod.h): a slice's channel offset in the pixel, real width, first logical channel."""
    _fields_ = [("off", c_int32), ("real", c_int32), ("first", c_int32)]


DRAW_MAX_GROUPS, DRAW_LIST_CAPACITY, DRAW_STRING_BYTES, DRAW_MAX_STYLE = 4, 64, 32, 32767   # TSOD_DRAW_*
DRAW_TAG_NONE, DRAW_TAG_ABOVE, DRAW_TAG_BELOW = 0, 1, 2


class DrawGroup(Structure):
    """Mirror of ``tsod_draw_group`` (include/tsod.h): one style over one box array of the overlay."""
    _fields_ = [("boxes", c_void_p), ("counts", c_void_p), ("keep", c_void_p), ("n_kept", c_void_p), ("labels", c_void_p),
                ("R", c_int32), ("pitch", c_int32), ("label_offset", c_int32), ("string_first", c_int32),
                ("string_count", c_int32), ("sx", c_float), ("sy", c_float),
                ("color", c_uint8 * 4), ("thickness", c_int32), ("tag", c_int32), ("text_rgb", c_uint8 * 4),
                ("tag_bg", c_uint8 * 4), ("font_scale", c_int32), ("padding", c_int32), ("score_line", c_int32)]


PLOT_MAX_SERIES, PLOT_MAX_WIDTH, PLOT_MAX_HEIGHT, PLOT_BLOCK_COLUMNS = 4, 15, 4096, 32        # TSOD_PLOT_*
PLOT_STRING_BYTES, PLOT_LIMITS_WORKSPACE_BYTES = 32, 2048
PLOT_MARKER_NONE, PLOT_MARKER_CIRCLE, PLOT_MARKER_SQUARE, PLOT_MARKER_TRIANGLE = 0, 1, 2, 3
PLOT_ITEM_RECT, PLOT_ITEM_TEXT, PLOT_ITEM_NUMBER = 0, 1, 2


class PlotSeries(Structure):
    """Mirror of ``tsod_plot_series`` (include/tsod.h): one curve of a plot rectangle."""
    _fields_ = [("y", c_void_p), ("n", c_int32), ("x_first", c_int32), ("x_step", c_int32), ("color", c_uint8 * 4),
                ("width", c_int32), ("marker", c_int32), ("marker_size", c_int32)]


class PlotItem(Structure):
    """Mirror of ``tsod_plot_item`` (include/tsod.h): one decoration - a rectangle, a string or a device-formatted number."""
    _fields_ = [("limits", c_void_p), ("kind", c_int32), ("x", c_int32), ("y", c_int32), ("w", c_int32), ("h", c_int32),
                ("dash_period", c_int32), ("dash_on", c_int32), ("scale", c_int32), ("align", c_int32), ("len", c_int32),
                ("tick", c_int32), ("ticks", c_int32), ("color", c_uint8 * 4), ("text", c_uint8 * 32)]


JPEG_IDCT_BLOCKS, JPEG_RGB_TILE_W, JPEG_RGB_TILE_H = 32, 256, 4                              # TSOD_JPEG_*


class JpegInfo(Structure):
    """Mirror of ``tsod_jpeg_info`` (include/tsod.h): what the markers of one JPEG file say, and the sizes that follow."""
    _fields_ = [("H", c_int32), ("W", c_int32), ("n_comp", c_int32), ("hmax", c_int32), ("vmax", c_int32), ("mcus_x", c_int32),
                ("mcus_y", c_int32), ("restart_interval", c_int32), ("h", c_int32 * 3), ("v", c_int32 * 3), ("tq", c_int32 * 3),
                ("blocks_w", c_int32 * 3), ("blocks_h", c_int32 * 3), ("plane_w", c_int32 * 3), ("plane_h", c_int32 * 3),
                ("reserved", c_int32), ("coef_count", c_int64 * 3), ("coef_total", c_int64), ("quant", (c_uint16 * 64) * 3)]


class JpegImage(Structure):
    """Mirror of ``tsod_jpeg_image`` (include/tsod.h): one image of a batch, as the two JPEG kernels see it."""
    _fields_ = [("coef_offset", c_int64 * 3), ("plane_offset", c_int64 * 3), ("quant_offset", c_int64), ("out_offset", c_int64),
                ("H", c_int32), ("W", c_int32), ("n_comp", c_int32), ("hs", c_int32), ("vs", c_int32),
                ("blocks_w", c_int32 * 3), ("blocks_h", c_int32 * 3), ("reserved", c_int32)]


JPEG_HUFF_TABLES, JPEG_MAX_SEGMENT_BITS = 6, 0x7FF00000                                      # TSOD_JPEG_*
JPEG_STATUS_ERROR, JPEG_STATUS_BLOCKS, JPEG_STATUS_LEFTOVER = 1, 2, 4


class JpegHuff(Structure):
    """Mirror of ``tsod_jpeg_huff`` (include/tsod.h): one Huffman code table in the fixed layout the device pass reads."""
    _fields_ = [("look", c_uint16 * 512), ("maxcode", c_int32 * 17), ("valoff", c_int32 * 17), ("vals", c_uint8 * 256)]


class JpegSegment(Structure):
    """Mirror of ``tsod_jpeg_segment`` (include/tsod.h): one restart interval of one image's unstuffed stream."""
    _fields_ = [("stream_offset", c_int64), ("bit_length", c_int64), ("image", c_int32), ("first_mcu", c_int32),
                ("n_mcu", c_int32), ("flags", c_int32)]


class AdamWGroup(Structure):
    """Mirror of ``tsod_adamw_group`` (include/tsod.h): the f32 scalars of one AdamW step."""
    _fields_ = [("decay", c_float), ("one_minus_beta1", c_float), ("beta2", c_float), ("one_minus_beta2", c_float),
                ("step_size", c_float), ("bias2_sqrt", c_float), ("eps", c_float), ("reserved", c_float)]


class GradNormResult(Structure):
    """Mirror of ``tsod_grad_norm_result`` (include/tsod.h): the f64 sum of squares, the norm and the clip coefficient."""
    _fields_ = [("sum_sq", c_double), ("norm", c_float), ("coef", c_float)]


# name -> (restype, argtypes); every symbol include/tsod.h declares
_SIGNATURES = {
    "tsod_status_str": (c_char_p, [c_int]),
    "tsod_version": (c_int, []),
    "tsod_device_cu_count": (c_int, []),
    "tsod_pack_conv_weight_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_conv_weight_bf16x3_bytes": (c_size_t, [c_int32, c_int32]),
    "tsod_pack_conv_weight_bf16x3": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_conv_weight_fp16x2_bytes": (c_size_t, [c_int32, c_int32]),
    "tsod_pack_conv_weight_fp16x2": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_conv2d_workspace_bytes": (c_size_t, [POINTER(ConvDesc)]),
    "tsod_conv2d_resolve": (c_int, [POINTER(ConvDesc), POINTER(c_int32), POINTER(c_int32)]),
    "tsod_conv2d_f32": (c_int, [POINTER(ConvDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_size_t, c_void_p]),
    "tsod_conv2d_dual_f32": (c_int, [POINTER(ConvDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_size_t, c_void_p]),
    "tsod_bottleneck_wstream_bytes": (c_size_t, [c_int32, c_int32]),
    "tsod_bottleneck_proj_wstream_bytes": (c_size_t, [c_int32, c_int32]),
    "tsod_bottleneck_fp16x2": (c_int, [POINTER(BottleneckDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tsod_stem_wfrag_bytes": (c_size_t, []),
    "tsod_stem_fp16x2": (c_int, [POINTER(StemDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tsod_linear_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32,
                                c_void_p, c_size_t, c_void_p]),
    "tsod_linear_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "tsod_maxpool3x3s2_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "tsod_dwconv3x3_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                   c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p]),
    "tsod_dwconv3x3_amax_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                        c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_gconv3x3_amax_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                       c_int32, c_int32, c_float, c_void_p, c_int32, c_void_p, c_void_p]),
    "tsod_gconv1x1_pair_amax_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "tsod_nchw_to_nhwc_amax_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_absmax_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "tsod_amax_reset": (c_int, [c_void_p, c_int32, c_void_p]),
    "tsod_host_mapped_pointer": (c_int, [c_void_p, c_void_p]),
    "tsod_word_publish_i32": (c_int, [c_void_p, c_void_p, c_void_p]),
    "tsod_gconv3x3_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                  c_int32, c_int32, c_float, c_void_p, c_int32, c_void_p]),
    "tsod_gconv1x1_pair_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "tsod_nchw_to_nhwc_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p]),
    "tsod_nhwc_to_nchw_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_rpn_decode_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                    c_int32, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tsod_proposal_decode_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_void_p,
                                         c_void_p, c_void_p]),
    "tsod_enumerate_anchors_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_loc2bbox_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "tsod_bbox2loc_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "tsod_sort_topk_desc_f32": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p]),
    "tsod_sort_topk_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "tsod_sort_topk_desc_ws_f32": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_nms_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "tsod_nms_f32": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_float, c_int32, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_bbox_iou_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_float, c_void_p, c_void_p]),
    "tsod_roi_pool_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_float,
                                  c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_roi_pool_avg_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                      c_float, c_float, c_float, c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "tsod_roi_align_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_float,
                                   c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_roi_align_avg_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                       c_float, c_float, c_float, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                       c_void_p]),
    "tsod_detections_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_resize_aa_taps": (c_int32, [c_int32, c_int32]),
    "tsod_resize_aa_tables_f32": (c_int, [c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "tsod_resize_bilinear_aa_u8_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p, c_int64,
                                               c_int64, c_int64, c_int32, c_void_p]),
    "tsod_augment_gray_mean_partials": (c_int, [c_void_p, c_int32, c_int32, c_int64, POINTER(Photometric), c_void_p,
                                                c_void_p]),
    "tsod_augment_resize_u8_f32": (c_int, [c_void_p, c_int32, c_int32, c_int64, POINTER(Photometric), c_void_p, c_int32,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                                           c_int64, c_int64, c_int64, c_int32, c_void_p]),
    "tsod_resize_bilinear_aa_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, c_int64, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                                            c_int64, c_int64, c_int64, c_int32, c_void_p]),
    "tsod_augment_boxes_f32": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "tsod_augment_color_host": (c_int, [c_void_p, c_int64, POINTER(Photometric), c_float, c_void_p]),
    "tsod_adamw_step_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p]),
    "tsod_adamw_step_host_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, POINTER(AdamWGroup), c_int32]),
    "tsod_grad_norm_workspace_bytes": (c_size_t, [c_int64]),
    "tsod_grad_norm_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int64, c_float, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_adamw_step_clipped_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p,
                                            c_void_p]),
    "tsod_grad_scale_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p]),
    "tsod_grad_norm_host_f32": (c_int, [c_void_p, c_void_p, c_int32, c_float, POINTER(GradNormResult)]),
    "tsod_detection_keys_f32": (c_int, [c_void_p, c_int64, c_float, c_int32, c_void_p, c_void_p]),
    "tsod_gather_rows_f32": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_detection_nms_f32": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_float, c_int32, c_void_p, c_void_p, c_void_p,
                                       c_size_t, c_void_p]),
    "tsod_anchor_targets_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "tsod_anchor_targets_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_float, c_float, c_int32, c_int32, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_proposal_targets_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "tsod_proposal_targets_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_float, c_float,
                                          c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_anchor_targets_batch_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32]),
    "tsod_anchor_targets_batch_f32": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_float, c_float, c_int32,
                                              c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_proposal_targets_batch_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "tsod_proposal_targets_batch_f32": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                                c_float, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_size_t, c_void_p]),
    "tsod_rpn_losses_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_float, c_void_p,
                                    c_void_p, c_void_p]),
    "tsod_roi_losses_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                    c_int32, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tsod_proposal_targets_src_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_float,
                                              c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_size_t, c_void_p]),
    "tsod_rpn_losses_grad_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_float, c_void_p,
                                         c_float, c_void_p, c_void_p, c_int32, c_void_p]),
    "tsod_roi_losses_grad_f32": (c_int, [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                                         c_int32, c_float, c_void_p, c_float, c_void_p, c_int32, c_void_p, c_void_p]),
    "tsod_rpn_roi_scatter_f32": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                         c_int32, c_void_p, c_int32, c_int32, c_float, c_float, c_void_p, c_int32, c_void_p]),
    "tsod_wgrad_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int32]),
    "tsod_wgrad_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                               c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_size_t, c_void_p]),
    "tsod_roi_pool_avg_grad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "tsod_roi_pool_avg_grad_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                           c_float, c_float, c_float, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                           c_int32, c_void_p, c_size_t, c_void_p]),
    "tsod_roi_align_avg_grad_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "tsod_roi_align_avg_grad_f32": (c_int, [c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_float, c_float,
                                            c_float, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_int32,
                                            c_int32, c_void_p, c_size_t, c_void_p]),
    "tsod_dwconv3x3_grad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "tsod_dwconv3x3_grad_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                        c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32,
                                        c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_gconv1x1_pair_grad_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "tsod_gconv1x1_pair_grad_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int32,
                                            c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_dwconv3x3_grad_act_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                            c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32,
                                            c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_relu6_grad_mask_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32,
                                         c_void_p]),
    "tsod_pw_wgrad_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int32]),
    "tsod_pw_wgrad_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, POINTER(PwSegs), c_void_p, c_void_p,
                                  c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_pw_dgrad_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, POINTER(PwSegs), c_void_p, c_int32,
                                  c_int32, c_void_p]),
    "tsod_prelu_grad_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "tsod_prelu_grad_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_int32, c_float, c_void_p, c_int32,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_conv3x3_dense_wgrad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "tsod_conv3x3_dense_wgrad_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32,
                                             c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                             c_void_p]),
    "tsod_conv3x3_strided_wgrad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    "tsod_conv3x3_strided_wgrad_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32,
                                               c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                               c_void_p]),
    "tsod_prelu_grad_d2s_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "tsod_prelu_grad_d2s_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_float,
                                        c_void_p, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_pixel_subsample_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                         c_void_p]),
    "tsod_pixel_upsample_add_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                            c_void_p]),
    "tsod_prelu_grad_pool_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "tsod_prelu_grad_pool_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_float,
                                         c_void_p, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_conv7x7s2_wgrad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32]),
    "tsod_conv7x7s2_wgrad_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_conv3x3_wgrad_workspace_bytes": (c_size_t, [c_int32, c_int32, c_int32, c_int32, c_int32]),
    "tsod_conv3x3_wgrad_f32": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p,
                                       c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_bn_train_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "tsod_bn_stats_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_double, c_double,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_bn_apply_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                  c_int32, c_int32, c_void_p, c_void_p]),
    "tsod_bn_train_grad_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int64, c_int32, c_int32, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t,
                                       c_void_p]),
    "tsod_bn_apply_prelu_f32": (c_int, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                                        c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_float, c_void_p, c_int32, c_int32,
                                        c_void_p, c_void_p]),
    "tsod_bn_prelu_train_grad_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "tsod_bn_prelu_train_grad_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32,
                                             c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int32,
                                             c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_size_t,
                                             c_void_p]),
    "tsod_dropout_segs_f32": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32,
                                      c_float, c_void_p, c_uint32, c_uint64, c_void_p]),
    "tsod_dropout_key_set": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p]),
    "tsod_dropout_params": (c_int, [c_float, POINTER(c_uint64), POINTER(c_float)]),
    "tsod_philox4x32_host": (None, [POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
    "tsod_eval_match_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "tsod_eval_match_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p,
                                    c_void_p, c_size_t, c_void_p]),
    "tsod_sort_pairs_workspace_bytes": (c_size_t, [c_int64]),
    "tsod_sort_pairs_u64": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                    c_size_t, c_void_p]),
    "tsod_eval_accumulate_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "tsod_eval_accumulate_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_eval_match_coco_workspace_bytes": (c_size_t, [c_int32, c_int32]),
    "tsod_eval_match_coco_f32": (c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32,
                                         c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_eval_accumulate_coco_workspace_bytes": (c_size_t, [c_int64, c_int32]),
    "tsod_eval_accumulate_coco_f64": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                              c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                              c_void_p]),
    "tsod_draw_groups_u8": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, POINTER(DrawGroup), c_int32, c_void_p,
                                    c_int32, c_void_p]),
    "tsod_draw_font5x7": (c_int, [c_void_p]),
    "tsod_ema_scan_f32": (c_int, [c_void_p, c_int32, c_int64, c_int64, c_float, c_float, c_void_p, c_int64, c_void_p]),
    "tsod_plot_limits_f32": (c_int, [POINTER(c_void_p), POINTER(c_int64), c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_plot_series_u8": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32, POINTER(PlotSeries),
                                    c_int32, c_int64, c_int64, c_void_p, c_void_p]),
    "tsod_plot_items_u8": (c_int, [c_void_p, c_int32, c_int32, c_int64, c_void_p, c_int32, c_void_p]),
    "tsod_jpeg_parse": (c_int, [c_void_p, c_size_t, POINTER(JpegInfo)]),
    "tsod_jpeg_entropy_decode": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t]),
    "tsod_jpeg_idct_u8": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_int64,
                                  c_void_p, c_int64, c_void_p]),
    "tsod_jpeg_to_rgb_u8": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_int64,
                                    c_void_p]),
    "tsod_jpeg_scan_sizes": (c_int, [POINTER(JpegInfo), c_size_t, POINTER(c_int64), POINTER(c_int32)]),
    "tsod_jpeg_scan_prepare": (c_int, [c_void_p, c_size_t, c_void_p, c_int64, POINTER(c_int64), c_void_p, c_int32, POINTER(c_int32),
                                       c_void_p]),
    "tsod_jpeg_huffman_i16": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                      c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32, c_void_p]),
    "tsod_jpeg_huffman_split_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int32]),
    "tsod_jpeg_huffman_split_i16": (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                                            c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_int32,
                                            c_void_p, c_size_t, c_void_p, c_void_p]),
    "tsod_allgather_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tsod_comm_unique_id": (c_int, [c_void_p]),
    "tsod_comm_init_rank": (c_int, [POINTER(c_void_p), c_int32, c_void_p, c_int32]),
    "tsod_comm_destroy": (c_int, [c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def lib() -> ctypes.CDLL:
    """The loaded libtsod.so.  Raises (no fallback) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TsodError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C two_stage_object_detection_amd/csrc`). There is no CPU fallback.")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        if l.tsod_version() != 242:
            raise TsodError(f"{LIB_PATH} is version {l.tsod_version()}, this package binds version 242 of include/tsod.h: rebuild it "
                            "(`make -C two_stage_object_detection_amd/csrc`)")
        _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise TsodError(f"{what or 'tsod call'} failed: {lib().tsod_status_str(rc).decode()} ({rc})")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t) -> int:
    """Raw device pointer of a tensor (or 0 for None)."""
    return 0 if t is None else t.data_ptr()


class NHWC4Images:
    """A batch of images already in the backbone's input layout: ``data`` is [N,H,W,4] f32 on the GPU (RGB + a zero
    4th channel), as written by ``dataset.transform.EvalTransform.batch``.  ``shape`` reports the NCHW shape the
    reference's code reads (``x.shape[1:]`` = (3,H,W), nets/frcnn.py:33), so the detector accepts it wherever it accepts
    an NCHW tensor and skips its own layout kernel."""

    def __init__(self, data: torch.Tensor):
        if data.dim() != 4 or data.shape[3] != 4 or data.dtype != torch.float32 or not data.is_contiguous():
            raise TsodError(f"NHWC4Images needs a contiguous f32 [N,H,W,4] tensor, got {tuple(data.shape)} {data.dtype}")
        self.data = data

    @property
    def shape(self):
        n, h, w, _ = self.data.shape
        return torch.Size((n, 3, h, w))

    device = property(lambda self: self.data.device)
    is_cuda = property(lambda self: self.data.is_cuda)
    dtype = property(lambda self: self.data.dtype)

    def dim(self):
        return 4


def require_cuda(t, what: str) -> None:
    if isinstance(t, NHWC4Images):
        t = t.data
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TsodError(f"{what}: this package is a HIP-only path and needs a CUDA/ROCm tensor "
                        "(the CPU restatement lives under oracle/ and is test infrastructure only)")
    if t.dtype != torch.float32:
        raise TsodError(f"{what}: float32 required, got {t.dtype}")


def make_conv_desc(*, N, H, W, in_pitch, segs, Cout, out_pitch, out_off=0, KH=1, KW=1, stride=1, pad_h=0, pad_w=0,
                   OH=None, OW=None, act=ACT_NONE, slope=0.0, res_pitch=0, res_off=0, tile=TILE_AUTO, split_k=0,
                   precision=0, src2=None) -> ConvDesc:
    """``src2`` = (channels, pitch, channel offset, stride, H2, W2) of the optional second source (tsod_conv2d_dual_f32)."""
    d = ConvDesc()
    d.N, d.H, d.W, d.in_pitch = N, H, W, in_pitch
    d.n_seg = len(segs)
    for i, (off, ln) in enumerate(segs):
        d.seg_off[i], d.seg_len[i] = off, ln
    d.Cout, d.out_pitch, d.out_off = Cout, out_pitch, out_off
    d.KH, d.KW, d.stride, d.pad_h, d.pad_w = KH, KW, stride, pad_h, pad_w
    d.OH = OH if OH is not None else (H + 2 * pad_h - KH) // stride + 1
    d.OW = OW if OW is not None else (W + 2 * pad_w - KW) // stride + 1
    d.act, d.slope = act, float(slope)
    d.res_pitch, d.res_off, d.tile, d.split_k = res_pitch, res_off, tile, split_k
    d.precision = int(precision)
    if src2 is not None:
        d.c2, d.in2_pitch, d.in2_off, d.stride2, d.H2, d.W2 = (int(v) for v in src2)
    return d


def make_bottleneck_desc(*, N, H, W, Cin, in_pitch, Cout, out_pitch, slope, w_exps, projection=False, Cmid=64,
                         a_scale_exp=4, range_flag=None, amax_in=None, amax_out=None) -> BottleneckDesc:
    """The descriptor of tsod_bottleneck_fp16x2; ``range_flag`` / ``amax_*`` are raw device pointers (0 / None: none)."""
    d = BottleneckDesc()
    d.N, d.H, d.W, d.Cin, d.in_pitch, d.Cmid, d.Cout, d.out_pitch = N, H, W, Cin, in_pitch, Cmid, Cout, out_pitch
    d.projection = 1 if projection else 0
    d.slope = float(slope)
    for k in range(3):
        d.w_exp[k] = int(w_exps[k])
    d.a_scale_exp = int(a_scale_exp)
    d.range_flag, d.amax_in, d.amax_out = range_flag or None, amax_in or None, amax_out or None
    return d


def stem_out_hw(H, W):
    """(oh, ow, ph, pw): the map after ResNet's 7x7/2 conv (pad 3) and after its 3x3/2 max pool (pad 1)."""
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return oh, ow, (oh - 1) // 2 + 1, (ow - 1) // 2 + 1


def make_stem_desc(*, N, H, W, in_layout, out_pitch, slope, w_exp, range_flag=None, amax_out=None) -> StemDesc:
    """The descriptor of tsod_stem_fp16x2; ``range_flag`` / ``amax_out`` are raw device pointers (0 / None: none)."""
    d = StemDesc()
    d.N, d.H, d.W, d.in_layout, d.out_pitch = N, H, W, in_layout, out_pitch
    d.slope, d.w_exp = float(slope), int(w_exp)
    d.range_flag, d.amax_out = range_flag or None, amax_out or None
    return d
