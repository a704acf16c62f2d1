"""ABI of the optimizer entry points (include/tsod.h): declared, bound and exported together, the
ctypes mirrors laid out as the C compiler lays out the structs, and bad arguments answered with status codes before anything
is dereferenced or launched - no GPU needed."""
import ctypes
import os
import re
import subprocess
from ctypes import byref

import numpy as np

from two_stage_object_detection_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -2
P = 0x10000          # a fake "device pointer": validation must fail before it is ever dereferenced
ENTRY_POINTS = ("tsod_adamw_step_f32", "tsod_adamw_step_host_f32")


def test_entry_points_declared_bound_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsod.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(tsod_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text)}
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in decl and name in _ffi.EXPORTED_SYMBOLS and hasattr(raw, name), name
        assert len(decl[name].split(",")) == len(_ffi._SIGNATURES[name][1]), name
    assert _ffi.lib().tsod_version() == 242


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsod.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n", '
                   'sizeof(tsod_adamw_tensor), offsetof(tsod_adamw_tensor, n), offsetof(tsod_adamw_tensor, group), '
                   'sizeof(tsod_adamw_chunk), sizeof(tsod_adamw_group), offsetof(tsod_adamw_group, step_size), '
                   'offsetof(tsod_adamw_group, eps), TSOD_ADAMW_CHUNK, TSOD_ADAMW_MAX_GROUPS); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = tuple(int(v) for v in subprocess.check_output([str(exe)]).split())
    G = _ffi.AdamWGroup
    # hip_ops.adamw_table writes a record as six int64 words, hip_ops.adamw_chunks a row as two int32
    assert got == (48, 32, 40, 8, ctypes.sizeof(G), G.step_size.offset, G.eps.offset, _ffi.ADAMW_CHUNK, _ffi.ADAMW_MAX_GROUPS)
    assert _ffi.ADAMW_CHUNK % 1024 == 0


def test_device_entry_point_validation():
    L = _ffi.lib()
    g = (_ffi.AdamWGroup * 2)()
    assert L.tsod_adamw_step_f32(None, 1, P, 1, g, 1, 0, None) == INVALID
    assert L.tsod_adamw_step_f32(P, 1, None, 1, g, 1, 0, None) == INVALID
    assert L.tsod_adamw_step_f32(P, 1, P, 1, None, 1, 0, None) == INVALID
    assert L.tsod_adamw_step_f32(P, -1, P, 1, g, 1, 0, None) == INVALID
    assert L.tsod_adamw_step_f32(P, 1, P, -1, g, 1, 0, None) == INVALID
    assert L.tsod_adamw_step_f32(P, 1, P, 2 ** 31, g, 1, 0, None) == INVALID
    assert L.tsod_adamw_step_f32(P, 1, P, 1, g, 0, 0, None) == INVALID
    assert L.tsod_adamw_step_f32(P, 1, P, 1, g, -3, 0, None) == INVALID
    assert L.tsod_adamw_step_f32(P, 1, P, 1, g, _ffi.ADAMW_MAX_GROUPS + 1, 0, None) == UNSUPPORTED
    # nothing to do is not an error, and launches nothing
    assert L.tsod_adamw_step_f32(P, 0, P, 0, g, 2, 1, None) == OK
    assert L.tsod_adamw_step_f32(P, 3, P, 0, g, 2, 1, None) == OK


def test_host_entry_point_validation():
    L = _ffi.lib()
    a = [np.full(4, 1.5, np.float32) for _ in range(4)]
    ptrs = [x.ctypes.data for x in a]
    g = _ffi.AdamWGroup(1.0, 0.1, 0.999, 0.001, 1e-3, 1.0, 1e-8, 0.0)
    for k in range(4):
        bad = list(ptrs)
        bad[k] = None
        assert L.tsod_adamw_step_host_f32(*bad, 4, byref(g), 1) == INVALID
    assert L.tsod_adamw_step_host_f32(*ptrs, 4, None, 1) == INVALID
    assert L.tsod_adamw_step_host_f32(*ptrs, -1, byref(g), 1) == INVALID
    assert all((x == 1.5).all() for x in a)                               # nothing was touched
    assert L.tsod_adamw_step_host_f32(*ptrs, 0, byref(g), 1) == OK
    assert all((x == 1.5).all() for x in a)
    assert L.tsod_adamw_step_host_f32(*ptrs, 3, byref(g), 1) == OK
    assert (a[1][:3] == 0).all() and a[1][3] == 1.5 and a[0][3] == 1.5 and (a[0][:3] != 1.5).all()


def test_adamw_kernel_uses_no_scratch_memory(tmp_path):
    """One instantiation, no scratch, no spills, at most 64 VGPRs (eight waves per SIMD for a kernel that only streams)."""
    from test_kernel_metadata import _kernel_notes
    found = {k: v for k, v in _kernel_notes(tmp_path).items() if "adamw_multi_tensor_kernel" in k}
    assert len(found) == 1, sorted(found)
    notes = next(iter(found.values()))
    assert notes.get("private_segment_fixed_size", 0) == 0 and notes.get("vgpr_spill_count", 0) == 0, notes
    assert notes.get("sgpr_spill_count", 0) == 0 and 0 < notes["vgpr_count"] <= 64, notes
