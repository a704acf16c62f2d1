"""ABI of the gradient-clipping entry points (include/tsod.h): declared, bound and exported together,
the result record laid out as the C compiler lays it out, bad arguments answered with status codes before anything is
dereferenced or launched, and the new kernels free of scratch - no GPU needed."""
import ctypes
import os
import re
import subprocess

from two_stage_object_detection_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, ALIGNMENT = 0, -1, -2, -3
P = 0x10000          # a fake "device pointer": validation must fail before it is ever dereferenced
ENTRY_POINTS = ("tsod_grad_norm_workspace_bytes", "tsod_grad_norm_f32", "tsod_adamw_step_clipped_f32", "tsod_grad_scale_f32",
                "tsod_grad_norm_host_f32")


def test_entry_points_declared_bound_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsod.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(tsod_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text)}
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in decl and name in _ffi.EXPORTED_SYMBOLS and hasattr(raw, name), name
        assert len(decl[name].split(",")) == len(_ffi._SIGNATURES[name][1]), name
    assert _ffi.lib().tsod_version() == 242                       # the change only adds exports


def test_result_record_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsod.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   'sizeof(tsod_grad_norm_result), offsetof(tsod_grad_norm_result, sum_sq), '
                   'offsetof(tsod_grad_norm_result, norm), offsetof(tsod_grad_norm_result, coef)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = tuple(int(v) for v in subprocess.check_output([str(exe)]).split())
    R = _ffi.GradNormResult
    assert got == (16, 0, 8, 12)
    assert got == (ctypes.sizeof(R), R.sum_sq.offset, R.norm.offset, R.coef.offset)


def test_workspace_bytes():
    L = _ffi.lib()
    assert L.tsod_grad_norm_workspace_bytes(0) == 0 and L.tsod_grad_norm_workspace_bytes(-5) == 0
    assert L.tsod_grad_norm_workspace_bytes(1) == 8 and L.tsod_grad_norm_workspace_bytes(1521) == 8 * 1521


def test_grad_norm_validation():
    L = _ffi.lib()
    f = L.tsod_grad_norm_f32
    assert f(None, 1, P, 1, 1.0, P, P, 8, None) == INVALID
    assert f(P, 1, None, 1, 1.0, P, P, 8, None) == INVALID
    assert f(P, 1, P, 1, 1.0, None, P, 8, None) == INVALID
    assert f(P, 1, P, 1, 1.0, P, None, 8, None) == INVALID
    assert f(P, -1, P, 1, 1.0, P, P, 8, None) == INVALID
    assert f(P, 1, P, -1, 1.0, P, P, 8, None) == INVALID
    assert f(P, 1, P, 2 ** 31, 1.0, P, P, 2 ** 40, None) == INVALID
    assert f(P, 1, P, 1, -1.0, P, P, 8, None) == INVALID
    assert f(P, 1, P, 1, -0.5e-30, P, P, 8, None) == INVALID
    assert f(P, 1, P, 1, float("nan"), P, P, 8, None) == INVALID
    assert f(P, 1, P, 1, 1.0, P, P, 7, None) == INVALID               # too small a workspace
    assert f(P, 1, P, 3, 1.0, P, P, 16, None) == INVALID
    assert f(P, 1, P, 1, 1.0, P, P + 4, 8, None) == ALIGNMENT
    assert f(P, 1, P, 1, 1.0, P + 4, P, 8, None) == ALIGNMENT


def test_clipped_step_validation():
    L = _ffi.lib()
    f = L.tsod_adamw_step_clipped_f32
    g = (_ffi.AdamWGroup * 2)()
    for clip in (None, P):                                            # the rules of tsod_adamw_step_f32, with and without a record
        assert f(None, 1, P, 1, g, 1, 0, clip, None) == INVALID
        assert f(P, 1, None, 1, g, 1, 0, clip, None) == INVALID
        assert f(P, 1, P, 1, None, 1, 0, clip, None) == INVALID
        assert f(P, -1, P, 1, g, 1, 0, clip, None) == INVALID
        assert f(P, 1, P, -1, g, 1, 0, clip, None) == INVALID
        assert f(P, 1, P, 2 ** 31, g, 1, 0, clip, None) == INVALID
        assert f(P, 1, P, 1, g, 0, 0, clip, None) == INVALID
        assert f(P, 1, P, 1, g, _ffi.ADAMW_MAX_GROUPS + 1, 0, clip, None) == UNSUPPORTED
        assert f(P, 0, P, 0, g, 2, 1, clip, None) == OK               # nothing to do is not an error, and launches nothing
        assert f(P, 3, P, 0, g, 2, 1, clip, None) == OK
    assert f(P, 1, P, 1, g, 1, 0, P + 4, None) == ALIGNMENT


def test_grad_scale_validation():
    L = _ffi.lib()
    f = L.tsod_grad_scale_f32
    assert f(None, 1, P, 1, P, None) == INVALID
    assert f(P, 1, None, 1, P, None) == INVALID
    assert f(P, 1, P, 1, None, None) == INVALID
    assert f(P, -1, P, 1, P, None) == INVALID
    assert f(P, 1, P, -1, P, None) == INVALID
    assert f(P, 1, P, 2 ** 31, P, None) == INVALID
    assert f(P, 1, P, 1, P + 4, None) == ALIGNMENT
    assert f(P, 0, P, 0, P, None) == OK
    assert f(P, 3, P, 0, P, None) == OK


def test_host_twin_validation():
    import numpy as np
    L = _ffi.lib()
    f = L.tsod_grad_norm_host_f32
    a = np.ones(4, np.float32)
    ptrs, numels = (ctypes.c_void_p * 1)(a.ctypes.data), (ctypes.c_int64 * 1)(4)
    out = _ffi.GradNormResult(-1.0, -1.0, -1.0)
    assert f(None, numels, 1, 1.0, ctypes.byref(out)) == INVALID
    assert f(ptrs, None, 1, 1.0, ctypes.byref(out)) == INVALID
    assert f(ptrs, numels, 1, 1.0, None) == INVALID
    assert f(ptrs, numels, -1, 1.0, ctypes.byref(out)) == INVALID
    assert f(ptrs, numels, 1, -1.0, ctypes.byref(out)) == INVALID
    assert f(ptrs, numels, 1, float("nan"), ctypes.byref(out)) == INVALID
    assert f(ptrs, (ctypes.c_int64 * 1)(-4), 1, 1.0, ctypes.byref(out)) == INVALID
    assert f((ctypes.c_void_p * 1)(None), numels, 1, 1.0, ctypes.byref(out)) == INVALID
    assert (out.sum_sq, out.norm, out.coef) == (-1.0, -1.0, -1.0)     # nothing was written
    assert f(ptrs, numels, 1, 4.0, ctypes.byref(out)) == OK
    assert (out.sum_sq, out.norm, out.coef) == (4.0, 2.0, 1.0)
    assert f(ptrs, numels, 0, 0.0, ctypes.byref(out)) == OK
    assert (out.sum_sq, out.norm, out.coef) == (0.0, 0.0, 1.0)


def test_new_kernels_use_no_scratch_memory(tmp_path):
    """One instantiation each, no scratch, no spills; the clipped step kernel stays at 64 VGPRs (eight waves per SIMD) like the
    plain one, which is still the only instantiation of its name."""
    from test_kernel_metadata import _kernel_notes
    kernels = _kernel_notes(tmp_path)
    for name, vgpr_cap in (("adamw_clipped_multi_tensor_kernel", 64), ("adamw_multi_tensor_kernel", 64),
                           ("grad_norm_partial_kernel", 64), ("grad_norm_finish_kernel", 64), ("grad_scale_kernel", 64)):
        found = {k: v for k, v in kernels.items() if name in k}
        assert len(found) == 1, (name, sorted(found))
        notes = next(iter(found.values()))
        print(name, notes)
        assert notes.get("private_segment_fixed_size", 0) == 0 and notes.get("vgpr_spill_count", 0) == 0, (name, notes)
        assert notes.get("sgpr_spill_count", 0) == 0 and 0 < notes["vgpr_count"] <= vgpr_cap, (name, notes)
