"""The gradient norm's host twin (tsod_grad_norm_host_f32) against the numpy restatement of its order,
bit for bit, and against the float64 definition - no GPU needed.  The GPU test holds the kernels to the host twin."""
import numpy as np
import pytest

import grad_clip_restated as C


def twin(grads, max_norm):
    from two_stage_object_detection_amd import hip_ops
    return hip_ops.grad_norm_host([np.ascontiguousarray(g.numpy()) for g in grads], max_norm)


def check(grads, max_norm, what):
    got, want = twin(grads, max_norm), C.restated(grads, max_norm)
    print(f"{what}: twin sum_sq {got[0]!r} norm {got[1]!r} coef {got[2]!r}; restated {want[0]!r} {want[1]!r} {want[2]!r}")
    assert got[0].dtype == np.float64 and got[1].dtype == np.float32 and got[2].dtype == np.float32
    assert C.same_record(got, want), (what, got, want)
    return got


SIZE_SETS = [C.SIZES] + [(n,) for n in C.SIZES]


@pytest.mark.parametrize("sizes", SIZE_SETS, ids=["all"] + [str(n) for n in C.SIZES])
def test_twin_equals_restatement(sizes):
    grads = C.draw_grads(sizes)
    sum_sq, norm, coef = check(grads, 1.0, f"sizes {sizes}")
    # one float32 ulp of the float64 definition: the squares are exact in f64 and the f64 summation error over <= 1e6 terms
    # is below 1e-10 relative, far under 2^-24; what is left is the one rounding of sqrt's f64 result to f32
    exact = C.exact_norm(grads)
    d = C.ulp_distance_f32(norm, exact)
    print(f"sizes {sizes}: norm {norm!r} float64 definition {exact!r}: {d:.3f} ulp")
    assert d <= 1.0
    assert C.same_bits(coef, C.coef_of(norm, 1.0))


def test_partition_matters_to_the_restatement_only_through_the_stated_order():
    """The same values as one tensor and cut into tensors take different chunk partitions: both twins follow their own."""
    whole = C.draw_grads((2049 + 4100,))
    cut = [whole[0][:2049].clone(), whole[0][2049:].clone()]
    a, b = check(whole, 1.0, "one tensor"), check(cut, 1.0, "two tensors")
    assert abs(float(a[1]) - float(b[1])) <= float(np.spacing(a[1]))


def test_all_zero_gradients():
    import torch
    got = check([torch.zeros(n) for n in C.SIZES], 1.0, "zeros")
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 1.0


def test_norm_below_max_gives_exactly_one():
    grads = C.draw_grads(scale=1e-3)
    norm = C.exact_norm(grads)
    got = check(grads, 2 * norm, "below")
    assert C.bits(got[2]) == C.bits(np.float32(1.0))
    got = check(grads, 1e30, "far below")
    assert C.bits(got[2]) == C.bits(np.float32(1.0))


def test_norm_above_max_clips():
    grads = C.draw_grads()
    norm = C.exact_norm(grads)
    assert norm > 1.0
    got = check(grads, 1.0, "above")
    assert 0.0 < got[2] < 1.0 and C.same_bits(got[2], C.coef_of(got[1], 1.0))
    assert abs(float(got[2]) * norm - 1.0) < 1e-5
    got = check(grads, 0.0, "max_norm 0")
    assert got[2] == 0.0


def test_one_inf_gives_inf_norm_and_zero_coefficient():
    grads = C.draw_grads()
    grads[4][2047] = float("inf")
    got = check(grads, 1.0, "inf")
    assert np.isinf(got[0]) and np.isinf(got[1]) and got[1] > 0 and got[2] == 0.0
    grads[4][2047] = float("-inf")
    got = check(grads, 1.0, "-inf")
    assert np.isinf(got[1]) and got[1] > 0 and got[2] == 0.0


def test_one_nan_gives_nan_for_both():
    grads = C.draw_grads()
    grads[6][4099] = float("nan")                      # the last element of a short quad
    got = check(grads, 1.0, "nan")
    assert np.isnan(got[0]) and np.isnan(got[1]) and np.isnan(got[2])


def test_more_than_256_chunks_take_a_second_round_of_the_finish():
    grads = C.draw_grads((2048 * 300 + 5,))
    got = check(grads, 1.0, "301 chunks")
    assert C.ulp_distance_f32(got[1], C.exact_norm(grads)) <= 1.0


def test_empty_inputs():
    import torch
    assert C.same_record(twin([], 1.0), C.restated([], 1.0))
    got = twin([torch.zeros(0), torch.zeros(0)], 0.0)
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 1.0
    # an empty tensor between others takes no chunk
    grads = C.draw_grads((18, 2049))
    with_empty = [grads[0], torch.zeros(0), grads[1]]
    assert C.same_record(twin(with_empty, 1.0), twin(grads, 1.0))


def test_rejected_arguments():
    from two_stage_object_detection_amd import hip_ops
    from two_stage_object_detection_amd._ffi import TsodError
    g = [np.ones(4, np.float32)]
    for bad in (-1.0, float("nan")):
        with pytest.raises(TsodError):
            hip_ops.grad_norm_host(g, bad)
    with pytest.raises(ValueError):
        hip_ops.grad_norm_host([np.ones(4, np.float64)], 1.0)
