"""Host-side contract of the registration-evaluation entry point (no GPU needed): the symbol, its
ctypes signature and result structure, the unchanged ABI version, the drop-in exports, and the
argument rules that are decided before any device work."""
import ctypes as C

import numpy as np
import pytest

from m3d import _lib


def test_library_exports_evaluate_registration_within_abi_13():
    lib = _lib.load()
    assert hasattr(lib, "m3d_evaluate_registration")
    assert "m3d_evaluate_registration" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["m3d_evaluate_registration"]
    assert res is C.c_int and len(args) == 11
    assert lib.m3d_abi_version() == _lib.ABI_VERSION == 13


def test_eval_result_layout():
    assert C.sizeof(_lib.EvalResult) == 8 * 39
    assert [f[0] for f in _lib.EvalResult._fields_] == ["fitness", "inlier_rmse", "num_correspondences",
                                                        "information"]
    assert _lib.EvalResult.information.offset == 24 and _lib.EVAL_INFORMATION == 1


def test_matcher_exports_the_three_functions():
    import matcher
    import matcher.evaluate as E

    for name in ("evaluate_registration", "get_information_matrix_from_point_clouds",
                 "compute_point_cloud_distance"):
        assert name in matcher.__all__
        assert getattr(matcher, name) is getattr(E, name)


@pytest.mark.parametrize("r", [0.0, -1.0])
def test_non_positive_radius_is_the_empty_result_without_a_device(r):
    import matcher

    rng = np.random.default_rng(0)
    src, tgt = rng.normal(size=(10, 3)), rng.normal(size=(12, 3))
    T = np.eye(4)
    T[0, 3] = 0.25
    out = matcher.evaluate_registration(src, tgt, r, T)
    assert (out.fitness, out.inlier_rmse) == (0.0, 0.0)
    assert out.correspondence_set.shape == (0, 2) and out.correspondence_set.dtype == np.int32
    np.testing.assert_array_equal(out.transformation, T)
    np.testing.assert_array_equal(matcher.evaluate_registration(src, tgt, r).transformation, np.eye(4))
    G = matcher.get_information_matrix_from_point_clouds(src, tgt, r, T)
    assert G.shape == (6, 6) and G.dtype == np.float64 and not G.any()


def test_bad_nn_string_raises_value_error():
    from m3d.core import evaluate

    with pytest.raises(ValueError, match="nn must be one of"):
        evaluate(None, None, np.eye(4), 0.1, nn="kdtree")
