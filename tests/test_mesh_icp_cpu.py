"""ICP against a mesh's surface, the part that needs no GPU: the numpy restatement of
csrc/mesh_icp.hip's contract (tests/mesh_icp_restatement.py) does what the feature is for, and the
library exports the entry points."""
import ctypes as C

import numpy as np

import icp_oracle as I
import mesh_icp_restatement as R
import mesh_restatement as M
from m3d import _lib


def test_surface_target_recovers_the_pose_the_vertex_target_does_not():
    """600 surface samples of the 384-triangle mesh, moved by a small rigid motion, radius
    0.1·extent, init I: against the surface the loop ends at the pose to rounding; against the
    mesh's 194 vertices with area-weighted vertex normals it barely moves."""
    c = R.clean_pair()
    assert len(c["f"]) == 384 and len(c["v"]) == 194 and abs(c["ext"] - 10.37) < 0.01
    start = R.worst_error(np.eye(4), c["T_true"], c["src"])
    evals = []
    ref = R.registration_icp_to_mesh(c["src"], c["v"], c["f"], c["radius"], on_eval=lambda k, p, t: evals.append(k))
    err = R.worst_error(ref["transformation"], c["T_true"], c["src"])
    vert = I.registration_icp(c["src"], c["v"], c["radius"], np.eye(4), R.vertex_normals(c["v"], c["f"]))
    err_v = R.worst_error(vert["transformation"], c["T_true"], c["src"])
    print(f"start {start:.3g}; surface {err:.3g} in {len(evals)} evaluations; vertices {err_v:.3g}")
    assert start > 0.4
    assert err < 1e-12 and ref["fitness"] == 1.0 and ref["converged"]
    assert err_v > 0.1


def test_coarser_mesh_the_same():
    c = R.clean_pair(6, 8)
    assert len(c["f"]) == 96
    ref = R.registration_icp_to_mesh(c["src"], c["v"], c["f"], c["radius"])
    vert = I.registration_icp(c["src"], c["v"], c["radius"], np.eye(4), R.vertex_normals(c["v"], c["f"]))
    assert R.worst_error(ref["transformation"], c["T_true"], c["src"]) < 1e-12
    assert R.worst_error(vert["transformation"], c["T_true"], c["src"]) > 0.1


def test_tukey_beats_the_unweighted_rows_on_outliers():
    o = R.outlier_pair()
    fits = []
    plain = R.registration_icp_to_mesh(o["src"], o["v"], o["f"], o["radius"],
                                       on_eval=lambda k, p, t: fits.append(float((t >= 0).mean())))
    tukey = R.registration_icp_to_mesh(o["src"], o["v"], o["f"], o["radius"], kind=R.TUKEY, k=o["k"])
    e0 = R.worst_error(plain["transformation"], o["T_true"], o["src"])
    e1 = R.worst_error(tukey["transformation"], o["T_true"], o["src"])
    print(f"unweighted {e0:.3g}, Tukey {e1:.3g}, ratio {e0 / e1:.2f}; fitness {fits[0]:.3f} → {fits[-1]:.3f}")
    assert e0 >= 5.0 * e1
    assert 0.5 < fits[0] < fits[-1] < 1.0  # the radius does work: not everything matches


def test_face_normals_are_unit():
    for shape in ((12, 16), (6, 8)):
        c = R.clean_pair(*shape)
        n = R.face_normals(c["v"], c["f"])
        np.testing.assert_allclose(np.sqrt((n * n).sum(axis=1)), 1.0, rtol=0, atol=1e-15)


def test_hand_case_one_triangle_three_points():
    """Dyadic numbers: three points at height h above the face of one triangle give r = h and
    J = [p × n | n] exactly, and the update is the pure translation −h·n."""
    v = np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]])
    f = np.array([[0, 1, 2]])
    h = 0.25
    p = np.array([[1.0, 1.0, h], [2.0, 0.5, h], [0.5, 2.0, h]])
    n = R.face_normals(v, f)
    np.testing.assert_array_equal(n, [[0.0, 0.0, 1.0]])
    ev = R.evaluate(p, v, f, 1.0)
    np.testing.assert_array_equal(ev["triangle"], [0, 0, 0])
    np.testing.assert_array_equal(ev["d2"], [h * h] * 3)
    np.testing.assert_array_equal(ev["point"], p * (1.0, 1.0, 0.0))
    assert ev["fitness"] == 1.0 and ev["rmse"] == h
    r, J, d2, idx = R.rows(p, v, f, ev)
    np.testing.assert_array_equal(r, [h, h, h])
    np.testing.assert_array_equal(J, np.concatenate([np.cross(p, n[[0, 0, 0]]), n[[0, 0, 0]]], axis=1))
    np.testing.assert_array_equal(J[:, :3], np.stack([p[:, 1], -p[:, 0], np.zeros(3)], axis=1))
    s, a = R.sums(p, v, f, ev)
    assert s[28] == 3.0 and s[29] == 3 * h * h and s[27] == 3 * h * h
    upd = R.update(p, v, f, ev)
    expect = np.eye(4)
    expect[2, 3] = -h
    np.testing.assert_allclose(upd, expect, rtol=0, atol=1e-15)
    # the radius is strict: d² = max_dist² is no match
    assert (R.evaluate(p, v, f, h)["triangle"] == -1).all()
    assert (R.evaluate(p, v, f, np.nextafter(h, 1.0))["triangle"] == 0).all()
    # a NaN point never matches
    q = p.copy()
    q[1, 0] = np.nan
    np.testing.assert_array_equal(R.evaluate(q, v, f, 1.0)["triangle"], [0, -1, 0])


def test_evaluate_is_the_mesh_contracts_winner_filtered():
    c = R.clean_pair()
    pts = c["src"][:100]
    ref = M.closest_points(c["v"], c["f"], pts)
    r = float(np.sqrt(np.median(ref["d2"])))  # about half of the points inside
    ev = R.evaluate(pts, c["v"], c["f"], r)
    hit = ref["d2"] < r * r
    assert 5 < hit.sum() < 95
    np.testing.assert_array_equal(ev["triangle"], np.where(hit, ref["triangle"], -1))
    assert ev["d2"].tobytes() == np.where(hit, ref["d2"], np.inf).tobytes()


def test_symbols_and_null_arguments():
    lib = _lib.load()
    for name in ("m3d_mesh_icp_terms", "m3d_mesh_icp_run"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    sums = (C.c_double * 32)()
    res = _lib.IcpResult()
    p = _lib.IcpParams(1e-6, 1e-6, 30, _lib.EST_POINT_TO_PLANE, _lib.NN_GRID, 0)
    T = (C.c_double * 16)(*np.eye(4).reshape(-1))
    fake = C.c_void_p(8)  # never dereferenced: the null argument is rejected first
    for ctx, mesh in ((None, None), (None, fake), (fake, None)):
        assert lib.m3d_mesh_icp_terms(ctx, mesh, None, T, 1.0, None, 0, None, sums, None, None, None) == \
            _lib.M3D_ERR_INVALID
        assert lib.m3d_mesh_icp_run(ctx, mesh, None, T, 1.0, C.byref(p), None, 0, 1, C.byref(res), None, None) == \
            _lib.M3D_ERR_INVALID
    import matcher

    for name in ("registration_icp_to_mesh", "evaluate_registration_to_mesh", "refine_registration_to_mesh"):
        assert callable(getattr(matcher, name))
