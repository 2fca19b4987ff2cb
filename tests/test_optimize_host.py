"""Host side of uf3_amd.regression.optimize: the reference's cut-off helpers against its own captures
(tests/golden/optimize_cases.json, make_optimize_golden.py), lower_column_map against the oracle's feature rows, the
regulariser pieces of the scan, fold assignment and the models a scan returns."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic
from uf3_amd.data import composition
from uf3_amd.regression import least_squares, optimize

from _util import GOLDEN

with open(os.path.join(GOLDEN, "optimize_cases.json")) as _f:
    GOLD = json.load(_f)
CASES = sorted(GOLD["cases"])


def _basis(case, **override):
    c = GOLD["cases"][case]
    cs = composition.ChemicalSystem(c["elements"], degree=3)
    return optimize.get_bspline_config(cs, leading_trim=0, trailing_trim=3, **{**c["args"], **override})


def _key(interaction):
    return "-".join(interaction)


@pytest.mark.parametrize("case", CASES)
def test_helpers_equal_the_reference_captures(case):
    c = GOLD["cases"][case]
    basis = _basis(case)
    assert basis.n_feats == c["n_feat"]
    assert sorted(_key(k) for k in basis.knots_map) == sorted(c["knots"])
    for interaction, knots in basis.knots_map.items():
        want = c["knots"][_key(interaction)]
        seqs, wseqs = (knots, want) if len(interaction) == 3 else ([knots], [want])
        for s, w in zip(seqs, wseqs):
            np.testing.assert_allclose(s, w, rtol=0, atol=1e-15)
    low = optimize.get_lower_cutoffs(basis)
    np.testing.assert_allclose(low["lower_rmax_2b"], c["lower_rmax_2b"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(low["lower_rmax_3b"], c["lower_rmax_3b"], rtol=0, atol=1e-15)
    for r, cols in c["drop_2b"].items():
        assert optimize.get_columns_to_drop_2b(basis, float(r), c["args"]["knot_spacing_2b"]) == cols
    for r, cols in c["drop_3b"].items():
        assert optimize.get_columns_to_drop_3b(basis, float(r), c["args"]["knot_spacing_3b"]) == cols


def test_helpers_raise_where_the_reference_raises():
    cs = composition.ChemicalSystem(["Nb", "Sn"], degree=3)
    for name, c in GOLD["raises"]["config"].items():
        with pytest.raises(ValueError) as exc:
            optimize.get_bspline_config(cs, leading_trim=c["leading_trim"], trailing_trim=c["trailing_trim"], **c["args"])
        assert str(exc.value) == c["message"], name
    basis = _basis("nbsn_config_1")
    args = GOLD["cases"]["nbsn_config_1"]["args"]
    for r, msg in GOLD["raises"]["drop_2b"].items():
        with pytest.raises(ValueError) as exc:
            optimize.get_columns_to_drop_2b(basis, float(r), args["knot_spacing_2b"])
        assert str(exc.value) == msg
    for r, msg in GOLD["raises"]["drop_3b"].items():
        with pytest.raises(ValueError) as exc:
            optimize.get_columns_to_drop_3b(basis, float(r), args["knot_spacing_3b"])
        assert str(exc.value) == msg


def _rows(basis, frame):
    ref = O.featurize(O.OracleBasis(basis), frame)
    return np.concatenate([ref["xe"][None], ref["xf"].reshape(-1, basis.n_feats)])


def _check_map(large, frame, pairs):
    big = _rows(large, frame)
    mask_o = least_squares.get_freezing_mask(large.n_feats, large.col_idx)
    scale = np.abs(big).max()
    for r2, r3 in pairs:
        low = optimize.lower_basis(large, r2, r3)
        cols = optimize.lower_column_map(large, low)
        small = _rows(low, frame)
        mask_l = least_squares.get_freezing_mask(low.n_feats, low.col_idx)
        assert cols.dtype == np.int64 and len(cols) == len(mask_l)
        assert np.abs(small[:, mask_l] - big[:, mask_o[cols]]).max() <= 1e-14 * scale, (r2, r3)
        assert np.abs(small[:, low.col_idx]).max() == 0.0       # (trimmed columns carry no features)


def test_lower_column_map_against_the_oracle_config_1():
    large = _basis("mow_config_1")
    frame = synthetic.lattice_frame("bcc", (3, 3, 3), 3.16, [42, 74], seed=5)
    low = optimize.get_lower_cutoffs(large)
    _check_map(large, frame, [(r2, r3) for r2 in low["lower_rmax_2b"] for r3 in low["lower_rmax_3b"]])


def test_lower_column_map_against_the_oracle_w_notebook():
    large = _basis("w_notebook")
    frame = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=6)
    low = optimize.get_lower_cutoffs(large)
    _check_map(large, frame, [(r2, r3) for r2 in low["lower_rmax_2b"][::3] for r3 in low["lower_rmax_3b"]])


def test_lower_column_map_rejects_what_is_not_a_column_drop():
    large = _basis("mow_config_1")
    with pytest.raises(ValueError):                              # another spacing
        optimize.lower_column_map(large, _basis("mow_config_1", rmax_2b=4.81, knot_spacing_2b=0.2))
    with pytest.raises(ValueError):                              # another r_min
        optimize.lower_column_map(large, _basis("mow_config_1", rmin_2b=0.41, rmax_2b=4.81))
    with pytest.raises(ValueError):                              # another chemical system
        optimize.lower_column_map(large, _basis("nbsn_config_1", rmax_2b=4.81))
    low = _basis("mow_config_1", rmax_2b=4.81, rmax_3b=3.2)
    assert len(optimize.lower_column_map(large, low))
    low.frozen_c = np.asarray(low.frozen_c, dtype=float).copy()
    low.frozen_c[0] = 0.5                                        # frozen values differ
    with pytest.raises(ValueError):
        optimize.lower_column_map(large, low)


@pytest.mark.parametrize("reg", [dict(), dict(ridge_3b=1e-8), dict(ridge_1b=1e-4, ridge_2b=1e-6, ridge_3b=1e-5,
                                                                    curvature_2b=1e-3, curvature_3b=1e-7),
                                 dict(curvature_2b=0.0, curvature_3b=0.0, ridge_2b=2.5),
                                 dict(ridge_map={3: 1e-3}, curvature_map={2: 0.1})])
def test_regulariser_pieces_sum_to_r_transpose_r(reg):
    for basis in (_basis("mow_config_1", rmax_2b=4.81, rmax_3b=3.2), _basis("w_notebook")):
        mask = least_squares.get_freezing_mask(basis.n_feats, basis.col_idx)
        r = least_squares.freeze_regularizer(basis.get_regularization_matrix(**reg), mask)
        want = r.T @ r
        got = optimize.regularizer_from_pieces(optimize.regularizer_pieces(basis), len(mask),
                                               optimize.resolve_regularizer(reg))
        assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()


def test_default_folds_and_explicit_fold_ids():
    for n, k in ((10, 3), (64, 5), (4, 5)):
        ids = optimize.fold_ids(n, k)
        want = np.concatenate([np.full(len(p), i) for i, p in enumerate(np.array_split(np.arange(n), k))])
        np.testing.assert_array_equal(ids, want)
    scan = optimize.CutoffScan.__new__(optimize.CutoffScan)     # (fold bookkeeping only: no featuriser, no device)
    scan.n_folds, scan.with_forces, scan._calls = 3, False, []
    scan._slots = scan._host_slots = None
    frames = [object()] * 7
    scan.add_frames(frames[:4], np.zeros(4))
    scan.add_frames(frames[4:], np.zeros(3))
    np.testing.assert_array_equal(scan.fold_of_frames(), [0, 0, 0, 1, 1, 2, 2])
    with pytest.raises(ValueError):
        scan.add_frames(frames[:2], np.zeros(2), folds=[0, 1])
    scan._calls = []
    scan.add_frames(frames[:3], np.zeros(3), folds=[2, 0, 2])
    scan.add_frames(frames[:2], np.zeros(2), folds=np.array([1, 1]))
    np.testing.assert_array_equal(scan.fold_of_frames(), [2, 0, 2, 1, 1])
    with pytest.raises(ValueError):
        scan.add_frames(frames[:1], np.zeros(1), folds=[3])
    with pytest.raises(ValueError):
        scan.add_frames(frames[:1], np.zeros(1))


def test_scan_result_model_places_coefficients_through_the_frozen_mask():
    large = _basis("mow_config_1")
    low = optimize.lower_basis(large, 4.81, 3.2)
    cols = optimize.lower_column_map(large, low)
    mask = least_squares.get_freezing_mask(low.n_feats, low.col_idx)
    x = np.arange(1, len(mask) + 1, dtype=float)

    class _Scan:                                                 # (training Gram column sums: every column covered)
        @staticmethod
        def _train_colsum(c, fold, ae, af):
            return np.ones(len(c))

    reg = dict(ridge_3b=1e-8)
    res = optimize.ScanResult(_Scan(), None, [low], [reg], [cols], [(0, 0, -1, 1.0, 0.0)], [x])
    model = res.model(0)
    assert model.bspline_config is low
    np.testing.assert_array_equal(model.coefficients[mask], x)
    np.testing.assert_array_equal(model.coefficients[low.col_idx], 0.0)
    np.testing.assert_array_equal(model.regularizer, low.get_regularization_matrix(**reg))
    assert model.data_coverage[mask].all() and not model.data_coverage[low.col_idx].any()


def test_scan_rejects_bases_get_bspline_config_could_not_make():
    from uf3_amd.representation import bspline
    cs = composition.ChemicalSystem(["W"], degree=3)
    with pytest.raises(ValueError):
        optimize.check_scan_basis(bspline.BSplineBasis(cs, r_min_map={("W", "W"): 1.0}, r_max_map={("W", "W"): 6.0},
                                                       resolution_map={("W", "W"): 10}))
    large = _basis("mow_config_1")
    with pytest.raises(ValueError, match="not a knot"):
        optimize.lower_basis(large, 0.01, 3.2)
    with pytest.raises(ValueError, match="not a knot"):
        optimize.lower_basis(large, 4.81, 0.8)
