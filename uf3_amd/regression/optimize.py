"""
Cut-off and regulariser scans (reference: ``uf3/regression/optimize.py``, the helpers :12-292, and the workflow of
``examples/tungsten_extxyz/radial_cutoff_hyperparameter_optimization_example.ipynb``).

Host side: ``get_bspline_config``, ``get_lower_cutoffs``, ``get_columns_to_drop_2b`` / ``_3b`` with the reference's
names, arguments, results and ``ValueError`` conditions, and ``lower_column_map``, the positional form of the column drop
the device path works with.

Device side: ``CutoffScan`` featurises every frame once at the largest cut-offs into one ``DeviceFitAccumulator`` per fold
and solves every (lower basis, regulariser, fold) system from those pieces in batched fp64 launches
(``uf3_scan_solve_dev``).  A lower basis on the same uniform knots is a column drop of the large one (its feature rows are
the large rows at the kept columns), so its normal equations are index-mapped sub-matrices of the large Grams, and the
squared error of any coefficient vector on any set of frames follows from that set's pieces:
``SSE = c^T G c - 2 c^T o + sum(y^2)``.
"""
import re

import numpy as np

from uf3_amd import _lib
from uf3_amd.representation import bspline
from uf3_amd.regression import least_squares, regularize

REG_KEYS = ("ridge_1b", "ridge_2b", "ridge_3b", "curvature_2b", "curvature_3b")


# ------------------------------------------------------------------------------------------------ the reference's helpers
def _on_grid(span, spacing):
    rest = span % spacing
    return np.isclose(rest, spacing) or np.isclose(rest, 0)


def get_bspline_config(chemical_system, rmin_2b, rmin_3b, rmax_2b, rmax_3b, knot_spacing_2b, knot_spacing_3b,
                       leading_trim, trailing_trim):
    """Basis on uniform knots whose lower cut-offs are column drops of it (optimize.py:12-145).  rmax_3b is the cut-off of
    the two legs that meet at the centre; the third leg runs to 2 rmax_3b."""
    if not _on_grid(rmax_2b - rmin_2b, knot_spacing_2b):
        raise ValueError("Provided rmax_2b does not conatin integer number of\n\
                knots, seperated by knot_spacing_2b")
    if not _on_grid(rmax_3b - rmin_3b, knot_spacing_3b):
        raise ValueError("Provided rmax_3b does not conatin integer number of\n\
                knots, seperated by knot_spacing_3b")
    if leading_trim != 0:
        raise ValueError("Currrent version is only tested for leading_trim=0")
    if trailing_trim != 3:
        raise ValueError("Currrent version is only tested for trailing_trim=3")
    rmax_3b_double = rmax_3b * 2
    if not _on_grid(rmax_3b_double - rmin_3b, knot_spacing_3b):
        raise ValueError(
            "Provided (rmax_3b-rmin_3b) contains integer number of knots \n\
                sperated by knot_spacing_3b, but rmax_3b_double does not. \n\
                Consider changing rmin_3b, rmax_3b, knot_spacing_3b so that \n\
                the following conditions are satisfied- \n\
                --(rmax_3b - rmin_3b)/knot_spacing_3b == integer \n\
                --(rmax_3b_double - rmin_3b)//knot_spacing_3b == integer, \n\
                    where rmax_3b_double = 2*rmax_3b, calculated internally"
        )
    reso_2b = round((rmax_2b - rmin_2b) / knot_spacing_2b)
    reso_3b = round((rmax_3b - rmin_3b) / knot_spacing_3b)
    reso_3b_double = round((rmax_3b_double - rmin_3b) / knot_spacing_3b)
    pairs, trios = chemical_system.interactions_map[2], chemical_system.interactions_map[3]
    r_min_map = {**{p: rmin_2b for p in pairs}, **{t: [rmin_3b] * 3 for t in trios}}
    r_max_map = {**{p: rmax_2b for p in pairs}, **{t: [rmax_3b, rmax_3b, rmax_3b_double] for t in trios}}
    resolution_map = {**{p: reso_2b for p in pairs}, **{t: [reso_3b, reso_3b, reso_3b_double] for t in trios}}
    return bspline.BSplineBasis(chemical_system, r_min_map=r_min_map, r_max_map=r_max_map, resolution_map=resolution_map,
                                trailing_trim=trailing_trim, leading_trim=leading_trim)


def get_lower_cutoffs(original_bspline_config):
    """{"lower_rmax_2b", "lower_rmax_3b"}: the cut-offs reachable by dropping columns of the original basis -- its knots
    between the first interior one and the end, taken from the first pair and the first trio (optimize.py:148-183)."""
    basis = original_bspline_config
    pair, trio = basis.interactions_map[2][0], basis.interactions_map[3][0]
    lower_rmax_2b = basis.knots_map[pair][4:-3]
    lower_rmax_3b = basis.knots_map[trio][0][4:-3]
    if not all(r in basis.knots_map[pair] for r in lower_rmax_2b):
        raise ValueError("Internal check failed-->2B!!")
    if not all(r in basis.knots_map[trio][0] for r in lower_rmax_3b):
        raise ValueError("Internal check failed-->3B_0!!")
    if not all(r in basis.knots_map[trio][1] for r in lower_rmax_3b):
        raise ValueError("Internal check failed-->3B_1!!")
    return {"lower_rmax_2b": lower_rmax_2b, "lower_rmax_3b": lower_rmax_3b}


def _check_trims(basis, degree):
    if basis.leading_trim[degree] != 0:
        raise ValueError("Currrent version is only tested for leading_trim=0")
    if basis.trailing_trim[degree] != 3:
        raise ValueError("Currrent version is only tested for trailing_trim=3")


def get_columns_to_drop_2b(original_bspline_config, modify_2b_cutoff, knot_spacing_2b):
    """Names of the pair columns to drop for a 2-body cut-off of ``modify_2b_cutoff`` (optimize.py:186-233): in every pair
    block, the functions between the new and the old end, the three trimmed ones at the end staying."""
    basis = original_bspline_config
    _check_trims(basis, 2)
    names = basis.get_column_names()
    sizes, offsets = basis.get_interaction_partitions()
    out = []
    for pair in basis.interactions_map[2]:
        knots = basis.knots_map[pair]
        if modify_2b_cutoff not in knots:
            raise ValueError("Provided modify_2b_cutoff is not a knot in the %s interaction" % (str(pair),))
        n_drop = round((knots[-4] - modify_2b_cutoff) / knot_spacing_2b)
        end = 1 + offsets[pair] + sizes[pair]              # (names[0] is the target column "y")
        out.extend(names[end - n_drop - 3:end - 3])
    return out


def _trio_drop_positions(basis, trio, n_drop):
    """Positions within the trio block of the columns a 3-body cut-off n_drop knots lower removes: (l, m, n) grid of
    the block's columns, the n_drop planes before the trimmed ends of l and m and the 2 n_drop ones of n deleted."""
    L, M, N = (len(s) - 4 for s in basis.knots_map[trio])
    grid = -np.ones(L * M * N, dtype=np.int64)
    mask = basis.template_mask[trio]
    grid[mask] = np.arange(len(mask))
    grid = grid.reshape(L, M, N)
    for axis, n in ((2, 2 * n_drop), (1, n_drop), (0, n_drop)):
        size = grid.shape[axis]
        grid = np.delete(grid, np.s_[size - 3 - n:size - 3], axis=axis)
    kept = grid[grid >= 0]
    return np.setdiff1d(np.arange(len(mask)), kept)


def get_columns_to_drop_3b(original_bspline_config, modify_3b_cutoff, knot_spacing_3b):
    """Names of the trio columns to drop for a 3-body cut-off of ``modify_3b_cutoff`` (optimize.py:236-292), per trio in
    the reference's order (np.setdiff1d of the names: sorted as strings)."""
    basis = original_bspline_config
    _check_trims(basis, 3)
    names = basis.get_column_names()
    sizes, offsets = basis.get_interaction_partitions()
    out = []
    for trio in basis.interactions_map[3]:
        for leg, (a, b) in enumerate(((trio[0], trio[1]), (trio[0], trio[2]))):
            if modify_3b_cutoff not in basis.knots_map[trio][leg]:
                raise ValueError("Provided modify_3b_cutoff is not a knot in %s leg of %s interaction"
                                 % (str((a, b)), str(trio)))
        n_drop = round((basis.knots_map[trio][0][-4] - modify_3b_cutoff) / knot_spacing_3b)
        start = 1 + offsets[trio]
        block = np.asarray(names[start:start + sizes[trio]])
        drop = block[_trio_drop_positions(basis, trio, int(n_drop))]
        out.extend(str(name) for name in np.sort(drop))
    return out


# ------------------------------------------------------------------------------------------------ lower bases as column maps
def _uniform_settings(basis):
    """(rmin_2b, rmin_3b, rmax_2b, rmax_3b, spacing_2b, spacing_3b) read off a basis' knots (first pair, first trio)."""
    pair = basis.interactions_map[2][0]
    k2 = np.asarray(basis.knots_map[pair])
    out = [k2[0], None, k2[-1], None, k2[4] - k2[3], None]
    if basis.degree > 2 and basis.interactions_map.get(3):
        k3 = np.asarray(basis.knots_map[basis.interactions_map[3][0]][0])
        out[1], out[3], out[5] = k3[0], k3[-1], k3[4] - k3[3]
    return tuple(out)


def _knots_equal(a, b, rtol=1e-12):
    for key in set(a) | set(b):
        if key not in a or key not in b:
            return False
        va, vb = a[key], b[key]
        seqs_a = va if len(key) == 3 else [va]
        seqs_b = vb if len(key) == 3 else [vb]
        for sa, sb in zip(seqs_a, seqs_b):
            sa, sb = np.asarray(sa, dtype=float), np.asarray(sb, dtype=float)
            if sa.shape != sb.shape or not np.allclose(sa, sb, rtol=rtol, atol=rtol):
                return False
    return True


def check_scan_basis(basis):
    """Raise (with the reference's messages where it has one) unless ``basis`` is one ``get_bspline_config`` makes: two- and
    three-body, uniform knots, leading trim 0, trailing trim 3."""
    if basis.degree != 3 or not basis.interactions_map.get(3):
        raise ValueError("cut-off scans need a basis with two- and three-body terms (get_bspline_config)")
    _check_trims(basis, 2)
    _check_trims(basis, 3)
    rmin_2b, rmin_3b, rmax_2b, rmax_3b, s2, s3 = _uniform_settings(basis)
    again = get_bspline_config(basis.chemical_system, rmin_2b, rmin_3b, rmax_2b, rmax_3b, s2, s3, 0, 3)
    if not _knots_equal(again.knots_map, basis.knots_map):
        raise ValueError("the basis' knots are not those get_bspline_config makes (uniform knots, every pair on one sequence, "
                         "every trio on (rmax_3b, rmax_3b, 2 rmax_3b))")
    return rmin_2b, rmin_3b, rmax_2b, rmax_3b, s2, s3


def lower_basis(original, rmax_2b, rmax_3b):
    """The basis ``get_bspline_config`` makes for the cut-offs (rmax_2b, rmax_3b) on the original basis' knots.  Raises
    unless both are lower cut-offs of the original (``get_lower_cutoffs``)."""
    rmin_2b, rmin_3b, _, _, s2, s3 = check_scan_basis(original)
    low = get_lower_cutoffs(original)
    pair, trio = original.interactions_map[2][0], original.interactions_map[3][0]
    if not np.any(low["lower_rmax_2b"] == rmax_2b):
        raise ValueError("Provided modify_2b_cutoff is not a knot in the %s interaction" % (str(pair),))
    if not np.any(low["lower_rmax_3b"] == rmax_3b):
        raise ValueError("Provided modify_3b_cutoff is not a knot in %s leg of %s interaction"
                         % (str((trio[0], trio[1])), str(trio)))
    return get_bspline_config(original.chemical_system, rmin_2b, rmin_3b, rmax_2b, rmax_3b, s2, s3, 0, 3)


def lower_column_map(original, lower):
    """
    int64 positions, among the ORIGINAL basis' unfrozen columns, of the LOWER basis' unfrozen columns, in the lower basis'
    order.  Derived from ``get_columns_to_drop_2b`` / ``_3b`` (positional: the lower basis numbers its columns afresh).

    Raises ValueError unless the lower basis is a column drop of the original -- same elements, knot spacing, r_min and
    trims, lower cut-offs on the original's knots --, every frozen column of the lower basis lands on a frozen column of
    the original with the same value, and every frozen column the drop removes is pinned to zero.  Those are the
    conditions under which folding the frozen columns out on the Gram level (``DeviceFitAccumulator.packed``) commutes with
    the drop.
    """
    if tuple(original.element_list) != tuple(lower.element_list) or original.degree != lower.degree:
        raise ValueError("the lower basis has another chemical system than the original")
    if original.leading_trim != lower.leading_trim or original.trailing_trim != lower.trailing_trim:
        raise ValueError("the lower basis has other trims than the original")
    if original.offset_1b != lower.offset_1b:
        raise ValueError("the lower basis treats the one-body columns differently from the original")
    rmin_2b, rmin_3b, _, _, s2, s3 = check_scan_basis(original)
    _, _, r2, r3, _, _ = _uniform_settings(lower)
    try:
        expect = lower_basis(original, r2, r3)
    except ValueError as exc:
        raise ValueError(f"the lower basis is not a column drop of the original: {exc}") from None
    if not _knots_equal(expect.knots_map, lower.knots_map):
        raise ValueError("the lower basis is not a column drop of the original (knot spacing or r_min differ)")
    names = original.get_column_names()[1:]
    drop = set(get_columns_to_drop_2b(original, r2, s2)) | set(get_columns_to_drop_3b(original, r3, s3))
    kept = np.array([i for i, name in enumerate(names) if name not in drop], dtype=np.int64)
    if len(kept) != lower.n_feats:
        raise ValueError(f"the drop keeps {len(kept)} columns, the lower basis has {lower.n_feats}")
    o_frozen = np.asarray(original.col_idx, dtype=np.int64)
    o_value = dict(zip(o_frozen.tolist(), np.asarray(original.frozen_c, dtype=float).reshape(-1).tolist()))
    l_frozen = np.asarray(lower.col_idx, dtype=np.int64)
    l_values = np.asarray(lower.frozen_c, dtype=float).reshape(-1)
    for col, value in zip(kept[l_frozen].tolist(), l_values.tolist()):
        if col not in o_value:
            raise ValueError(f"frozen column of the lower basis maps onto unfrozen column {col} of the original")
        if o_value[col] != value:
            raise ValueError(f"frozen column {col}: value {value} in the lower basis, {o_value[col]} in the original")
    dropped_frozen = set(o_value) - set(kept[l_frozen].tolist())
    if any(o_value[c] != 0 for c in dropped_frozen):
        raise ValueError("a frozen column the drop removes has a non-zero value")
    o_mask = least_squares.get_freezing_mask(original.n_feats, o_frozen)
    l_mask = least_squares.get_freezing_mask(lower.n_feats, l_frozen)
    cols = kept[l_mask]
    pos = np.searchsorted(o_mask, cols)
    if np.any(pos >= len(o_mask)) or np.any(o_mask[np.minimum(pos, len(o_mask) - 1)] != cols):
        raise ValueError("an unfrozen column of the lower basis maps onto a frozen column of the original")
    return pos.astype(np.int64)


# ------------------------------------------------------------------------------------------------ regulariser pieces
def resolve_regularizer(reg):
    """The five strengths ``basis.get_regularization_matrix(**reg)`` uses (keys REG_KEYS): unspecified ones take
    ``DEFAULT_REGULARIZER_GRID``; ``ridge_map`` / ``curvature_map`` and keyword spellings as that method parses them."""
    reg = dict(reg or {})
    ridge_map = dict(reg.pop("ridge_map", None) or {})
    curvature_map = dict(reg.pop("curvature_map", None) or {})
    for k, v in reg.items():
        order = int(re.sub('[^0-9]', '', k))
        if k.lower()[0] == 'r':
            ridge_map[order] = float(v)
        elif k.lower()[0] == 'c':
            curvature_map[order] = float(v)
    d = regularize.DEFAULT_REGULARIZER_GRID
    ridge_map = {1: d["ridge_1b"], 2: d["ridge_2b"], 3: d["ridge_3b"], **ridge_map}
    curvature_map = {2: d["curve_2b"], 3: d["curve_3b"], **curvature_map}
    return dict(ridge_1b=float(ridge_map[1]), ridge_2b=float(ridge_map[2]), ridge_3b=float(ridge_map[3]),
                curvature_2b=float(curvature_map[2]), curvature_3b=float(curvature_map[3]))


def regularizer_pieces(basis):
    """The unit pieces P_k = R_k^T R_k of the five families (REG_KEYS) on the unfrozen columns, as one COO pattern:
    (rows, cols, values [nnz][5]).  R_k is ``get_regularization_matrix`` with strength 1 for family k and 0 for the others
    (curvature rows exist only for a strength > 0), restricted through ``freeze_regularizer``'s mask; R^T R is linear in
    the strengths, so sum_k lambda_k P_k is the regulariser of any strength setting."""
    from scipy import sparse
    mask = least_squares.get_freezing_mask(basis.n_feats, basis.col_idx)
    zero = {k: 0.0 for k in REG_KEYS}
    mats = []
    for k in REG_KEYS:
        r = least_squares.freeze_regularizer(basis.get_regularization_matrix(**{**zero, k: 1.0}), mask)
        r = sparse.csr_matrix(r)
        mats.append((r.T @ r).tocsr())
    pattern = sum(abs(m) for m in mats).tocoo()
    rows, cols = pattern.row.astype(np.int32), pattern.col.astype(np.int32)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    values = np.stack([np.asarray(m[rows, cols]).reshape(-1) for m in mats], axis=1)
    return rows, cols, np.ascontiguousarray(values)


def regularizer_from_pieces(pieces, n, strengths):
    """Dense sum_k lambda_k P_k (n x n) of ``regularizer_pieces``; ``strengths`` as ``resolve_regularizer`` returns."""
    rows, cols, values = pieces
    lam = np.array([strengths[k] for k in REG_KEYS])
    out = np.zeros((n, n))
    np.add.at(out, (rows, cols), values @ lam)
    return out


# ------------------------------------------------------------------------------------------------ folds
def fold_ids(n_frames, n_folds):
    """Default fold of every frame: ``np.array_split`` of the frame order into n_folds (the notebook's split)."""
    out = np.empty(n_frames, dtype=np.int64)
    for k, part in enumerate(np.array_split(np.arange(n_frames), n_folds)):
        out[part] = k
    return out


# ------------------------------------------------------------------------------------------------ the device scan
def _weights(m_e, m_f, weight, with_forces):
    """(alpha_e, alpha_f) of ``fit_from_pieces`` on training moments m_e / m_f (n, sum, sum of squares)."""
    if not with_forces:
        return 1.0, 0.0
    w_e, w_f = least_squares.calc_E_F_weights(m_e[0], m_f[0], least_squares.std_from_moments(m_e),
                                              least_squares.std_from_moments(m_f))
    return weight * w_e ** 2, (1 - weight) * w_f ** 2


def _rmse(sse, n):
    # (SSE = c^T G c - 2 c^T o + sum y^2 cancels: at a near-exact fit rounding of order eps * sum y^2 can leave it slightly
    # negative; it is clamped to 0)
    return float(np.sqrt(max(sse, 0.0) / n)) if n > 0 and np.isfinite(sse) else float("nan")


class ScanResult:
    """Outcome of ``CutoffScan.run``: ``table`` (one row per system) and ``model(i)`` (the fit of row i)."""

    def __init__(self, scan, table, bases, regs, maps, systems, coefficients):
        self._scan, self.table, self._bases, self._regs, self._maps = scan, table, bases, regs, maps
        self._systems, self._coefficients = systems, coefficients

    def __len__(self):
        return len(self.table)

    def coefficients(self, i):
        """Solution of row i on the lower basis' unfrozen columns."""
        return self._coefficients[i]

    def model(self, i):
        """``WeightedLinearModel`` of row i: the lower basis, its regulariser ``get_regularization_matrix(**reg)``, the
        coefficients with the frozen ones put back (``revert_frozen_coefficients``) and ``data_coverage`` as
        ``fit_with_gram`` sets it (columns whose training Gram column is not zero)."""
        b, r, fold, alpha_e, alpha_f = self._systems[i]
        basis = self._bases[b]
        model = least_squares.WeightedLinearModel(basis, regularizer=basis.get_regularization_matrix(**self._regs[r]))
        mask = least_squares.get_freezing_mask(basis.n_feats, basis.col_idx)
        model.coefficients = least_squares.revert_frozen_coefficients(
            np.asarray(self._coefficients[i], dtype=float), basis.n_feats, mask, basis.frozen_c, basis.col_idx)
        colsum = self._scan._train_colsum(self._maps[b], fold, alpha_e, alpha_f)
        coverage = least_squares.revert_frozen_coefficients(colsum != 0, basis.n_feats, mask, basis.frozen_c, basis.col_idx)
        model.data_coverage = np.logical_or(model.data_coverage, coverage)
        return model


class CutoffScan:
    """
    Cut-off and regulariser scan with k-fold validation from one featurisation (the notebook's loop of ``fit_from_file`` /
    ``batched_predict`` with ``drop_columns``, without rebuilding anything per cut-off or fold).

        scan = CutoffScan(featurizer_of_large_basis, n_folds=5, weight=0.5, with_forces=True)
        scan.add_frames(frames, energies, forces, folds=None)      # any number of calls
        res = scan.run(cutoffs=None, regularizers=[dict(ridge_3b=1e-8), ...])
        res.table, res.model(i)

    Frames are featurised once, at the large basis' cut-offs, into one ``DeviceFitAccumulator`` per fold (the first
    ``run``; frames added later start the accumulation over).  Folds: ``np.array_split`` of the frame order over all
    calls, or an integer fold id per frame given with every call.  Each system (lower basis, regulariser, held-out fold or
    -1 for all data) is assembled, solved and scored on the device from the fold slots (``uf3_scan_solve_dev``); one whose
    Cholesky factorisation fails is solved again on the host with ``np.linalg.solve`` on the same A and b and flagged
    ``solver = "host"``.
    """

    def __init__(self, featurizer, n_folds=5, weight=0.5, with_forces=True, max_atoms_per_chunk=320000):
        self.fz = featurizer
        self.basis = featurizer.bspline_config
        self.settings = check_scan_basis(self.basis)
        if np.any(np.asarray(self.basis.frozen_c, dtype=float) != 0):
            raise ValueError("cut-off scans need the frozen columns pinned to 0 (as get_bspline_config makes them)")
        self.n_folds = int(n_folds)
        if not 1 <= self.n_folds <= 32:
            raise ValueError("n_folds must lie in 1 .. 32")
        self.weight, self.with_forces = float(weight), bool(with_forces)
        self.max_atoms = int(max_atoms_per_chunk)
        self.model = least_squares.WeightedLinearModel(self.basis, regularizer=np.zeros((0, self.basis.n_feats)))
        self._calls = []              # (frames, energies, forces, folds or None)
        self._slots = None
        self._host_slots = None
        self.timing = {}

    # -- data -------------------------------------------------------------------------------------------------------------
    def add_frames(self, frames, energies, forces=None, folds=None):
        frames = list(frames)
        energies = np.asarray(energies, dtype=float).reshape(-1)
        if len(energies) != len(frames):
            raise ValueError("one energy per frame")
        if self.with_forces and forces is None and len(frames):
            raise ValueError("this scan fits forces: pass them")
        if folds is not None:
            folds = np.asarray(folds).reshape(-1)
            if len(folds) != len(frames) or not np.issubdtype(folds.dtype, np.integer):
                raise ValueError("folds: one integer fold id per frame")
            if len(folds) and (folds.min() < 0 or folds.max() >= self.n_folds):
                raise ValueError(f"fold ids must lie in 0 .. {self.n_folds - 1}")
        if self._calls and (folds is None) != (self._calls[0][3] is None):
            raise ValueError("give fold ids with every call or with none")
        self._calls.append((frames, energies, None if forces is None else list(forces), folds))
        self._slots = self._host_slots = None

    def fold_of_frames(self):
        """Fold id of every frame added so far, in order."""
        n = sum(len(c[0]) for c in self._calls)
        if not self._calls or self._calls[0][3] is None:
            return fold_ids(n, self.n_folds)
        return np.concatenate([c[3] for c in self._calls]).astype(np.int64)

    def _accumulate(self):
        import time
        import torch
        from uf3_amd import pipeline
        folds = self.fold_of_frames()
        frames = [a for c in self._calls for a in c[0]]
        energies = np.concatenate([c[1] for c in self._calls]) if self._calls else np.zeros(0)
        forces = [f for c in self._calls for f in c[2]] if self.with_forces else None
        t0 = time.perf_counter()
        slots = None
        for k in range(self.n_folds):
            pick = np.flatnonzero(folds == k)
            acc = pipeline.DeviceFitAccumulator(self.model, self.fz, with_forces=self.with_forces,
                                                max_atoms_per_chunk=self.max_atoms)
            attempt = 0
            while True:                 # (the retry protocol of pipeline.fit_frames)
                try:
                    acc.add_frames([frames[i] for i in pick], energies[pick],
                                   [forces[i] for i in pick] if self.with_forces else None)
                    flat = acc.packed()
                    break
                except _lib.UF3Error as exc:
                    try:
                        acc.ctx.synchronize()
                    except _lib.UF3Error:
                        pass
                    acc.reset()
                    attempt += 1
                    if not isinstance(exc, _lib.RetryError) or attempt >= 16:
                        raise
            if slots is None:
                slots = torch.empty((self.n_folds, flat.numel()), dtype=torch.float64, device=flat.device)
                self.ctx, self.dev = acc.ctx, acc.dev
            slots[k].copy_(flat)
        torch.cuda.synchronize(self.dev)
        self.timing["accumulate_s"] = time.perf_counter() - t0
        self._slots = slots
        self.n_cols = int(acc._keep.numel())
        n = self.n_cols
        mom = slots[:, 2 * n * n + 2 * n:].cpu().numpy()
        self._m_e, self._m_f = mom[:, :3], mom[:, 3:]

    def slots(self):
        """Device tensor [n_folds][2 F'^2 + 2 F' + 6]: the packed pieces of every fold (``DeviceFitAccumulator.packed``)."""
        if self._slots is None:
            self._accumulate()
        return self._slots

    def host_slots(self):
        if self._host_slots is None:
            self._host_slots = self.slots().cpu().numpy()
        return self._host_slots

    def _train(self, fold):
        return [f for f in range(self.n_folds) if f != fold]

    def _train_colsum(self, cols, fold, alpha_e, alpha_f):
        """Column sums of alpha_e G_e + alpha_f G_f over the training slots, restricted to ``cols`` (rows and columns)."""
        import torch
        n = self.n_cols
        slots = self.slots()
        keep = torch.tensor(self._train(fold), dtype=torch.int64, device=slots.device)
        idx = torch.as_tensor(np.asarray(cols, dtype=np.int64), device=slots.device)
        g = slots.index_select(0, keep)[:, :2 * n * n].sum(0).view(2, n, n)
        g = alpha_e * g[0] + alpha_f * g[1]
        return g.index_select(0, idx).index_select(1, idx).sum(0).cpu().numpy()

    def host_system(self, cols, pieces, fold, alpha_e, alpha_f, strengths):
        """A and b of one system, assembled on the host from the fold slots (the host route, for comparisons)."""
        n = self.n_cols
        s = self.host_slots()[self._train(fold)].sum(0)
        ge, gf = s[:n * n].reshape(n, n), s[n * n:2 * n * n].reshape(n, n)
        oe, of = s[2 * n * n:2 * n * n + n], s[2 * n * n + n:2 * n * n + 2 * n]
        ix = np.ix_(cols, cols)
        a = alpha_e * ge[ix] + alpha_f * gf[ix] + regularizer_from_pieces(pieces, len(cols), strengths)
        return a, alpha_e * oe[cols] + alpha_f * of[cols]

    def host_sse(self, cols, x, fold):
        """(train e, train f, held-out e, held-out f) squared errors of x from the fold slots, on the host."""
        n = self.n_cols
        out = np.zeros(4)
        hs = self.host_slots()
        ix = np.ix_(cols, cols)
        for f in range(self.n_folds):
            s = hs[f]
            ge, gf = s[:n * n].reshape(n, n)[ix], s[n * n:2 * n * n].reshape(n, n)[ix]
            oe, of = s[2 * n * n:2 * n * n + n][cols], s[2 * n * n + n:2 * n * n + 2 * n][cols]
            m = s[2 * n * n + 2 * n:]
            k = 2 if f == fold else 0
            out[k] += x @ ge @ x - 2 * x @ oe + m[2]
            out[k + 1] += x @ gf @ x - 2 * x @ of + m[5]
        return out

    # -- the scan -----------------------------------------------------------------------------------------------------------
    def cutoff_pairs(self):
        low = get_lower_cutoffs(self.basis)
        return [(float(r2), float(r3)) for r2 in low["lower_rmax_2b"] for r3 in low["lower_rmax_3b"]]

    def run(self, cutoffs=None, regularizers=None, workspace_bytes=2 << 30):
        """
        cutoffs: (rmax_2b, rmax_3b) pairs from ``get_lower_cutoffs`` (None: all of them); regularizers: dicts as
        ``get_regularization_matrix(**reg)`` takes them (None: one, the defaults); workspace_bytes: cap on the device
        workspace of one launch (A, its diagonal and b of every system of a batch; batches are planned on the host).

        Table columns: rmax_2b, rmax_3b, the five strengths (REG_KEYS), fold (-1: all data), n_feat (columns of the lower
        basis), n_fit (its unfrozen columns, the system size), train_rmse_e, train_rmse_f, val_rmse_e, val_rmse_f (energies
        per atom; NaN where there are no rows, e.g. held-out of fold -1), solver ("device" or "host").
        """
        import time
        import pandas as pd
        import torch
        cutoffs = self.cutoff_pairs() if cutoffs is None else [(float(a), float(b)) for a, b in cutoffs]
        regularizers = [dict()] if regularizers is None else [dict(r) for r in regularizers]
        strengths = [resolve_regularizer(r) for r in regularizers]
        slots = self.slots()
        dev = slots.device
        t0 = time.perf_counter()
        bases, maps, pieces = [], [], []
        for r2, r3 in cutoffs:
            low = lower_basis(self.basis, r2, r3)
            bases.append(low)
            maps.append(lower_column_map(self.basis, low))
            pieces.append(regularizer_pieces(low))
        sizes = np.array([len(m) for m in maps], dtype=np.int64)
        col_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        nnz = np.array([len(p[0]) for p in pieces], dtype=np.int64)
        reg_off = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
        to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
        d_cols = to_dev(np.concatenate(maps).astype(np.int32))
        d_col_off = to_dev(col_off)
        d_reg_rc = to_dev(np.concatenate([np.stack([p[0], p[1]], axis=1) for p in pieces]).astype(np.int32).reshape(-1, 2))
        d_reg_v = to_dev(np.concatenate([p[2] for p in pieces]).reshape(-1, 5))
        d_reg_off = to_dev(reg_off)
        # systems: (basis, regulariser, fold, alpha_e, alpha_f); the weights from each training set's moments
        systems = []
        for b in range(len(bases)):
            for r in range(len(regularizers)):
                for fold in [-1] + list(range(self.n_folds)):
                    tr = self._train(fold)
                    ae, af = _weights(self._m_e[tr].sum(0), self._m_f[tr].sum(0), self.weight, self.with_forces)
                    systems.append((b, r, fold, ae, af))
        self.timing["prepare_s"] = time.perf_counter() - t0
        # batches: consecutive systems while their workspace (m^2 + 2m doubles each) fits the cap
        cap = int(workspace_bytes) // 8
        batches, cur, used = [], [], 0
        for i, (b, _, _, _, _) in enumerate(systems):
            need = int(sizes[b] * sizes[b] + 2 * sizes[b])
            if need > cap:
                raise ValueError(f"one system needs {8 * need} bytes of workspace, above workspace_bytes={workspace_bytes}")
            if used + need > cap:
                batches.append(cur)
                cur, used = [], 0
            cur.append(i)
            used += need
        if cur:
            batches.append(cur)
        n_sys = len(systems)
        sse = np.zeros((n_sys, 4))
        status = np.zeros(n_sys, dtype=np.int32)
        coefficients = [None] * n_sys
        ws = torch.empty(max((sum(int(sizes[systems[i][0]] ** 2 + 2 * sizes[systems[i][0]]) for i in bt) for bt in batches),
                             default=1), dtype=torch.float64, device=dev)
        t0 = time.perf_counter()
        n_host = 0
        stream = torch.cuda.current_stream(dev)
        for bt in batches:
            sys = np.zeros((len(bt), 6), dtype=np.int64)
            w = np.zeros((len(bt), 7))
            ws_off = x_off = 0
            for q, i in enumerate(bt):
                b, r, fold, ae, af = systems[i]
                m = int(sizes[b])
                sys[q] = (b, fold, ws_off, x_off, x_off, 0)
                w[q] = [ae, af] + [strengths[r][k] for k in REG_KEYS]
                ws_off += m * m + 2 * m
                x_off += m
            d_sys, d_w = to_dev(sys), to_dev(w)
            d_x = torch.empty(max(x_off, 1), dtype=torch.float64, device=dev)
            d_sse = torch.empty((len(bt), 4), dtype=torch.float64, device=dev)
            d_status = torch.empty(len(bt), dtype=torch.int32, device=dev)
            prev = self.ctx.set_stream(stream.cuda_stream)
            try:
                _lib.scan_solve_dev(self.ctx, self.n_cols, self.n_folds, slots.data_ptr(), d_cols.data_ptr(),
                                    d_col_off.data_ptr(), d_reg_rc.data_ptr() if len(d_reg_rc) else 0, d_reg_v.data_ptr()
                                    if len(d_reg_v) else 0, d_reg_off.data_ptr(), len(bt), x_off, d_sys.data_ptr(),
                                    d_w.data_ptr(), ws.data_ptr(), ws.numel(), d_x.data_ptr(), d_x.numel(),
                                    d_sse.data_ptr(), d_status.data_ptr())
            finally:
                self.ctx.restore_stream(prev)
            x_h, sse_h, st_h = d_x.cpu().numpy(), d_sse.cpu().numpy(), d_status.cpu().numpy()
            if np.any(st_h < 0):
                raise _lib.UF3Error(1, f"uf3_scan_solve_dev: bad system records (status {st_h[st_h < 0][0]})")
            for q, i in enumerate(bt):
                b = systems[i][0]
                m = int(sizes[b])
                status[i], sse[i] = st_h[q], sse_h[q]
                coefficients[i] = x_h[sys[q, 3]:sys[q, 3] + m].copy()
                if st_h[q] != 0:     # the same A and b, from the workspace: strict upper triangle, saved diagonal, rhs
                    n_host += 1
                    seg = ws[sys[q, 2]:sys[q, 2] + m * m + 2 * m].cpu().numpy()
                    up = np.triu(seg[:m * m].reshape(m, m), 1)
                    a = up + up.T + np.diag(seg[m * m:m * m + m])
                    try:
                        x = np.linalg.solve(a, seg[m * m + m:])
                        coefficients[i] = x
                        sse[i] = self.host_sse(maps[b], x, systems[i][2])
                    except np.linalg.LinAlgError:
                        coefficients[i] = np.full(m, np.nan)
                        sse[i] = np.nan
        self.timing["solve_s"] = time.perf_counter() - t0
        self.timing["n_batches"] = len(batches)
        self.timing["n_host"] = n_host
        rows = []
        for i, (b, r, fold, ae, af) in enumerate(systems):
            tr = self._train(fold)
            held = [fold] if fold >= 0 else []
            n_e_tr, n_f_tr = self._m_e[tr, 0].sum(), self._m_f[tr, 0].sum()
            n_e_va, n_f_va = self._m_e[held, 0].sum(), self._m_f[held, 0].sum()
            r2, r3 = cutoffs[b]
            row = dict(rmax_2b=r2, rmax_3b=r3, **strengths[r], fold=fold, n_feat=bases[b].n_feats, n_fit=int(sizes[b]),
                       train_rmse_e=_rmse(sse[i, 0], n_e_tr),
                       train_rmse_f=_rmse(sse[i, 1], n_f_tr) if self.with_forces else float("nan"),
                       val_rmse_e=_rmse(sse[i, 2], n_e_va),
                       val_rmse_f=_rmse(sse[i, 3], n_f_va) if self.with_forces else float("nan"),
                       solver="device" if status[i] == 0 else "host")
            rows.append(row)
        table = pd.DataFrame(rows)
        self.last_status, self.last_sse = status, sse
        return ScanResult(self, table, bases, regularizers, maps, [(b, r, fold, ae, af) for b, r, fold, ae, af in systems],
                          coefficients)
