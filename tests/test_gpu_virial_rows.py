"""
Virial rows of the featurizer (``uf3_featurize_virial[_dev]``, ``BasisFeaturizer.featurize_virials``: x_v [n_frames, 6, F], the
strain derivative of the energy row in the convention of ``uf3_eval_virial``) and stress targets in the device fit.

The rows are held against the oracle's strain derivative (pinned to finite differences of its own energy in
tests/test_oracle_virial.py, whose cases are imported here) through coefficient vectors and column by column, against strain
differences of the featurizer's own energy rows, across frame boundaries of ragged batches, on the route that adds straight to
HBM, and under lattice translations of single atoms.
"""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import _lib, pipeline, synthetic
from uf3_amd.data import composition
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator
from uf3_amd.regression import least_squares as ls
from uf3_amd.representation import bspline, process
from _util import worst_elementwise
from test_oracle_virial import CASES, FD_TOL, H, VOIGT, _assert_clear_of_cuts, _case, _random_coeff, _strain, _strained

pytestmark = pytest.mark.gpu
MOW, NUMS = ['Mo', 'W'], [42, 74]


def _rows(basis, frames, energy=False):
    return process.BasisFeaturizer(basis).featurize_virials(frames, energy=energy)


def _all_rows(basis, frames):
    """(x_e, x_f, x_v) of one uf3_featurize_virial call"""
    fz = process.BasisFeaturizer(basis)
    ctx, db = fz._dev()
    batch = _lib.FrameBatch(frames)
    F = db.n_feat
    x_e, x_f, x_v = np.empty((len(frames), F)), np.empty((batch.n_atoms, 3, F)), np.empty((len(frames), 6, F))
    ctx.check(ctx.lib.uf3_featurize_virial(db.handle, C.byref(batch.struct), _lib._p(batch.pos), _lib._p(batch.z),
                                           _lib._p(x_e), _lib._p(x_f), _lib._p(x_v)))
    return x_e, x_f, x_v


def _against_oracle_through_coefficients(basis, atoms, seed, x_v, label):
    ob = O.OracleBasis(basis)
    worst = 0.0
    for k in range(4):
        c = _random_coeff(basis, seed + k)
        v_o = O.evaluate(ob, atoms, c, virial=True)[2]
        w = worst_elementwise(x_v @ c, v_o, rtol=1e-9, floor=1e-11)
        worst = max(worst, w)
    print(f"\n{label}: F = {basis.n_feats}, worst_elementwise(x_v @ c, oracle; 1e-9, 1e-11) = {worst:.2e}")
    assert worst <= 1.0, label


@pytest.mark.parametrize("name", CASES)
def test_rows_against_the_oracle_through_coefficients(name):
    """x_v[0] @ c is the oracle's strain derivative for four coefficient vectors (frozen entries zero), the bound of
    tests/test_gpu_virial.py."""
    basis, atoms, seed = _case(name)
    x_v = _rows(basis, [atoms])
    assert x_v.shape == (1, 6, basis.n_feats) and np.all(np.isfinite(x_v))
    assert not np.any(x_v[0][:, :len(basis.element_list)])                 # one-body columns
    _against_oracle_through_coefficients(basis, atoms, seed, x_v[0], name)


@pytest.mark.parametrize("name", ["primitive_2atom", "bcc_mow_222", "two_body_only"])
def test_rows_against_the_oracle_column_by_column(name):
    """every unfrozen column k is the oracle's strain derivative for the unit vector e_k; every frozen column is exactly zero"""
    basis, atoms, _ = _case(name)
    ob = O.OracleBasis(basis)
    x_v = _rows(basis, [atoms])[0]
    frozen = np.zeros(basis.n_feats, dtype=bool)
    frozen[np.asarray(basis.col_idx, dtype=int)] = True
    assert np.all(x_v[:, frozen] == 0.0)
    ref = np.zeros_like(x_v)
    for k in np.flatnonzero(~frozen):
        e_k = np.zeros(basis.n_feats)
        e_k[k] = 1.0
        ref[:, k] = O.evaluate(ob, atoms, e_k, virial=True)[2]
    worst = worst_elementwise(x_v[:, ~frozen], ref[:, ~frozen], rtol=1e-9, floor=1e-11)
    print(f"\n{name}: {int((~frozen).sum())} unfrozen columns, worst_elementwise = {worst:.2e}")
    assert np.abs(ref).max() > 0 and worst <= 1.0


@pytest.mark.parametrize("name", ["primitive_2atom", "bcc_mow_222", "two_body_only", "triclinic"])
def test_rows_against_strain_differences_of_the_energy_rows(name):
    """Richardson pair of central differences of featurize_frames(energy=True, forces=False) on strained frames"""
    basis, atoms, _ = _case(name)
    _assert_clear_of_cuts(O.OracleBasis(basis), atoms)
    fz = process.BasisFeaturizer(basis)
    x_v = fz.featurize_virials([atoms])[0]
    frames = [_strained(atoms, _strain(i, j, s * h)) for (i, j) in VOIGT for h in H for s in (1.0, -1.0)]
    x_e = fz.featurize_frames(frames, energy=True, forces=False)[0].reshape(6, 2, 2, -1)
    d = [(x_e[:, q, 0] - x_e[:, q, 1]) / (2 * h) for q, h in enumerate(H)]
    fd = (4 * d[1] - d[0]) / 3
    err = np.abs(x_v - fd).max() / np.abs(fd).max()
    print(f"\n{name}: max|x_v - fd| / max|fd| = {err:.1e}")
    assert err <= FD_TOL


def _ragged_batch():
    cell1 = np.array([[2.9, 0.0, 0.0], [0.7, 2.8, 0.0], [0.4, -0.6, 3.1]])
    one = Atoms(numbers=[74], positions=np.array([[0.03, 0.02, 0.01]]) @ cell1, cell=cell1, pbc=True)
    two = Atoms(numbers=[42, 74], positions=np.array([[0.03, 0.02, 0.01], [0.52, 0.47, 0.55]]) @ cell1, cell=cell1, pbc=True)

    def with_pbc(a, pbc):
        return Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions(), cell=a.get_cell(), pbc=pbc)
    b16 = [synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, NUMS, seed=60 + k) for k in range(3)]
    b16[1] = with_pbc(b16[1], [True, True, False])
    b16[2] = with_pbc(b16[2], False)
    b128 = synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, NUMS, seed=70)
    b54 = with_pbc(synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, NUMS, seed=71), [True, False, True])
    return [one, two] + b16 + [b128, b54]


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_ragged_batch_and_frame_boundaries(order):
    """Many frames in one workgroup, one frame across several: every frame's block is the block of a call on that frame alone
    (only the order of summation differs); x_e and x_f beside x_v are featurize_frames' own."""
    basis = synthetic.notebook_basis(MOW)
    frames = _ragged_batch()
    assert [len(a) for a in frames] == [1, 2, 16, 16, 16, 128, 54]
    if order == "reverse":
        frames = frames[::-1]
    fz = process.BasisFeaturizer(basis)
    fz.featurize_frames(frames)                                            # (capacities settled)
    x_e, x_f, x_v = _all_rows(basis, frames)
    for k, a in enumerate(frames):
        alone = fz.featurize_virials([a])[0]
        scale = np.abs(alone).max()
        err = np.abs(x_v[k] - alone).max() / scale
        print(f"\nframe {k} ({len(a)} atoms): max|batch - alone| / max|alone| = {err:.1e}")
        assert scale > 0 and err <= 1e-12, k
    r_e, r_f, _ = fz.featurize_frames(frames)
    assert np.array_equal(x_f, r_f)
    assert np.abs(x_e - r_e).max() <= 1e-13 * np.abs(r_e).max()
    xe2, xv2 = fz.featurize_virials(frames, energy=True)
    assert np.abs(xe2 - r_e).max() <= 1e-13 * np.abs(r_e).max()
    assert np.abs(xv2 - x_v).max() <= 1e-12 * np.abs(x_v).max()


def _resolution_basis(res3, lead3=3, elements=('Mo', 'W')):
    cs = composition.ChemicalSystem(list(elements), 3)
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    return bspline.BSplineBasis(
        cs, r_min_map={**{p: 0.001 for p in pairs}, **{t: [1.5, 1.5, 1.5] for t in trios}},
        r_max_map={**{p: 5.5 for p in pairs}, **{t: [3.5, 3.5, 7.0] for t in trios}},
        resolution_map={**{p: 15 for p in pairs}, **{t: list(res3) for t in trios}},
        leading_trim={2: 0, 3: lead3}, trailing_trim={2: 3, 3: 3})


def _routes(err_text):
    """{mode: 'lds' | 'hbm'} of the launch reports on stderr"""
    return {int(m.group(1)): m.group(2) for m in re.finditer(r"uf3 virial rows mode (\d+): lds \d+ B, rows in (lds|hbm)", err_text)}


@pytest.mark.parametrize("which", ["energy_row_past_lds", "six_rows_past_lds", "rows_in_lds"])
def test_rows_straight_to_hbm(which, monkeypatch, capfd):
    """Where the six rows [6][FE] do not fit beside the launch's other LDS the adds go straight to HBM: the basis of
    test_energy_row_longer_than_lds (F = 16 770: not even the energy row fits), lead3 = 0 (F = 1798: the energy row fits, six rows
    of the 3-body columns, 6 x 1742 x 8 B = 83.6 KB, pass the 79.5 KB at which a second workgroup still fits the CU), and the
    notebook basis (F = 434) as the control on the LDS route.  The launch report says which route ran."""
    if which == "energy_row_past_lds":
        basis = _resolution_basis([9, 9, 17], lead3=0, elements=('Al', 'Cu', 'Zr'))
        assert basis.n_feats * 8 > 48 * 1024
        atoms, seed = synthetic.lattice_frame("bcc", (3, 3, 3), 3.1, [13, 29, 40], 41, rattle=0.1), 12
    elif which == "six_rows_past_lds":
        basis, atoms, seed = _case("lead3_0")
        assert basis.n_feats * 8 <= 48 * 1024
    else:
        basis, atoms, seed = _case("bcc_mow_222")
    monkeypatch.setenv("UF3_DEBUG_LDS", "1")
    capfd.readouterr()
    x_v = _rows(basis, [atoms])
    routes = _routes(capfd.readouterr().err)
    monkeypatch.delenv("UF3_DEBUG_LDS")
    print(f"\n{which}: F = {basis.n_feats}, routes {routes}")
    trio_routes = {m: r for m, r in routes.items() if m >= 1}
    assert routes.get(0) == "lds" and trio_routes
    assert set(trio_routes.values()) == ({"lds"} if which == "rows_in_lds" else {"hbm"})
    _against_oracle_through_coefficients(basis, atoms, seed, x_v[0], which)


def _window(basis, atoms):
    """fractional window [lo, hi] per axis inside which a frame's atoms are not 'far outside their cell'"""
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    normals = [np.cross(cell[1], cell[2]), np.cross(cell[2], cell[0]), np.cross(cell[0], cell[1])]
    lo, hi = np.full(3, -np.inf), np.full(3, np.inf)
    for k in np.flatnonzero(np.asarray(atoms.get_pbc(), dtype=bool)):
        h = abs(np.dot(cell[k], normals[k])) / np.linalg.norm(normals[k])
        w = np.ceil(basis.r_cut / h) + 1.0 - basis.r_cut / h - 1e-6
        lo[k], hi[k] = 0.5 - 0.5 * w, 0.5 + 0.5 * w
    return lo, hi


def _shifts_inside(frac, lo, hi, pbc, seed):
    """per atom and periodic axis a shift drawn from -2 .. 2, taken towards zero until the atom is inside the window"""
    shift = np.random.default_rng(seed).integers(-2, 3, frac.shape) * pbc
    for _ in range(2):
        out = ((frac + shift < lo) | (frac + shift > hi)) & pbc
        shift = shift - np.sign(shift) * out
    return shift


@pytest.mark.parametrize("name", ["primitive_2atom", "bcc_mow_222", "triclinic", "slab", "ternary"])
def test_rows_are_invariant_under_lattice_translations(name):
    """Single atoms moved by whole lattice vectors, as far as the batch is not flagged as holding atoms far outside their cell:
    the same rows (they come from image vectors, not positions).  Moved further, the call is refused and says to wrap.  (The
    window around the cell is fac + 1 - r_cut / h wide: 1.01 cells on the skewed primitive cell, where no atom can move a
    lattice vector and stay inside -- there only the refusal is checked --, 1.13 on the 2 x 2 x 2 cells, 1.42 on the others.)"""
    basis, atoms, seed = _case(name)
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    pbc = np.asarray(atoms.get_pbc(), dtype=bool)
    x_v = _rows(basis, [atoms])[0]
    frac = np.asarray(atoms.get_positions()) @ np.linalg.inv(cell)
    lo, hi = _window(basis, atoms)
    shift = _shifts_inside(frac, lo, hi, pbc, seed)
    assert np.all((frac + shift >= lo) & (frac + shift <= hi))
    assert np.abs(shift).max() >= 1 or name == "primitive_2atom"
    if np.abs(shift).max() >= 1:
        moved = Atoms(numbers=atoms.get_atomic_numbers(), positions=np.asarray(atoms.get_positions()) + shift @ cell,
                      cell=cell, pbc=atoms.get_pbc())
        x_m = _rows(basis, [moved])[0]
        err = np.abs(x_m - x_v).max() / np.abs(x_v).max()
        print(f"\n{name}: {int(np.any(shift != 0, axis=1).sum())} of {len(atoms)} atoms moved, max|moved - original| / max = {err:.1e}")
        assert err <= 1e-12
    far = np.zeros((len(atoms), 3))
    far[0, int(np.flatnonzero(pbc)[0])] = 2.0
    flagged = Atoms(numbers=atoms.get_atomic_numbers(), positions=np.asarray(atoms.get_positions()) + far @ cell,
                    cell=cell, pbc=atoms.get_pbc())
    with pytest.raises(_lib.UF3Error, match="wrap the atoms"):
        _rows(basis, [flagged])
    assert np.abs(_rows(basis, [atoms])[0] - x_v).max() <= 1e-12 * np.abs(x_v).max()       # (the context serves the next call)


def _fit_frames_and_targets():
    basis = synthetic.notebook_basis(MOW)
    rng = np.random.default_rng(2024)
    frames = []
    for k in range(12):
        a = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, NUMS, seed=300 + k)
        eps = rng.uniform(-0.03, 0.03, (3, 3))
        eps = np.eye(3) + 0.5 * (eps + eps.T)
        frames.append(_strained(a, eps))
    model = ls.WeightedLinearModel(basis)
    c_true = _random_coeff(basis, 77)
    model.coefficients = c_true
    e, f, off, v = calculator.UFCalculator(model, md_skin=0.0).evaluate_frames(frames, virial=True)
    volumes = [abs(np.linalg.det(np.asarray(a.get_cell(), dtype=float).reshape(3, 3))) for a in frames]
    stresses = [v[k] / volumes[k] for k in range(12)]
    for k in (1, 6, 11):
        stresses[k] = None
    forces = [f[off[k]:off[k + 1]] for k in range(12)]
    return basis, frames, np.asarray(e), forces, stresses, volumes


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def test_device_fit_with_stress_targets():
    """DeviceFitAccumulator.add_frames(..., stresses=...) in two calls, three frames without a stress: G_v, o_v, m_v are the NumPy
    products of the host rows (per-atom normalised, frozen columns out); fit_frames(virial_weight=0.3) solves the documented
    combination of the pieces; virial_weight = 0 is bit for bit the fit of the same pieces without the virial ones."""
    basis, frames, e, forces, stresses, volumes = _fit_frames_and_targets()
    fz = process.BasisFeaturizer(basis)
    model = ls.WeightedLinearModel(basis)
    acc = pipeline.DeviceFitAccumulator(model, fz, with_forces=True)
    acc.add_frames(frames[:5], e[:5], forces[:5], stresses=stresses[:5])
    acc.add_frames(frames[5:], e[5:], forces[5:], stresses=stresses[5:])
    got = acc.pieces()
    counts = [len(a) for a in frames]
    y_v, kept = ls.virial_targets(stresses, volumes, counts, return_index=True)
    assert len(kept) == 9
    x_v = fz.featurize_virials([frames[k] for k in kept]) / np.array([counts[k] for k in kept], dtype=float)[:, None, None]
    mask = np.asarray(model.mask)
    assert not np.any(x_v[:, :, np.asarray(model.col_idx, dtype=int)])
    xv = x_v.reshape(-1, basis.n_feats)[:, mask]
    yv = y_v.reshape(-1)
    for key, ref in (("gram_v", xv.T @ xv), ("ord_v", xv.T @ yv), ("m_v", ls.moments(yv))):
        err = _rel(got[key], ref)
        print(f"\n{key}: max|device - numpy| / max|numpy| = {err:.1e}")
        assert err <= 1e-11, key
    # the fit: a NumPy restatement of the combined system, solved on the pieces fit_frames returns
    lam, kappa = 0.3, 0.5
    m_fit = ls.WeightedLinearModel(basis)
    p = pipeline.fit_frames(m_fit, fz, frames, e, forces, weight=kappa, stresses=stresses, virial_weight=lam)
    w_e, w_f = ls.calc_E_F_weights(p["m_e"][0], p["m_f"][0], ls.std_from_moments(p["m_e"]), ls.std_from_moments(p["m_f"]))
    w_v = 1 / np.sqrt(p["m_v"][0]) / ls.std_from_moments(p["m_v"])
    G = (1 - lam) * (kappa * w_e ** 2 * p["gram_e"] + (1 - kappa) * w_f ** 2 * p["gram_f"]) + lam * w_v ** 2 * p["gram_v"]
    o = (1 - lam) * (kappa * w_e ** 2 * p["ord_e"] + (1 - kappa) * w_f ** 2 * p["ord_f"]) + lam * w_v ** 2 * p["ord_v"]
    reg = np.asarray(m_fit.regularizer)[:, mask]
    c_ref = np.zeros(basis.n_feats)
    c_ref[mask] = np.linalg.solve(G + reg.T @ reg, o)
    c_ref[np.asarray(model.col_idx, dtype=int)] = model.frozen_c
    err = _rel(m_fit.coefficients, c_ref)
    print(f"\ncoefficients at virial_weight 0.3: max|fit - numpy| / max = {err:.1e}")
    assert err <= 1e-9
    # virial_weight = 0: the arithmetic performed is that of a fit given no stresses.  Held on ONE accumulation's pieces: two
    # accumulations on the device differ in the last bits with or without stresses (the energy rows' atomics reorder), and
    # the data of 12 small frames leave the short-range pair columns to the regulariser, which amplifies those bits.
    m_zero, m_none = ls.WeightedLinearModel(basis), ls.WeightedLinearModel(basis)
    p0 = pipeline.fit_frames(m_zero, fz, frames, e, forces, weight=kappa, stresses=stresses, virial_weight=0.0)
    assert p0["m_v"][0] == 54
    m_none.fit_from_pieces({k: v for k, v in p0.items() if not k.endswith("_v")}, weight=kappa)
    assert np.array_equal(m_zero.coefficients, m_none.coefficients)
    assert not np.array_equal(m_fit.coefficients, m_zero.coefficients)
    for key in ("gram_e", "gram_f", "ord_e", "ord_f", "m_e", "m_f"):          # the energy / force pieces do not see the stresses
        err = _rel(p[key], p0[key])
        print(f"{key}: two accumulations differ by {err:.1e} relative")
        assert err <= 1e-12, key
