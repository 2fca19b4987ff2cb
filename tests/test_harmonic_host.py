"""Host side of the analytic Hessian: the NumPy restatement (_harmonic_ref) against finite differences of the oracle, and the
phonon / elastic algebra of uf3_amd.forcefield.harmonic on hand-built inputs (no GPU)."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import harmonic
from uf3_amd.regression import least_squares as ls
import _harmonic_ref as HR
from _util import GOLDEN, basis_from_meta, load_case


def _unary():
    m = ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json"))
    return m.bspline_config, np.asarray(m.coefficients, dtype=float)


def _mow():
    basis = synthetic.notebook_basis(["Mo", "W"])
    coeff = np.random.default_rng(31).normal(0, 0.05, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    return basis, coeff


def _nexe():
    _, meta, atoms = load_case("case_nexe32")
    basis = basis_from_meta(meta)
    coeff = np.random.default_rng(37).normal(0, 0.05, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    return basis, coeff, atoms


def _strained(atoms, v, t):
    eps = np.eye(3)
    a, b = harmonic._VOIGT[v]
    if a == b:
        eps[a, a] += t
    else:
        eps[a, b] += 0.5 * t
        eps[b, a] += 0.5 * t
    return Atoms(numbers=atoms.get_atomic_numbers(), positions=np.asarray(atoms.get_positions()) @ eps.T,
                 cell=np.asarray(atoms.get_cell()) @ eps.T, pbc=atoms.get_pbc())


def _frames():
    w = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=3)
    mow = synthetic.lattice_frame("bcc", (2, 2, 2), 3.2, [42, 74], seed=5)
    cluster = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=7)
    cluster = Atoms(numbers=cluster.get_atomic_numbers(), positions=cluster.get_positions(), cell=np.zeros((3, 3)), pbc=False)
    slab = synthetic.lattice_frame("bcc", (2, 2, 2), 3.2, [42, 74], seed=9)
    slab = Atoms(numbers=slab.get_atomic_numbers(), positions=slab.get_positions(), cell=slab.get_cell(), pbc=[True, True, False])
    nexe = _nexe()[2]        # 2-body only: no 3-body list, reach = the largest pair r_max
    return [("w16", _unary, w), ("mow16", _mow, mow), ("w_cluster", _unary, cluster), ("mow_slab", _mow, slab),
            ("nexe32_2body", lambda: _nexe()[:2], nexe)]


@pytest.mark.parametrize("label,model,atoms", _frames(), ids=[f[0] for f in _frames()])
def test_restatement_against_oracle_differences(label, model, atoms):
    basis, coeff = model()
    ob = O.OracleBasis(basis)
    H, L, B = HR.hessian(ob, atoms, coeff)
    pos = np.asarray(atoms.get_positions(), dtype=float)
    n = len(pos)
    h = 1e-5
    Hfd = np.zeros_like(H)
    for k in range(3 * n):
        fs = []
        for sgn in (1, -1):
            p = pos.copy()
            p[k // 3, k % 3] += sgn * h
            a = Atoms(numbers=atoms.get_atomic_numbers(), positions=p, cell=atoms.get_cell(), pbc=atoms.get_pbc())
            fs.append(O.evaluate(ob, a, coeff)[1].ravel())
        Hfd[:, k] = -(fs[0] - fs[1]) / (2 * h)
    scale = np.abs(H).max()
    assert scale > 0
    assert np.abs(H - Hfd).max() <= 1e-6 * scale, (label, np.abs(H - Hfd).max() / scale)
    assert np.abs(H - H.T).max() <= 1e-12 * scale
    if not np.all(atoms.get_pbc()):
        return
    # mixed: -dF/dt by central differences of forces under strain
    Lfd = np.zeros_like(L)
    for v in range(6):
        fp = O.evaluate(ob, _strained(atoms, v, h), coeff)[1].ravel()
        fm = O.evaluate(ob, _strained(atoms, v, -h), coeff)[1].ravel()
        Lfd[:, v] = -(fp - fm) / (2 * h)
    assert np.abs(L - Lfd).max() <= 1e-6 * np.abs(L).max(), (label, np.abs(L - Lfd).max() / np.abs(L).max())
    # born: four-point second differences of energies, Richardson from d = 2e-4 and 1e-4
    def second(u, v, d):
        def en(tu, tv):
            eps = np.eye(3)
            for w, t in ((u, tu), (v, tv)):
                a, b = harmonic._VOIGT[w]
                if a == b:
                    eps[a, a] += t
                else:
                    eps[a, b] += 0.5 * t
                    eps[b, a] += 0.5 * t
            at = Atoms(numbers=atoms.get_atomic_numbers(), positions=pos @ eps.T, cell=np.asarray(atoms.get_cell()) @ eps.T,
                       pbc=atoms.get_pbc())
            return O.evaluate(ob, at, coeff)[0]
        return (en(d, d) - en(d, -d) - en(-d, d) + en(-d, -d)) / (4 * d * d)

    Bfd = np.zeros((6, 6))
    for u in range(6):
        for v in range(u, 6):
            Bfd[u, v] = Bfd[v, u] = (4 * second(u, v, 1e-4) - second(u, v, 2e-4)) / 3
    # (a rattled frame: knot crossings within +-2d leave an O(d) error the extrapolation does not remove: small d)
    assert np.abs(B - Bfd).max() <= 1e-4 * np.abs(B).max(), (label, np.abs(B - Bfd).max() / np.abs(B).max())


# ---------------------------------------------------------------------------------------------- phonon algebra
def _spring_sc(n_super, k=1.7, k2=0.6, a=2.5, mass=3.0):
    """Force constants, as supercell rows, of a simple cubic lattice (one atom) with longitudinal springs to the first (k) and
    the second (k2, two cells along an axis) neighbours along the axes.  The folded supercell holds each spring's two images at
    one supercell atom when they coincide (the second neighbours at n_super = 4: the minimum-image tie)."""
    atoms = Atoms(numbers=[18], positions=[[0.3, 0.1, 0.2]], cell=np.eye(3) * a, pbc=True)
    n_sc = n_super ** 3
    fc = np.zeros((1, n_sc, 3, 3))
    for ax in range(3):
        for dist, kk in ((1, k), (2, k2)):
            for sgn in (1, -1):
                t = np.zeros(3, dtype=int)
                t[ax] = sgn * dist
                t %= n_super
                p = (t[0] * n_super + t[1]) * n_super + t[2]
                fc[0, p, ax, ax] -= kk
                fc[0, 0, ax, ax] += kk
    return atoms, fc, k, k2, mass


@pytest.mark.parametrize("n_super", [4, 5])
def test_spring_model_dispersion(n_super):
    atoms, fc, k, k2, mass = _spring_sc(n_super)
    q = np.random.default_rng(1).uniform(-0.5, 0.5, (25, 3))
    q[0] = [0.5, 0.5, 0.5]
    q[1] = [0.25, 0.125, 0.375]
    D = harmonic.dynamical_matrices(fc, atoms, q, n_super, [mass])
    lam = np.linalg.eigvalsh(D)
    want = np.sort(np.stack([(2 * k * (1 - np.cos(2 * np.pi * q[:, a])) + 2 * k2 * (1 - np.cos(4 * np.pi * q[:, a]))) / mass
                             for a in range(3)], axis=1), axis=1)
    assert np.abs(lam - want).max() <= 1e-12
    f = harmonic.frequencies_from(D)
    assert np.allclose(f, np.sqrt(want) * harmonic.THZ, rtol=0, atol=1e-10)


def test_minimum_image_weights_at_the_tie():
    cell = np.eye(3) * 2.0
    w = harmonic.minimum_image_weights(cell, np.zeros((1, 3)), 2)
    # supercell atom (1, 0, 0) is 2 A away on both sides: two images, weight 1/2
    R, wt = w[0][4]
    assert len(R) == 2 and wt == 0.5
    R, wt = w[0][7]
    assert len(R) == 8 and wt == 0.125


# ---------------------------------------------------------------------------------------------- elastic algebra
def test_relaxed_tensor_algebra():
    rng = np.random.default_rng(4)
    n = 4
    # a quadratic energy E = 1/2 x^T H x + x^T Lam t + 1/2 t^T B t with rigid translations free (H annihilates them)
    A = rng.normal(size=(3 * n, 3 * n))
    T = np.zeros((3 * n, 3))
    for k in range(3):
        T[k::3, k] = 1.0
    P = np.eye(3 * n) - T @ np.linalg.pinv(T)
    H = P @ (A @ A.T + 3 * np.eye(3 * n)) @ P
    Lam = P @ rng.normal(size=(3 * n, 6))
    Bm = rng.normal(size=(6, 6))
    Bm = Bm @ Bm.T + 50 * np.eye(6)
    C = harmonic.relaxed_tensor(H, Lam, Bm)
    # minimise over x for every t: x = -H^+ Lam t
    want = Bm - Lam.T @ np.linalg.pinv(H) @ Lam
    assert np.abs(C - want).max() <= 1e-10 * np.abs(want).max()
    # a singular H (a soft internal mode with no strain coupling) changes nothing
    v = P @ rng.normal(size=3 * n)
    v /= np.linalg.norm(v)
    H2 = (np.eye(3 * n) - np.outer(v, v)) @ H @ (np.eye(3 * n) - np.outer(v, v))
    Lam2 = (np.eye(3 * n) - np.outer(v, v)) @ Lam
    C2 = harmonic.relaxed_tensor(H2, Lam2, Bm)
    want2 = Bm - Lam2.T @ np.linalg.pinv(H2, rcond=1e-10) @ Lam2
    assert np.abs(C2 - want2).max() <= 1e-10 * np.abs(want2).max()
    assert np.all(np.linalg.eigvalsh(Bm - C2) >= -1e-9)


def test_cubic_constants():
    C = np.zeros((6, 6))
    C[:3, :3] = 150.0
    C[[0, 1, 2], [0, 1, 2]] = 500.0
    C[[3, 4, 5], [3, 4, 5]] = 120.0
    c11, c12, c44, B = harmonic.cubic_constants(C)
    assert (c11, c12, c44) == (500.0, 150.0, 120.0) and abs(B - 800.0 / 3) < 1e-12
    C[0, 1] = C[1, 0] = 151.0
    with pytest.raises(ValueError, match="elastic_tensor"):
        harmonic.cubic_constants(C)


# ---------------------------------------------------------------------------------------------- lattices and paths
def _bcc_conv(a=3.17):
    return Atoms(numbers=[74, 74], positions=[[0, 0, 0], [a / 2] * 3], cell=np.eye(3) * a, pbc=True)


def _bcc_prim(a=3.17):
    cell = 0.5 * a * np.array([[-1, 1, 1], [1, -1, 1], [1, 1, -1]])
    return Atoms(numbers=[74], positions=[[0, 0, 0]], cell=cell, pbc=True)


def _fcc_prim(a=4.05):
    cell = 0.5 * a * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]])
    return Atoms(numbers=[13], positions=[[0, 0, 0]], cell=cell, pbc=True)


def test_lattice_recognition_and_paths():
    for atoms, kind, a in ((_bcc_conv(), "cI", 3.17), (_bcc_prim(), "cI", 3.17), (_fcc_prim(), "cF", 4.05),
                           (Atoms(numbers=[84], positions=[[0, 0, 0]], cell=np.eye(3) * 3.35, pbc=True), "cP", 3.35)):
        k, a_found = harmonic.cubic_lattice(atoms)
        assert k == kind and abs(a_found - a) < 1e-9
    coords, path = harmonic.standard_path(_bcc_prim())
    assert path == [("GAMMA", "H"), ("H", "N"), ("N", "GAMMA"), ("GAMMA", "P"), ("P", "H"), ("P", "N")]
    # H = (0, 0, 1) 2 pi / a: reduced coordinates of the primitive cell's reciprocal lattice
    assert np.allclose(coords["H"], [0.5, 0.5, -0.5])
    coords_c, _ = harmonic.standard_path(_bcc_conv())
    assert np.allclose(coords_c["H"], [0, 0, 1]) and np.allclose(coords_c["P"], [0.5, 0.5, 0.5])
    # a rotated cubic cell is refused
    from _util import rotation
    Q = rotation([1, 2, 3], 0.3)
    rot = _bcc_conv()
    rot = Atoms(numbers=rot.get_atomic_numbers(), positions=np.asarray(rot.get_positions()) @ Q.T,
                cell=np.asarray(rot.get_cell()) @ Q.T, pbc=True)
    assert harmonic.cubic_lattice(rot) is None
    with pytest.raises(ValueError, match="explicit path"):
        harmonic.standard_path(rot)


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_checks():
    with pytest.raises(ValueError, match="row span"):
        harmonic._row_span((3, 3), 4)
    with pytest.raises(ValueError, match="row span"):
        harmonic._row_span((0, 5), 4)
    with pytest.raises(ValueError, match="contiguous"):
        harmonic._row_span(range(0, 4, 2), 4)
    assert harmonic._row_span(slice(1, 3), 4) == (1, 3) and harmonic._row_span(None, 4) == (0, 4)
    cluster = Atoms(numbers=[74, 74], positions=[[0, 0, 0], [2.7, 0, 0]], cell=np.zeros((3, 3)), pbc=False)
    for call in (lambda: harmonic.phonon_frequencies(None, cluster, [[0, 0, 0]], masses={"W": 183.84}),
                 lambda: harmonic.band_structure(None, cluster, masses={"W": 183.84}),
                 lambda: harmonic.elastic_tensor(None, cluster)):
        with pytest.raises(ValueError, match="periodic"):
            call()
    with pytest.raises(ValueError, match="no mass"):
        harmonic._masses(_bcc_conv(), {"Mo": 95.95})
    with pytest.raises(ValueError, match="masses"):
        harmonic._masses(_bcc_conv(), [1.0])
