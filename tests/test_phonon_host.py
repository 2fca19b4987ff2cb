"""Host side of the q-mesh phonons (uf3_amd.forcefield.harmonic): the mesh and its time-reversal reduction, the flat term list
against ``dynamical_matrices``, and the NumPy reference of the thermodynamics against closed forms.  No GPU."""
import itertools

import numpy as np
import pytest

from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import harmonic
import _phonon_ref as PR


@pytest.mark.parametrize("mesh", [(3, 3, 3), (4, 4, 4), (2, 3, 5), (1, 1, 1), (6, 1, 4)])
@pytest.mark.parametrize("gamma_centred", [True, False])
def test_qmesh_time_reversal_reproduces_the_full_mesh(mesh, gamma_centred):
    n = np.array(mesh)
    full, w_full = harmonic.qmesh(mesh, gamma_centred=gamma_centred, time_reversal=False)
    assert len(full) == n.prod() and np.all(w_full == 1)
    shift = 0.0 if gamma_centred else 0.5
    want = np.array(list(itertools.product(*(range(k) for k in mesh)))) + shift
    assert np.array_equal(full, want / n)
    q, w = harmonic.qmesh(mesh, gamma_centred=gamma_centred, time_reversal=True)
    assert w.dtype == np.int64 and w.sum() == n.prod() and set(w.tolist()) <= {1, 2}
    # twice the points: exact integers 2 (a + shift)
    a2 = np.rint(2 * q * n).astype(np.int64)
    assert np.array_equal(a2 / (2.0 * n), q)
    neg = (-a2) % (2 * n)
    both = {tuple(r) for r in a2.tolist()} | {tuple(r) for r in neg.tolist()}
    assert both == {tuple(r) for r in np.rint(2 * want).astype(np.int64).tolist()}
    self_conj = np.all(neg == a2, axis=1)
    assert np.array_equal(w, np.where(self_conj, 1, 2))
    assert len(q) == (n.prod() + self_conj.sum()) // 2


def test_qmesh_refuses_bad_meshes():
    for bad in ((0, 2, 2), (2, 2), (2, -1, 2)):
        with pytest.raises(ValueError):
            harmonic.qmesh(bad)


def _structures():
    a = 3.17
    conv = Atoms(numbers=[74, 74], positions=[[0, 0, 0], [a / 2] * 3], cell=np.eye(3) * a, pbc=True)
    fcc = Atoms(numbers=[29], positions=[[0.1, 0.2, 0.3]], cell=0.5 * 3.6 * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0.0]]), pbc=True)
    ortho = Atoms(numbers=[42, 74, 74], positions=[[0.1, 0.0, 0.2], [1.4, 1.9, 0.3], [0.7, 3.1, 2.2]],
                  cell=np.diag([2.9, 4.1, 3.3]), pbc=True)
    return [("bcc_conventional", conv, [183.84, 183.84]), ("fcc_primitive", fcc, [63.5]), ("ortho3", ortho, [95.95, 183.84, 183.84])]


@pytest.mark.parametrize("n_super", [2, 3, 5])
@pytest.mark.parametrize("label,atoms,masses", _structures(), ids=[s[0] for s in _structures()])
def test_image_terms_reproduce_dynamical_matrices(label, atoms, masses, n_super):
    n = len(masses)
    n_sc = n * n_super ** 3
    rng = np.random.default_rng(100 + n_super)
    full = rng.normal(size=(3 * n_sc, 3 * n_sc))
    full = 0.5 * (full + full.T)
    fc = full[:3 * n].reshape(n, 3, n_sc, 3).transpose(0, 2, 1, 3).copy()
    terms, w = harmonic.image_terms(atoms, n_super)
    assert terms.dtype == np.int32 and terms.shape == (len(w), 5)
    # the same images and weights as minimum_image_weights, in its order
    cell = np.asarray(atoms.get_cell(), dtype=float)
    ref = harmonic.minimum_image_weights(cell, atoms.get_positions(), n_super)
    k = 0
    for i in range(n):
        for p in range(n_sc):
            R, wt = ref[i][p]
            for r in R:
                assert terms[k, 0] == i and terms[k, 1] == p and w[k] == wt
                assert np.abs(terms[k, 2:] @ cell - r).max() < 1e-9
                k += 1
    assert k == len(w)
    # each (i, p) has weights summing to one
    tot = np.zeros((n, n_sc))
    np.add.at(tot, (terms[:, 0], terms[:, 1]), w)
    assert np.allclose(tot, 1.0, rtol=0, atol=1e-14)
    q = rng.uniform(-0.5, 0.5, (10, 3))
    want = harmonic.dynamical_matrices(fc, atoms, q, n_super, masses)
    got = PR.dynamical_from_terms(fc, terms, w, q, masses)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_reference_thermodynamics_single_mode_closed_forms():
    f = np.array([[5.0]])
    w = np.array([1])
    hf = PR.H * 5.0
    # T -> 0: F = U = hf / 2, S = C_v = 0 (x = 240 at 1 K: e^-x is below 1e-104)
    r = PR.thermo(f, w, [0.0, 1.0])
    assert r["zpe"] == 0.5 * hf and r["n_excluded"] == 0
    for k in range(2):
        assert abs(r["F"][k] - 0.5 * hf) <= 1e-16 and abs(r["U"][k] - 0.5 * hf) <= 1e-16
        assert 0.0 <= r["S"][k] <= 1e-100 and 0.0 <= r["Cv"][k] <= 1e-95
    # x << 1: C_v / k_B = 1 - x^2 / 12 + x^4 / 240 - ..., S / k_B = 1 - log x + x^2 / 24 - ..., U = k_B T (1 + x^2 / 12 - ...)
    for T in (3000.0, 30000.0):
        x = hf / (PR.KB * T)
        r = PR.thermo(f, w, [T])
        assert abs(r["Cv"][0] / PR.KB - (1 - x * x / 12 + x ** 4 / 240)) <= x ** 6 / 6000 + 1e-15
        assert abs(r["S"][0] / PR.KB - (1 - np.log(x) + x * x / 24)) <= x ** 4 / 900 + 1e-14
        assert abs(r["U"][0] / (PR.KB * T) - (1 + x * x / 12)) <= x ** 4 / 700 + 1e-15
        assert abs(r["F"][0] - (r["U"][0] - T * r["S"][0])) <= 1e-14 * abs(r["U"][0])
    # the cut-off leaves modes out and counts them by weight
    r = PR.thermo(np.array([[1e-4, 5.0], [-2.0, 5.0]]), np.array([1, 2]), [300.0])
    one = PR.thermo(f, w, [300.0])
    assert r["n_excluded"] == 3 and abs(r["F"][0] - one["F"][0]) <= 1e-16 and abs(r["zpe"] - one["zpe"]) <= 1e-18
    # a Gaussian integrates to one
    s = np.linspace(3.0, 7.0, 1601)
    g = PR.smeared_dos(f, w, s, 0.1)
    assert abs(np.sum(0.5 * (g[1:] + g[:-1]) * np.diff(s)) - 1.0) <= 1e-12


def test_mesh_entry_points_check_their_arguments_before_the_device():
    atoms = Atoms(numbers=[74] * 33, positions=np.random.default_rng(0).uniform(0, 9, (33, 3)), cell=np.eye(3) * 9.0, pbc=True)
    with pytest.raises(ValueError, match="at most 32 atoms"):
        harmonic.mesh_eigenvalues(np.zeros((33, 33, 3, 3)), atoms, [[0, 0, 0]], 1, np.ones(33))
    with pytest.raises(ValueError, match="either mesh or qpoints"):
        harmonic.mesh_frequencies(None, _structures()[1][1], masses=[63.5])
    with pytest.raises(ValueError, match="strictly increasing"):
        harmonic.dos_from_eigenvalues(np.ones((2, 3)), edges=[0.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="sigma"):
        harmonic.dos_from_eigenvalues(np.ones((2, 3)), samples=[0.0, 1.0], sigma=0.0)
    with pytest.raises(ValueError, match="temperatures"):
        harmonic.thermo_from_eigenvalues(np.ones((2, 3)), [-1.0])
