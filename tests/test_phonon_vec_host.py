"""The eigenvector routes' NumPy restatement (``_phonon_vec_ref``) against identities that do not involve it, and the Python
layer's argument checks and grouping -- no device."""
import numpy as np
import pytest

from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import harmonic
import _phonon_ref as PR
import _phonon_vec_ref as VR


def _synthetic(seed=3, n=3, n_sc=12, n_terms=60):
    """Random force-constant rows, term records and masses: a D(q) without symmetry, so without degeneracies."""
    rng = np.random.default_rng(seed)
    fc = rng.normal(size=(n, n_sc, 3, 3))
    terms = np.empty((n_terms, 5), dtype=np.int32)
    terms[:, 0] = rng.integers(0, n, n_terms)
    terms[:, 1] = rng.integers(0, n_sc, n_terms)
    terms[:, 2:] = rng.integers(-3, 4, (n_terms, 3))
    w = rng.uniform(0.2, 1.0, n_terms)
    m = rng.uniform(20, 200, n)
    cell = np.array([[3.2, 0.0, 0.0], [0.5, 3.3, 0.0], [0.4, 0.6, 4.9]])
    return fc, terms, w, m, cell


def _random_eigen(seed, nq, n3):
    rng = np.random.default_rng(seed)
    H = rng.normal(size=(nq, n3, n3)) + 1j * rng.normal(size=(nq, n3, n3))
    H = H @ np.conj(np.transpose(H, (0, 2, 1))) / n3 + 0.05 * np.eye(n3)      # positive definite: real frequencies
    return np.linalg.eigh(H)


def test_reference_pdos_sums_to_the_total_dos():
    lam, vec = _random_eigen(1, 40, 9)
    f = PR.frequencies(lam)
    w = np.random.default_rng(2).integers(1, 3, 40)
    s = np.linspace(f.min() - 1, f.max() + 1, 23)
    g = VR.projected_dos(f, vec, w, s, 0.7)
    tot = PR.smeared_dos(f, w, s, 0.7)
    assert g.shape == (9, 23) and np.all(g >= 0)
    assert np.abs(g.sum(axis=0) - tot).max() <= 1e-13 * tot.max()


def test_reference_displacements_trace_identity():
    """sum_i m_i tr U_i = (1 / sum w) sum_q w_q sum_s E_s / lam_s: V is unitary."""
    lam, vec = _random_eigen(4, 30, 12)
    lam[0, :3] = 1e-12                                                        # three modes under the cut-off
    w = np.random.default_rng(5).integers(1, 3, 30)
    m = np.random.default_rng(6).uniform(20, 200, 4)
    temps = [0.0, 1.0, 300.0, 3000.0]
    U, A, n_excl = VR.displacement_tensors(lam, vec, w, m, temps)
    assert n_excl == 3 * w[0]
    f = PR.frequencies(lam)
    inc = f > 1e-3
    for it, T in enumerate(temps):
        e = PR.mode_terms(f[inc], T)[1]
        want = float((np.broadcast_to(w[:, None], f.shape)[inc] * e / lam[inc]).sum()) / w.sum()
        got = float((m[:, None] * U[it, :, :3]).sum())
        assert abs(got - want) <= 1e-12 * want, (T, got, want)
        assert np.all(U[it, :, :3] > 0) and np.all(np.abs(U[it]) <= A[it] * (1 + 1e-12))
    assert np.all(U[3, :, :3] > U[2, :, :3]) and np.all(U[2, :, :3] > U[0, :, :3])        # the diagonal grows with temperature


def test_reference_velocities_against_central_differences():
    fc, terms, w, m, cell = _synthetic()
    q = np.random.default_rng(8).uniform(-0.5, 0.5, (6, 3))
    D = PR.dynamical_from_terms(fc, terms, w, q, m)
    lam, vec = np.linalg.eigh(D)
    gaps = np.diff(lam, axis=1).min() / np.abs(lam).max()
    assert gaps > 1e-4                                                         # no degeneracy: the diagonal is defined
    v = VR.velocities(VR.d_dynamical_from_terms(fc, terms, w, q, m), vec, lam, cell, cutoff=0.0)
    # d f / d k_c by central differences: k = q inv(cell)^T, so a step h along k_c moves q by h cell[:, c]
    # step: the phases turn by 2 pi n.cell h, |n.cell| <= 3 * 9 A here, so the truncation h^2 f''' / 6 is ~ (170 h)^2 / 6 of the
    # slope, 5e-9 at h = 1e-6; rounding, 1e-16 |f| / h against slopes of ~ 100 |f|, is 1e-12.  Bound: 1e-6 of the largest slope.
    h = 1e-6
    fd = np.empty_like(v)
    for c in range(3):
        dq = h * cell[:, c]
        fp = PR.frequencies(np.linalg.eigvalsh(PR.dynamical_from_terms(fc, terms, w, q + dq, m)))
        fm = PR.frequencies(np.linalg.eigvalsh(PR.dynamical_from_terms(fc, terms, w, q - dq, m)))
        fd[:, :, c] = (fp - fm) / (2 * h)
    err = np.abs(v - fd).max() / np.abs(fd).max()
    assert err <= 1e-6, err
    # cluster sums: one cluster per mode here, and a forced pair
    groups = VR.clusters(lam[0])
    assert groups == [[k] for k in range(lam.shape[1])]
    assert VR.clusters(np.array([1.0, 1.0 + 1e-9, 2.0])) == [[0, 1], [2]]
    assert np.array_equal(VR.cluster_sums(v[0], [[0, 1], [2]])[0], v[0, 0] + v[0, 1])


def test_unit_phase():
    x = np.random.default_rng(1).uniform(-40, 40, 2000)
    assert np.abs(VR.unit_phase(x) - np.exp(2j * np.pi * x)).max() <= 1e-13           # (np.exp's own argument error at |x| = 40)
    k = np.arange(-12, 13) / 4.0
    want = np.array([1, 1j, -1, -1j])[np.arange(-12, 13) % 4]
    assert np.array_equal(VR.unit_phase(k), want)
    # at a time-reversal-invariant point D is real and dD / dq is i times an antisymmetric matrix: no velocity for real vectors
    fc, terms, w, m, cell = _synthetic(seed=5)
    dD = VR.d_dynamical_from_terms(fc, terms, w, [[0.5, 0.0, -0.5]], m)
    assert np.all(dD.real == 0) and np.abs(dD.imag).max() > 0


def test_cutoff_zeroes_the_velocity():
    fc, terms, w, m, cell = _synthetic(seed=9)
    q = np.array([[0.11, -0.23, 0.37]])
    D = PR.dynamical_from_terms(fc, terms, w, q, m)
    lam, vec = np.linalg.eigh(D)
    f = np.abs(PR.frequencies(lam))
    cut = float(np.sort(f.ravel())[2]) * (1 + 1e-12)
    v = VR.velocities(VR.d_dynamical_from_terms(fc, terms, w, q, m), vec, lam, cell, cutoff=cut)
    assert np.all(v[0][f[0] <= cut] == 0) and (f[0] <= cut).sum() == 3 and np.any(v != 0)


def _mow3():
    cell = np.array([[3.2, 0.0, 0.0], [0.5, 3.3, 0.0], [0.4, 0.6, 4.9]])
    frac = np.array([[0.02, 0.05, 0.01], [0.48, 0.53, 0.34], [0.55, 0.41, 0.69]])
    return Atoms(numbers=[42, 74, 74], positions=frac @ cell, cell=cell, pbc=True)


def test_grouping():
    ch = np.arange(9 * 4, dtype=float).reshape(9, 4)
    atoms = _mow3()
    g, labels = harmonic.group_pdos(ch, atoms, "channel")
    assert g is ch or np.array_equal(g, ch)
    assert labels == [(0, "x"), (0, "y"), (0, "z"), (1, "x"), (1, "y"), (1, "z"), (2, "x"), (2, "y"), (2, "z")]
    g, labels = harmonic.group_pdos(ch, atoms, "atom")
    assert labels == [0, 1, 2] and np.array_equal(g, ch.reshape(3, 3, 4).sum(axis=1))
    g, labels = harmonic.group_pdos(ch, atoms, "species")
    assert len(labels) == 2 and g.shape == (2, 4)
    assert np.array_equal(g[0], ch[:3].sum(axis=0)) and np.array_equal(g[1], ch[3:].sum(axis=0))
    assert np.array_equal(g.sum(axis=0), ch.sum(axis=0))
    with pytest.raises(ValueError, match="by must be"):
        harmonic.group_pdos(ch, atoms, "element")


def test_argument_checks_before_the_device():
    assert harmonic.vector_slab(3) == (1 << 28) // (16 * 9)
    assert harmonic.vector_slab(63) == (1 << 28) // (16 * 63 * 63) == 4227
    assert harmonic.vector_slab(10 ** 6) == 1
    u = harmonic.voigt6_to_tensors(np.arange(1.0, 7.0))
    assert np.array_equal(u, [[1, 6, 5], [6, 2, 4], [5, 4, 3]])
    rng = np.random.default_rng(0)
    big = Atoms(numbers=[74] * 22, positions=rng.uniform(0, 9, (22, 3)), cell=np.eye(3) * 9.0, pbc=True)
    with pytest.raises(ValueError, match="at most 21 atoms"):
        harmonic.mesh_eigenvectors(np.zeros((22, 22, 3, 3)), big, [[0, 0, 0]], 1, np.ones(22))
    atoms = _mow3()
    fc = np.zeros((3, 3, 3, 3))
    with pytest.raises(ValueError, match="fc_rows must be"):
        harmonic.mesh_eigenvectors(np.zeros((3, 4, 3, 3)), atoms, [[0, 0, 0]], 1, np.ones(3))
    with pytest.raises(ValueError, match="qpoints must be"):
        harmonic.mesh_eigenvectors(fc, atoms, np.zeros((2, 2)), 1, np.ones(3))
    with pytest.raises(ValueError, match="positive mass"):
        harmonic.mesh_eigenvectors(fc, atoms, [[0, 0, 0]], 1, [1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="nothing asked for"):
        harmonic.mesh_eigenvectors(fc, atoms, [[0, 0, 0]], 1, np.ones(3), vectors=False)
    with pytest.raises(ValueError, match="cutoff_THz"):
        harmonic.mesh_eigenvectors(fc, atoms, [[0, 0, 0]], 1, np.ones(3), velocities=True, cutoff_THz=-1.0)
    with pytest.raises(ValueError, match="by must be"):
        harmonic.projected_dos(None, atoms, (2, 2, 2), by="element")
    lam, vec = np.ones((2, 3)), np.zeros((2, 3, 3), dtype=complex)
    with pytest.raises(ValueError, match="vec"):
        harmonic.pdos_from_eigenvectors(lam, vec[:, :2], samples=[0.0], sigma=0.1)
    with pytest.raises(ValueError, match="sigma"):
        harmonic.pdos_from_eigenvectors(lam, vec, samples=[0.0], sigma=0.0)
    with pytest.raises(ValueError, match="temperatures"):
        harmonic.tdisp_from_eigenvectors(lam, vec, [1.0], [-1.0])
    with pytest.raises(ValueError, match="positive mass"):
        harmonic.tdisp_from_eigenvectors(lam, vec, [1.0, 2.0], [300.0])
