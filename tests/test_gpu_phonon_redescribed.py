"""The phonon stack on re-described crystals (tests/_phonon_redescribed.py; the host side is tests/test_phonon_redescribed_host.py):
supercell Hessian rows, ``harmonic.image_terms``, D(q) and the Jacobi sweeps of k_ph_mesh_lane / k_ph_mesh_wave, and what is built
on the eigenpairs, on skewed, turned, permuted, shifted, folded and unwrapped descriptions of one crystal, against the base frame
through the mappings; and the eigensolvers at every size they take.

a. the description is given the base's own device force constants, mapped: what is left is image terms, phases and the solver;
   ``|lam_B(q') - lam_A(mapped q, folded)| <= 2e-11 scale`` per q, twice the bound of
   ``test_gpu_phonon.test_eigenvalues_against_the_host_route`` (scale: ``_phonon_redescribed.spectrum_scale``), sweeps <= 15;
b. the description's own device Hessian rows: the same, plus Weyl's bound on what the two sets of rows differ by;
c. eigenvectors: residual and orthonormality, group velocities turned by Q, per-atom PDOS and displacement tensors through src;
d. whole meshes: identical histogram counts, smeared DOS and thermodynamics;
e. every N from 1 to 32 (vectors: to 21) on random force constants, and exact degeneracies at 3N = 48.

Where two device results are compared, each is already held by the existing tests to a bound against its restatement (the host
route's eigenvalues 1e-11; the smeared DOS, the PDOS, the thermodynamics and the displacement tensors 1e-12 of max g or of the sum
of the terms' absolute values; velocities 1e-12 of their scale per mode): the bounds here are those, doubled.

Measured on the MI355X: see DESIGN.md section 3.24."""
import functools
import os

import numpy as np
import pytest

from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator, harmonic
from uf3_amd.regression import least_squares as ls
import _phonon_redescribed as P
import _phonon_ref as PR
import _phonon_vec_ref as VR
import test_redescribed_host as RH
from _util import GOLDEN
from test_gpu_phonon import CUTOFF, _guarded_edges, _test_points
from test_gpu_phonon_vec import _pair_errors

pytestmark = pytest.mark.gpu

LAM_TOL = 2e-11                    # twice test_eigenvalues_against_the_host_route's
END_TOL = 2e-12                    # twice the DOS, PDOS, thermodynamics and displacement tests' against their restatements
VEL_TOL = 2e-12                    # twice the velocity tests', of VR.velocity_scale
TEMPS = [0.0, 1.0, 300.0, 3000.0]

MOW = [("bcc_mow", lab, n, n) for lab in ("skew_821", "skew_351", "skew_751", "perm_rotation_shift", "skew_751_reflection")
       for n in (1, 2)]
LANE = [("bcc_w_primitive", "skew_rotation", 2, 2), ("bcc_w_primitive", "skew_rotation", 3, 3), ("w_conv2", "skew_821", 1, 1),
        ("w_conv2", "skew_821", 2, 2), ("w_conv2", "skew_821", 3, 3)]                               # N = 1, 2
WAVE = [("mow_skew3", "skew_821", 1, 1), ("mow_skew3", "skew_821", 2, 2), ("mow_skew3", "skew_821", 3, 3),
        ("bcc_w_primitive", "folded_222", 2, 1), ("bcc_w_primitive", "folded_222", 4, 2),
        ("bcc_mow_unwrapped", "every_atom", 2, 2)] + MOW                                            # N = 3, 8, 16


def _id(case):
    return "-".join(str(x) for x in case)


@functools.lru_cache(maxsize=None)
def _calc(key):
    if key == "unary":
        return calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json")), md_skin=0.0)
    return calculator.UFCalculator(RH.model(key), md_skin=0.0)


@functools.lru_cache(maxsize=None)
def _device_rows(frame, label, n_super):
    """The device's Hessian rows of the n_super^3 supercell of a description (label None: of the base), computed once."""
    atoms = P.base(frame) if label is None else P.description(frame, label).atoms
    fc = harmonic._supercell_rows(_calc(P.frames()[frame][2]), atoms, n_super).copy()
    fc.setflags(write=False)
    return fc


def _points():
    return np.concatenate([np.random.default_rng(29).uniform(-0.5, 0.5, (40, 3)), _test_points()[200:212]])


def _base_union(frame, label, n_a, q_b):
    """The base's device eigenvalues at the wave vectors that fold onto q_b, as the description's sorted rows."""
    a, d = P.base(frame), P.description(frame, label)
    q_a = P.fold_q(a, d, q_b)
    lam, sweeps = harmonic.mesh_eigenvalues(_device_rows(frame, None, n_a), a, q_a.reshape(-1, 3), n_a, P.masses(a))
    assert 0 <= sweeps.min() and sweeps.max() <= 15
    return P.folded_union(lam.reshape(len(q_b), d.scale, -1))


def _gap(lam_b, want, q_b):
    assert lam_b.shape == want.shape
    return float((np.abs(lam_b - want).max(axis=1) / P.spectrum_scale(want, q_b)).max())


def _mapped_case(case):
    frame, label, n_a, n_b = case
    a, d = P.base(frame), P.description(frame, label)
    assert P.same_supercell(a, n_a, d, n_b)
    q = _points()
    fc_b = P.mapped_rows(_device_rows(frame, None, n_a), a, n_a, d, n_b)
    lam_b, sweeps = harmonic.mesh_eigenvalues(fc_b, d.atoms, q, n_b, P.masses(d.atoms))
    return _gap(lam_b, _base_union(frame, label, n_a, q), q), sweeps


# ---- a. mapped force constants ---------------------------------------------------------------------------------------------------
def test_the_cases_reach_both_kernels_at_every_size_asked_for():
    sizes = lambda cases: sorted({len(P.description(f, lab).atoms) for f, lab, _, _ in cases})          # noqa: E731
    assert sizes(LANE) == [1, 2] and sizes(WAVE) == [3, 8, 16]                        # 3N <= 6: the lane kernel
    have = set(P.all_pairs())
    assert all(c in have for c in LANE + WAVE)


@pytest.mark.parametrize("case", LANE + WAVE, ids=_id)
def test_mapped_force_constants(case):
    gap, sweeps = _mapped_case(case)
    print(f"[phonon-redescribed] a {_id(case)}: max |dlam| / scale = {gap:.3e}, sweeps {sweeps.min()} .. {sweeps.max()}")
    assert 0 <= sweeps.min() and sweeps.max() <= 15
    assert gap <= LAM_TOL


@pytest.mark.parametrize("case", LANE, ids=_id)
def test_mapped_force_constants_on_the_wave_kernel_at_small_cells(case, monkeypatch):
    monkeypatch.setenv("UF3_PHONON_WAVE", "1")
    gap, sweeps = _mapped_case(case)
    print(f"[phonon-redescribed] a (wave kernel) {_id(case)}: max |dlam| / scale = {gap:.3e}, sweeps {sweeps.min()} .. {sweeps.max()}")
    assert 0 <= sweeps.min() and sweeps.max() <= 15
    assert gap <= LAM_TOL


# ---- b. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LANE + WAVE, ids=_id)
def test_own_hessian_rows_end_to_end(case):
    """By Weyl |dlam| <= |dD|_2 <= sum over (i', p') of |Phi_B[i', p'] - Q Phi_A[i, p] Q^T|_F / sqrt(m_i m_j) (every block enters D
    with weights that sum to one and phases of modulus one), from the two sets of device rows; the solver's 2e-11 on top.  The Weyl
    part itself stays within the Hessian's 1e-10 of the largest (mass-weighted) entry."""
    frame, label, n_a, n_b = case
    a, d = P.base(frame), P.description(frame, label)
    q = _points()
    own = _device_rows(frame, label, n_b)
    fc_a = _device_rows(frame, None, n_a)
    mapped = P.mapped_rows(fc_a, a, n_a, d, n_b)
    m_b = P.masses(d.atoms)
    m_sc = np.tile(m_b, n_b ** 3)
    inv = 1.0 / np.sqrt(m_b[:, None] * m_sc[None, :])
    weyl = float((np.sqrt(((own - mapped) ** 2).sum(axis=(2, 3))) * inv).sum())
    largest = float((np.abs(mapped).max(axis=(2, 3)) * inv).max())
    lam_b, sweeps = harmonic.mesh_eigenvalues(own, d.atoms, q, n_b, m_b)
    want = _base_union(frame, label, n_a, q)
    scale = P.spectrum_scale(want, q)
    err = np.abs(lam_b - want).max(axis=1)
    print(f"[phonon-redescribed] b {_id(case)}: max |dlam| / scale = {(err / scale).max():.3e}; Weyl part {weyl:.3e} = "
          f"{weyl / largest:.3e} of the largest entry, solver part {LAM_TOL * scale.min():.3e} .. {LAM_TOL * scale.max():.3e}; "
          f"sweeps {sweeps.min()} .. {sweeps.max()}")
    assert 0 <= sweeps.min() and sweeps.max() <= 15
    assert weyl <= 1e-10 * largest
    assert np.all(err <= weyl + LAM_TOL * scale)


# ---- c. vectors ------------------------------------------------------------------------------------------------------------------
VEC = [("bcc_w_primitive", "skew_rotation", 3, 3), ("w_conv2", "skew_821", 2, 2), ("mow_skew3", "skew_821", 2, 2),
       ("bcc_w_primitive", "folded_222", 4, 2), ("bcc_mow", "skew_751_reflection", 2, 2), ("bcc_mow", "skew_821", 1, 1),
       ("bcc_mow", "perm_rotation_shift", 2, 2)]


@pytest.mark.parametrize("case", VEC, ids=_id)
def test_eigenpairs_of_the_described_cells(case):
    frame, label, n_a, n_b = case
    d = P.description(frame, label)
    q = _points()
    fc_b = _device_rows(frame, label, n_b)
    lam, vec = harmonic.mesh_eigenvectors(fc_b, d.atoms, q, n_b, P.masses(d.atoms))
    lam0, _ = harmonic.mesh_eigenvalues(fc_b, d.atoms, q, n_b, P.masses(d.atoms))
    assert np.array_equal(lam, lam0)
    res, orth = _pair_errors(harmonic.dynamical_matrices(fc_b, d.atoms, q, n_b, P.masses(d.atoms)), lam, vec)
    print(f"[phonon-redescribed] c {_id(case)}: max residual / |D|_F = {res:.3e}, max |V^H V - I| = {orth:.3e}")
    assert res <= 1e-11 and orth <= 1e-11


ALLOY = [("bcc_mow", "skew_751_reflection", 2, 2), ("bcc_mow", "perm_rotation_shift", 2, 2), ("bcc_mow", "skew_821", 1, 1),
         ("mow_skew3", "skew_821", 2, 2), ("mow_skew3", "skew_821", 3, 3)]
MIN_GAP = 1e-3                     # of max |lam|: between every two neighbouring modes of a q-point that is compared


@pytest.mark.parametrize("case", ALLOY, ids=_id)
def test_group_velocities_turn_with_the_crystal(case):
    """v_B(q', s) = Q v_A(q, s), mode by mode in ascending order, where no two modes are close: the q-points of a seeded list at
    which the host route's eigenvalues (``eigvalsh`` on the base's device rows) keep a gap of MIN_GAP max|lam| between every two
    neighbours -- at least four of them, asserted -- so that a mode's vector is defined to ~1e-16 / MIN_GAP."""
    frame, label, n_a, n_b = case
    a, d = P.base(frame), P.description(frame, label)
    fc_a = _device_rows(frame, None, n_a)
    fc_b = P.mapped_rows(fc_a, a, n_a, d, n_b)
    q_b = np.random.default_rng(37).uniform(-0.5, 0.5, (128, 3))
    q_a = P.map_q(a, d, q_b)
    host = np.linalg.eigvalsh(harmonic.dynamical_matrices(fc_a, a, q_a, n_a, P.masses(a)))
    gap = np.diff(host, axis=1).min(axis=1) / np.abs(host).max(axis=1)
    keep = np.zeros(len(gap), dtype=bool)
    keep[np.flatnonzero(gap >= MIN_GAP)[:16]] = True                   # (the first sixteen such points)
    assert keep.sum() >= 4, keep.sum()
    q_a, q_b = q_a[keep], q_b[keep]
    assert (np.diff(host[keep], axis=1).min(axis=1) / np.abs(host[keep]).max(axis=1)).min() >= MIN_GAP
    lam_a, _, vel_a = harmonic.mesh_eigenvectors(fc_a, a, q_a, n_a, P.masses(a), velocities=True, cutoff_THz=CUTOFF)
    lam_b, _, vel_b = harmonic.mesh_eigenvectors(fc_b, d.atoms, q_b, n_b, P.masses(d.atoms), velocities=True, cutoff_THz=CUTOFF)
    terms, w = harmonic.image_terms(a, n_a)
    cell = np.asarray(a.get_cell(), float)
    scale = VR.velocity_scale(VR.d_dynamical_from_terms(fc_a, terms, w, q_a, P.masses(a)), lam_a, cell)
    err = np.abs(vel_b - vel_a @ d.Q.T).max(axis=2)
    print(f"[phonon-redescribed] c {_id(case)}: {int(keep.sum())} q-points with gaps >= {MIN_GAP:.0e} (smallest {gap[keep].min():.2e}); "
          f"max velocity error / scale = {(err / scale).max():.3e}, max |v| {np.abs(vel_a).max():.3e} THz A")
    assert _gap(lam_b, lam_a, q_b) <= LAM_TOL
    assert np.any(vel_a != 0) and np.all(np.isfinite(vel_b))
    assert np.all(err <= VEL_TOL * scale)


MESHES = [("bcc_mow", "skew_751_reflection", 1, 1, (3, 3, 3), (3, 3, 3)), ("bcc_mow", "perm_rotation_shift", 2, 2, (2, 2, 2), (2, 2, 2)),
          ("mow_skew3", "skew_821", 2, 2, (4, 4, 4), (4, 4, 4)), ("w_conv2", "skew_821", 3, 3, (5, 5, 5), (5, 5, 5)),
          ("bcc_w_primitive", "skew_rotation", 3, 3, (6, 6, 6), (6, 6, 6)), ("bcc_w_primitive", "folded_222", 4, 2, (4, 4, 4), (2, 2, 2))]


def _mesh_bijection(a, d, mesh_a, mesh_b):
    """The description's full mesh, mapped, is the base's full mesh modulo reciprocal lattice vectors: every point of mesh_a is
    hit by exactly ``1`` folded image of the points of mesh_b (asserted on integers)."""
    q_b, _ = harmonic.qmesh(mesh_b, time_reversal=False)
    q_a = P.fold_q(a, d, q_b).reshape(-1, 3)
    idx = q_a * np.asarray(mesh_a)
    assert np.abs(idx - np.rint(idx)).max() <= 1e-9
    flat = np.ravel_multi_index(tuple((np.rint(idx).astype(np.int64) % np.asarray(mesh_a)).T), mesh_a)
    assert np.array_equal(np.sort(flat), np.arange(int(np.prod(mesh_a))))
    return q_b, q_a


@functools.lru_cache(maxsize=None)
def _mesh_pairs(case, time_reversal):
    """(lam, vec, w, masses) of the base on mesh_a and of the description (mapped force constants) on mesh_b"""
    frame, label, n_a, n_b, mesh_a, mesh_b = case
    a, d = P.base(frame), P.description(frame, label)
    _mesh_bijection(a, d, mesh_a, mesh_b)
    fc_a = _device_rows(frame, None, n_a)
    fc_b = P.mapped_rows(fc_a, a, n_a, d, n_b)
    out = []
    for atoms, fc, n, mesh in ((a, fc_a, n_a, mesh_a), (d.atoms, fc_b, n_b, mesh_b)):
        q, w = harmonic.qmesh(mesh, time_reversal=time_reversal)
        lam, vec = harmonic.mesh_eigenvectors(fc, atoms, q, n, P.masses(atoms))
        out.append((lam, vec, w, P.masses(atoms), q))
    return out


def _flat_gamma(lam, q):
    """The eigenvalues with Gamma's three acoustic modes at their exact value, 0 (tests/test_gpu_phonon_vec.py: rounding under
    the square root there is a different 1e-7 THz on every route)."""
    f = PR.frequencies(lam)
    flat = np.abs(f) <= CUTOFF
    assert flat.sum() == 3 and flat[np.all(q == 0, axis=1)].sum() == 3
    return np.where(flat, 0.0, lam)


@pytest.mark.parametrize("case", MESHES, ids=_id)
def test_pdos_and_displacement_tensors_through_src(case):
    """Per atom: g_B[k] = g_A[src[k]] and U_B[k] = Q U_A[src[k]] Q^T, on meshes that map onto each other; on the folded
    primitive cell all eight atoms carry the primitive atom's."""
    frame, label = case[:2]
    d = P.description(frame, label)
    (lam_a, vec_a, w_a, m_a, q_a), (lam_b, vec_b, w_b, m_b, q_b) = _mesh_pairs(case, True)
    f = harmonic.eigenvalues_to_frequencies(lam_a)
    sigma = 0.15
    s = np.linspace(f.min() - 6 * sigma, f.max() + 6 * sigma, 121)
    per_atom = lambda g: g.reshape(g.shape[0] // 3, 3, -1).sum(axis=1)                                  # noqa: E731
    g_a = per_atom(harmonic.pdos_from_eigenvectors(_flat_gamma(lam_a, q_a), vec_a, w_a, samples=s, sigma=sigma))
    g_b = per_atom(harmonic.pdos_from_eigenvectors(_flat_gamma(lam_b, q_b), vec_b, w_b, samples=s, sigma=sigma))
    e_pdos = np.abs(g_b - g_a[d.src]).max() / g_a.max()
    u_a, nx_a = harmonic.tdisp_from_eigenvectors(lam_a, vec_a, m_a, TEMPS, w_a, cutoff_THz=CUTOFF)
    u_b, nx_b = harmonic.tdisp_from_eigenvectors(lam_b, vec_b, m_b, TEMPS, w_b, cutoff_THz=CUTOFF)
    _, abs_a, _ = VR.displacement_tensors(lam_a, vec_a, w_a, m_a, TEMPS, cutoff=CUTOFF)
    turn = lambda t, Q: np.einsum("ab,tkbc,dc->tkad", Q, harmonic.voigt6_to_tensors(t)[:, d.src], Q)    # noqa: E731
    want, scale = turn(u_a, d.Q), turn(abs_a, np.abs(d.Q))
    e_u = (np.abs(harmonic.voigt6_to_tensors(u_b) - want) / scale).max()
    print(f"[phonon-redescribed] c {_id(case)}: per-atom PDOS err / max g = {e_pdos:.3e}, U err / sum|terms| = {e_u:.3e}")
    # (the seeded Mo/W model has imaginary modes, excluded and counted with Gamma's three; tungsten has none)
    assert nx_a == nx_b and (nx_a == 3 or P.frames()[frame][2] != "unary")
    assert g_b.shape[0] == len(d.atoms) and e_pdos <= END_TOL
    assert np.all(np.abs(harmonic.voigt6_to_tensors(u_b) - want) <= END_TOL * scale)
    if label == "folded_222":
        assert len(d.atoms) == 8 and np.all(d.src == 0)


# ---- d. mesh level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("time_reversal", [True, False])
@pytest.mark.parametrize("case", MESHES, ids=_id)
def test_histogram_dos_and_thermodynamics_of_mapped_meshes(case, time_reversal):
    frame, label = case[:2]
    d = P.description(frame, label)
    (lam_a, _, w_a, _, q_a), (lam_b, _, w_b, _, q_b) = _mesh_pairs(case, time_reversal)
    f_a = harmonic.eigenvalues_to_frequencies(lam_a)
    edges = _guarded_edges(f_a)
    # the edges, as eigenvalues, are clear of every eigenvalue of either side by more than the eigenvalue bound
    lam_e = np.sign(edges) * (edges / harmonic.THZ) ** 2
    clear = min(np.abs(lam_a.ravel()[None, :] - lam_e[:, None]).min(), np.abs(lam_b.ravel()[None, :] - lam_e[:, None]).min())
    assert clear > LAM_TOL * np.abs(lam_a).max(), clear
    c_a, _ = harmonic.dos_from_eigenvalues(lam_a, w_a, edges=edges)
    c_b, _ = harmonic.dos_from_eigenvalues(lam_b, w_b, edges=edges)
    assert c_a.dtype == np.int64 and np.array_equal(c_a, c_b) and c_a.sum() == lam_a.shape[1] * w_a.sum()
    sigma = 0.15
    s = np.linspace(f_a.min() - 6 * sigma, f_a.max() + 6 * sigma, 201)
    _, g_a = harmonic.dos_from_eigenvalues(_flat_gamma(lam_a, q_a), w_a, samples=s, sigma=sigma)
    _, g_b = harmonic.dos_from_eigenvalues(_flat_gamma(lam_b, q_b), w_b, samples=s, sigma=sigma)
    e_dos = np.abs(d.scale * g_a - g_b).max() / g_b.max()
    t_a = harmonic.thermo_from_eigenvalues(lam_a, TEMPS, w_a, cutoff_THz=CUTOFF)
    t_b = harmonic.thermo_from_eigenvalues(lam_b, TEMPS, w_b, cutoff_THz=CUTOFF)
    ref = PR.thermo(f_a, w_a, TEMPS, cutoff=CUTOFF)
    worst = 0.0
    for key, short in (("free_energy", "F"), ("internal_energy", "U"), ("entropy", "S"), ("heat_capacity", "Cv")):
        rel = np.abs(t_b[key] - d.scale * t_a[key])[1:] / (d.scale * ref["abs_" + short][1:])
        worst = max(worst, float(rel.max()))
        assert np.all(rel <= END_TOL), (key, rel)
    print(f"[phonon-redescribed] d {_id(case)} time_reversal={time_reversal}: counts identical ({int(c_a.sum())} modes), smeared DOS "
          f"err / max g = {e_dos:.3e}, thermodynamics max rel = {worst:.3e}")
    assert e_dos <= END_TOL
    assert abs(t_b["zero_point_energy"] - d.scale * t_a["zero_point_energy"]) <= END_TOL * d.scale * t_a["zero_point_energy"]
    assert t_a["n_excluded"] == t_b["n_excluded"] and (t_a["n_excluded"] == 3 or P.frames()[frame][2] != "unary")


# ---- e. sizes --------------------------------------------------------------------------------------------------------------------
def _random_problem(n):
    rng = np.random.default_rng(100 + n)
    atoms = Atoms(numbers=[74] * n, positions=rng.uniform(0, 40, (n, 3)), cell=np.eye(3) * 40.0, pbc=True)
    return rng.normal(size=(n, n, 3, 3)), rng.uniform(20, 200, n), atoms, rng.uniform(-0.5, 0.5, (3, 3))


def test_eigenvalues_at_every_size():
    """N = 1 .. 32 through n_super = 1 (``test_random_hermitian_at_the_size_limit``'s construction): the round-robin pairing and
    the lane split depend on 3N's parity and on the pair count modulo the wave."""
    worst = {}
    for n in range(1, harmonic.MESH_MAX_ATOMS + 1):
        fc, m, atoms, q = _random_problem(n)
        lam, sweeps = harmonic.mesh_eigenvalues(fc, atoms, q, 1, m)
        ref = np.linalg.eigvalsh(harmonic.dynamical_matrices(fc, atoms, q, 1, m))
        worst[n] = float((np.abs(lam - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())
        assert 0 <= sweeps.min() and sweeps.max() <= 15, (n, sweeps)
        assert np.all(np.diff(lam, axis=1) >= 0), n
    top = max(worst, key=worst.get)
    print(f"[phonon-redescribed] e eigenvalues N = 1 .. 32: worst max |dlam| / max|lam| = {worst[top]:.3e} at N = {top}")
    assert all(v <= 1e-11 for v in worst.values()), worst


def test_eigenvectors_at_every_size():
    worst_r, worst_o = {}, {}
    for n in range(1, harmonic.VEC_MAX_ATOMS + 1):
        fc, m, atoms, q = _random_problem(n)
        lam, vec = harmonic.mesh_eigenvectors(fc, atoms, q, 1, m)
        assert np.array_equal(lam, harmonic.mesh_eigenvalues(fc, atoms, q, 1, m)[0]), n
        worst_r[n], worst_o[n] = _pair_errors(harmonic.dynamical_matrices(fc, atoms, q, 1, m), lam, vec)
    print(f"[phonon-redescribed] e eigenvectors N = 1 .. 21: worst residual / |D|_F = {max(worst_r.values()):.3e}, "
          f"worst |V^H V - I| = {max(worst_o.values()):.3e}")
    assert all(v <= 1e-11 for v in worst_r.values()), worst_r
    assert all(v <= 1e-11 for v in worst_o.values()), worst_o


def test_exact_degeneracies_at_48_modes():
    """The unrattled 2 x 2 x 2 conventional W cell at Gamma and at the zone-boundary point (1/2, 0, 0): clusters of up to 12
    and 8 exactly equal eigenvalues, within 15 sweeps (13 and 13 on the MI355X).  At (1/2, 1/2, 1/2) -- clusters of 16 -- the
    same accuracy, but 16 sweeps: the stopping test off(D)_F <= 2^-52 |D|_F sits at the level of the rounding a sweep itself
    leaves inside a degenerate cluster.  That point is held to convergence within the kernel's own guard, PH_MAX_SWEEPS = 30
    (a status >= 0), not to 15."""
    atoms = P.conv16()
    m = P.masses(atoms)
    fc = harmonic._supercell_rows(_calc("unary"), atoms, 1)
    q = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.5, 0.5, 0.5]])
    lam, sweeps = harmonic.mesh_eigenvalues(fc, atoms, q, 1, m)
    D = harmonic.dynamical_matrices(fc, atoms, q, 1, m)
    ref = np.linalg.eigvalsh(D)
    err = float((np.abs(lam - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())
    lam2, vec = harmonic.mesh_eigenvectors(fc, atoms, q, 1, m)
    res, orth = _pair_errors(D, lam2, vec)
    biggest = [max(len(g) for g in VR.clusters(ref[k])) for k in range(len(q))]
    print(f"[phonon-redescribed] e degenerate 48 x 48: max |dlam| / max|lam| = {err:.3e}, residual {res:.3e}, |V^H V - I| {orth:.3e}, "
          f"sweeps {sweeps.tolist()}, largest clusters {biggest}")
    assert min(biggest) >= 3 and lam.shape == (3, 48)
    assert np.array_equal(lam, lam2)
    assert err <= 1e-11 and res <= 1e-11 and orth <= 1e-11
    assert 0 <= sweeps[:2].min() and sweeps[:2].max() <= 15
    assert 0 <= sweeps[2] <= 30
