"""Eigenvectors on the q-mesh (uf3_phonon_mesh_vec / _pdos / _tdisp): eigenvalues bit for bit those of
uf3_phonon_mesh, eigenpairs against the host route's D(q) by residual and orthonormality (never against ``eigh``'s basis), group
velocities against the Hellmann-Feynman restatement on the device's own vectors, against ``eigh`` by cluster sums and against
central differences of the device's eigenvalues, the projected DOS and the displacement tensors against ``_phonon_vec_ref``,
repeatability, slab invariance, refusals, the calculator's methods.  Cells and force constants are ``test_gpu_phonon``'s."""
import warnings

import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import harmonic
import _phonon_ref as PR
import _phonon_vec_ref as VR
from test_gpu_phonon import CASES, CUTOFF, W_MASS, MOW_MASS, _calc, _case, _prim, _test_points, _unary_model

pytestmark = pytest.mark.gpu

ALL = list(CASES) + ["w_conv4"]
TEMPS = [0.0, 1.0, 300.0, 3000.0]
_memo = {}


def _points(name):
    """200 random q, Gamma and the zone-boundary points of ``test_gpu_phonon``, and (0, 1/2, 3/8); a 4^3 mesh on the 16-atom cell."""
    if name == "mow16":
        return harmonic.qmesh((4, 4, 4), time_reversal=False)[0]
    return np.concatenate([_test_points()[:212], [[0.0, 0.5, 0.375]]])


def _setup(name, q):
    calc, atoms, m, n_super, fc = _case(name)
    return harmonic._mesh_vec_setup(fc, atoms, q, n_super, m, "test"), harmonic._mesh_context(calc.device)


def _dev_vec(name, q, evec=True, gvel=True, cutoff=CUTOFF):
    """(lam, status, vec, vel) of one uf3_phonon_mesh_vec call."""
    (n, n_sc, flat, ism, terms, w, q, cell), ctx = _setup(name, q)
    return harmonic._mesh_vec_call(ctx, n, n_sc, flat, ism, terms, w, q, cell, cutoff, evec, gvel)


def _data(name):
    """The case's points, the device's eigenpairs and velocities there, the host route's D(q) and the restated dD / dq: once."""
    if name not in _memo:
        calc, atoms, m, n_super, fc = _case(name)
        q = _points(name)
        lam, status, vec, vel = _dev_vec(name, q)
        terms, w = harmonic.image_terms(atoms, n_super)
        _memo[name] = dict(q=q, lam=lam, status=status, vec=vec, vel=vel, m=m,
                           D=harmonic.dynamical_matrices(fc, atoms, q, n_super, m),
                           dD=VR.d_dynamical_from_terms(fc, terms, w, q, m),
                           cell=np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3))
    return _memo[name]


def _pair_errors(D, lam, vec):
    """(max_s |D v_s - lam_s v_s|_2 / |D|_F, max |V^H V - I|), the worst over the q-points."""
    r = D @ vec - vec * lam[:, None, :]
    res = np.sqrt((np.abs(r) ** 2).sum(axis=1)).max(axis=1) / np.sqrt((np.abs(D) ** 2).sum(axis=(1, 2)))
    orth = np.abs(np.conj(np.transpose(vec, (0, 2, 1))) @ vec - np.eye(vec.shape[1])).max()
    return float(res.max()), float(orth)


def _velocity_errors(vel, ref, scale):
    """(every |v - v_ref| within 1e-12 scale -- also where the scale is 0 --, the worst error / scale where the scale is not 0)."""
    err = np.abs(vel - ref).max(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(scale > 0, err / scale, 0.0)
    return bool(np.all(err <= 1e-12 * scale)), float(ratio.max())


@pytest.mark.parametrize("name", ALL)
def test_eigenvalues_are_those_of_the_eigenvalue_entry(name):
    d = _data(name)
    calc, atoms, m, n_super, fc = _case(name)
    lam, status = harmonic.mesh_eigenvalues(fc, atoms, d["q"], n_super, m, device=calc.device)
    assert np.array_equal(d["lam"], lam) and np.array_equal(d["status"], status)
    lam2, _, none, vel = _dev_vec(name, d["q"], evec=False)
    lam3, _, vec, none2 = _dev_vec(name, d["q"], gvel=False)
    assert none is None and none2 is None
    assert np.array_equal(lam2, lam) and np.array_equal(lam3, lam)
    assert np.array_equal(vel, d["vel"]) and np.array_equal(vec, d["vec"])


@pytest.mark.parametrize("name", ALL)
def test_eigenpairs_by_residual_and_orthonormality(name):
    """max_s |D v_s - lam_s v_s| <= 1e-11 |D|_F and max |V^H V - I| <= 1e-11 per q, D the host route's: any orthonormal set with
    these residuals is a correct decomposition, degenerate cells included."""
    d = _data(name)
    res, orth = _pair_errors(d["D"], d["lam"], d["vec"])
    print(f"[phonon-vec] {name}: max residual / |D|_F = {res:.3e}, max |V^H V - I| = {orth:.3e}")
    assert res <= 1e-11 and orth <= 1e-11


def test_random_hermitian_at_the_vector_size_limit():
    """N = 21 (3N = 63: D, V and the rotation records take 128 544 bytes of LDS) on random force constants, n_super = 1; one
    atom more is refused."""
    n = harmonic.VEC_MAX_ATOMS
    rng = np.random.default_rng(11)
    fc = rng.normal(size=(n, n, 3, 3))
    m = rng.uniform(20, 200, n)
    atoms = Atoms(numbers=[74] * n, positions=rng.uniform(0, 40, (n, 3)), cell=np.eye(3) * 40.0, pbc=True)
    q = rng.uniform(-0.5, 0.5, (5, 3))
    lam, vec, vel = harmonic.mesh_eigenvectors(fc, atoms, q, 1, m, velocities=True)
    lam0, _ = harmonic.mesh_eigenvalues(fc, atoms, q, 1, m)
    assert np.array_equal(lam, lam0)
    res, orth = _pair_errors(harmonic.dynamical_matrices(fc, atoms, q, 1, m), lam, vec)
    print(f"[phonon-vec] random 63 x 63: max residual / |D|_F = {res:.3e}, max |V^H V - I| = {orth:.3e}")
    assert res <= 1e-11 and orth <= 1e-11
    terms, w = harmonic.image_terms(atoms, 1)
    dD = VR.d_dynamical_from_terms(fc, terms, w, q, m)
    cell = np.eye(3) * 40.0
    ok, worst = _velocity_errors(vel, VR.velocities(dD, vec, lam, cell, CUTOFF), VR.velocity_scale(dD, lam, cell))
    print(f"[phonon-vec] random 63 x 63: max velocity error / scale = {worst:.3e}")
    assert ok
    big = Atoms(numbers=[74] * (n + 1), positions=rng.uniform(0, 40, (n + 1, 3)), cell=np.eye(3) * 40.0, pbc=True)
    with pytest.raises(ValueError, match="at most 21 atoms"):
        harmonic.mesh_eigenvectors(rng.normal(size=(n + 1, n + 1, 3, 3)), big, q, 1, np.ones(n + 1))


@pytest.mark.parametrize("name", ["w_prim", "w_conv"])
def test_wave_kernel_at_small_cells(name, monkeypatch):
    """UF3_PHONON_WAVE sends the small cells through the wave-per-q instance (3N = 3: an odd dimension with a padding index)."""
    d = _data(name)
    q = d["q"]
    calc, atoms, m, n_super, fc = _case(name)
    monkeypatch.setenv("UF3_PHONON_WAVE", "1")
    lam0, status0 = harmonic.mesh_eigenvalues(fc, atoms, q, n_super, m, device=calc.device)
    lam, status, vec, vel = _dev_vec(name, q)
    monkeypatch.delenv("UF3_PHONON_WAVE")
    assert np.array_equal(lam, lam0) and np.array_equal(status, status0)
    res, orth = _pair_errors(d["D"], lam, vec)
    print(f"[phonon-vec] {name} (wave kernel): max residual / |D|_F = {res:.3e}, max |V^H V - I| = {orth:.3e}")
    assert res <= 1e-11 and orth <= 1e-11
    ok, worst = _velocity_errors(vel, VR.velocities(d["dD"], vec, lam, d["cell"], CUTOFF), VR.velocity_scale(d["dD"], lam, d["cell"]))
    print(f"[phonon-vec] {name} (wave kernel): max velocity error / scale = {worst:.3e}")
    assert ok


@pytest.mark.parametrize("name", ["w_prim", "w_conv", "mow16"])
def test_repeatable_and_slab_invariant(name, monkeypatch):
    d = _data(name)
    q = d["q"]
    lam, status, vec, vel = _dev_vec(name, q)
    assert np.array_equal(vec, d["vec"]) and np.array_equal(vel, d["vel"])
    cut = 37
    a, b = _dev_vec(name, q[:cut]), _dev_vec(name, q[cut:])
    for k in range(4):
        assert np.array_equal(np.concatenate([a[k], b[k]]), (lam, status, vec, vel)[k]), k
    # the Python layer's own slabs: 7 q-points each
    calc, atoms, m, n_super, fc = _case(name)
    monkeypatch.setattr(harmonic, "VEC_SLAB_BYTES", 7 * 16 * lam.shape[1] ** 2)
    assert harmonic.vector_slab(lam.shape[1]) == 7
    l2, v2, g2 = harmonic.mesh_eigenvectors(fc, atoms, q, n_super, m, velocities=True, device=calc.device)
    assert np.array_equal(l2, lam) and np.array_equal(v2, vec) and np.array_equal(g2, vel)


# ---------------------------------------------------------------------------------------------------------------- projected DOS
def _mesh_pairs(name, mesh):
    key = (name, "mesh", mesh)
    if key not in _memo:
        calc, atoms, m, n_super, fc = _case(name)
        q, w = harmonic.qmesh(mesh)
        lam, vec = harmonic.mesh_eigenvectors(fc, atoms, q, n_super, m, device=calc.device)
        hl, hv = np.linalg.eigh(harmonic.dynamical_matrices(fc, atoms, q, n_super, m))
        _memo[key] = (q, w, lam, vec, hl, hv, m)
    return _memo[key]


PDOS_CASES = [("w_prim", (8, 8, 8)), ("w_conv", (8, 8, 8)), ("mow16", (4, 4, 4)), ("w_conv4", (4, 4, 4))]


@pytest.mark.parametrize("name,mesh", PDOS_CASES)
def test_projected_dos(name, mesh):
    """Against the restatement on the device's own lam and evec (1e-12 of max g), summed over channels against uf3_phonon_dos
    (1e-12), end to end against eigh on the host route's D (1e-9).  As computed, the end-to-end figure is 9.4e-16 (W primitive),
    1.5e-9 (conventional), 9.0e-10 (16-atom), 7.5e-9 (4-atom) on the MI355X: all of it Gamma's three acoustic modes, see below;
    with their eigenvalues at the exact 0 on both sides it is <= 8.1e-14."""
    q, w, lam, vec, hl, hv, m = _mesh_pairs(name, mesh)
    f = harmonic.eigenvalues_to_frequencies(lam)
    sigma = 0.15
    s = np.linspace(f.min() - 6 * sigma, f.max() + 6 * sigma, 301)
    g = harmonic.pdos_from_eigenvectors(lam, vec, w, samples=s, sigma=sigma)
    assert g.shape == (lam.shape[1], len(s))
    assert np.array_equal(g, harmonic.pdos_from_eigenvectors(lam, vec, w, samples=s, sigma=sigma))
    pick = np.linspace(0, len(s) - 1, 25).astype(int)
    ref = VR.projected_dos(f, vec, w, s[pick], sigma)
    _, total = harmonic.dos_from_eigenvalues(lam, w, samples=s, sigma=sigma)
    e_ref = np.abs(g[:, pick] - ref).max() / ref.max()
    e_sum = np.abs(g.sum(axis=0) - total).max() / total.max()
    # End to end against eigh on the host route's D.  Gamma's three acoustic modes have lam = 0 by the sum rule and +-1e-16 |D| of
    # rounding on either route, which the square root turns into +-1e-7 THz -- a different figure per mode and per solver, so
    # that a channel's Gaussians there differ by 1e-8 of max g between ANY two correct routes (measured: the raw figure printed
    # below).  The modes under the cut-off on both routes therefore take their exact eigenvalue, 0, on both sides; every vector,
    # and every other frequency, is as computed.
    fh = PR.frequencies(hl)
    flat = (np.abs(f) <= CUTOFF) & (np.abs(fh) <= CUTOFF)
    assert flat.sum() == 3 and flat[np.all(q == 0, axis=1)].sum() == 3
    g0 = harmonic.pdos_from_eigenvectors(np.where(flat, 0.0, lam), vec, w, samples=s, sigma=sigma)
    end = VR.projected_dos(np.where(flat, 0.0, fh), hv, w, s[pick], sigma)
    e_end = np.abs(g0[:, pick] - end).max() / end.max()
    e_raw = np.abs(g[:, pick] - VR.projected_dos(fh, hv, w, s[pick], sigma)).max() / end.max()
    print(f"[phonon-vec] {name} {mesh}: PDOS err / max g: restatement {e_ref:.3e}, channel sum against the total DOS {e_sum:.3e}, "
          f"end to end {e_end:.3e} (with both routes' noise at Gamma's acoustic modes: {e_raw:.3e})")
    assert e_ref <= 1e-12
    assert e_sum <= 1e-12
    assert e_end <= 1e-9
    # ... and the raw figure within what 1e-5 THz (section 3.12's bound on that noise) can move three Gaussians of weight 1 / sum w
    slope = np.exp(-0.5) / (sigma * sigma * np.sqrt(2.0 * np.pi))
    assert e_raw <= 1e-9 + 3.0 / w.sum() * slope * 1e-5 / end.max()
    # without weights: the full mesh gives what the reduced one gives with them
    if name == "w_prim":
        calc, atoms, mm, n_super, fc = _case(name)
        qf, _ = harmonic.qmesh(mesh, time_reversal=False)
        lf, vf = harmonic.mesh_eigenvectors(fc, atoms, qf, n_super, mm, device=calc.device)
        gf = harmonic.pdos_from_eigenvectors(lf, vf, None, samples=s, sigma=sigma)
        assert np.abs(gf - g).max() <= 1e-12 * g.max()


def test_projected_dos_by_species_sums_to_the_total():
    calc, atoms, m, n_super, fc = _case("mow16")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        res = harmonic.projected_dos(calc, atoms, (2, 2, 2), n_super=n_super, masses=MOW_MASS, by="species", n_samples=101)
        tot = harmonic.density_of_states(calc, atoms, (2, 2, 2), n_super=n_super, masses=MOW_MASS, sigma=res["sigma"],
                                         frequencies=res["frequencies"])
    assert res["labels"] == ["Mo", "W"] and res["pdos"].shape == (2, 101) and res["channels"].shape == (48, 101)
    assert np.all(res["pdos"] >= 0) and res["pdos"][0].max() > 0 and res["pdos"][1].max() > 0
    assert np.abs(res["pdos"].sum(axis=0) - tot["dos"]).max() <= 1e-12 * tot["dos"].max()
    assert np.array_equal(res["mode_frequencies"], tot["mode_frequencies"])
    z = np.asarray(atoms.get_atomic_numbers())
    per_atom = res["channels"].reshape(16, 3, -1).sum(axis=1)
    assert np.abs(res["pdos"][0] - per_atom[z == 42].sum(axis=0)).max() <= 1e-14 * res["pdos"].max()


# ---------------------------------------------------------------------------------------------------------------- displacements
@pytest.mark.parametrize("name,mesh", PDOS_CASES)
def test_displacement_tensors(name, mesh):
    q, w, lam, vec, hl, hv, m = _mesh_pairs(name, mesh)
    u6, n_excl = harmonic.tdisp_from_eigenvectors(lam, vec, m, TEMPS, w, cutoff_THz=CUTOFF)
    u6b, _ = harmonic.tdisp_from_eigenvectors(lam, vec, m, TEMPS, w, cutoff_THz=CUTOFF)
    assert np.array_equal(u6, u6b)
    ref, scale, n_ref = VR.displacement_tensors(lam, vec, w, m, TEMPS, cutoff=CUTOFF)
    e_ref = (np.abs(u6 - ref) / scale).max()
    end, scale_end, _ = VR.displacement_tensors(hl, hv, w, m, TEMPS, cutoff=CUTOFF)
    e_end = (np.abs(u6 - end) / scale_end).max()
    print(f"[phonon-vec] {name} {mesh}: U err / sum|terms|: restatement {e_ref:.3e}, end to end {e_end:.3e}; "
          f"u_iso(300 K) = {u6[2, :, :3].mean(axis=1).tolist()}")
    assert np.all(np.abs(u6 - ref) <= 1e-12 * scale)
    assert np.all(np.abs(u6 - end) <= 1e-9 * scale_end)
    assert n_excl == n_ref == harmonic.thermo_from_eigenvalues(lam, TEMPS, w, cutoff_THz=CUTOFF)["n_excluded"]
    assert np.all(u6[:, :, :3] > 0) and np.all(np.diff(u6[:, :, :3], axis=0) >= 0) and np.all(u6[2:, :, :3] > u6[1:3, :, :3])
    if name in ("w_prim", "w_conv"):
        # cubic sites: U is isotropic
        bound = 1e-9 * scale_end
        assert np.all(np.abs(u6[:, :, 3:]) <= bound[:, :, 3:])
        assert np.all(np.abs(u6[:, :, 0] - u6[:, :, 1]) <= bound[:, :, 0]) and np.all(np.abs(u6[:, :, 1] - u6[:, :, 2]) <= bound[:, :, 1])


# ------------------------------------------------------------------------------------------------------------------- velocities
@pytest.mark.parametrize("name", ALL)
def test_velocities_against_the_restatement_on_the_device_vectors(name):
    """|v_dev - v_ref| <= 1e-12 |dD / dk|_F THZ / (2 sqrt|lam_s|) per mode, v_ref Hellmann-Feynman on the device's own vectors with
    dD / dq restated from the term records: no basis enters."""
    d = _data(name)
    ref = VR.velocities(d["dD"], d["vec"], d["lam"], d["cell"], CUTOFF)
    ok, worst = _velocity_errors(d["vel"], ref, VR.velocity_scale(d["dD"], d["lam"], d["cell"]))
    low = np.abs(PR.frequencies(d["lam"])) <= CUTOFF
    print(f"[phonon-vec] {name}: max velocity error / scale = {worst:.3e}; {int(low.sum())} mode(s) under the cut-off")
    assert ok
    assert np.all(d["vel"][low] == 0) and np.all(np.isfinite(d["vel"])) and np.any(d["vel"] != 0)
    # Gamma's three acoustic modes (and (1, 0, 0), the same matrix) are under the cut-off, and nothing else is
    same = np.all(d["q"] == np.round(d["q"]), axis=1)
    assert np.all(low[same].sum(axis=1) == 3) and not low[~same].any() and same.sum() >= 1


def test_velocity_cluster_sums_at_symmetric_points():
    """W primitive along Gamma-H and Gamma-P: the transverse branch is doubly degenerate, the members' velocities depend on the
    basis and their sum does not.  Cluster sums (clusters: gaps above 1e-6 max|lam|) against the restatement on ``eigh``'s
    vectors, within 1e-12 |dD / dk|_F THZ / (2 sqrt|lam|) times the cluster's size."""
    calc, atoms, m, n_super, fc = _case("w_prim")
    coords, _ = harmonic.standard_path(atoms)
    t = np.linspace(0.1, 0.9, 9)[:, None]
    q = np.concatenate([t * np.asarray(coords["H"])[None], t * np.asarray(coords["P"])[None]])
    lam, _, _, vel = _dev_vec("w_prim", q)
    D = harmonic.dynamical_matrices(fc, atoms, q, n_super, m)
    hl, hv = np.linalg.eigh(D)
    terms, w = harmonic.image_terms(atoms, n_super)
    dD = VR.d_dynamical_from_terms(fc, terms, w, q, m)
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    ref = VR.velocities(dD, hv, hl, cell, CUTOFF)
    scale = VR.velocity_scale(dD, hl, cell)
    worst, pairs = 0.0, 0
    for k in range(len(q)):
        groups = VR.clusters(hl[k])
        assert groups == VR.clusters(lam[k])
        pairs += any(len(g) >= 2 for g in groups)
        got, want = VR.cluster_sums(vel[k], groups), VR.cluster_sums(ref[k], groups)
        for gi, g in enumerate(groups):
            bound = 1e-12 * scale[k][g].max() * len(g)
            err = np.abs(got[gi] - want[gi]).max()
            worst = max(worst, err / bound)
            assert err <= bound, (k, g, err, bound)
    print(f"[phonon-vec] w_prim Gamma-H, Gamma-P: worst cluster-sum error / bound = {worst:.3e}, {pairs} points with a degenerate cluster")
    assert pairs == len(q)


@pytest.mark.parametrize("name,nq", [("mow16", 4), ("mow_skew3", 12)])
def test_velocities_against_central_differences(name, nq):
    """Modes whose gap to both neighbours exceeds 1e-3 max|lam|, at random q: the device's velocities against central differences
    of the device's eigenvalues at h = 1e-4 in reduced coordinates.  Tolerance: 4 x the discrepancy the NumPy pair shows on the
    same D(q) (``eigvalsh`` differences against Hellmann-Feynman on ``eigh``'s vectors), floor 1e-9 max|v| -- the differences'
    truncation error dominates both."""
    calc, atoms, m, n_super, fc = _case(name)
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    q = np.random.default_rng(17).uniform(-0.5, 0.5, (nq, 3))
    h = 1e-4
    steps = np.concatenate([s * h * np.eye(3) for s in (1.0, -1.0)])                    # +0 +1 +2 -0 -1 -2
    qs = np.concatenate([q] + [q + d for d in steps])
    lam_all, _, _, vel_all = _dev_vec(name, qs)
    lam, vel = lam_all[:nq], vel_all[:nq]
    D = harmonic.dynamical_matrices(fc, atoms, qs, n_super, m)
    hl_all = np.linalg.eigvalsh(D)
    hl, hv = np.linalg.eigh(D[:nq])
    terms, w = harmonic.image_terms(atoms, n_super)
    host_hf = VR.velocities(VR.d_dynamical_from_terms(fc, terms, w, q, m), hv, hl, cell, CUTOFF)

    def differences(l_all, l0):
        dq = np.stack([(l_all[(1 + a) * nq:(2 + a) * nq] - l_all[(4 + a) * nq:(5 + a) * nq]) / (2 * h) for a in range(3)], axis=-1)
        return PR.THZ * (dq @ cell) / (2.0 * np.sqrt(np.abs(l0)))[:, :, None]      # d lam / d k_c = sum_a (d lam / d q_a) cell[a][c]

    gap = np.diff(lam, axis=1) / np.abs(lam).max(axis=1, keepdims=True)
    big = np.ones_like(lam, dtype=bool)
    big[:, 1:] &= gap > 1e-3
    big[:, :-1] &= gap > 1e-3
    keep = big & (np.abs(PR.frequencies(lam)) > CUTOFF)
    assert keep.sum() * 2 >= keep.size, (keep.sum(), keep.size)
    host_gap = np.abs(differences(hl_all, hl) - host_hf)[keep].max()
    dev_gap = np.abs(differences(lam_all, lam) - vel)[keep].max()
    tol = max(4.0 * host_gap, 1e-9 * np.abs(vel[keep]).max())
    print(f"[phonon-vec] {name}: velocities against central differences, {int(keep.sum())} of {keep.size} modes kept: NumPy pair "
          f"{host_gap:.3e}, device {dev_gap:.3e} THz A (max |v| {np.abs(vel[keep]).max():.3e})")
    assert dev_gap <= tol


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_abi_refusals():
    """The library's own checks, called directly: UF3_EINVAL with a message, nothing launched."""
    ctx = _lib.get_context(0)
    lib, addr = ctx.lib, _lib._addr

    def err():
        return lib.uf3_last_error(ctx.handle).decode()

    def mesh(n=2, n_sc=16, nq=3, terms=None, null=None, cell=None, cutoff=1e-3, evec=True, gvel=True):
        fc = np.zeros((3 * n, 3 * n_sc))
        ism = np.ones(n)
        t = np.array([[0, 0, 0, 0, 0], [1, 1, 0, 0, 0]], dtype=np.int32) if terms is None else np.asarray(terms, dtype=np.int32)
        w = np.ones(len(t))
        k = max(nq, 1)
        q = np.zeros((k, 3))
        lam = np.zeros((k, 3 * n))
        st = np.zeros(k, dtype=np.int32)
        vec = np.zeros((k, 3 * n, 3 * n), dtype=complex)
        vel = np.zeros((k, 3 * n, 3))
        h = np.eye(3) * 3.0 if cell is None else np.asarray(cell, dtype=float)
        args = dict(fc=addr(fc), ism=addr(ism), t=addr(t), w=addr(w), q=addr(q), lam=addr(lam), st=addr(st), cell=addr(h))
        if null:
            args[null] = None
        return lib.uf3_phonon_mesh_vec(ctx.handle, n, n_sc, args["fc"], args["ism"], len(t), args["t"], args["w"], nq, args["q"],
                                       args["lam"], args["st"], args["cell"], cutoff, addr(vec) if evec else None,
                                       addr(vel) if gvel else None)

    assert mesh() == 0
    assert mesh(evec=False) == 0 and mesh(gvel=False) == 0
    assert mesh(evec=False, gvel=False) == 1 and "both NULL" in err()
    assert mesh(n=22, n_sc=22) == 1 and "limit with eigenvectors is 21" in err()
    assert mesh(n=33, n_sc=33) == 1 and "limit is 32" in err()
    assert mesh(nq=0) == 1 and "nq" in err()
    assert mesh(n_sc=15) == 1 and "multiple" in err()
    for bad in ([[2, 0, 0, 0, 0]], [[0, 16, 0, 0, 0]], [[0, -1, 0, 0, 0]]):
        assert mesh(terms=bad) == 1 and "outside" in err(), bad
    for name in ("lam", "st", "q", "fc", "t"):
        assert mesh(null=name) == 1 and "null" in err(), name
    singular = [[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]]
    assert mesh(cell=singular) == 1 and "singular" in err()
    assert mesh(cell=[[np.nan, 0, 0], [0, 1, 0], [0, 0, 1]]) == 1 and "finite" in err()
    assert mesh(cell=[[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]]) == 1 and "finite" in err()
    assert mesh(null="cell") == 1 and "cell" in err()
    assert mesh(cutoff=-1.0) == 1 and "cut-off" in err()
    assert mesh(cell=singular, gvel=False) == 0          # the cell is not looked at without the velocities
    assert mesh(null="cell", gvel=False) == 0

    lam = np.ones((4, 3))
    vec = np.zeros((4, 3, 3), dtype=complex)
    vec[:] = np.eye(3)
    samples = np.array([0.0, 1.0, 2.0])
    out = np.zeros((3, 3))

    def run_pdos(n_modes=3, nq=4, sigma=0.1, null=None, n_samples=3):
        a = dict(lam=addr(lam), vec=addr(vec), s=addr(samples), out=addr(out))
        if null:
            a[null] = None
        return lib.uf3_phonon_pdos(ctx.handle, n_modes, nq, a["lam"], a["vec"], None, n_samples, a["s"], sigma, a["out"])

    assert run_pdos() == 0
    assert run_pdos(nq=0) == 1 and "nq" in err()
    assert run_pdos(n_modes=4) == 1 and "multiple of 3" in err()
    assert run_pdos(n_modes=66) == 1 and "multiple of 3" in err()
    assert run_pdos(sigma=0.0) == 1 and "sigma" in err()
    assert run_pdos(n_samples=0) == 1 and "n_samples" in err()
    for name in ("lam", "vec", "out"):
        assert run_pdos(null=name) == 1 and "null" in err(), name
    assert run_pdos(null="s") == 1 and "sample" in err()

    u = np.zeros((2, 1, 6))
    nx = np.zeros(1, dtype=np.int64)

    def run_tdisp(n=1, nq=4, temps=(0.0, 300.0), cutoff=1e-3, ism=(0.1,), null=None):
        t = np.array(temps, dtype=float)
        mass = np.array(ism, dtype=float)
        a = dict(lam=addr(lam), vec=addr(vec), m=addr(mass), out=addr(u), nx=addr(nx))
        if null:
            a[null] = None
        return lib.uf3_phonon_tdisp(ctx.handle, n, nq, a["lam"], a["vec"], None, a["m"], len(t), addr(t), cutoff, a["out"], a["nx"])

    assert run_tdisp() == 0
    assert run_tdisp(nq=0) == 1 and "nq" in err()
    assert run_tdisp(n=22) == 1 and "[1, 21]" in err()
    assert run_tdisp(temps=(10.0, -1.0)) == 1 and "negative" in err()
    assert run_tdisp(cutoff=-1.0) == 1 and "cut-off" in err()
    assert run_tdisp(ism=(0.0,)) == 1 and "masses" in err()
    for name in ("lam", "vec", "m", "out", "nx"):
        assert run_tdisp(null=name) == 1 and "null" in err(), name
    # the Python layer refuses an oversized cell itself
    rng = np.random.default_rng(0)
    big = Atoms(numbers=[74] * 22, positions=rng.uniform(0, 9, (22, 3)), cell=np.eye(3) * 9.0, pbc=True)
    for fn in (lambda c: c.get_phonon_pdos(big, mesh=(2, 2, 2), masses=W_MASS),
               lambda c: c.get_thermal_displacements(big, [300.0], mesh=(2, 2, 2), masses=W_MASS),
               lambda c: c.get_group_velocities(big, [[0.1, 0, 0]], masses=W_MASS)):
        with pytest.raises(ValueError, match="at most 21 atoms"):
            fn(_calc(_unary_model()))


def test_calculator_surface():
    calc = _calc(_unary_model())
    prim = _prim()
    td = calc.get_thermal_displacements(prim, [0.0, 300.0], mesh=(8, 8, 8), n_super=4, masses=W_MASS)
    assert td["U"].shape == (2, 1, 3, 3) and td["u_iso"].shape == (2, 1) and td["n_excluded"] == 3 and td["n_imaginary"] == 0
    u = td["U"][1, 0]
    assert td["u_iso"][1, 0] > td["u_iso"][0, 0] > 0
    assert np.abs(u - np.eye(3) * td["u_iso"][1, 0]).max() <= 1e-9 * td["u_iso"][1, 0]
    assert 1e-4 < td["u_iso"][1, 0] < 1e-1                     # Angstrom^2: a metal at room temperature
    # near Gamma along x: |v| = f / |k| within 1 % (acoustic linearity), the longitudinal branch the fastest
    cell = np.asarray(prim.get_cell(), dtype=float)
    k = np.array([0.01, 0.0, 0.0])                              # Cartesian, 1 / Angstrom without 2 pi
    f, v = calc.get_group_velocities(prim, [cell @ k], n_super=4, masses=W_MASS)
    assert f.shape == (1, 3) and v.shape == (1, 3, 3)
    speed = np.linalg.norm(v[0], axis=1)
    assert np.all(f[0] > 0) and np.all(np.abs(speed - f[0] / 0.01) <= 0.01 * f[0] / 0.01)
    assert np.all(np.abs(v[0][:, 1:]) <= 1e-6 * speed.max())    # along the axis
    assert speed[2] > speed[1] * 1.05 and abs(speed[1] - speed[0]) <= 1e-6 * speed[1]
    pd = calc.get_phonon_pdos(prim, mesh=(8, 8, 8), n_super=4, masses=W_MASS, n_samples=201, by="channel")
    assert pd["pdos"].shape == (3, 201) and pd["labels"] == [(0, "x"), (0, "y"), (0, "z")] and pd["dos"].shape == (201,)
    g, s = pd["dos"], pd["frequencies"]
    assert abs(np.sum(0.5 * (g[1:] + g[:-1]) * np.diff(s)) - 3.0) <= 1e-6
    # cubic: the three channels alike, but for Gamma's acoustic modes -- rounding under a square root, up to 1e-5 THz each
    # (section 3.12), so three Gaussians of weight 1 / 512 may each sit that far apart: slope e^-1/2 / (sigma^2 sqrt(2 pi))
    slope = np.exp(-0.5) / (pd["sigma"] ** 2 * np.sqrt(2.0 * np.pi))
    assert np.abs(pd["pdos"][0] - pd["pdos"][1]).max() <= 1e-12 * g.max() + 3.0 / 512.0 * slope * 1e-5
    for fn in (lambda: calc.get_phonon_pdos(prim, mesh=(2, 2, 2), n_super=2),
               lambda: calc.get_thermal_displacements(prim, [300.0], mesh=(2, 2, 2), n_super=2),
               lambda: calc.get_group_velocities(prim, [[0.1, 0, 0]], n_super=2)):
        with pytest.raises(ValueError, match="harmonic: no masses"):
            fn()
