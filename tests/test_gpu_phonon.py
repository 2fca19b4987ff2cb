"""Phonons on a q-mesh (uf3_phonon_mesh / _dos / _thermo, uf3_amd.forcefield.harmonic): device eigenvalues against the host route
(``np.linalg.eigvalsh(harmonic.dynamical_matrices(...))``), the density of states and the thermodynamics against the NumPy
reference of ``_phonon_ref`` evaluated on the frequencies the device returned, repeatability, time reversal, refusals."""
import os

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator, harmonic
from uf3_amd.regression import least_squares as ls
import _phonon_ref as PR
from _util import GOLDEN

pytestmark = pytest.mark.gpu

A0_W = 3.17352
W_MASS = {"W": 183.84}
MOW_MASS = {"Mo": 95.95, "W": 183.84}
TEMPS = [0.0, 1.0, 10.0, 100.0, 300.0, 1000.0, 3000.0]
CUTOFF = 1e-3


def _unary_model():
    return ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json"))


def _mow_model():
    basis = synthetic.notebook_basis(["Mo", "W"])
    model = ls.WeightedLinearModel(basis)
    coeff = np.random.default_rng(31).normal(0, 0.05, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    model.coefficients = coeff
    return model


def _calc(model):
    return calculator.UFCalculator(model, md_skin=0.0)


def _prim(a=A0_W):
    return Atoms(numbers=[74], positions=[[0, 0, 0]], cell=0.5 * a * np.array([[-1, 1, 1], [1, -1, 1], [1, 1, -1]]), pbc=True)


def _conv(a=A0_W):
    return Atoms(numbers=[74, 74], positions=[[0, 0, 0], [a / 2] * 3], cell=np.eye(3) * a, pbc=True)


def _mow16():
    a = 3.2
    base = np.array([[0, 0, 0], [0.5, 0.5, 0.5]])
    grid = np.array(list(np.ndindex(2, 2, 2)), dtype=float)
    pos = ((grid[:, None, :] + base[None]) * a).reshape(-1, 3)
    rng = np.random.default_rng(5)
    pos = pos + rng.uniform(-0.05, 0.05, pos.shape)
    z = np.where(rng.random(16) < 0.5, 42, 74)
    z[0], z[1] = 42, 74
    return Atoms(numbers=z, positions=pos, cell=np.eye(3) * 2 * a, pbc=True)


def _skew3():
    cell = np.array([[3.2, 0.0, 0.0], [0.5, 3.3, 0.0], [0.4, 0.6, 4.9]])
    frac = np.array([[0.02, 0.05, 0.01], [0.48, 0.53, 0.34], [0.55, 0.41, 0.69]])
    return Atoms(numbers=[42, 74, 74], positions=frac @ cell, cell=cell, pbc=True)


def _conv4(a=A0_W):
    return Atoms(numbers=[74] * 4, positions=[[0, 0, 0], [a / 2] * 3, [a, 0, 0], [1.5 * a, a / 2, a / 2]],
                 cell=np.diag([2 * a, a, a]), pbc=True)


CASES = {
    "w_prim": (_unary_model, _prim, W_MASS, 5),
    "w_conv": (_unary_model, _conv, W_MASS, 5),
    "mow16": (_mow_model, _mow16, MOW_MASS, 2),
    "mow_skew3": (_mow_model, _skew3, MOW_MASS, 3),
}
EXTRA = {"w_conv4": (_unary_model, _conv4, W_MASS, 5)}      # (not among the cases every test runs over)
_cache = {}


def _case(name):
    """(calc, atoms, masses [N], n_super, fc_rows) of a case, the force constants computed once."""
    if name not in _cache:
        model, atoms, masses, n_super = CASES.get(name) or EXTRA[name]
        calc, atoms = _calc(model()), atoms()
        m = harmonic._masses(atoms, masses)
        _cache[name] = (calc, atoms, m, n_super, harmonic._supercell_rows(calc, atoms, n_super))
    return _cache[name]


def _host_lam(name, q):
    calc, atoms, m, n_super, fc = _case(name)
    return np.linalg.eigvalsh(harmonic.dynamical_matrices(fc, atoms, q, n_super, m))


def _host_freqs(name, q):
    calc, atoms, m, n_super, fc = _case(name)
    return harmonic.frequencies_from(harmonic.dynamical_matrices(fc, atoms, q, n_super, m))


def _dev_lam(name, q):
    calc, atoms, m, n_super, fc = _case(name)
    return harmonic.mesh_eigenvalues(fc, atoms, q, n_super, m, device=calc.device)


def _test_points():
    rng = np.random.default_rng(7)
    special = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5],
                        [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [1.0, 0, 0], [0.25, 0.25, 0.25], [-0.5, 0.5, 0.5]], dtype=float)
    return np.concatenate([rng.uniform(-0.5, 0.5, (200, 3)), special, harmonic.qmesh((8, 8, 8), time_reversal=False)[0]])


@pytest.mark.parametrize("name", list(CASES))
def test_eigenvalues_against_the_host_route(name):
    """|lam_dev - lam_host| <= 1e-11 max|lam| per q: the two differ by the order of a sum of ~1e3 terms per entry and by two
    backward-stable eigensolvers, ~1e-13 of the scale.  Every q converged in <= 15 sweeps."""
    q = _test_points()
    lam, sweeps = _dev_lam(name, q)
    ref = _host_lam(name, q)
    assert lam.shape == ref.shape
    assert np.all(np.diff(lam, axis=1) >= 0)
    scale = np.abs(ref).max(axis=1)
    err = np.abs(lam - ref).max(axis=1) / scale
    print(f"[phonon] {name}: max |dlam| / max|lam| = {err.max():.3e}, sweeps {sweeps.min()} .. {sweeps.max()}")
    assert sweeps.min() >= 0 and sweeps.max() <= 15
    assert err.max() <= 1e-11


def test_random_hermitian_at_the_size_limit():
    """N = 32 (3N = 96, 147 KB of LDS per wave) on random force constants and masses, n_super = 1."""
    n = harmonic.MESH_MAX_ATOMS
    rng = np.random.default_rng(11)
    fc = rng.normal(size=(n, n, 3, 3))
    m = rng.uniform(20, 200, n)
    atoms = Atoms(numbers=[74] * n, positions=rng.uniform(0, 40, (n, 3)), cell=np.eye(3) * 40.0, pbc=True)
    q = rng.uniform(-0.5, 0.5, (5, 3))
    lam, sweeps = harmonic.mesh_eigenvalues(fc, atoms, q, 1, m)
    ref = np.linalg.eigvalsh(harmonic.dynamical_matrices(fc, atoms, q, 1, m))
    err = np.abs(lam - ref).max() / np.abs(ref).max()
    print(f"[phonon] random 96 x 96: max |dlam| / max|lam| = {err:.3e}, sweeps {sweeps.max()}")
    assert err <= 1e-11 and 0 <= sweeps.min() and sweeps.max() <= 15


@pytest.mark.parametrize("name", ["w_prim", "w_conv"])
def test_wave_kernel_at_small_cells(name, monkeypatch):
    """UF3_PHONON_WAVE sends 3N <= 6 through the wave-per-q kernel (3N = 3: an odd dimension, one padding index in the round
    robin): the same eigenvalues within the bound, the lane-per-q ones to rounding."""
    q = _test_points()[:260]
    lane, _ = _dev_lam(name, q)
    monkeypatch.setenv("UF3_PHONON_WAVE", "1")
    wave, sweeps = _dev_lam(name, q)
    monkeypatch.delenv("UF3_PHONON_WAVE")
    ref = _host_lam(name, q)
    scale = np.abs(ref).max(axis=1)
    assert (np.abs(wave - ref).max(axis=1) / scale).max() <= 1e-11
    assert (np.abs(wave - lane).max(axis=1) / scale).max() <= 1e-13
    assert sweeps.min() >= 0 and sweeps.max() <= 15
    assert np.array_equal(_dev_lam(name, q)[0], lane)


def test_consistent_with_the_existing_surface():
    calc, atoms, m, n_super, fc = _case("w_conv")
    q = np.random.default_rng(2).uniform(-0.5, 0.5, (20, 3))
    f_dev, q_out, w = harmonic.mesh_frequencies(calc, atoms, qpoints=q, n_super=5, masses=W_MASS)
    f_host = harmonic.phonon_frequencies(calc, atoms, q, n_super=5, masses=W_MASS)
    assert np.array_equal(q_out, q) and np.all(w == 1)
    assert np.abs(f_dev - f_host).max() <= 1e-8          # (random q: no eigenvalue near zero)
    # the primitive cell's 3 bands are among the conventional cell's 6 at the same Cartesian q, on a 6^3 mesh
    prim = _prim()
    fp, qp, _ = harmonic.mesh_frequencies(calc, prim, mesh=(6, 6, 6), n_super=5, masses=W_MASS, time_reversal=False)
    kc = qp @ np.linalg.inv(np.asarray(prim.get_cell())).T
    qc = kc @ np.asarray(atoms.get_cell()).T
    fcv, _, _ = harmonic.mesh_frequencies(calc, atoms, qpoints=qc, n_super=5, masses=W_MASS)
    for k in range(len(qp)):
        away = np.abs(fp[k]) > 1e-2                      # sqrt near lam = 0 turns rounding into 1e-5 THz
        assert all(np.abs(fcv[k] - x).min() <= 1e-8 for x in fp[k][away]), k
        assert all(np.abs(fcv[k] - x).min() <= 1e-4 for x in fp[k][~away]), k


@pytest.mark.parametrize("name", ["w_prim", "mow16"])
def test_repeatable_and_slab_invariant(name):
    q = harmonic.qmesh((6, 6, 6))[0]
    a, _ = _dev_lam(name, q)
    b, _ = _dev_lam(name, q)
    assert np.array_equal(a, b)
    cut = 37
    parts = np.concatenate([_dev_lam(name, q[:cut])[0], _dev_lam(name, q[cut:])[0]])
    assert np.array_equal(parts, a)


def _guarded_edges(f_ref, n_edges=12):
    """Edges at the midpoints of the widest gaps between the sorted reference frequencies, none within 1e-2 THz of zero, plus
    one below and one above everything."""
    s = np.sort(np.asarray(f_ref).ravel())
    gaps = np.diff(s)
    mids = 0.5 * (s[1:] + s[:-1])
    ok = np.abs(mids) > 1e-2
    order = np.argsort(-(gaps * ok))[:n_edges]
    edges = np.sort(np.concatenate([[s[0] - 1.0], mids[order], [s[-1] + 1.0]]))
    edges = edges[np.concatenate([[True], np.diff(edges) > 0])]
    assert np.abs(s[None, :] - edges[:, None]).min() > 1e-6
    assert np.abs(edges).min() > 1e-2
    return edges


@pytest.mark.parametrize("name,mesh", [("w_prim", (12, 12, 12)), ("w_conv", (12, 12, 12)), ("w_conv", (5, 5, 5)), ("mow16", (4, 4, 4))])
def test_histogram_time_reversal_and_numpy(name, mesh):
    q_full, w_full = harmonic.qmesh(mesh, time_reversal=False)
    q_red, w_red = harmonic.qmesh(mesh, time_reversal=True)
    f_ref = _host_freqs(name, q_full)
    edges = _guarded_edges(f_ref)
    lam_full, _ = _dev_lam(name, q_full)
    lam_red, _ = _dev_lam(name, q_red)
    c_full, _ = harmonic.dos_from_eigenvalues(lam_full, w_full, edges=edges)
    c_red, _ = harmonic.dos_from_eigenvalues(lam_red, w_red, edges=edges)
    c_none, _ = harmonic.dos_from_eigenvalues(lam_full, None, edges=edges)
    want, _ = np.histogram(f_ref.ravel(), bins=edges)
    assert c_full.dtype == np.int64
    assert np.array_equal(c_full, want) and np.array_equal(c_none, want)
    assert np.array_equal(c_red, c_full)
    assert c_full.sum() == f_ref.shape[1] * w_full.sum()
    # numpy's bin rule at the edges themselves: half-open bins, the last one closed
    lam = (np.array([[1.0, 2.0, 3.0, 0.5, 3.5, 2.0]]) / harmonic.THZ) ** 2
    f = harmonic.eigenvalues_to_frequencies(lam)
    e = np.array([f[0, 0], f[0, 1], f[0, 2]])
    got, _ = harmonic.dos_from_eigenvalues(lam, [3], edges=e)
    assert np.array_equal(got, 3 * np.histogram(f.ravel(), bins=e)[0]) and got.tolist() == [3, 9]


@pytest.mark.parametrize("name,mesh", [("w_prim", (12, 12, 12)), ("w_conv", (12, 12, 12)), ("mow16", (4, 4, 4))])
def test_smeared_dos_against_the_reference(name, mesh):
    q, w = harmonic.qmesh(mesh)
    lam, _ = _dev_lam(name, q)
    f = harmonic.eigenvalues_to_frequencies(lam)
    assert np.array_equal(f, PR.frequencies(lam))
    sigma = 0.15
    lo, hi = f.min() - 6 * sigma, f.max() + 6 * sigma
    n_s = int(np.ceil((hi - lo) / (sigma / 4))) + 1
    s = np.linspace(lo, hi, n_s)
    assert s[1] - s[0] <= sigma / 4
    _, g = harmonic.dos_from_eigenvalues(lam, w, samples=s, sigma=sigma)
    _, g2 = harmonic.dos_from_eigenvalues(lam, w, samples=s, sigma=sigma)
    assert np.array_equal(g, g2)
    pick = np.linspace(0, n_s - 1, 97).astype(int)
    ref = PR.smeared_dos(f, w, s[pick], sigma)
    err = np.abs(g[pick] - ref).max() / ref.max()
    integral = float(np.sum(0.5 * (g[1:] + g[:-1]) * np.diff(s)))
    print(f"[phonon] {name} {mesh}: smeared DOS max err / max g = {err:.3e}, integral - 3N = {integral - f.shape[1]:.3e}")
    assert err <= 1e-12
    assert abs(integral - f.shape[1]) <= 1e-9


@pytest.mark.parametrize("name,mesh,gamma", [("w_prim", (12, 12, 12), True), ("w_conv", (12, 12, 12), True),
                                             ("w_conv", (12, 12, 12), False), ("mow16", (4, 4, 4), True)])
def test_thermodynamics_against_the_reference(name, mesh, gamma):
    q, w = harmonic.qmesh(mesh, gamma_centred=gamma)
    lam, _ = _dev_lam(name, q)
    f = harmonic.eigenvalues_to_frequencies(lam)
    n3 = f.shape[1]
    got = harmonic.thermo_from_eigenvalues(lam, TEMPS, w, cutoff_THz=CUTOFF)
    ref = PR.thermo(f, w, TEMPS, cutoff=CUTOFF)
    keys = (("free_energy", "F"), ("internal_energy", "U"), ("entropy", "S"), ("heat_capacity", "Cv"))
    for key, short in keys:
        err = np.abs(got[key] - ref[short])
        bound = 1e-12 * ref["abs_" + short]
        print(f"[phonon] {name} {mesh} gamma={gamma} {short}: max err / sum|terms| = "
              f"{(err[1:] / ref['abs_' + short][1:]).max():.3e}")
        assert np.all(err <= bound), (key, err, bound)
    assert abs(got["zero_point_energy"] - ref["zpe"]) <= 1e-12 * ref["zpe"]
    assert got["n_excluded"] == ref["n_excluded"]
    # the excluded modes, stated: with the host route alone, nothing but Gamma's three acoustic modes lies below 0.05 THz
    f_host = _host_freqs(name, q)
    is_gamma = np.all(q == 0, axis=1)
    unstable = name == "mow16" and bool((f_host < -CUTOFF).any())
    if not unstable:
        low = np.abs(f_host) < 0.05
        assert low.sum() == (3 if gamma else 0)
        assert not low[~is_gamma].any() and (not gamma or (w[is_gamma] == 1).all())
        assert got["n_excluded"] == (3 if gamma else 0)
    else:
        # a dynamically unstable cell: its imaginary modes are excluded and counted with the acoustic ones
        n_imag = int((w[:, None] * (f_host < -CUTOFF)).sum())
        assert got["n_excluded"] == n_imag + 3
    # end to end: the reference on the host-route frequencies, the device's excluded modes matched by index
    inc = f > CUTOFF
    assert unstable or np.array_equal(inc, f_host > CUTOFF)
    assert np.all(f_host[inc] > 0)
    end = PR.thermo(f_host, w, TEMPS, include=inc)
    for key, short in keys:
        rel = np.abs(got[key] - end[short])[1:] / end["abs_" + short][1:]
        print(f"[phonon] {name} {mesh} gamma={gamma} {short}: end-to-end max rel = {rel.max():.3e}")
        assert np.all(rel <= 1e-9), (key, rel)
    # anchors
    n_inc = float((w[:, None] * inc).sum()) / w.sum()
    x_max = PR.H * f.max() / (PR.KB * 3000.0)
    cv = got["heat_capacity"][-1] / (PR.KB * n_inc)
    assert 1 - x_max ** 2 / 12 <= cv <= 1.0
    assert np.all(got["entropy"] >= 0) and got["entropy"][0] == 0 and got["heat_capacity"][0] == 0
    assert got["free_energy"][0] == got["zero_point_energy"] == got["internal_energy"][0]
    zpe = 0.5 * PR.H * float((w[:, None] * f * inc).sum()) / w.sum()
    assert abs(got["zero_point_energy"] - zpe) <= 1e-12 * zpe
    # dF / dT = -S by a centred difference over +-1 K; its own error is delta^2 F''' / 6 = delta^2 (C_v / T)' / 6, bounded from
    # the reference's C_v: |(C_v / T)'| <= |C_v'| / T + C_v / T^2 with C_v' from the reference at T +- 1 K
    for T in (100.0, 300.0, 1000.0):
        d = 1.0
        t3 = harmonic.thermo_from_eigenvalues(lam, [T - d, T, T + d], w, cutoff_THz=CUTOFF)
        r3 = PR.thermo(f, w, [T - 2 * d, T, T + 2 * d], cutoff=CUTOFF)
        slope = (t3["free_energy"][2] - t3["free_energy"][0]) / (2 * d)
        cv_prime = np.abs(np.diff(r3["Cv"])).max() / (2 * d)
        bound = d * d / 6 * (cv_prime / (T - 2 * d) + r3["Cv"].max() / (T - 2 * d) ** 2) + 4e-12 * r3["abs_F"][1] / d
        assert abs(slope + t3["entropy"][1]) <= bound, (T, slope, t3["entropy"][1], bound)


def test_abi_refusals():
    """The library's own checks, called directly: UF3_EINVAL with a message, nothing launched."""
    ctx = _lib.get_context(0)
    lib, addr = ctx.lib, _lib._addr

    def err():
        return lib.uf3_last_error(ctx.handle).decode()

    def mesh(n=2, n_sc=16, nq=3, terms=None, null=None):
        fc = np.zeros((3 * n, 3 * n_sc))
        ism = np.ones(n)
        t = np.array([[0, 0, 0, 0, 0], [1, 1, 0, 0, 0]], dtype=np.int32) if terms is None else np.asarray(terms, dtype=np.int32)
        w = np.ones(len(t))
        q = np.zeros((max(nq, 1), 3))
        lam = np.zeros((max(nq, 1), 3 * n))
        st = np.zeros(max(nq, 1), dtype=np.int32)
        args = dict(fc=addr(fc), ism=addr(ism), t=addr(t), w=addr(w), q=addr(q), lam=addr(lam), st=addr(st))
        if null:
            args[null] = None
        return lib.uf3_phonon_mesh(ctx.handle, n, n_sc, args["fc"], args["ism"], len(t), args["t"], args["w"], nq, args["q"],
                                   args["lam"], args["st"])

    assert mesh() == 0
    assert mesh(n=33, n_sc=33) == 1 and "limit is 32" in err()
    assert mesh(nq=0) == 1 and "nq" in err()
    assert mesh(n_sc=15) == 1 and "multiple" in err()
    for bad in ([[2, 0, 0, 0, 0]], [[-1, 0, 0, 0, 0]], [[0, 16, 0, 0, 0]], [[0, -1, 0, 0, 0]]):
        assert mesh(terms=bad) == 1 and "outside" in err(), bad
    for name in ("lam", "st", "q", "fc", "t"):
        assert mesh(null=name) == 1 and "null" in err(), name

    lam = np.ones((4, 3))
    counts = np.zeros(2, dtype=np.int64)
    dos = np.zeros(3)
    samples = np.array([0.0, 1.0, 2.0])

    def run_dos(nq=4, edges=(0.0, 1.0, 2.0), sigma=0.1, c=True, d=True):
        e = np.array(edges, dtype=float)
        return lib.uf3_phonon_dos(ctx.handle, 3, nq, addr(lam), None, len(e) - 1, addr(e), addr(counts) if c else None, 3,
                                  addr(samples), sigma, addr(dos) if d else None)

    assert run_dos() == 0
    assert run_dos(nq=0) == 1 and "nq" in err()
    assert run_dos(edges=(0.0, 1.0, 1.0)) == 1 and "increasing" in err()
    assert run_dos(edges=(0.0, 2.0, 1.0)) == 1 and "increasing" in err()
    assert run_dos(sigma=0.0) == 1 and "sigma" in err()
    assert run_dos(sigma=-1.0) == 1 and "sigma" in err()
    assert run_dos(c=False, d=False) == 1 and "NULL" in err()
    assert run_dos(sigma=0.0, d=False) == 0          # sigma is not looked at without the smeared output

    out = np.zeros((2, 4))
    zpe = np.zeros(1)
    nx = np.zeros(1, dtype=np.int64)

    def run_thermo(nq=4, temps=(0.0, 300.0), cutoff=1e-3, null_out=False):
        t = np.array(temps, dtype=float)
        return lib.uf3_phonon_thermo(ctx.handle, 3, nq, addr(lam), None, len(t), addr(t), cutoff, None if null_out else addr(out),
                                     addr(zpe), addr(nx))

    assert run_thermo() == 0
    assert run_thermo(nq=0) == 1 and "nq" in err()
    assert run_thermo(temps=(10.0, -1.0)) == 1 and "negative" in err()
    assert run_thermo(cutoff=-1.0) == 1 and "cut-off" in err()
    assert run_thermo(null_out=True) == 1 and "null" in err()
    # the Python layer refuses an oversized cell itself
    rng = np.random.default_rng(0)
    big = Atoms(numbers=[74] * 33, positions=rng.uniform(0, 9, (33, 3)), cell=np.eye(3) * 9.0, pbc=True)
    with pytest.raises(ValueError, match="at most 32 atoms"):
        harmonic.mesh_frequencies(_calc(_unary_model()), big, mesh=(2, 2, 2), masses=W_MASS)


def test_calculator_surface():
    calc = _calc(_unary_model())
    prim = _prim()
    dos = calc.get_phonon_dos(prim, mesh=(8, 8, 8), n_super=4, masses=W_MASS, n_samples=201, n_bins=40)
    assert {"frequencies", "dos", "counts", "n_imaginary", "edges", "sigma"} <= set(dos)
    assert dos["frequencies"].shape == (201,) and dos["dos"].shape == (201,) and dos["counts"].shape == (40,)
    assert dos["counts"].dtype == np.int64 and dos["counts"].sum() == 3 * 512 and dos["n_imaginary"] == 0
    g, s = dos["dos"], dos["frequencies"]
    assert abs(np.sum(0.5 * (g[1:] + g[:-1]) * np.diff(s)) - 3.0) <= 1e-6
    th = calc.get_thermal_properties(prim, [0.0, 300.0, 1000.0], mesh=(8, 8, 8), n_super=4, masses=W_MASS)
    for key in ("free_energy", "internal_energy", "entropy", "heat_capacity", "temperatures"):
        assert th[key].shape == (3,)
    assert th["n_excluded"] == 3 and th["n_imaginary"] == 0 and th["zero_point_energy"] > 0
    assert th["free_energy"][0] == th["zero_point_energy"]
    assert 0.9 < th["heat_capacity"][2] / (3 * harmonic.KB_EV_PER_K) < 1.0         # Dulong-Petit, minus Gamma's 3 of 1536 modes
    for fn in (lambda: calc.get_phonon_dos(prim, mesh=(2, 2, 2), n_super=2),
               lambda: calc.get_thermal_properties(prim, [300.0], mesh=(2, 2, 2), n_super=2)):
        with pytest.raises(ValueError, match="harmonic: no masses"):
            fn()
    # an unstable structure warns and counts
    calc2, atoms, m, n_super, fc = _case("mow16")
    f_host = _host_freqs("mow16", harmonic.qmesh((2, 2, 2))[0])
    if (f_host < -CUTOFF).any():
        with pytest.warns(RuntimeWarning, match="imaginary"):
            res = calc2.get_thermal_properties(atoms, [300.0], mesh=(2, 2, 2), n_super=2, masses=MOW_MASS)
        assert res["n_imaginary"] > 0 and res["n_excluded"] >= res["n_imaginary"]
        with pytest.warns(RuntimeWarning, match="imaginary"):
            assert calc2.get_phonon_dos(atoms, mesh=(2, 2, 2), n_super=2, masses=MOW_MASS)["n_imaginary"] == res["n_imaginary"]


@pytest.mark.parametrize("name", ["w_conv", "w_conv4"])
def test_dos_outputs_and_weights_are_independent_sections(name):
    """uf3_phonon_dos stages the q-weights, the counts and the smeared DOS only when they are passed: counts alone, the DOS alone
    and both give the same arrays, with the weights and without."""
    q, w = harmonic.qmesh((4, 4, 4))
    lam, _ = _dev_lam(name, q)
    f = harmonic.eigenvalues_to_frequencies(lam)
    assert f.shape[1] == (6 if name == "w_conv" else 12)
    edges = _guarded_edges(f)
    s = np.linspace(f.min() - 1.0, f.max() + 1.0, 41)
    for wq in (w, None):
        c_only, no_d = harmonic.dos_from_eigenvalues(lam, wq, edges=edges)
        no_c, d_only = harmonic.dos_from_eigenvalues(lam, wq, samples=s, sigma=0.15)
        c_both, d_both = harmonic.dos_from_eigenvalues(lam, wq, edges=edges, samples=s, sigma=0.15)
        assert no_d is None and no_c is None
        assert np.array_equal(c_only, c_both) and np.array_equal(d_only, d_both)
        assert c_both.sum() == f.shape[1] * (len(q) if wq is None else w.sum())
        assert d_both.max() > 0
        if wq is None:
            assert np.array_equal(c_both, np.histogram(f.ravel(), bins=edges)[0])
