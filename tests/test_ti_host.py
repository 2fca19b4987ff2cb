"""Free energies by switching (``uf3_amd.forcefield.free_energy``, ``MolecularDynamics.switch``), the part that needs no
device: the NumPy restatement of the device scheme (tests/_ti_ref.py) against tests/_md_ref.py and against the exact free-energy
difference of a quadratic energy, the reversible-scaling formula, the centre-of-mass correction, the schedules and the
argument checks."""
import numpy as np
import pytest

from uf3_amd.forcefield import free_energy as fe, md
from uf3_amd.forcefield.md import ACC, KB
from _md_ref import init_velocities, run as ref_run
from _ti_ref import constrained_logdet, run_switch

U0 = -3.25              # the quadratic energy's minimum, eV


def _network(seed=3, n=8):
    """A seeded translation-invariant spring network on ``n`` atoms of two masses: A [3n, 3n] (eV / A^2), sites, masses."""
    rng = np.random.default_rng(seed)
    w = np.triu(rng.uniform(0.3, 1.5, (n, n)), 1)
    w = w + w.T
    lap = np.diag(w.sum(1)) - w
    shape = rng.normal(size=(3, 3))
    a = np.kron(lap, np.eye(3) + 0.2 * shape @ shape.T)
    sites = rng.uniform(0, 6, (n, 3))
    masses = np.where(np.arange(n) % 2 == 0, 20.0, 45.0)
    return a, sites, masses


def _quadratic(a, sites, n_rep):
    tiled = np.tile(sites, (n_rep, 1))

    def forces_of(x):
        u = (x - tiled).reshape(n_rep, -1)
        au = u @ a
        return U0 + 0.5 * np.sum(u * au, axis=1), -au.reshape(-1, 3)
    return forces_of, tiled


@pytest.mark.parametrize("friction", [0.0, 0.05])
def test_restatement_reduces_to_the_md_restatement(friction):
    a, sites, masses = _network()
    forces_of, x0 = _quadratic(a, sites, 2)
    m, off = np.tile(masses, 2), np.array([0, 8, 16])
    v0 = init_velocities(m, off, 300.0, 4, 0)
    x_start = x0 + 0.05 * np.random.default_rng(1).normal(size=x0.shape)
    sched = fe.switching_schedule(40, "smooth")
    x, v, work, rec = run_switch(x_start, v0, m, forces_of, off, x0, np.zeros(16), 40, 1.0, 300.0, friction, 9, 1.0, 1.0, sched,
                                 False, step0=7, every=10)
    xr, vr, er, _ = ref_run(x_start, v0, m, forces_of, 40, 1.0, 300.0, friction, 9, step0=7)
    assert np.abs(x - xr).max() <= 1e-13 and np.abs(v - vr).max() <= 1e-13
    assert np.all(work == 0.0) and rec.shape == (4, 2, 5)
    assert np.abs(rec[-1, :, 1] - er).max() <= 1e-12 and np.all(rec[..., 0] == 1.0) and np.all(rec[..., 2] == 0.0)
    assert np.abs(x - x_start).max() > 1e-3


def test_frenkel_ladd_reproduces_the_exact_difference_of_a_quadratic_energy():
    """Sign, the factor 1/2, the schedule and both projections: Delta F = U0 + kT / 2 [logdet(Q^T A Q) - logdet(Q^T K Q)]."""
    n_rep, temp, n_eq, n_sw = 64, 300.0, 500, 2000
    a, sites, masses = _network()
    forces_of, x0 = _quadratic(a, sites, n_rep)
    m, off = np.tile(masses, n_rep), 8 * np.arange(n_rep + 1)
    k = np.tile(np.where(np.arange(8) % 2 == 0, 4.0, 6.5), n_rep)
    x, v = x0.copy(), init_velocities(m, off, temp, 11, 0)
    sched, hold = fe.switching_schedule(n_sw, "smooth"), np.zeros(n_eq + 1)
    step, work = 0, {}
    for name, lo, hi in (("forward", 0.0, 1.0), ("backward", 1.0, 0.0)):
        x, v, _, _ = run_switch(x, v, m, forces_of, off, x0, k, n_eq, 1.0, temp, 0.05, 5, lo, lo, hold, True, step0=step)
        step += n_eq
        x, v, work[name], _ = run_switch(x, v, m, forces_of, off, x0, k, n_sw, 1.0, temp, 0.05, 5, lo, hi, sched, True, step0=step)
        step += n_sw
    delta = 0.5 * (work["forward"] - work["backward"])
    exact = U0 + 0.5 * KB * temp * (constrained_logdet(a, masses) - constrained_logdet(np.diag(np.repeat(k[:8], 3)), masses))
    se = delta.std(ddof=1) / np.sqrt(n_rep)
    print(f"Delta F {delta.mean():.6f} +- {se:.6f} eV, exact {exact:.6f} eV, dissipation {0.5 * np.mean(work['forward'] + work['backward']):.6f}")
    assert abs(delta.mean() - exact) <= 4 * se, (delta.mean(), exact, se)
    assert se < 0.01 * abs(KB * temp * 21)                     # (the comparison is a sharp one)
    # momentum stayed where init_velocities put it
    p = np.add.reduceat(m[:, None] * v, off[:-1], axis=0)
    assert np.abs(p).max() <= 1e-10 * np.abs(m[:, None] * v).sum()


def test_reversible_scaling_curve_on_the_exact_harmonic_work():
    rng = np.random.default_rng(5)
    omega, t0, n_dof = rng.uniform(0.01, 0.06, 21), 250.0, 21
    harmonic = lambda t: U0 + KB * t * np.sum(np.log(fe.HBAR * omega / (KB * t)))      # noqa: E731
    lam = np.linspace(1.0, 0.2, 33)
    work = U0 * (lam - 1.0) + 0.5 * n_dof * KB * t0 * np.log(lam)
    temperature, free = fe.reversible_scaling_curve(work, lam, harmonic(t0), t0, n_dof)
    assert np.array_equal(temperature, t0 / lam)
    ref = np.array([harmonic(t) for t in temperature])
    assert np.abs(free - ref).max() <= 1e-12 * np.abs(ref).max()


def test_com_correction_reduces_to_the_one_species_form():
    n, mass, k, temp, vol = 54, 183.84, 7.3, 450.0, 855.3
    omega2 = k * ACC / mass                                   # rad^2 / fs^2; m omega^2 in eV / A^2 is mass * omega2 / ACC
    kt = KB * temp
    ref = kt * np.log((n / vol) * (2 * np.pi * kt / (n * mass * omega2 / ACC)) ** 1.5)
    got = fe.fixed_com_correction(k, np.full(n, mass), temp, vol)
    assert abs(got - ref) <= 1e-13 * max(1.0, abs(ref))
    # two species: one translation by default, and the mass-weighted sum
    m2, k2 = np.array([20.0, 45.0] * 4), np.array([4.0, 6.5] * 4)
    mu = m2 / m2.sum()
    ref2 = kt * np.log(1 / vol) + 1.5 * kt * np.log(2 * np.pi * kt * np.sum(mu ** 2 / k2))
    assert abs(fe.fixed_com_correction(k2, m2, temp, vol) - ref2) <= 1e-13


def test_einstein_free_energy_is_the_classical_oscillators():
    m, k, temp = np.array([20.0, 45.0, 96.0]), np.array([4.0, 6.5, 1.25]), 300.0
    ref = KB * temp * sum(3 * np.log(fe.HBAR * np.sqrt(kk * ACC / mm) / (KB * temp)) for kk, mm in zip(k, m))
    assert abs(fe.einstein_free_energy(k, m, temp) - ref) <= 1e-13
    with pytest.raises(ValueError):
        fe.einstein_free_energy(0.0, m, temp)


@pytest.mark.parametrize("n", [1, 7, 100, 3000])
def test_schedules(n):
    for kind in ("linear", "smooth"):
        s = fe.switching_schedule(n, kind)
        assert s.shape == (n + 1,) and s[0] == 0.0 and s[-1] == 1.0
        assert np.all(np.diff(s) >= 0)
        assert np.abs(s + s[::-1] - 1.0).max() <= 1e-12           # symmetric: s(1 - tau) = 1 - s(tau)
    if n >= 100:
        # s(tau) = 126 tau^5 + O(tau^6): the first difference at either end is of order n^-5, far inside C / n^4
        d = np.diff(fe.switching_schedule(n, "smooth"))
        assert d[0] <= 200.0 / n ** 4 and d[-1] <= 200.0 / n ** 4
        assert d[n // 2] > 2.0 / n                              # (630 / 256 per unit tau in the middle)
    with pytest.raises(ValueError):
        fe.switching_schedule(10, "cubic")
    assert np.array_equal(fe.switching_schedule(0, "smooth"), [0.0])


def test_switch_and_set_reference_check_their_arguments_before_the_device():
    obj = md.MolecularDynamics.__new__(md.MolecularDynamics)
    obj.handle, obj.timestep_fs, obj.temperature_K, obj.friction_per_fs, obj.seed, obj.skin = None, 1.0, 0.0, 0.0, 0, 0.5
    for bad, word in ((dict(n_steps=-1), "n_steps"), (dict(n_steps=2.5), "n_steps"), (dict(every=-1), "every"),
                      (dict(fix_com=1), "fix_com"), (dict(lambda_start=1.5), "lambda_start"), (dict(lambda_end=-0.1), "lambda_end"),
                      (dict(lambda_start=float("nan")), "lambda_start"), (dict(schedule="cubic"), "schedule"),
                      (dict(schedule=np.linspace(0, 1, 10)), "schedule"), (dict(schedule=np.linspace(0, 2, 11)), "schedule"),
                      (dict(temperatures_K=-1.0), "temperatures_K"), (dict(temperatures_K=[[1.0]]), "temperatures_K")):
        args = dict(n_steps=10, lambda_start=0.0, lambda_end=1.0)
        args.update(bad)
        with pytest.raises(ValueError, match=word):
            obj.switch(**args)
    obj.timestep_fs = 0.0
    with pytest.raises(ValueError, match="timestep_fs"):
        obj.switch(10, 0.0, 1.0)
    for bad in (-1.0, float("inf"), "stiff"):
        with pytest.raises(ValueError, match="spring"):
            obj.set_reference(spring=bad)
