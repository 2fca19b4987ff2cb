"""Switching molecular dynamics on the device (``uf3_md_set_reference``, ``uf3_md_run_switch``, uf3_amd/csrc/uf3_ti.h;
``MolecularDynamics.switch`` and ``uf3_amd.forcefield.free_energy``) against the NumPy restatement in tests/_ti_ref.py, whose
forces come from ``UFCalculator.evaluate_frames``: trajectories, work and records; the reduction to ``run``; block
invariance; the work against the energy actually gained; the held centre of mass; determinism; refusals; and one
Frenkel-Ladd free energy against the harmonic value.  Frames, models and masses are tests/test_gpu_md.py's."""
import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.forcefield import free_energy as fe, md
from uf3_amd.forcefield.md import KB
from _md_ref import init_velocities
from _ti_ref import constrained_logdet, run_switch
from test_gpu_md import MASSES, TOL, _cluster, _forces_of, _mow, _unary, _w128

pytestmark = pytest.mark.gpu


def _w432():
    return synthetic.lattice_frame("bcc", (6, 6, 6), 3.165, [74], seed=6)


def _mow54():
    return synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [42, 74], seed=84)


# name -> (calculator, frames, springs, lambda_start, lambda_end, temperatures): the 432-atom frame spans two chunks of the
# chunk table, the second one partial, and has more atoms than a workgroup has threads
CASES = {"w_batch": (_unary, lambda: [_w128(1), _w432(), _cluster()], 5.0, (0.0, 1.0, 0.5), (1.0, 0.3, 0.5), (300.0, 600.0, 0.0)),
         "mow54": (_mow, lambda: [_mow54()], {"Mo": 4.0, "W": 0.0}, (0.0,), (1.0,), (300.0,))}


def _setup(name):
    make_calc, make_frames, spring, lam_a, lam_b, temps = CASES[name]
    calc, frames = make_calc(), make_frames()
    forces_of, off = _forces_of(calc, frames)
    m = md.resolve_masses(frames, MASSES)
    x = np.concatenate([a.get_positions() for a in frames])
    sites = x + np.random.default_rng(2).normal(0, 0.03, x.shape)      # (the springs pull from the first step on)
    v = init_velocities(m, off, 300.0, 4, 0)
    return calc, frames, forces_of, off, m, x, sites, v, spring, np.array(lam_a), np.array(lam_b), np.array(temps)


@pytest.mark.parametrize("fix_com", [True, False])
@pytest.mark.parametrize("friction", [0.05, 0.0])
@pytest.mark.parametrize("name", ["w_batch", "mow54"])
def test_switch_parity_with_the_restatement(name, friction, fix_com):
    calc, frames, forces_of, off, m, x0, sites, v0, spring, lam_a, lam_b, temps = _setup(name)
    n_steps, every = 30, 5
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, friction_per_fs=friction, seed=9) as dyn:
        dyn.set_velocities(v0)
        dyn.set_reference(sites, spring)
        k = dyn.spring.copy()
        out = dyn.switch(n_steps, lam_a, lam_b, schedule="smooth", temperatures_K=temps, fix_com=fix_com, every=every)
        assert dyn.step == n_steps
        x, v = dyn.get_positions(), dyn.get_velocities()
    xr, vr, wr, rec = run_switch(x0, v0, m, forces_of, off, sites, k, n_steps, 1.0, temps, friction, 9, lam_a, lam_b,
                                 fe.switching_schedule(n_steps, "smooth"), fix_com, step0=0, every=every)
    assert np.abs(x - xr).max() <= TOL, np.abs(x - xr).max()
    assert np.abs(v - vr).max() <= TOL, np.abs(v - vr).max()
    assert np.all(np.abs(out["work"] - wr) <= 1e-9 * np.maximum(1.0, np.abs(wr))), (out["work"], wr)
    assert np.array_equal(out["step"], every * np.arange(1, n_steps // every + 1))
    for col, key in enumerate(("lambda", "potential_energy", "einstein_energy", "kinetic_energy", "work_so_far")):
        assert out[key].shape == rec[..., col].shape
        assert np.all(np.abs(out[key] - rec[..., col]) <= 1e-9 * np.maximum(1.0, np.abs(rec[..., col]))), key
    assert np.array_equal(out["work_so_far"][-1], out["work"])
    assert np.abs(wr).max() > 1e-3 and np.abs(x - x0).max() > 1e-3      # (work was done and the atoms did move)


@pytest.mark.parametrize("friction", [0.0, 0.05])
def test_switch_at_lambda_one_without_springs_is_run(friction):
    calc, frames = _unary(), [_w128(1), _cluster()]
    out = []
    for switching in (False, True):
        with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=300.0, friction_per_fs=friction, seed=21) as dyn:
            dyn.initialize_velocities(300.0)
            if switching:
                dyn.set_reference(None, None)
                work = dyn.switch(40, 1.0, 1.0, fix_com=False)["work"]
                assert np.all(work == 0.0) and not np.any(np.signbit(work))
            else:
                dyn.run(40)
            out.append((dyn.get_positions(), dyn.get_velocities()))
    assert np.abs(out[0][0] - out[1][0]).max() <= 1e-10
    assert np.abs(out[0][1] - out[1][1]).max() <= 1e-10


def test_switch_in_blocks_equals_one_switch():
    calc, frames = _unary(), [_w128(1), _cluster()]
    sched = fe.switching_schedule(60, "smooth")
    out = []
    for blocks in ([(0, 60)], [(0, 25), (25, 60)]):
        with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=300.0, friction_per_fs=0.05, seed=21) as dyn:
            dyn.initialize_velocities(300.0)
            dyn.set_reference(None, 5.0)
            work = sum(dyn.switch(hi - lo, [0.1, 0.9], [0.8, 0.2], schedule=sched[lo:hi + 1])["work"] for lo, hi in blocks)
            assert dyn.step == 60
            out.append((dyn.get_positions(), dyn.get_velocities(), work))
    for a, b in zip(*out):
        assert np.abs(a - b).max() <= 1e-10
    assert np.abs(out[0][2]).min() > 1e-4


def test_work_is_the_energy_the_integrated_dynamics_gained():
    """|H_end(end) - H_start(start) - W| is velocity Verlet's O(dt^2) error: the work belongs to the trajectory that was made."""
    calc, err = _unary(), {}
    for dt in (1.0, 0.5):
        n = int(round(200.0 / dt))
        with md.MolecularDynamics(calc, [_w128(3)], dt, masses=MASSES, seed=5) as dyn:
            dyn.initialize_velocities(300.0)
            dyn.set_reference(None, 5.0)
            h_start = md.kinetic_energy(dyn.get_velocities(), dyn.masses) + 0.2 * dyn.get_potential_energies()[0]    # (U_E = 0)
            rec = dyn.switch(n, 0.2, 0.9, temperatures_K=300.0, fix_com=True, every=n)
            lam = rec["lambda"][-1, 0]                  # (0.2 + 0.7 * 1.0: 0.9 to an ulp)
            assert abs(lam - 0.9) <= 2e-16
            h_end = rec["kinetic_energy"][-1, 0] + lam * rec["potential_energy"][-1, 0] + (1 - lam) * rec["einstein_energy"][-1, 0]
            err[dt] = abs(h_end - h_start - rec["work"][0])
            assert abs(rec["work"][0]) > 0.1
    print("energy balance errors", err)
    assert 3.0 <= err[1.0] / err[0.5] <= 5.0, err


def _momentum_ratio(dyn, off):
    p = dyn.masses[:, None] * dyn.get_velocities()
    return np.array([np.linalg.norm(p[lo:hi].sum(0)) / np.abs(p[lo:hi]).sum() for lo, hi in zip(off[:-1], off[1:])])


@pytest.mark.parametrize("name", ["w_batch", "mow54"])
def test_fixed_centre_of_mass(name):
    make_calc, make_frames, spring, lam_a, lam_b, temps = CASES[name]
    calc, frames = make_calc(), make_frames()
    if name == "w_batch":
        frames, lam_a, lam_b, temps = [frames[0], frames[2]], (0.0, 0.5), (1.0, 0.5), (300.0, 600.0)
    off = np.cumsum([0] + [len(a) for a in frames])
    ratio = {}
    for fix_com in (True, False):
        with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, friction_per_fs=0.05, seed=3) as dyn:
            dyn.initialize_velocities(300.0)
            dyn.set_reference(None, spring)
            dyn.switch(200, lam_a, lam_b, temperatures_K=temps, fix_com=fix_com)
            ratio[fix_com] = _momentum_ratio(dyn, off)
    assert np.all(ratio[True] <= 1e-10), ratio
    assert np.all(ratio[False] > 1e-10), ratio


def test_switch_repeats_bit_for_bit():
    calc, frames, _, _, _, _, sites, v0, spring, lam_a, lam_b, temps = _setup("w_batch")
    out = []
    for _ in range(2):
        with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, friction_per_fs=0.05, seed=9) as dyn:
            dyn.set_velocities(v0)
            dyn.set_reference(sites, spring)
            rec = dyn.switch(40, lam_a, lam_b, temperatures_K=temps, fix_com=True, every=10)
            out.append([dyn.get_positions(), dyn.get_velocities()] + [rec[key] for key in sorted(rec)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def _raw_switch(dyn, n_steps=4, lam_a=0.0, lam_b=1.0, sched=None):
    """The library entry with nothing checked in front of it."""
    nf = dyn._batch.n_frames
    temps, la, lb, work = np.full(nf, 300.0), np.full(nf, lam_a), np.full(nf, lam_b), np.zeros(nf)
    sched = np.ascontiguousarray(np.linspace(0.0, 1.0, n_steps + 1) if sched is None else sched, dtype=float)
    dyn.ctx.check(dyn.ctx.lib.uf3_md_run_switch(dyn.handle, n_steps, 1.0, _lib._p(temps), 0.0, 0, 0.5, _lib._p(la), _lib._p(lb),
                                                _lib._p(sched), 1, 0, None, _lib._p(work)))


def test_refusals():
    calc, frames = _unary(), [_w128(1)]
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, wrap=True) as dyn:
        with pytest.raises(_lib.UF3Error, match="uf3_md_set_reference: the object wraps"):
            dyn.set_reference(None, 5.0)
        with pytest.raises(_lib.UF3Error, match="uf3_md_run_switch: the object wraps"):
            dyn.switch(4, 0.0, 1.0)
        with pytest.raises(_lib.UF3Error, match="uf3_md_set_reference: the object wraps"):
            dyn.ctx.check(dyn.ctx.lib.uf3_md_set_reference(dyn.handle, None, None))
        with pytest.raises(_lib.UF3Error, match="uf3_md_run_switch: the object wraps"):
            _raw_switch(dyn)
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=300.0, pressure_eV_A3=0.0, barostat_time_fs=500.0) as dyn:
        with pytest.raises(_lib.UF3Error, match="uf3_md_set_reference: the object runs at a pressure"):
            dyn.set_reference(None, 5.0)
        with pytest.raises(_lib.UF3Error, match="uf3_md_run_switch: the object runs at a pressure"):
            dyn.switch(4, 0.0, 1.0)
        dyn.run(2)
        with pytest.raises(_lib.UF3Error, match="uf3_md_run_switch: the object runs at a pressure"):
            _raw_switch(dyn)
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES) as dyn:
        with pytest.raises(_lib.UF3Error, match="uf3_md_run_switch: no reference"):
            dyn.switch(4, 0.0, 1.0)
        dyn.set_reference(None, 5.0)
        with pytest.raises(_lib.UF3Error, match="uf3_md_set_reference: spring must be finite and >= 0"):
            bad = np.full(128, -1.0)
            dyn.ctx.check(dyn.ctx.lib.uf3_md_set_reference(dyn.handle, None, _lib._p(bad)))
        dyn.set_reference(None, 5.0)
        for bad in (1.5, -0.25, float("nan")):
            with pytest.raises(_lib.UF3Error, match=r"uf3_md_run_switch: lambda must be finite and lie in \[0, 1\]"):
                _raw_switch(dyn, lam_b=bad)
            with pytest.raises(ValueError, match="lambda_end"):
                dyn.switch(4, 0.0, bad)
        with pytest.raises(_lib.UF3Error, match=r"uf3_md_run_switch: schedule entries must be finite and lie in \[0, 1\]"):
            _raw_switch(dyn, sched=[0.0, 0.5, 1.5, 1.0, 1.0])
        with pytest.raises(ValueError, match=r"schedule must hold n_steps \+ 1 = 5 values"):
            dyn.switch(4, 0.0, 1.0, schedule=np.linspace(0, 1, 4))
        assert dyn.step == 0                        # (nothing above made a step)
        assert dyn.switch(4, 0.0, 1.0)["work"].shape == (1,)


def test_frenkel_ladd_free_energy_of_bcc_tungsten_near_the_harmonic_value():
    """64 replicas of 54-atom bcc W at 100 K (3 % of the melting point): the mean Delta F of the switch lies within 4 standard
    errors + 0.05 * 3 (N - 1) k_B T of U0 + kT / 2 [logdet(Q^T H Q) - logdet(Q^T K Q)], and the dissipation is not negative."""
    calc = _unary()
    atoms = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=0, rattle=0.0, strain=0.0)
    n, temp, n_rep = len(atoms), 100.0, 64
    hess = calc.get_hessian(atoms)
    hess = 0.5 * (hess + hess.T)
    spring = float(np.mean(np.diag(hess)))
    masses = md.resolve_masses([atoms], MASSES)
    u0 = calc.evaluate_frames([atoms])[0][0]
    harmonic = u0 + 0.5 * KB * temp * (constrained_logdet(hess, masses) - constrained_logdet(spring * np.eye(3 * n), masses))
    out = fe.frenkel_ladd(calc, atoms, temp, masses=MASSES, n_replicas=n_rep, n_equilibrate=1000, n_switch=3000, spring=spring,
                          friction_per_fs=0.02, seed=17)
    delta, se = out["delta_F"][0].mean(), out["standard_error"][0]
    diss = out["dissipation"][0]
    diss_se = diss.std(ddof=1) / np.sqrt(n_rep)
    print(f"Delta F {delta:.6f} +- {se:.6f} eV, harmonic {harmonic:.6f} eV, dissipation {diss.mean():.6f} +- {diss_se:.6f} eV, "
          f"F {out['free_energy'][0]:.6f} eV")
    assert se == pytest.approx(out["delta_F"][0].std(ddof=1) / np.sqrt(n_rep))
    assert abs(delta - harmonic) <= 4 * se + 0.05 * 3 * (n - 1) * KB * temp, (delta, harmonic, se)
    assert diss.mean() >= -4 * diss_se, (diss.mean(), diss_se)
    expected = (fe.einstein_free_energy(spring, masses, temp) + fe.fixed_com_correction(spring, masses, temp, atoms.get_volume())
                + delta)
    assert out["free_energy"][0] == pytest.approx(expected, abs=1e-12)


def _bcc54():
    return synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=0, rattle=0.0, strain=0.0)


def test_spring_constants_follow_the_harmonic_displacements():
    """The centre-of-mass-removed <|dr|^2> of a harmonic crystal is kT sum_nonzero 1 / eig / N: k = 3 N / sum 1 / eig.  A
    thousand samples of 162 coordinates with a correlation time near 100 fs leave a few per cent of noise, and at 100 K the
    anharmonic shift is smaller: 30 % holds both and is far from a factor 2 (an origin off the sites) or 3."""
    calc, atoms = _unary(), _bcc54()
    eig = np.linalg.eigvalsh(calc.get_hessian(atoms))[3:]
    expected = 3 * len(atoms) / np.sum(1.0 / eig)
    with md.MolecularDynamics(calc, [atoms], 1.0, masses=MASSES, temperature_K=100.0, friction_per_fs=0.02, seed=3) as dyn:
        dyn.initialize_velocities(100.0)
        k = fe.spring_constants(dyn, 2000)
    print("spring", k, "harmonic", expected)
    assert set(k) == {"W"} and abs(k["W"] - expected) <= 0.3 * expected
    out = fe.frenkel_ladd(calc, atoms, [100.0, 150.0], masses=MASSES, n_replicas=2, n_equilibrate=50, n_switch=100, n_spring=400)
    assert out["delta_F"].shape == (2, 2) and out["free_energy"].shape == (2,) and out["spring"].shape == (54,)
    assert np.all(out["spring"] == out["spring"][0]) and abs(out["spring"][0] - expected) <= 0.5 * expected
    assert np.all(np.isfinite(out["free_energy"])) and np.all(np.isfinite(out["standard_error"]))


def test_reversible_scaling_follows_the_harmonic_free_energy():
    """F(T) from 100 K to 200 K, started from the classical harmonic F(100 K) of the 3 N - 3 modes with the centre of mass held,
    stays within 0.05 * 3 (N - 1) k_B T of the harmonic F(T): the allowance of the Frenkel-Ladd test, for the same reason, and
    far below what a misplaced record (the backward work read at another lambda) or a wrong kinetic term costs (the term
    (n_dof / 2) k_B T0 ln(lambda) / lambda alone is 0.95 eV at 200 K)."""
    calc, atoms = _unary(), _bcc54()
    n = len(atoms)
    eig = np.linalg.eigvalsh(calc.get_hessian(atoms))[3:]
    omega = np.sqrt(eig * md.ACC / MASSES["W"])
    u0 = calc.evaluate_frames([atoms])[0][0]
    harmonic = lambda t: u0 + KB * t * np.sum(np.log(fe.HBAR * omega / (KB * t)))      # noqa: E731
    out = fe.reversible_scaling(calc, atoms, 100.0, 200.0, harmonic(100.0), masses=MASSES, n_replicas=16, n_equilibrate=500,
                                n_switch=2000, n_points=10, seed=4)
    t, f = out["temperature"], out["free_energy"]
    assert t.shape == f.shape == (10,) and np.all(np.diff(t) > 0) and t[-1] == pytest.approx(200.0, rel=1e-12)
    ref = np.array([harmonic(x) for x in t])
    print("reversible scaling: F - harmonic", f - ref, "dissipation", out["dissipation"].mean())
    assert np.all(np.abs(f - ref) <= 0.05 * 3 * (n - 1) * KB * t), (f - ref)
    assert out["dissipation"].mean() >= -4 * out["dissipation"].std(ddof=1) / 4.0
