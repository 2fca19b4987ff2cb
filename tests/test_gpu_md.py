"""Device-resident molecular dynamics (``uf3_md_*``, ``uf3_amd.forcefield.md``) against the NumPy restatement in
tests/_md_ref.py, whose forces come from ``UFCalculator.evaluate_frames``: the generator bit for bit, the initialisation, NVE
and Langevin trajectories on 3-body and 2-body models, block invariance, velocity Verlet's dt^2 energy error, Langevin
sampling, thermo records, and the context left as it was found.  Masses are test values, not a periodic table."""
import ctypes as C
import os

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator, md
from uf3_amd.regression import least_squares as ls
from _md_ref import init_velocities, philox, run as ref_run
from _util import GOLDEN, load_case

pytestmark = pytest.mark.gpu
MASSES = {"W": 180.0, "Mo": 96.0, "Ne": 20.0, "Xe": 131.0}
TOL = 1e-9


def _unary():
    return calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json")), md_skin=0.0)


def _mow():
    basis = synthetic.notebook_basis(["Mo", "W"])
    model = ls.WeightedLinearModel(basis)
    coeff = np.random.default_rng(31).normal(0, 0.05, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    model.coefficients = coeff
    return calculator.UFCalculator(model, md_skin=0.0)


def _w128(seed):
    return synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, [74], seed=seed)


def _cluster():
    a = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=5)
    return Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions(), cell=a.get_cell(), pbc=False)


def _batches():
    return {"w_batch": (_unary, lambda: [_w128(1), _w128(2), _cluster()]),
            "mow54": (_mow, lambda: [synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [42, 74], seed=84)]),
            "nexe_2body": (lambda: calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_binary.json")),
                                                           md_skin=0.0),
                           lambda: [load_case("case_nexe32")[2]])}


def _forces_of(calc, frames):
    off = np.cumsum([0] + [len(a) for a in frames])

    def f(x):
        moved = [Atoms(numbers=a.get_atomic_numbers(), positions=x[off[k]:off[k + 1]], cell=a.get_cell(), pbc=a.get_pbc())
                 for k, a in enumerate(frames)]
        e, frc, _ = calc.evaluate_frames(moved)
        return e, frc
    return f, off


def _parity(name, n_steps, temperature_K, friction, seed=9):
    make_calc, make_frames = _batches()[name]
    calc, frames = make_calc(), make_frames()
    forces_of, off = _forces_of(calc, frames)
    m = md.resolve_masses(frames, MASSES)
    x0 = np.concatenate([a.get_positions() for a in frames])
    v0 = init_velocities(m, off, 300.0, 4, 0)
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=temperature_K, friction_per_fs=friction,
                              seed=seed) as dyn:
        dyn.set_velocities(v0)
        dyn.run(n_steps)
        assert dyn.step == n_steps
        x, v, e, f = dyn.get_positions(), dyn.get_velocities(), dyn.get_potential_energies(), dyn.get_forces()
    xr, vr, er, fr = ref_run(x0, v0, m, forces_of, n_steps, 1.0, temperature_K, friction, seed)
    assert np.abs(x - xr).max() <= TOL, np.abs(x - xr).max()
    assert np.abs(v - vr).max() <= TOL, np.abs(v - vr).max()
    assert np.all(np.abs(e - er) <= TOL * np.maximum(1.0, np.abs(er))), (e, er)
    assert np.abs(f - fr).max() <= 1e-8 * max(1.0, np.abs(fr).max())
    assert np.abs(x - x0).max() > 1e-3                  # (the atoms did move)


def test_philox_on_the_device_is_the_restatement():
    ctx = _lib.get_context()
    from test_md_host import KAT
    rng = np.random.default_rng(12)
    ctr = np.ascontiguousarray(np.concatenate([np.array([k[0] for k in KAT], dtype=np.uint32),
                                               rng.integers(0, 1 << 32, (100000, 4), dtype=np.uint64).astype(np.uint32)]))
    key = np.ascontiguousarray(np.concatenate([np.array([k[1] for k in KAT], dtype=np.uint32),
                                               rng.integers(0, 1 << 32, (100000, 2), dtype=np.uint64).astype(np.uint32)]))
    out = np.zeros_like(ctr)
    ctx.check(ctx.lib.uf3_philox_debug(ctx.handle, len(ctr), _lib._p(ctr), _lib._p(key), _lib._p(out)))
    assert [tuple(int(w) for w in r) for r in out[:3]] == [k[2] for k in KAT]
    assert np.array_equal(out, philox(ctr, key))


def test_initialize_velocities_matches_the_host_and_removes_momentum():
    calc, frames = _unary(), [_w128(1), _w128(2), _cluster()]
    m = md.resolve_masses(frames, MASSES)
    off = np.cumsum([0] + [len(a) for a in frames])
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, seed=77) as dyn:
        dyn.initialize_velocities(300.0)
        v = dyn.get_velocities()
        ref = init_velocities(m, off, 300.0, 77, 0)
        assert np.abs(v - ref).max() <= 1e-12 * np.abs(ref).max()
        for lo, hi in zip(off[:-1], off[1:]):
            p = m[lo:hi, None] * v[lo:hi]
            assert np.abs(p.sum(0)).max() <= 1e-12 * np.abs(p).sum()
        dyn.initialize_velocities(450.0, seed=3, exact=True)
        v = dyn.get_velocities()
        assert np.abs(v - init_velocities(m, off, 450.0, 3, 0, exact=True)).max() <= 1e-12 * np.abs(v).max()
        for lo, hi in zip(off[:-1], off[1:]):
            assert md.temperature(md.kinetic_energy(v[lo:hi], m[lo:hi]), hi - lo) == pytest.approx(450.0, rel=1e-12)


@pytest.mark.parametrize("name", ["w_batch", "mow54"])
def test_nve_parity(name):
    _parity(name, 30, 0.0, 0.0)


@pytest.mark.parametrize("name", ["w_batch", "mow54"])
def test_langevin_parity(name):
    _parity(name, 30, 300.0, 0.05)


def test_two_body_basis_parity_on_the_rebuild_route():
    _parity("nexe_2body", 20, 300.0, 0.05)


def test_run_in_blocks_equals_one_run():
    calc, frames = _unary(), [_w128(1), _cluster()]
    out = []
    for blocks in ([60], [25, 35]):
        with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=300.0, friction_per_fs=0.05, seed=21) as dyn:
            dyn.initialize_velocities(300.0)
            for n in blocks:
                dyn.run(n)
            assert dyn.step == 60
            out.append((dyn.get_positions(), dyn.get_velocities()))
    assert np.abs(out[0][0] - out[1][0]).max() <= 1e-10
    assert np.abs(out[0][1] - out[1][1]).max() <= 1e-10


def test_nve_energy_error_scales_with_dt_squared():
    calc = _unary()
    drift = {}
    for dt, every in ((1.0, 1), (0.5, 2)):
        with md.MolecularDynamics(calc, [_w128(3)], dt, masses=MASSES, seed=5) as dyn:
            dyn.initialize_velocities(300.0, exact=True)
            m = dyn.masses
            e0 = dyn.get_potential_energies()[0] + md.kinetic_energy(dyn.get_velocities(), m)
            rec = dyn.run(int(round(200 / dt)), thermo_every=every)
            et = rec["potential_energy"][:, 0] + rec["kinetic_energy"][:, 0]
            assert len(et) == 200
            drift[dt] = np.abs(et - e0).max()
            v = dyn.get_velocities()
            p = m[:, None] * v
            assert np.abs(p.sum(0)).max() <= 1e-10 * np.abs(p).sum()
    ratio = drift[1.0] / drift[0.5]
    assert 3.0 <= ratio <= 5.0, (drift, ratio)
    assert drift[1.0] < 0.05 * 128 * 1.5 * md.KB * 300.0 * 10, drift        # (loose: the ratio is the check)


def test_langevin_samples_the_target_temperature():
    calc = _unary()
    frames = [_w128(100 + k) for k in range(32)]
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=600.0, friction_per_fs=0.02, seed=2024) as dyn:
        dyn.initialize_velocities(600.0)
        dyn.run(400)
        rec = dyn.run(1000, thermo_every=10)
    t = rec["temperature"].mean()
    assert abs(t - 600.0) <= 0.03 * 600.0, t


def test_thermo_records_match_direct_evaluation():
    calc, frames = _unary(), [_w128(1), _w128(2)]
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=300.0, friction_per_fs=0.05, seed=8) as dyn:
        dyn.initialize_velocities(300.0)
        rec = dyn.run(10, thermo_every=5, stress=True)
        assert rec["step"].tolist() == [5, 10] and rec["stress"].shape == (2, 2, 6)
        atoms, v, m = dyn.get_atoms(), dyn.get_velocities(), dyn.masses
    e, _, off, w = calc.evaluate_frames(atoms, virial=True)
    for k, a in enumerate(atoms):
        lo, hi = off[k], off[k + 1]
        assert abs(rec["potential_energy"][-1, k] - e[k]) <= TOL * max(1.0, abs(e[k]))
        assert abs(rec["kinetic_energy"][-1, k] - md.kinetic_energy(v[lo:hi], m[lo:hi])) <= 1e-12 * rec["kinetic_energy"][-1, k]
        kin = md.KE_UNIT * np.einsum("i,ij,ik->jk", m[lo:hi], v[lo:hi], v[lo:hi])
        kv = np.array([kin[0, 0], kin[1, 1], kin[2, 2], kin[1, 2], kin[0, 2], kin[0, 1]])
        vol = abs(np.linalg.det(a.get_cell()))
        s = rec["stress"][-1, k]
        assert np.abs(s * vol + kv - w[k]).max() <= TOL * max(1.0, np.abs(w[k]).max())
        assert np.abs(calc.get_stress(a) - kv / vol - s).max() <= 1e-9 * max(1.0, np.abs(s).max())
        assert rec["pressure"][-1, k] == pytest.approx(-s[:3].sum() / 3, rel=1e-14)


def test_runs_leave_the_context_and_the_calculator_as_they_were():
    calc = _unary()
    ctx = _lib.get_context(calc.device)
    other = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=61)
    e0, f0, _ = calc.evaluate_frames([other])                    # (md_skin 0: the context's skin is 0)
    steps0 = ctx.md_stats()["steps"]
    with md.MolecularDynamics(calc, [_w128(1)], 1.0, masses=MASSES, skin=0.7) as dyn:
        dyn.run(5)
    foreign = _w128(2)
    foreign.numbers[:3] = 42                                      # Mo: outside the unary basis
    dyn = md.MolecularDynamics(calc, [foreign], 1.0, masses=MASSES)
    with pytest.raises(_lib.SpeciesError):
        dyn.run(3)
    assert dyn.step == 0
    dyn.close()
    steps1 = ctx.md_stats()["steps"]
    e1, f1, _ = calc.evaluate_frames([other])
    e2, f2, _ = calc.evaluate_frames([other])
    # the skin is the caller's 0 again: these calls did not take the MD route, and their results are bit for bit the same
    assert ctx.md_stats()["steps"] == steps1 and getattr(ctx, "_md_skin", 0.0) == 0.0
    assert steps1 > steps0
    assert np.array_equal(e0, e1) and np.array_equal(f0, f1) and np.array_equal(e1, e2)


def test_run_rejects_a_thermo_buffer_that_does_not_match():
    calc = _unary()
    with md.MolecularDynamics(calc, [_w128(1)], 1.0, masses=MASSES) as dyn:
        lib, h = dyn.ctx.lib, dyn.handle
        buf = np.zeros((4, 1, 2))
        assert lib.uf3_md_run(h, 10, 1.0, 0.0, 0.0, 0, 0.5, 5, 0, None) == 1
        assert lib.uf3_md_run(h, 10, 1.0, 0.0, 0.0, 0, 0.5, 0, 0, _lib._p(buf)) == 1
        assert lib.uf3_md_run(h, 10, -1.0, 0.0, 0.0, 0, 0.5, 0, 0, None) == 1
        assert "dt" in lib.uf3_last_error(dyn.ctx.handle).decode()
        assert dyn.step == 0


def test_run_arguments_are_checked_in_one_order_under_each_entry_s_name():
    """Two bad arguments at once: the message is that of the one checked first, under the prefix of the entry whose check it is."""
    calc = _unary()
    w16 = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=3)
    with md.MolecularDynamics(calc, [w16], 1.0, masses=MASSES) as dyn:
        lib, h = dyn.ctx.lib, dyn.handle
        buf, done = _lib._p(np.zeros((4, 1, 6))), C.c_int64(-1)

        def said(rc):
            assert rc == 1
            return lib.uf3_last_error(dyn.ctx.handle).decode()

        def run(n=4, dt=1.0, temp=0.0, gamma=0.0, skin=0.5, every=0, thermo=None):
            return said(lib.uf3_md_run(h, n, dt, temp, gamma, 0, skin, every, 0, thermo))

        def flux(n=4, dt=1.0, every=0, flux_every=0, out=None):
            return said(lib.uf3_md_run_flux(h, n, dt, 0.0, 0.0, 0, 0.5, every, 0, None, flux_every, out))

        def grade(n=4, dt=1.0, every=0, grade_every=0, stop=0.0, out=None):
            return said(lib.uf3_md_run_grade(h, n, dt, 0.0, 0.0, 0, 0.5, every, 0, None, None, grade_every, stop, out, C.byref(done)))

        # the sampler's own checks come first, under its entry's name
        assert flux(n=-1, flux_every=-2) == "uf3_md_run_flux: flux_every must be >= 0"
        assert flux(n=-1, flux_every=2, out=buf) == "uf3_md_run_flux: a flux buffer was given but no record is due"
        assert flux(n=4, dt=-1.0, flux_every=2) == "uf3_md_run_flux: flux records are due but the flux buffer is NULL"
        assert grade(n=-1, grade_every=-2) == "uf3_md_run_grade: grade_every must be >= 0"
        assert grade(dt=-1.0, stop=float("nan")) == "uf3_md_run_grade: grade_stop is not a number"
        assert grade(n=4, dt=-1.0, grade_every=2) == "uf3_md_run_grade: grade records are due but the grades buffer is NULL"
        assert grade(n=1, dt=-1.0, grade_every=2, out=buf) == "uf3_md_run_grade: a grades buffer was given but no record is due"
        assert grade(n=4, dt=-1.0, grade_every=2, out=buf) == "uf3_md_run_grade: null argument (w)"
        # the shared checks, in the order of the parameter list, under uf3_md_run's name from all three entries
        for entry in (run, flux, grade):
            assert entry(n=-1, dt=-1.0) == "uf3_md_run: n_steps must be >= 0"
            assert entry(dt=-1.0, every=-1) == "uf3_md_run: dt must be positive and finite"
            assert entry(every=-1) == "uf3_md_run: thermo_every must be >= 0"
            assert entry(every=2) == "uf3_md_run: thermo records are due but the thermo buffer is NULL"
        assert run(dt=-1.0, temp=-5.0) == "uf3_md_run: dt must be positive and finite"
        assert run(temp=-5.0, gamma=-1.0) == "uf3_md_run: temperature must be finite and >= 0"
        assert run(gamma=-1.0, every=-1) == "uf3_md_run: friction must be finite and >= 0"
        assert run(every=-1, skin=9.0) == "uf3_md_run: thermo_every must be >= 0"
        assert run(skin=9.0, every=2) == "uf3_md_run: skin must lie in [0, 4] Angstrom"
        assert run(every=5, thermo=buf) == "uf3_md_run: a thermo buffer was given but no record is due"
        assert dyn.step == 0 and done.value == 0
