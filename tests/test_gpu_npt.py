"""Constant-pressure dynamics on the device (``uf3_md_run_npt``, uf3_amd/csrc/uf3_npt.h) against the NumPy restatement in
tests/_npt_ref.py, whose energies, forces and strain derivatives come from ``UFCalculator.evaluate_frames`` at the
restatement's own cells: NPH and Langevin-piston NPT trajectories, block invariance, the dt^2 error of the NPH conserved
quantity, batch independence, the static equilibrium volume against ``get_stress``, that a run stays on the evaluator's
persistent lists while its cells change (and rebuilds them when a compression uses up the skin), sampling, and the context
left as it was found.  Masses are test values, not a periodic table."""
import os

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator, md
from uf3_amd.regression import least_squares as ls
from _md_ref import init_velocities
from _npt_ref import Pistons, run as ref_run
from _util import GOLDEN

pytestmark = pytest.mark.gpu
MASSES = {"W": 180.0, "Mo": 96.0}
TOL = 1e-9                                # test_gpu_md.py's


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


def _batches():
    # (frames of different size in one batch; all periodic: a cluster cannot be run at a pressure)
    return {"w_batch": (_unary, lambda: [_w128(1), synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=7), _w128(2)]),
            # 54 | 300 | 128 atoms: the middle frame spans two chunks of the chunk table (256 + 44) at non-zero offsets
            "w300_two_chunks": (_unary, lambda: [synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=7),
                                                 synthetic.lattice_frame("bcc", (5, 5, 6), 3.165, [74], seed=17), _w128(2)]),
            "mow54": (_mow, lambda: [synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [42, 74], seed=84)])}


def _evaluate(calc, frames):
    off = np.cumsum([0] + [len(a) for a in frames])
    cells0 = [np.asarray(a.get_cell(), dtype=float).reshape(3, 3) for a in frames]

    def f(x, s):
        moved = [Atoms(numbers=a.get_atomic_numbers(), positions=x[off[k]:off[k + 1]], cell=cells0[k] * s[k], pbc=True)
                 for k, a in enumerate(frames)]
        e, frc, _, w = calc.evaluate_frames(moved, virial=True)
        return np.asarray(e, dtype=float), frc, np.asarray(w)[:, :3].sum(1)
    return f, off, np.abs(np.linalg.det(np.array(cells0)))


def _parity(name, n_steps, temperature_K, friction, p0, tau, gamma_p=0.0, t_piston=None, skin=0.5, moved=1e-3, seed=9):
    make_calc, make_frames = _batches()[name]
    calc, frames = make_calc(), make_frames()
    evaluate, off, vol0 = _evaluate(calc, frames)
    m = md.resolve_masses(frames, MASSES)
    x0 = np.concatenate([a.get_positions() for a in frames])
    v0 = init_velocities(m, off, 300.0, 4, 0)
    ctx = _lib.get_context(calc.device)
    b0 = ctx.md_stats()["builds"]
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=temperature_K, friction_per_fs=friction, seed=seed,
                              skin=skin, pressure_eV_A3=p0, barostat_time_fs=tau, barostat_friction_per_fs=gamma_p,
                              piston_temperature_K=t_piston) as dyn:
        dyn.set_velocities(v0)
        dyn.run(n_steps)
        assert dyn.step == n_steps
        x, v, e, f = dyn.get_positions(), dyn.get_velocities(), dyn.get_potential_energies(), dyn.get_forces()
        s, ve, cells = dyn.cell_scales, dyn.strain_rates, dyn.cells
    builds = ctx.md_stats()["builds"] - b0
    P = Pistons(off, vol0, tau, temperature_K if t_piston is None else t_piston)
    xr, vr, sr, ver, er, fr = ref_run(x0, v0, m, P, np.ones(len(frames)), np.zeros(len(frames)), evaluate, n_steps, 1.0, p0,
                                      temperature_K, friction, gamma_p, seed)
    print(f"{name}: s - 1 = {sr - 1}, v_eps = {ver}, |dx| {np.abs(x - xr).max():.2e} |dv| {np.abs(v - vr).max():.2e} "
          f"|ds| {np.abs(s - sr).max():.2e} |dveps| {np.abs(ve - ver).max():.2e} |df| {np.abs(f - fr).max():.2e} builds {builds}")
    assert np.abs(x - xr).max() <= TOL, np.abs(x - xr).max()
    assert np.abs(v - vr).max() <= TOL, np.abs(v - vr).max()
    assert np.abs(s - sr).max() <= TOL and np.abs(ve - ver).max() <= TOL, (s - sr, ve - ver)
    assert np.all(np.abs(e - er) <= TOL * np.maximum(1.0, np.abs(er))), (e, er)
    assert np.abs(f - fr).max() <= 1e-8 * max(1.0, np.abs(fr).max())
    for k, a in enumerate(frames):
        assert np.abs(cells[k] - np.asarray(a.get_cell()) * sr[k]).max() <= TOL
    assert np.all(np.abs(sr - 1.0) > moved), sr                     # (the cells did move)
    return sr, builds


@pytest.mark.parametrize("name", ["w_batch", "w300_two_chunks", "mow54"])
def test_nph_parity(name):
    _parity(name, 30, 300.0, 0.0, 0.02, 1000.0)


@pytest.mark.parametrize("name", ["w_batch", "w300_two_chunks", "mow54"])
def test_npt_langevin_piston_parity(name):
    _parity(name, 30, 300.0, 0.05, 0.02, 1000.0, gamma_p=0.02)


def test_a_compression_that_uses_up_the_skin_rebuilds_and_still_matches():
    # r_cut (1 / s - 1) reaches the skin: with r_cut = 5.5 and skin 0.2 at s = 0.965; far before, the list test must have rebuilt.
    # The piston under 0.3 eV/A^3 oscillates (W_p ~ tau^2, the lattice is its spring): tau = 1000 fs gives a period of about
    # 80 steps whose first turning point, s ~ 0.95, lies at step 39, so the run ends while the cells are compressed that far
    sr, builds = _parity("w_batch", 40, 300.0, 0.0, 0.3, 1000.0, skin=0.2, moved=0.036)
    assert builds >= 2, builds


def _npt(calc, frames, dt=1.0, **kw):
    args = dict(masses=MASSES, temperature_K=300.0, friction_per_fs=0.05, seed=21, pressure_eV_A3=0.01, barostat_time_fs=500.0,
                barostat_friction_per_fs=0.01)
    args.update(kw)
    return md.MolecularDynamics(calc, frames, dt, **args)


def test_run_in_blocks_equals_one_run():
    calc, frames = _unary(), [_w128(1), synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=7)]
    out = []
    for blocks in ([60], [25, 35]):
        with _npt(calc, frames) as dyn:
            dyn.initialize_velocities(300.0)
            for n in blocks:
                dyn.run(n)
            assert dyn.step == 60
            out.append((dyn.get_positions(), dyn.get_velocities(), dyn.cell_scales, dyn.strain_rates))
    for a, b in zip(*out):
        assert np.abs(a - b).max() <= 1e-10, np.abs(a - b).max()
    assert np.all(np.abs(out[0][2] - 1.0) > 1e-4)


def test_nph_conserved_quantity_error_scales_with_dt_squared():
    calc = _unary()
    drift = {}
    for dt, every in ((1.0, 1), (0.5, 2)):
        with _npt(calc, [_w128(3)], dt, friction_per_fs=0.0, barostat_friction_per_fs=0.0, seed=5, barostat_time_fs=300.0) as dyn:
            dyn.initialize_velocities(300.0, exact=True)
            rec0 = dyn.run(0)
            assert rec0["conserved"].shape == (0, 1)
            m = dyn.masses
            h0 = dyn.get_potential_energies()[0] + md.kinetic_energy(dyn.get_velocities(), m) + 0.01 * dyn.volumes[0]
            rec = dyn.run(int(round(200 / dt)), thermo_every=every)
            h = rec["conserved"][:, 0]
            assert len(h) == 200
            drift[dt] = np.abs(h - h0).max()
            assert np.abs(rec["cell_scale"][:, 0] - 1.0).max() > 1e-3
            assert np.allclose(rec["volume"][:, 0], abs(np.linalg.det(_w128(3).get_cell())) * rec["cell_scale"][:, 0] ** 3, rtol=1e-12)
            assert rec["volume"][-1, 0] == pytest.approx(dyn.volumes[0], rel=1e-12)
    ratio = drift[1.0] / drift[0.5]
    print("NPH conserved-quantity drift", drift, ratio)
    assert 3.0 <= ratio <= 5.0, (drift, ratio)


def test_a_frame_alone_and_inside_a_batch_agree():
    calc = _unary()
    frames = [_w128(11), synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=12), _w128(13)]
    m = md.resolve_masses(frames, MASSES)
    off = np.cumsum([0] + [len(a) for a in frames])
    v0 = init_velocities(m, off, 300.0, 4, 0)
    with _npt(calc, frames, friction_per_fs=0.0, barostat_friction_per_fs=0.0) as dyn:
        dyn.set_velocities(v0)
        dyn.run(40)
        xb, sb = dyn.get_positions(), dyn.cell_scales
    for k in (1, 2):
        with _npt(calc, [frames[k]], friction_per_fs=0.0, barostat_friction_per_fs=0.0) as dyn:
            dyn.set_velocities(v0[off[k]:off[k + 1]])
            dyn.run(40)
            assert np.abs(dyn.get_positions() - xb[off[k]:off[k + 1]]).max() <= 1e-8
            assert abs(dyn.cell_scales[0] - sb[k]) <= 1e-8


# Steps the damped run below needs to reach |P - P0| <= 1e-5 eV/A^3, measured on the MI355X in blocks of 250: 500 for both
# pressures (then P - P0 = -5.9e-7 and 3.2e-6, V / V(s*) - 1 = 3.4e-7 and -1.8e-6).  The cap is twice that.
EQUILIBRIUM_STEPS = 500


@pytest.mark.parametrize("p0", [0.0, 0.006])              # 0.006 eV/A^3 = 0.96 GPa
def test_damped_dynamics_finds_the_static_equilibrium_volume(p0):
    """V must equal V(s*) to 5e-5 relative: dV/V = dp / B with B ~ 2 eV/A^3 and |dp| <= 1e-5 gives 5e-6, times ten."""
    calc = _unary()
    perfect = synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, [74], seed=0, rattle=0.0, strain=0.0)
    cell0, x0 = np.asarray(perfect.get_cell(), dtype=float), perfect.get_positions()

    def pressure(s):
        a = Atoms(numbers=perfect.get_atomic_numbers(), positions=x0 * s, cell=cell0 * s, pbc=True)
        return -calc.get_stress(a)[:3].sum() / 3.0
    lo, hi = 0.9, 1.1
    assert pressure(lo) > p0 > pressure(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if pressure(mid) > p0 else (lo, mid)
    s_star = 0.5 * (lo + hi)
    strained = 1.015 * s_star
    start = Atoms(numbers=perfect.get_atomic_numbers(),
                  positions=x0 * strained + np.random.default_rng(2).normal(0, 0.03, x0.shape), cell=cell0 * strained, pbc=True)
    steps, p = 0, np.inf
    with md.MolecularDynamics(calc, [start], 2.0, masses=MASSES, temperature_K=0.0, friction_per_fs=0.02, seed=1, pressure_eV_A3=p0,
                              barostat_time_fs=100.0, barostat_friction_per_fs=0.02, piston_temperature_K=300.0) as dyn:
        while abs(p - p0) > 1e-5 and steps < 2 * EQUILIBRIUM_STEPS:
            rec = dyn.run(250, thermo_every=250)
            steps += 250
            p = rec["pressure"][-1, 0]
        vol = dyn.volumes[0]
    print(f"P0 {p0}: s* {s_star:.8f}, {steps} steps, P - P0 {p - p0:.2e}, V / V(s*) - 1 {vol / (abs(np.linalg.det(cell0)) * s_star ** 3) - 1:.2e}")
    assert abs(p - p0) <= 1e-5, (p, steps)
    assert abs(vol / (abs(np.linalg.det(cell0)) * s_star ** 3) - 1.0) <= 5e-5


def test_a_run_stays_on_the_persistent_lists():
    calc = _unary()
    ctx = _lib.get_context(calc.device)
    with _npt(calc, [_w128(5)], friction_per_fs=0.01, barostat_friction_per_fs=0.002, pressure_eV_A3=0.0, skin=0.5) as dyn:
        dyn.initialize_velocities(300.0)
        dyn.run(1)                                       # (forces at the start: one call more than steps otherwise)
        st0 = ctx.md_stats()
        dyn.run(200)
        st1 = ctx.md_stats()
        assert abs(dyn.cell_scales[0] - 1.0) > 1e-5
    steps, builds = st1["steps"] - st0["steps"], st1["builds"] - st0["builds"]
    print("200 NPT steps: list steps", steps, "builds", builds, "redone", st1["redone"] - st0["redone"])
    assert steps >= 200                                  # every force call of the run was served from the lists
    assert builds < 50, builds                           # fewer than a quarter of them (NVE needs about one per 20 steps there)


def test_npt_samples_temperature_and_pressure():
    calc = _unary()
    frames = [_w128(100 + k) for k in range(32)]
    tau = 200.0
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=600.0, friction_per_fs=0.02, seed=2024,
                              pressure_eV_A3=0.0, barostat_time_fs=tau, barostat_friction_per_fs=0.005) as dyn:
        dyn.initialize_velocities(600.0)
        dyn.run(2000)
        rec = dyn.run(8000, thermo_every=10)
    t = rec["temperature"].mean()
    assert abs(t - 600.0) <= 0.03 * 600.0, t
    # standard error from the run's own block averages: blocks of 10 tau_p = 2000 fs = 200 records, every replica its own series
    p = rec["pressure"]
    blocks = p.reshape(4, 200, 32).mean(axis=1).reshape(-1)              # 4 blocks x 32 replicas
    err = blocks.std(ddof=1) / np.sqrt(len(blocks))
    print(f"NPT sampling: T {t:.1f} K, P {p.mean():.3e} +- {err:.1e} eV/A^3")
    assert abs(p.mean() - 0.0) <= 3.0 * err, (p.mean(), err)


def test_runs_leave_the_context_as_they_found_it_and_no_pressure_is_the_parent():
    calc = _unary()
    ctx = _lib.get_context(calc.device)
    other = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=61)
    e0, f0, _ = calc.evaluate_frames([other])
    assert not ctx.md_live()
    with _npt(calc, [_w128(1)], skin=0.7) as dyn:
        dyn.run(5)
        assert not ctx.md_live() and getattr(ctx, "_md_skin", 0.0) == 0.0
    foreign = _w128(2)
    foreign.numbers[:3] = 42                                      # Mo: outside the unary basis
    dyn = _npt(calc, [foreign])
    with pytest.raises(_lib.SpeciesError):
        dyn.run(3)
    assert dyn.step == 0 and not ctx.md_live()
    dyn.close()
    steps1 = ctx.md_stats()["steps"]
    e1, f1, _ = calc.evaluate_frames([other])
    assert ctx.md_stats()["steps"] == steps1 and getattr(ctx, "_md_skin", 0.0) == 0.0
    assert np.array_equal(e0, e1) and np.array_equal(f0, f1)
    # without a pressure: the records, the cells and the volumes of the parent
    with md.MolecularDynamics(calc, [_w128(1)], 1.0, masses=MASSES) as dyn:
        rec = dyn.run(4, thermo_every=2, stress=True)
        assert sorted(rec) == ["kinetic_energy", "potential_energy", "pressure", "step", "stress", "temperature"]
        assert np.array_equal(dyn.cells[0], np.asarray(_w128(1).get_cell())) and dyn.cell_scales[0] == 1.0
        assert dyn.volumes[0] == abs(np.linalg.det(np.asarray(_w128(1).get_cell())))
        assert np.array_equal(np.asarray(dyn.get_atoms()[0].get_cell()), np.asarray(_w128(1).get_cell()))


def test_atoms_and_wrapped_positions_use_the_current_cell():
    calc = _unary()
    with _npt(calc, [_w128(1)], pressure_eV_A3=0.05, barostat_time_fs=300.0) as dyn:
        dyn.initialize_velocities(300.0)
        rec = dyn.run(20, thermo_every=20)
        cell, s = dyn.cells[0], dyn.cell_scales[0]
        assert abs(s - 1.0) > 1e-4 and np.abs(cell - np.asarray(_w128(1).get_cell()) * s).max() <= 1e-12
        atoms = dyn.get_atoms()[0]
        assert np.array_equal(np.asarray(atoms.get_cell()), cell)
        frac = dyn.get_positions(wrap=True) @ np.linalg.inv(cell)
        assert frac.min() >= -1e-12 and frac.max() <= 1.0 + 1e-12
        e, _, _, w = calc.evaluate_frames([atoms], virial=True)
        assert abs(rec["potential_energy"][-1, 0] - e[0]) <= TOL * max(1.0, abs(e[0]))
        v, m = dyn.get_velocities(), dyn.masses
        tr_k = md.KE_UNIT * float(np.sum(m * np.sum(v * v, axis=1)))
        assert rec["pressure"][-1, 0] == pytest.approx((tr_k - w[0][:3].sum()) / (3 * dyn.volumes[0]), rel=1e-8, abs=1e-10)
        assert rec["cell_scale"][-1, 0] == s


def test_run_arguments_are_checked_in_the_order_of_the_parameter_list():
    """Two bad arguments at once: the message is that of the one checked first -- the barostat's four between friction and
    thermo_every -- under uf3_md_run_npt's name."""
    calc = _unary()
    with _npt(calc, [synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=3)]) as dyn:
        lib, h = dyn.ctx.lib, dyn.handle

        def run(n=4, dt=1.0, temp=300.0, gamma=0.0, p0=0.0, tau=500.0, gamma_p=0.0, t_piston=300.0, skin=0.5, every=0, thermo=None):
            assert lib.uf3_md_run_npt(h, n, dt, temp, gamma, p0, tau, gamma_p, t_piston, 0, skin, every, thermo) == 1
            return lib.uf3_last_error(dyn.ctx.handle).decode()

        assert run(n=-1, dt=-1.0) == "uf3_md_run_npt: n_steps must be >= 0"
        assert run(dt=-1.0, temp=-5.0) == "uf3_md_run_npt: dt must be positive and finite"
        assert run(temp=-5.0, gamma=-1.0) == "uf3_md_run_npt: temperature must be finite and >= 0"
        assert run(gamma=-1.0, p0=float("nan")) == "uf3_md_run_npt: friction must be finite and >= 0"
        assert run(p0=float("nan"), tau=0.0) == "uf3_md_run_npt: pressure must be finite"
        assert run(tau=0.0, gamma_p=-1.0) == "uf3_md_run_npt: barostat time must be positive and finite"
        assert run(gamma_p=-1.0, t_piston=0.0) == "uf3_md_run_npt: barostat friction must be finite and >= 0"
        assert run(t_piston=0.0, every=-1) == "uf3_md_run_npt: piston temperature must be positive and finite"
        assert run(every=-1, skin=9.0) == "uf3_md_run_npt: thermo_every must be >= 0"
        assert run(skin=9.0, every=2) == "uf3_md_run_npt: skin must lie in [0, 4] Angstrom"
        assert run(every=2) == "uf3_md_run_npt: thermo records are due but the thermo buffer is NULL"
        assert run(every=5, thermo=_lib._p(np.zeros((4, 1, 17)))) == "uf3_md_run_npt: a thermo buffer was given but no record is due"
        assert dyn.step == 0
