"""Species-swap Monte Carlo on the device (``uf3_mc_*``, ``uf3_amd.forcefield.mc``) against ``UFCalculator.evaluate_frames`` and
the NumPy restatement in tests/_mc_ref.py: the energy difference of every move on five geometries (a cell thinner than the reach,
a cluster, a three-species slab, a 2-body model) and against the oracle, trial-for-trial parity of whole chains, block and batch
invariance, bookkeeping, the limits T = 0 and T -> infinity, the semi-grand-canonical site occupancy, and the context left as
it was found.

Tolerance on any energy or energy difference: 1e-9 max(1, |E_frame|), the bar tests/test_gpu_md.py holds the evaluator to."""
import ctypes as C
import os

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.data.composition import atomic_numbers
from uf3_amd.forcefield import calculator, mc
from uf3_amd.regression import least_squares as ls
import _mc_ref as R
from _util import GOLDEN, load_case

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _model(basis, seed, scale=0.05):
    model = ls.WeightedLinearModel(basis)
    coeff = np.random.default_rng(seed).normal(0, scale, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    model.coefficients = coeff
    return model


def _mow():
    basis = synthetic.notebook_basis(["Mo", "W"])
    model = _model(basis, 31)
    model.coefficients[:2] = [-0.3, 0.2]                      # unlike one-body terms
    return calculator.UFCalculator(model, md_skin=0.0)


def _ternary():
    _, meta, _ = load_case("case_ternary24_slab")
    basis = synthetic.notebook_basis(list(meta["element_list"]))
    model = _model(basis, 47)
    model.coefficients[:3] = [0.1, -0.2, 0.05]
    return calculator.UFCalculator(model, md_skin=0.0)


def _binary():
    return calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_binary.json")), md_skin=0.0)


def _bcc16():
    # cell edge 6.33 A against a reach of 7 A: every atom is its own image-neighbour, i and j meet through several images
    return synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [42, 74], seed=5, rattle=0.05, strain=0.0)


def _mow54():
    return synthetic.lattice_frame("bcc", (3, 3, 3), 3.2, [42, 74], seed=84, rattle=0.05)


def _cluster54():
    a = _mow54()
    return Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions(), cell=a.get_cell(), pbc=False)


def _with_numbers(a, z):
    return Atoms(numbers=np.asarray(z), positions=a.get_positions(), cell=a.get_cell(), pbc=a.get_pbc())


def _energies(calc, frames):
    return calc.evaluate_frames(frames, forces=False)[0]


def _all_moves(calc, atoms):
    """Every ordered swap of unlike atoms and every transmutation of one frame: (i, j, frame after) and (i, symbol, frame after)."""
    z = np.asarray(atoms.get_atomic_numbers())
    swaps, muts = [], []
    for i in range(len(z)):
        for j in range(len(z)):
            if z[i] != z[j]:
                zz = z.copy()
                zz[i], zz[j] = z[j], z[i]
                swaps.append((i, j, _with_numbers(atoms, zz)))
        for el in calc.bspline_config.element_list:
            if atomic_numbers[el] != z[i]:
                zz = z.copy()
                zz[i] = atomic_numbers[el]
                muts.append((i, el, _with_numbers(atoms, zz)))
    return swaps, muts


def _check_deltas(calc, atoms, energies_of):
    swaps, muts = _all_moves(calc, atoms)
    assert swaps and muts
    e0 = float(energies_of([atoms])[0])
    tol = TOL * max(1.0, abs(e0))
    mu = {el: 0.0 for el in calc.bspline_config.element_list}
    for mode, moves, kw in (("swap", swaps, {}), ("transmute", muts, dict(chemical_potentials=mu))):
        want = np.concatenate([energies_of([m[2] for m in moves[k:k + 256]]) for k in range(0, len(moves), 256)]) - e0
        with mc.MonteCarlo(calc, atoms, 300.0, mode=mode, **kw) as chain:
            got = chain.delta_energy(np.zeros(len(moves), dtype=int), np.array([m[0] for m in moves]), [m[1] for m in moves])
        err = np.abs(got - want)
        print(f"{mode}: {len(moves)} moves, |E| = {abs(e0):.3f}, max |dE| = {np.abs(want).max():.3e}, worst error {err.max():.3e} (tol {tol:.1e})")
        assert np.abs(want).max() > 1e-3                     # (the moves do change the energy: an all-zero answer would not pass)
        assert err.max() <= tol, (mode, moves[int(err.argmax())][:2], err.max())


CASES = {"bcc16": (_mow, _bcc16), "mow54": (_mow, _mow54), "cluster54": (_mow, _cluster54),
         "ternary24_slab": (_ternary, lambda: load_case("case_ternary24_slab")[2]),
         "nexe32_2body": (_binary, lambda: load_case("case_nexe32")[2])}


@pytest.mark.parametrize("name", list(CASES))
def test_delta_energy_is_the_difference_of_two_evaluations(name):
    make_calc, make_atoms = CASES[name]
    calc = make_calc()
    _check_deltas(calc, make_atoms(), lambda frames: _energies(calc, frames))


def test_delta_energy_against_the_oracle():
    from oracle import oracle as O
    calc = _mow()
    ob = O.OracleBasis(calc.bspline_config)
    coeff = calc.model.coefficients
    _check_deltas(calc, _bcc16(), lambda frames: np.array([O.evaluate(ob, a, coeff, forces=False)[0] for a in frames]))


# ---- whole chains ---------------------------------------------------------------------------------------------------------
TEMPS = [300.0, 1000.0, 3000.0]
SEEDS = {"swap": 11, "transmute": 12}
MU = {"Mo": 0.0, "W": 0.05}


def _three():
    return [_bcc16(), _mow54(), _cluster54()]


def _reference(calc, frames, mode, seed, temps=TEMPS, swappable=None):
    els = list(calc.bspline_config.element_list)
    zs = np.array([atomic_numbers[e] for e in els])
    species = [np.searchsorted(zs, a.get_atomic_numbers()) for a in frames]
    assert list(zs) == sorted(zs)

    def energies_of(spec):
        return _energies(calc, [_with_numbers(a, zs[s]) for a, s in zip(frames, spec)])
    mu = None if mode == "swap" else [MU[e] for e in els]
    return R.Chains(energies_of, species, temps, R.SWAP if mode == "swap" else R.TRANSMUTE, seed, len(els), mu=mu,
                    swappable=swappable), zs


def _chain(calc, frames, mode, seed, temps=TEMPS, **kw):
    extra = dict(chemical_potentials=MU) if mode == "transmute" else {}
    return mc.MonteCarlo(calc, frames, temps, mode=mode, seed=seed, **extra, **kw)


@pytest.mark.parametrize("mode", ["swap", "transmute"])
def test_trajectory_parity_with_the_restatement(mode):
    calc, frames = _mow(), _three()
    ref, zs = _reference(calc, frames, mode, SEEDS[mode])
    want = ref.run(400, record_every=50)
    # a property of the input (seed, model, frames): no decision of the reference hangs on the last digits of exp()
    worst = min(ref.margins)
    n_live = sum(1 for d in ref.decisions if not d[2])
    print(f"{mode}: {n_live} non-null trials of {len(ref.decisions)}, {int(ref.accepted.sum())} accepted, smallest |exp(-dE'/kT) - u| = {worst:.3e}")
    assert worst >= 1e-6
    assert n_live > 300 and ref.accepted.sum() > 30
    with _chain(calc, frames, mode, SEEDS[mode]) as chain:
        out = chain.run(400, record_every=50)
        got_z = chain.numbers
    off = np.cumsum([0] + [len(a) for a in frames])
    for f in range(3):
        assert np.array_equal(got_z[off[f]:off[f + 1]], zs[ref.species[f]]), f
    assert np.array_equal(out["accepted"], ref.accepted) and np.array_equal(out["trials"], ref.trials)
    tol = TOL * np.maximum(1.0, np.abs(ref.energy))
    print("running energies", out["energy"], "reference", ref.energy, "tol", tol)
    assert np.all(np.abs(out["energy"] - ref.energy) <= tol)
    rec = out["records"]
    assert np.array_equal(rec["trial"], 50 * np.arange(1, 9))
    assert np.array_equal(rec["accepted"], want[..., 1].astype(np.int64)) and np.array_equal(rec["trials"], want[..., 2].astype(np.int64))
    assert np.array_equal(rec["composition"], want[..., 3:].astype(np.int64))
    assert np.all(np.abs(rec["energy"] - want[..., 0]) <= tol[None, :])


def _final(chain):
    s = chain._state("z", "energies", "accepted", "trials")
    return s["z"], s["energies"], s["accepted"], s["trials"]


@pytest.mark.parametrize("mode", ["swap", "transmute"])
def test_blocks_and_batches_do_not_change_a_chain(mode):
    calc, frames = _mow(), _three()
    with _chain(calc, frames, mode, 5) as whole:
        whole.run(400)
        want = _final(whole)
    with _chain(calc, frames, mode, 5) as split:
        split.run(150)
        split.run(250)
        got = _final(split)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    # one object per frame: the frame index is part of the Philox counter, so a lone frame repeats the batch's frame 0 only
    with _chain(calc, [frames[0]], mode, 5, temps=[TEMPS[0]]) as alone:
        alone.run(400)
        z, e, acc, tri = _final(alone)
    n0 = len(frames[0])
    assert np.array_equal(z, want[0][:n0]) and e[0] == want[1][0] and acc[0] == want[2][0] and tri[0] == want[3][0]
    # ... and the other frames do not depend on what stands next to them: the same frames behind a different first frame
    with _chain(calc, [frames[2], frames[1], frames[2]], mode, 5, temps=[TEMPS[0], TEMPS[1], TEMPS[2]]) as other:
        other.run(400)
        z2, e2, acc2, tri2 = _final(other)
    off = np.cumsum([0] + [len(a) for a in frames])
    assert np.array_equal(z2[len(frames[2]):len(frames[2]) + len(frames[1])], want[0][off[1]:off[2]])
    assert np.array_equal(z2[-len(frames[2]):], want[0][off[2]:off[3]])
    assert np.array_equal(e2[1:], want[1][1:]) and np.array_equal(acc2[1:], want[2][1:]) and np.array_equal(tri2[1:], want[3][1:])


def test_bookkeeping_after_many_trials():
    calc, frames = _mow(), _three()
    n = sum(len(a) for a in frames)
    mask = np.ones(n, dtype=bool)
    mask[::3] = False
    z0 = np.concatenate([a.get_atomic_numbers() for a in frames])
    with mc.MonteCarlo(calc, frames, [800.0, 1500.0, 3000.0], seed=3, swappable=mask) as chain:
        comp0 = mc.composition(chain.numbers, chain._batch.offsets, chain.element_list)
        out = chain.run(2000)
        final = chain.get_atoms()
        z1 = chain.numbers
        energy = chain.get_potential_energies()
        acceptance = chain.acceptance
    assert np.array_equal(out["composition"], comp0)                          # swaps conserve every frame's composition
    assert np.array_equal(z1[~mask], z0[~mask]) and np.any(z1[mask] != z0[mask])
    assert np.all(out["trials"] == 2000) and np.all(out["accepted"] > 20)
    assert np.allclose(acceptance, out["accepted"] / 2000.0)
    want = _energies(calc, final)
    err = np.abs(energy - want)
    print("running energy after 2000 trials", energy, "evaluator", want, "error", err)
    assert np.all(err <= TOL * np.maximum(1.0, np.abs(want)))
    assert np.array_equal(energy, out["energy"])


def test_limits():
    calc, frames = _mow(), _three()
    with mc.MonteCarlo(calc, frames, 0.0, seed=9) as cold:
        rec = cold.run(600, record_every=20)["records"]
    assert np.all(np.diff(rec["energy"], axis=0) <= 0.0) and np.all(rec["energy"][-1] < rec["energy"][0])
    ref, _ = _reference(calc, frames, "swap", 9, temps=[1e9] * 3)
    ref.run(300)
    live = np.array([sum(1 for d in ref.decisions if d[0] == f and not d[2]) for f in range(3)])
    with mc.MonteCarlo(calc, frames, 1e9, seed=9) as hot:
        out = hot.run(300)
    assert np.array_equal(out["accepted"], live) and np.all(live > 100)       # every non-null trial accepted
    pure = _with_numbers(frames[1], np.full(len(frames[1]), 74))
    with mc.MonteCarlo(calc, [pure], 3000.0, seed=9) as one:
        out = one.run(500)
        d = one.delta_energy(np.zeros(6, dtype=int), np.arange(6), np.arange(6)[::-1].copy())
    assert out["accepted"][0] == 0 and out["trials"][0] == 500
    assert np.array_equal(d, np.zeros(6))                                     # like atoms: exactly 0


def test_semi_grand_canonical_site_occupancy():
    # one-body terms only: the sites are independent, P(W) = 1 / (1 + exp((de1 - dmu) / kT)) by detailed balance
    basis = synthetic.notebook_basis(["Mo", "W"])
    model = ls.WeightedLinearModel(basis)
    coeff = np.zeros(basis.n_feats)
    coeff[:2] = [0.0, 0.1]
    model.coefficients = coeff
    calc = calculator.UFCalculator(model, md_skin=0.0)
    frames = [synthetic.lattice_frame("bcc", (3, 3, 3), 3.2, [42, 74], seed=200 + k, rattle=0.05) for k in range(64)]
    with mc.MonteCarlo(calc, frames, 1200.0, mode="transmute", chemical_potentials={"Mo": 0.0, "W": 0.04}, seed=21) as chain:
        out = chain.run(100 * 54)
        z = chain.numbers
    n = z.size
    p = R.site_occupancy(0.1, 0.04, 1200.0)
    sigma = np.sqrt(p * (1 - p) / n)
    frac = np.mean(z == 74)
    print(f"W fraction {frac:.4f} of {n} sites, expected {p:.4f} +- {sigma:.4f}, acceptance {out['accepted'].sum() / out['trials'].sum():.3f}")
    assert n == 3456 and abs(frac - p) <= 5 * sigma
    assert np.array_equal(out["composition"].sum(0), [np.sum(z == 42), np.sum(z == 74)])


# ---- the library's edges ---------------------------------------------------------------------------------------------------
def test_library_refuses_bad_arguments():
    calc = _mow()
    a = _mow54()
    with mc.MonteCarlo(calc, [a], 300.0) as chain:
        lib, h, ctx = chain.ctx.lib, chain.handle, chain.ctx
        t, buf = np.array([300.0]), np.zeros((2, 1, 5))
        mu = np.zeros(2)
        assert lib.uf3_mc_run(h, -1, 0, _lib._p(t), None, 0, 0, None) == 1
        assert lib.uf3_mc_run(h, 10, 2, _lib._p(t), None, 0, 0, None) == 1
        assert lib.uf3_mc_run(h, 10, 0, None, None, 0, 0, None) == 1
        assert lib.uf3_mc_run(h, 10, 0, _lib._p(np.array([-1.0])), None, 0, 0, None) == 1
        assert lib.uf3_mc_run(h, 10, 0, _lib._p(t), _lib._p(mu), 0, 0, None) == 1          # mu in swap mode
        assert lib.uf3_mc_run(h, 10, 1, _lib._p(t), None, 0, 0, None) == 1                  # no mu in transmute mode
        assert lib.uf3_mc_run(h, 10, 0, _lib._p(t), None, 0, 5, None) == 1
        assert lib.uf3_mc_run(h, 10, 0, _lib._p(t), None, 0, 0, _lib._p(buf)) == 1
        one = np.zeros(1, dtype=np.int32)
        out = np.zeros(1)
        assert lib.uf3_mc_delta(h, 1, _lib._p(one), _lib._p(one), _lib._p(np.array([54], dtype=np.int32)), 0, _lib._p(out)) == 1
        assert lib.uf3_mc_delta(h, 1, _lib._p(np.array([1], dtype=np.int32)), _lib._p(one), _lib._p(one), 0, _lib._p(out)) == 1
        assert chain.run(0)["trials"][0] == 0                                             # (the object still works)
        batch, db = chain._batch, chain._dbasis
        new = C.c_void_p()
        args = lambda pos, z, mask: (db.handle, C.byref(batch.struct), _lib._p(pos), _lib._p(z), _lib._p(mask), _lib._p(calc._c1),
                                     _lib._p(calc._c2), _lib._p(calc._c3), C.byref(new))
        bad_pos = batch.pos.copy()
        bad_pos[3, 1] = np.nan
        assert lib.uf3_mc_create(*args(bad_pos, batch.z, None)) == 1
        assert lib.uf3_mc_create(*args(None, batch.z, None)) == 1
        assert lib.uf3_mc_create(*args(batch.pos, batch.z, np.full(54, 2, dtype=np.uint8))) == 1
        foreign = batch.z.copy()
        foreign[0] = 23
        assert lib.uf3_mc_create(*args(batch.pos, foreign, None)) == 2
        assert not new.value


def test_runs_leave_the_context_and_the_calculator_as_they_were():
    calc = _mow()
    ctx = _lib.get_context(calc.device)
    other = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [42, 74], seed=61)
    e0, f0, _ = calc.evaluate_frames([other])                    # (md_skin 0: the context's skin is 0)
    stats0 = ctx.md_stats()
    with mc.MonteCarlo(calc, _three(), TEMPS, seed=2) as chain:
        chain.run(300)
        with pytest.raises(_lib.UF3Error):                       # an error return
            chain.ctx.check(chain.ctx.lib.uf3_mc_run(chain.handle, 10, 3, None, None, 0, 0, None))
        chain.run(50, record_every=10)
        chain.get_potential_energies()
    foreign = _mow54()
    foreign.numbers[:3] = 23                                      # V: outside the basis
    with pytest.raises(ValueError):
        mc.MonteCarlo(calc, [foreign], 300.0)
    assert ctx.md_stats() == stats0 and getattr(ctx, "_md_skin", 0.0) == 0.0
    e1, f1, _ = calc.evaluate_frames([other])
    assert np.array_equal(e0, e1) and np.array_equal(f0, f1)


def test_set_positions_rebuilds_the_table():
    calc = _mow()
    with mc.MonteCarlo(calc, _three(), TEMPS, seed=2) as chain:
        chain.run(100)
        z = chain.numbers[16:70]
        i, j = 3, int(np.flatnonzero(z != z[3])[0])
        before = chain.delta_energy(1, i, j)
        chain.set_positions(chain._batch.pos + np.random.default_rng(0).normal(0, 0.05, chain._batch.pos.shape))
        after = chain.delta_energy(1, i, j)
        moved = chain.get_atoms()[1]
        running = chain.get_potential_energies()
    zz = np.asarray(moved.get_atomic_numbers()).copy()
    zz[i], zz[j] = zz[j], zz[i]
    e = _energies(calc, [moved, _with_numbers(moved, zz)])
    tol = TOL * max(1.0, abs(e[0]))
    print("dE before", before, "after", after, "evaluator", e[1] - e[0], "running", running[1], "evaluator", e[0])
    assert abs(before - after) > 1e-6                                         # the difference follows the new positions
    assert abs(after - (e[1] - e[0])) <= tol
    assert abs(running[1] - e[0]) <= tol                                      # ... and so do the running energies
