"""Every device kernel that walks triplets outside the featurizer, on bases whose l and m legs differ (tests/_uneven.py): the
uneven three-species basis (leading trim 0 and 3), where the per-trio masks of all three legs reject list entries, and the two
symmetry-1 bases, where two neighbours of one species sit on unequal legs.

The rule: a triplet's energy is the reference's -- leg l takes the neighbour of lower atomic number, for equal
species the one with the lower reference supercell index as seen from the real copy of the centre -- and every other quantity is
the exact derivative or partition of that energy.  So energies and strain derivatives are held against the oracle, forces against
_flux_ref.term_forces (the oracle's own on the uneven bases; on symmetry-1 bases the oracle's forces, like the reference's, are
not the gradient of its energy: tests/test_uneven_legs_host.py), the rest against the NumPy restatements.

Every bound is the one the existing test of the same kernel uses; its source is named next to it.  tests/test_uneven_legs_host.py
shows that these frames make the masks reject, that a wrong assignment moves the numbers by more than 1e-3, and that the references
agree with each other."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import _lib, parallel
from uf3_amd.data.composition import atomic_numbers
from uf3_amd.forcefield import calculator, harmonic, mc
from uf3_amd.regression import least_squares as ls
from uf3_amd.representation import process
import _flux_ref as FR
import _harmonic_ref as HR
import _mc_ref as R
import _uneven as U
from _util import dbg, tensor_to_voigt, worst_elementwise  # noqa: F401  (dbg: the fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-9                   # tests/test_gpu_virial.py, tests/test_gpu_species.py, tests/test_gpu_mc.py
FLUX_RTOL = 1e-10            # tests/test_gpu_flux.py::test_device_against_restatement
MASS = {41: 92.906, 42: 95.95, 74: 183.84}


@functools.lru_cache(maxsize=None)
def _ob(name):
    return O.OracleBasis(U.basis(name))


@functools.lru_cache(maxsize=None)
def _model(name):
    model = ls.WeightedLinearModel(U.basis(name))
    model.coefficients = U.coefficients(U.basis(name))
    return model


def _calc(name, skin=0.0):
    return calculator.UFCalculator(_model(name), md_skin=skin)


def _coeff(name):
    return np.asarray(_model(name).coefficients, dtype=float)


def _reference(name, atoms):
    """(E, F, dE/d strain): the oracle's energy and strain derivative; minus the gradient of that energy"""
    e, f, v = O.evaluate(_ob(name), atoms, _coeff(name), virial=True)
    if not name.startswith("uneven"):
        f = FR.term_forces(_ob(name), atoms, _coeff(name))
    return e, f, v


@functools.lru_cache(maxsize=None)
def _frame_reference(name, k):
    """of frame k of the basis' batch (-1: the small frame): computed once, shared, never changed"""
    out = _reference(name, U.small_frame(name) if k < 0 else U.frames(name)[k])
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _check_frame(e, f, v, ref, label):
    """tests/test_gpu_virial.py::_check_frame (also what tests/test_gpu_species.py applies)"""
    e_o, f_o, v_o = ref
    err_f = None if f is None else worst_elementwise(f, f_o, TOL)
    err_v = worst_elementwise(v, v_o, rtol=1e-9, floor=1e-11)
    print(f"{label}: |dE| / max(1, |E|) = {abs(e - e_o) / max(1.0, abs(e_o)):.2e} (bound {TOL:.0e}), worst_elementwise F "
          f"{'-' if err_f is None else format(err_f, '.2e')}, dE/dstrain {err_v:.2e} (bound 1)")
    assert abs(e - e_o) <= TOL * max(1.0, abs(e_o)), (label, e, e_o)
    if f is not None:
        assert err_f <= 1.0, label
    assert err_v <= 1.0, (label, v, v_o)


# ------------------------------------------------------------------------------------------------ uf3_eval_virial
@pytest.mark.parametrize("name", U.BASES)
def test_plain_and_gather_routes_batch_and_alone(name, dbg, monkeypatch):
    """md_skin = 0: the ragged batch through the centre pass + collection pass, through the gather instance (UF3_EVAL_GATHER,
    and without forces), and one frame alone.  Bounds: tests/test_gpu_virial.py::test_plain_route_on_a_ragged_batch_host_and_
    device_entries, tests/test_gpu_species.py::test_evaluator_plain_and_gather_routes."""
    dbg.basis(U.basis(name))
    calc = _calc(name)
    frames = list(U.frames(name))
    for _ in range(2):
        calc.evaluate_frames(frames, virial=True)                     # (list capacity tuned)
    dbg.launches()
    for label, env, forces in (("plain", {}, True), ("gather", {"UF3_EVAL_GATHER": "1"}, True), ("forces=False", {}, False)):
        for key, val in env.items():
            monkeypatch.setenv(key, val)
        e, f, off, v = calc.evaluate_frames(frames, forces=forces, virial=True)
        for key in env:
            monkeypatch.delenv(key)
        said = dbg.launches()
        gather = int(label != "plain")
        assert said and all(s["vir"] == 1 and s["md"] == 0 and s["gather"] == gather for s in said), said
        assert (f is None) == (not forces)
        for k in range(len(frames)):
            _check_frame(e[k], None if f is None else f[off[k]:off[k + 1]], v[k], _frame_reference(name, k), f"{name} {label} frame {k}")
    e, f, off, v = calc.evaluate_frames(frames[1:2], virial=True)
    _check_frame(e[0], f, v[0], _frame_reference(name, 1), f"{name} frame 1 alone")


@pytest.mark.parametrize("name", U.BASES)
def test_md_route_on_a_walk(name, dbg):
    """The MD route (skin 0.5) over six displaced steps, every step against the references; the steps are served from the kept
    lists.  Bounds: tests/test_gpu_virial.py::test_md_route_instances_on_every_step_of_a_walk."""
    dbg.basis(U.basis(name))
    start = U.frames(name)[0]
    plain = _calc(name)
    for _ in range(2):
        plain.evaluate_frames([start], virial=True)                   # (capacity tuned: the MD route starts from a tuned context)
    calc = _calc(name, skin=0.5)
    rng = np.random.default_rng(6)
    pos = np.asarray(start.get_positions(), dtype=float)
    ctx = _lib.get_context(None)
    before = ctx.md_stats()
    dbg.launches()
    for step in range(6):
        pos = pos + rng.uniform(-0.03, 0.03, pos.shape)
        atoms = U.displaced(start, pos)
        assert U.inside_cell(atoms)                                   # (sym-1: the references and the device see the same images)
        e, f, _, v = calc.evaluate_frames([atoms], virial=True)
        said = dbg.launches()
        assert said and said[-1]["vir"] == 1 and said[-1]["md"] == 1 and said[-1]["gather"] == 0, said
        _check_frame(e[0], f, v[0], _reference(name, atoms), f"{name} md step {step}")
    after = ctx.md_stats()
    print(f"{name}: md_stats before {before}, after {after}")
    assert after["steps"] - before["steps"] >= 5 and after["builds"] - before["builds"] < 6, (before, after)   # (served from lists)


# ------------------------------------------------------------------------------------------------ uf3_eval_atoms, uf3_eval_centres
@pytest.mark.parametrize("name", U.BASES)
def test_atom_and_centre_shares(name, dbg):
    """Three disjoint ranges of uf3_eval_atoms (the gather role) and of uf3_eval_centres (the centre pass on a block + its halo):
    each family adds up to the whole frame's result and to the references; single-atom uf3_eval_atoms energies are the site
    energies U_i.  Bounds: tests/test_gpu_species.py::test_evaluator_atom_and_centre_shares (against the whole frame: the same),
    tests/test_gpu_flux.py::test_device_against_restatement (U_i)."""
    dbg.basis(U.basis(name))
    calc = _calc(name)
    atoms = U.frames(name)[0]
    n = len(atoms)
    ref = _frame_reference(name, 0)
    for _ in range(2):
        whole = calc.evaluate_frames([atoms], virial=True)
    dbg.launches()
    for which in ("atoms", "centres"):
        share = calc.evaluate_atom_range if which == "atoms" else calc.evaluate_centre_range
        parts = [share(atoms, *parallel.shard_range(n, r, 3), virial=True) for r in range(3)]
        said = dbg.launches()
        assert len(said) >= 3 and all(s["vir"] == 1 and s["centres"] == int(which == "centres") for s in said), said
        assert all(s["gather"] == int(which == "atoms") for s in said), said
        e, f, v = sum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts)
        _check_frame(float(np.ravel(e)[0]), f, np.ravel(v), (whole[0][0], whole[1], whole[3][0]), f"{name} {which} against the whole frame")
        _check_frame(float(np.ravel(e)[0]), f, np.ravel(v), ref, f"{name} {which} against the references")
    U_ref = FR.site_terms(_ob(name), atoms, _coeff(name))[0]
    singles = np.array([float(np.ravel(calc.evaluate_atom_range(atoms, i, i + 1, forces=False)[0])[0]) for i in range(n)])
    err = np.abs(singles - U_ref).max() / np.abs(U_ref).max()
    print(f"{name}: single-atom shares against U_i {err:.2e} (bound {FLUX_RTOL:.0e})")
    assert err <= FLUX_RTOL


# ------------------------------------------------------------------------------------------------ uf3_hessian
@pytest.mark.parametrize("name", U.BASES)
def test_hessian_with_mixed_and_born_terms(name):
    """Bounds: tests/test_gpu_harmonic.py::test_device_against_restatement (1e-10 of the largest entry) and, on sym1_unary,
    ::test_device_against_device_force_differences (h = 1e-5, 1e-6 of the largest entry)."""
    calc = _calc(name)
    atoms = U.small_frame(name)
    n = len(atoms)
    ref_H, ref_L, ref_B = HR.hessian(_ob(name), atoms, _coeff(name))
    H, L, B, _ = harmonic.hessian(calc, atoms, strain=True)
    errs = [np.abs(a - b).max() / np.abs(b).max() for a, b in ((H, ref_H), (L, ref_L), (B, ref_B))]
    print(f"{name}: H {errs[0]:.2e}, mixed {errs[1]:.2e}, Born {errs[2]:.2e} of the largest entry (bound 1e-10)")
    assert np.array_equal(harmonic.hessian(calc, atoms), H)
    assert max(errs) <= 1e-10, errs
    if name == "sym1_unary":
        pos = np.asarray(atoms.get_positions(), dtype=float)
        h = 1e-5
        frames = []
        for k in range(3 * n):
            for sgn in (1, -1):
                p = pos.copy()
                p[k // 3, k % 3] += sgn * h
                frames.append(U.displaced(atoms, p))
        assert all(U.inside_cell(a) for a in frames)
        f = calc.evaluate_frames(frames)[1].reshape(3 * n, 2, 3 * n)
        Hfd = -(f[:, 0] - f[:, 1]).T / (2 * h)
        err = np.abs(H - Hfd).max() / np.abs(H).max()
        print(f"{name}: H against differences of device forces {err:.2e} (bound 1e-6)")
        assert err <= 1e-6


# ------------------------------------------------------------------------------------------------ uf3_site_terms, uf3_heat_flux
def _vel(atoms, seed):
    return np.random.default_rng(seed).normal(0, 0.01, (len(atoms), 3))


def _masses(atoms):
    return np.array([MASS[int(q)] for q in atoms.get_atomic_numbers()])


@pytest.mark.parametrize("name", U.BASES)
def test_site_terms_and_heat_flux(name):
    """The ragged batch: U, W, J_conv and J_pot of every frame.  Bounds: tests/test_gpu_flux.py::test_device_against_restatement
    (1e-10 of each quantity's largest magnitude; J_pot: of the sum of its terms' absolute values)."""
    calc = _calc(name)
    frames = list(U.frames(name))
    vel = [_vel(a, 50 + k) for k, a in enumerate(frames)]
    masses = [_masses(a) for a in frames]
    Us, Ws = calc.site_terms(frames)
    flux = calc.heat_flux(frames, np.concatenate(vel), np.concatenate(masses))
    for k, a in enumerate(frames):
        rU, rW = FR.site_terms(_ob(name), a, _coeff(name))
        rJc, rJp, scale = FR.heat_flux(_ob(name), a, vel[k], masses[k], _coeff(name), with_scale=True)
        errs = (np.abs(Us[k] - rU).max() / np.abs(rU).max(), np.abs(Ws[k] - rW).max() / np.abs(rW).max(),
                np.abs(flux[k][0] - rJc).max() / np.abs(rJc).max(), (np.abs(flux[k][1] - rJp) / scale).max())
        print(f"{name} frame {k}: U {errs[0]:.2e}, W {errs[1]:.2e}, J_conv {errs[2]:.2e}, J_pot {errs[3]:.2e} (bound {FLUX_RTOL:.0e})")
        assert scale.min() > 0 and max(errs) <= FLUX_RTOL, (k, errs)
        e_o, _, v_o = _frame_reference(name, k)
        assert abs(Us[k].sum() - e_o) <= TOL * max(1.0, abs(e_o))
        Wsum = Ws[k].sum(axis=0)
        assert worst_elementwise(tensor_to_voigt(0.5 * (Wsum + Wsum.T)), v_o, rtol=1e-9, floor=1e-11) <= 1.0


# ------------------------------------------------------------------------------------------------ uf3_mc_delta, uf3_mc_run
MC_BASES = ["uneven_lead0", "uneven_lead3", "sym1_binary"]
MC_TEMPERATURE = 3000.0
MC_SEED = 11


def _oracle_energies(name, frames):
    return np.array([O.evaluate(_ob(name), a, _coeff(name), forces=False)[0] for a in frames])


@pytest.mark.parametrize("name", MC_BASES)
def test_mc_delta_energy_is_the_difference_of_two_oracle_energies(name):
    """48 swaps and 48 transmutations drawn from all there are (a species change moves triplets in and out of their trio's
    ranges and, on sym1_binary, onto other legs).  Bound: tests/test_gpu_mc.py::_check_deltas, 1e-9 max(1, |E|)."""
    calc = _calc(name)
    atoms = U.mc_frame(name)
    z = np.asarray(atoms.get_atomic_numbers())
    els = list(calc.bspline_config.element_list)
    rng = np.random.default_rng(3)
    swaps = [(i, j) for i in range(len(z)) for j in range(len(z)) if z[i] != z[j]]
    muts = [(i, el) for i in range(len(z)) for el in els if atomic_numbers[el] != z[i]]
    swaps = [swaps[k] for k in rng.choice(len(swaps), 48, replace=False)]
    muts = [muts[k] for k in rng.choice(len(muts), 48, replace=False)]
    e0 = float(_oracle_energies(name, [atoms])[0])
    tol = TOL * max(1.0, abs(e0))
    mu = {el: 0.0 for el in els}
    for mode, moves, kw in (("swap", swaps, {}), ("transmute", muts, dict(chemical_potentials=mu))):
        after = []
        for i, second in moves:
            zz = z.copy()
            if mode == "swap":
                zz[i], zz[second] = z[second], z[i]
            else:
                zz[i] = atomic_numbers[second]
            after.append(U.with_numbers(atoms, zz))
        want = _oracle_energies(name, after) - e0
        with mc.MonteCarlo(calc, atoms, 300.0, mode=mode, **kw) as chain:
            got = chain.delta_energy(np.zeros(len(moves), dtype=int), np.array([m[0] for m in moves]), [m[1] for m in moves])
        err = np.abs(got - want)
        print(f"{name} {mode}: {len(moves)} moves, |E| = {abs(e0):.3f}, max |dE| = {np.abs(want).max():.3e}, worst error {err.max():.3e} (tol {tol:.1e})")
        assert np.abs(want).max() > 1e-3
        assert err.max() <= tol, (mode, moves[int(err.argmax())], err.max())


@pytest.mark.parametrize("mode", ["swap", "transmute"])
@pytest.mark.parametrize("name", MC_BASES)
def test_mc_chain_follows_the_restatement_driven_by_oracle_energies(name, mode):
    """200 trials on one frame (24 or 54 atoms) against _mc_ref.Chains with the oracle's energies: the same decisions, species and counters, the
    running energy within 1e-9 max(1, |E|).  tests/test_gpu_mc.py::test_trajectory_parity_with_the_restatement."""
    calc = _calc(name)
    atoms = U.mc_frame(name)
    els = list(calc.bspline_config.element_list)
    zs = np.array([atomic_numbers[e] for e in els])
    assert list(zs) == sorted(zs)
    mu = None if mode == "swap" else {e: 0.02 * k for k, e in enumerate(els)}
    ref = R.Chains(lambda spec: _oracle_energies(name, [U.with_numbers(atoms, zs[s]) for s in spec]),
                   [np.searchsorted(zs, atoms.get_atomic_numbers())], [MC_TEMPERATURE], R.SWAP if mode == "swap" else R.TRANSMUTE,
                   MC_SEED, len(els), mu=None if mu is None else [mu[e] for e in els])
    ref.run(200)
    n_live = sum(1 for d in ref.decisions if not d[2])
    worst = min(ref.margins)
    print(f"{name} {mode}: {n_live} non-null trials of 200, {int(ref.accepted.sum())} accepted, smallest |exp(-dE'/kT) - u| = {worst:.3e}")
    # properties of the input: no decision of the reference hangs on the last digits, and the chain does move (two species in
    # equal shares: half of the swap proposals pick like atoms, 100 +- 7 live trials of 200)
    assert worst >= 1e-6 and n_live > 60 and ref.accepted.sum() > 10
    extra = dict(chemical_potentials=mu) if mode == "transmute" else {}
    with mc.MonteCarlo(calc, [atoms], [MC_TEMPERATURE], mode=mode, seed=MC_SEED, **extra) as chain:
        out = chain.run(200)
        got_z = chain.numbers
    assert np.array_equal(got_z, zs[ref.species[0]])
    assert np.array_equal(out["accepted"], ref.accepted) and np.array_equal(out["trials"], ref.trials)
    tol = TOL * np.maximum(1.0, np.abs(ref.energy))
    print(f"{name} {mode}: running energy {out['energy']}, reference {ref.energy}, tol {tol}")
    assert np.all(np.abs(out["energy"] - ref.energy) <= tol)


# ------------------------------------------------------------------------------------------------ uf3_featurize_virial
@pytest.mark.parametrize("name", U.BASES)
def test_virial_rows_through_coefficients(name):
    """x_v @ c is the oracle's strain derivative for four coefficient vectors.  Bound: tests/test_gpu_virial_rows.py::
    test_rows_against_the_oracle_through_coefficients (worst_elementwise, rtol 1e-9, floor 1e-11)."""
    b = U.basis(name)
    atoms = U.frames(name)[0]
    x_v = process.BasisFeaturizer(b).featurize_virials([atoms])[0]
    assert x_v.shape == (6, b.n_feats) and np.all(np.isfinite(x_v))
    worst = 0.0
    for k in range(4):
        c = U.coefficients(b, 100 + k)
        v_o = O.evaluate(_ob(name), atoms, c, virial=True)[2]
        worst = max(worst, worst_elementwise(x_v @ c, v_o, rtol=1e-9, floor=1e-11))
    print(f"{name}: F = {b.n_feats}, worst_elementwise(x_v @ c, oracle; 1e-9, 1e-11) = {worst:.2e} (bound 1)")
    assert worst <= 1.0
