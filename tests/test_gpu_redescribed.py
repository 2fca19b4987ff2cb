"""The Hessian, the site terms and the heat current, the Monte Carlo table and the virial rows on re-described frames.

These families enumerate periodic images with code of their own (uf3_hessian.h: hess_geometry + hess_lists_atom, shared by the
batched lists of uf3_flux.h; uf3_hip.hip: mc_build_table; uf3_virial_rows.h: its own strain kernel on the shared walk).  Here
they meet the frames that the featurizer and the evaluator are held to (tests/_util.py: equivalence_cases): image ranges
[8, 2, 1], [3, 5, 1] and [7, 5, 1], reflections, permutations, a slab, a wire (36 atoms: its Hessian restatement takes 3 s on
the CPU, so the 36-atom wire itself is used), the 1-atom primitive cell, five and eight species.

1. device against the restatement (tests/test_redescribed_host.py: HARD), every listed description directly;
2. device against device through every description's mapping, supercells of 128, 216 and 432 atoms included;
3. positions outside the cell: which rule each entry follows (include/uf3_hip.h says the same).

Bounds, none of them new: H, mixed, born 1e-10 of the largest entry (tests/test_gpu_harmonic.py); U, W, J_conv 1e-10 of the
largest entry, J_pot 1e-10 of the sum of its terms' absolute values (tests/test_gpu_flux.py: _check); Monte Carlo 1e-9
max(1, |E|) (tests/test_gpu_mc.py: _check_deltas); virial rows worst_elementwise(rtol 1e-9, floor 1e-11) <= 1
(tests/test_gpu_virial_rows.py); the evaluator 1e-9 (tests/test_gpu_invariance.py)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.data.composition import atomic_numbers
from uf3_amd.forcefield import calculator, harmonic, mc
from uf3_amd.forcefield.md import MolecularDynamics
from uf3_amd.regression import least_squares as ls
from uf3_amd.representation import process
import _mc_ref as R
import _uneven as UN
import test_redescribed_host as RH
from _util import dbg, worst_elementwise  # noqa: F401  (dbg: the fixture)
from test_gpu_mc import _check_deltas
from test_gpu_virial import _MD_ROUTES

pytestmark = pytest.mark.gpu

RTOL = 1e-10                # site terms, heat current, Hessian: of the largest entry
MC_TOL = 1e-9               # x max(1, |E|)
EVAL_TOL = 1e-9
ORIGINAL = RH.ORIGINAL
MC_HARD = [(c, l) for c, l in RH.HARD if c != "bcc_w_primitive"]          # (one species, one atom: no move to propose)
VIRIAL_HARD = [("quinary", "skew_351"), (RH.S8, ORIGINAL), ("bcc_mow", "skew_821")]
_ids = lambda pairs: [f"{c}-{l}" for c, l in pairs]                       # noqa: E731


@functools.lru_cache(maxsize=None)
def _calc(case):
    return calculator.UFCalculator(RH.model(case), md_skin=0.0)


def _periodic(atoms):
    return bool(np.all(atoms.get_pbc()))


@functools.lru_cache(maxsize=None)
def _site(case, label):
    """U, W, flux [2, 3] of one description on the device (computed once)"""
    calc, atoms = _calc(case), RH.frame(case, label)
    U, W = calc.site_terms([atoms])
    flux, Uf = calc.heat_flux([atoms], RH.velocities(case, label), RH.masses(atoms), site_energies=True)
    assert np.array_equal(Uf, U[0])
    return RH._frozen(U[0], W[0], flux[0])


@functools.lru_cache(maxsize=None)
def _hess(case, label):
    """H, mixed, born (None, None on a slab or wire) of one description on the device (computed once)"""
    calc, atoms = _calc(case), RH.frame(case, label)
    if not _periodic(atoms):
        return RH._frozen(harmonic.hessian(calc, atoms)) + (None, None)
    H, L, B, _ = harmonic.hessian(calc, atoms, strain=True)
    return RH._frozen(H, L, B)


@functools.lru_cache(maxsize=None)
def _hessian_scales(case):
    """RH.hessian_scales from the device's own values (the original's largest entries; on the primitive cell what cancels)."""
    H0, L0, _ = _hess(case, ORIGINAL)
    if case != "bcc_w_primitive":
        return float(np.abs(H0).max()), (None if L0 is None else float(np.abs(L0).max()))
    h = float(np.abs(_hess(case, "conventional")[0]).max())
    a = RH.frame(case, ORIGINAL)
    return h, h * float(abs(np.linalg.det(np.asarray(a.get_cell(), float))) / len(a)) ** (1.0 / 3.0)


# =========================================================================================== 1. device against the restatement
@pytest.mark.parametrize("case,label", RH.HARD, ids=_ids(RH.HARD))
def test_hessian_against_the_restatement(case, label):
    atoms = RH.frame(case, label)
    rH, rL, rB = RH.hessian_reference(case, label)
    H, L, B = _hess(case, label)
    if case == "bcc_w_primitive":      # H and mixed vanish by symmetry: relative to what cancels (RH.hessian_scales)
        sH, sL = RH.hessian_scales(case)
    else:
        sH, sL = float(np.abs(rH).max()), float(np.abs(rL).max())
    errs = [RH.rel(H, rH, sH)]
    if _periodic(atoms):
        errs += [RH.rel(L, rL, sL), RH.rel(B, rB)]
    print(f"{case} {label}: H, mixed, born against the restatement {errs} (bound {RTOL:.0e})")
    assert max(errs) <= RTOL, (case, label, errs)


def _check_site(got, want, scale, what):
    """tests/test_gpu_flux.py: _check, with its references passed in"""
    U, W, flux = got
    rU, rW, rJc, rJp = want
    errs = dict(U=RH.rel(U, rU), W=RH.rel(W, rW), J_conv=RH.rel(flux[0], rJc), J_pot=RH.rel(flux[1], rJp, scale))
    assert np.min(scale) > 0
    assert max(errs.values()) <= RTOL, (what, errs)
    return errs


@pytest.mark.parametrize("case,label", RH.HARD, ids=_ids(RH.HARD))
def test_site_terms_and_heat_flux_against_the_restatement(case, label):
    rU, rW, rJc, rJp, scale = RH.site_reference(case, label)
    errs = _check_site(_site(case, label), (rU, rW, rJc, rJp), scale, (case, label))
    e = RH.oracle_energy(case, label)
    U = _site(case, label)[0]
    print(f"{case} {label}: against the restatement " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items())
          + f"; sum U - E_oracle {abs(U.sum() - e):.1e}")
    assert abs(U.sum() - e) <= MC_TOL * max(1.0, abs(e))


def _oracle_energies(case):
    ob, c = RH.oracle_basis(case), RH.coefficients(case)
    return lambda frames: np.array([O.evaluate(ob, a, c, forces=False)[0] for a in frames])


@pytest.mark.parametrize("case,label", MC_HARD, ids=_ids(MC_HARD))
def test_mc_deltas_against_differences_of_oracle_energies(case, label):
    """Every ordered swap of unlike atoms and every transmutation; about 350 moves on the eight-species frame."""
    _check_deltas(_calc(case), RH.frame(case, label), _oracle_energies(case))


@functools.lru_cache(maxsize=None)
def _sym1_calc():
    b = UN.sym1_binary()           # (an object of its own: device tables hang on the basis object, and tests/_uneven.py shares its own)
    model = ls.WeightedLinearModel(b)
    coeff = UN.coefficients(b)
    coeff[:2] = [-0.3, 0.2]
    model.coefficients = coeff
    return calculator.UFCalculator(model, md_skin=0.0)


@pytest.mark.parametrize("label", ["skew_821", "skew_351", "skew_751"])
def test_mc_deltas_on_a_symmetry_1_basis_in_a_skewed_cell(label):
    """Equal neighbour species on unequal legs (tests/_uneven.py: sym1_binary): which of two Mo (or two W) neighbours takes leg l is
    decided by their order in the table, the reference supercell's -- b slowest, a middle, c fastest, each axis 0, +1, -1, ... --
    and the skewed cells have another image count on every axis ([8, 2, 1], [3, 5, 1], [7, 5, 1]).  On the notebook bases above no
    number depends on that order."""
    calc = _sym1_calc()
    ob, coeff = O.OracleBasis(calc.bspline_config), np.asarray(calc.model.coefficients, dtype=float)
    _check_deltas(calc, RH.frame("bcc_mow", label), lambda frames: np.array([O.evaluate(ob, a, coeff, forces=False)[0] for a in frames]))


MC_TEMPERATURE, MC_SEED, MC_TRIALS = 3000.0, 11, 300


@functools.lru_cache(maxsize=None)
def _chain_reference(mode):
    """_mc_ref.Chains on quinary / skew_351 driven by the oracle's energies, run once"""
    case, label = "quinary", "skew_351"
    atoms = RH.frame(case, label)
    els = list(RH.basis(case).element_list)
    zs = np.array([atomic_numbers[e] for e in els])
    assert list(zs) == sorted(zs)
    mu = None if mode == "swap" else {e: 0.02 * k for k, e in enumerate(els)}
    energies = _oracle_energies(case)
    with_z = lambda z: Atoms(numbers=z, positions=atoms.get_positions(), cell=atoms.get_cell(), pbc=atoms.get_pbc())  # noqa: E731
    ref = R.Chains(lambda spec: energies([with_z(zs[s]) for s in spec]), [np.searchsorted(zs, atoms.get_atomic_numbers())],
                   [MC_TEMPERATURE], R.SWAP if mode == "swap" else R.TRANSMUTE, MC_SEED, len(els),
                   mu=None if mu is None else [mu[e] for e in els])
    ref.run(MC_TRIALS)
    return ref, zs, mu


@pytest.mark.parametrize("mode", ["swap", "transmute"])
def test_mc_chain_on_the_skewed_five_species_cell(mode):
    """300 trials against _mc_ref.Chains with the oracle's energies: the same species, counters and, within 1e-9 max(1, |E|),
    running energy (tests/test_gpu_uneven_legs.py::test_mc_chain_follows_the_restatement_driven_by_oracle_energies)."""
    ref, zs, mu = _chain_reference(mode)
    n_live = sum(1 for d in ref.decisions if not d[2])
    worst = min(ref.margins)
    print(f"quinary skew_351 {mode}: {n_live} non-null trials of {MC_TRIALS}, {int(ref.accepted.sum())} accepted, smallest "
          f"|exp(-dE'/kT) - u| = {worst:.3e}")
    # properties of the input: no decision hangs on the last digits, and the chain does move
    assert worst >= 1e-6 and n_live > 60 and ref.accepted.sum() > 10
    extra = dict(chemical_potentials=mu) if mode == "transmute" else {}
    with mc.MonteCarlo(_calc("quinary"), [RH.frame("quinary", "skew_351")], [MC_TEMPERATURE], mode=mode, seed=MC_SEED, **extra) as chain:
        out = chain.run(MC_TRIALS)
        got_z = chain.numbers
    assert np.array_equal(got_z, zs[ref.species[0]])
    assert np.array_equal(out["accepted"], ref.accepted) and np.array_equal(out["trials"], ref.trials)
    tol = MC_TOL * np.maximum(1.0, np.abs(ref.energy))
    print(f"running energy {out['energy']}, reference {ref.energy}, tol {tol}")
    assert np.all(np.abs(out["energy"] - ref.energy) <= tol)


def _virial_coefficients(b, seed):
    c = np.random.default_rng(seed).normal(0, 0.05, b.n_feats)
    c[b.col_idx] = 0.0
    return c


@functools.lru_cache(maxsize=None)
def _virial_rows(case, label):
    x_v = process.BasisFeaturizer(RH.basis(case)).featurize_virials([RH.frame(case, label)])[0]
    x_v.setflags(write=False)
    return x_v


@pytest.mark.parametrize("case,label", VIRIAL_HARD, ids=_ids(VIRIAL_HARD))
def test_virial_rows_through_coefficients(case, label):
    b, atoms = RH.basis(case), RH.frame(case, label)
    x_v = _virial_rows(case, label)
    assert x_v.shape == (6, b.n_feats) and np.all(np.isfinite(x_v))
    worst = 0.0
    for k in range(4):
        c = _virial_coefficients(b, 100 + k)
        v_o = O.evaluate(RH.oracle_basis(case), atoms, c, virial=True)[2]
        worst = max(worst, worst_elementwise(x_v @ c, v_o, rtol=1e-9, floor=1e-11))
    print(f"{case} {label}: F = {b.n_feats}, worst_elementwise(x_v @ c, oracle; 1e-9, 1e-11) = {worst:.2e} (bound 1)")
    assert worst <= 1.0


# ======================================================================================= 2. device against device, by mapping
MAPPED = [c for c in RH.CASES if RH.CASES[c][1]]


@pytest.mark.parametrize("case", MAPPED)
def test_site_terms_and_heat_flux_through_the_mappings(case):
    calc = _calc(case)
    U0, W0, flux0 = _site(case, ORIGINAL)
    scale0 = RH.site_reference(case, ORIGINAL)[4]
    e0 = float(calc.evaluate_frames([RH.frame(case, ORIGINAL)], forces=False)[0][0])
    assert abs(U0.sum() - e0) <= RTOL * np.abs(U0).sum()
    worst = {}
    for label in RH.labels(case)[1:]:
        d = RH.description(case, label)
        mU, mW = RH.mapped_site_terms(d, U0, W0)
        mJc, mJp, ms = RH.mapped_flux(d, flux0[0], flux0[1], scale0)
        errs = _check_site(_site(case, label), (mU, mW, mJc, mJp), ms, (case, label))
        U = _site(case, label)[0]
        errs["sum_U"] = abs(U.sum() - d.scale * e0) / np.abs(U).sum()
        assert errs["sum_U"] <= RTOL, (case, label, errs)
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"{case}: site terms and heat current through the mappings, worst " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items())
          + f" (bound {RTOL:.0e})")


@pytest.mark.parametrize("case", MAPPED)
def test_hessian_through_the_mappings(case):
    H0, L0, B0 = _hess(case, ORIGINAL)
    n0 = len(RH.frame(case, ORIGINAL))
    sH, sL = _hessian_scales(case)
    worst = {}
    for label in RH.labels(case)[1:]:
        d = RH.description(case, label)
        H, L, B = _hess(case, label)
        errs = dict(H=RH.rel(RH.folded_hessian(d, H, n0), H0, sH), rows=RH.folded_rows_agree(d, H, n0, sH))
        if L0 is not None and RH.is_identity(d.Q):
            errs.update(mixed=RH.rel(L, RH.mapped_mixed(d, L0), sL), born=RH.rel(B, d.scale * B0))
        assert max(errs.values()) <= RTOL, (case, label, errs)
        for k, v in errs.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"{case}: Hessian through the mappings, worst " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) + f" (bound {RTOL:.0e})")


def _moves(atoms, elements):
    """every ordered swap of unlike atoms (i, j) and every transmutation (i, element)"""
    z = np.asarray(atoms.get_atomic_numbers())
    swaps = [(i, j) for i in range(len(z)) for j in range(len(z)) if z[i] != z[j]]
    muts = [(i, el) for i in range(len(z)) for el in elements if atomic_numbers[el] != z[i]]
    return swaps, muts


def _deltas(calc, atoms, mode, first, second):
    kw = dict(chemical_potentials={el: 0.0 for el in calc.bspline_config.element_list}) if mode == "transmute" else {}
    with mc.MonteCarlo(calc, atoms, 300.0, mode=mode, **kw) as chain:
        return chain.delta_energy(np.zeros(len(first), dtype=int), np.asarray(first), list(second))


@pytest.mark.parametrize("case", [c for c in MAPPED if c != "bcc_w_primitive"])
def test_mc_deltas_through_the_mappings(case):
    """A description with scale 1 holds the same atoms: the delta of (i', j') is the original's of (src[i'], src[j'])."""
    calc, base = _calc(case), RH.frame(case, ORIGINAL)
    els = list(calc.bspline_config.element_list)
    e0 = float(calc.evaluate_frames([base], forces=False)[0][0])
    tol = MC_TOL * max(1.0, abs(e0))
    worst, seen = 0.0, 0
    for d in (d for d in RH.CASES[case][1] if d.scale == 1):
        swaps, muts = _moves(d.atoms, els)
        assert swaps and muts
        for mode, moves in (("swap", swaps), ("transmute", muts)):
            first = [m[0] for m in moves]
            got = _deltas(calc, d.atoms, mode, first, [m[1] for m in moves])
            second0 = [int(d.src[m[1]]) for m in moves] if mode == "swap" else [m[1] for m in moves]
            want = _deltas(calc, base, mode, [int(d.src[i]) for i in first], second0)
            assert np.abs(want).max() > 1e-3
            err = np.abs(got - want).max()
            assert err <= tol, (case, d.label, mode, moves[int(np.abs(got - want).argmax())], err)
            worst, seen = max(worst, err), seen + len(moves)
    assert seen
    print(f"{case}: {seen} Monte Carlo moves through the mappings, worst |dE' - dE| = {worst:.2e} (tol {tol:.1e})")


@pytest.mark.parametrize("case", [c for c in MAPPED if any(RH.is_identity(d.Q) for d in RH.CASES[c][1])])
def test_virial_rows_through_the_mappings(case):
    """Q = I: x_v' = scale x_v, column by column (every column to the virial-row bound on its own: none hides behind a larger one)"""
    x0 = _virial_rows(case, ORIGINAL)
    worst = 0.0
    for d in (d for d in RH.CASES[case][1] if RH.is_identity(d.Q)):
        x = _virial_rows(case, d.label)
        w = max(worst_elementwise(x[:, k], d.scale * x0[:, k], rtol=1e-9, floor=1e-11) for k in range(x0.shape[1]))
        assert w <= 1.0, (case, d.label, w)
        worst = max(worst, w)
    print(f"{case}: virial rows through the mappings, worst_elementwise by column {worst:.2e} (bound 1)")


def test_every_call_repeats_bit_for_bit_on_a_skewed_frame():
    """uf3_site_terms, uf3_heat_flux, uf3_hessian and uf3_mc_delta add in a fixed order (include/uf3_hip.h says so of each): two
    calls, the same bits.  uf3_featurize_virial adds its rows up with atomics, in whatever order the waves arrive, and promises no
    bits: two calls agree to the virial-row bound."""
    case, label = "bcc_mow", "skew_751"
    calc, atoms = _calc(case), RH.frame(case, label)
    vel, m = RH.velocities(case, label), RH.masses(atoms)
    swaps, muts = _moves(atoms, list(calc.bspline_config.element_list))

    def everything():
        U, W = calc.site_terms([atoms])
        H, L, B, _ = harmonic.hessian(calc, atoms, strain=True)
        return dict(U=U[0], W=W[0], flux=calc.heat_flux([atoms], vel, m), H=H, mixed=L, born=B,
                    swaps=_deltas(calc, atoms, "swap", [s[0] for s in swaps], [s[1] for s in swaps]),
                    transmutations=_deltas(calc, atoms, "transmute", [s[0] for s in muts], [s[1] for s in muts]))
    a, b = everything(), everything()
    differ = [k for k in a if not np.array_equal(a[k], b[k])]
    assert not differ, differ
    assert np.array_equal(a["U"], _site(case, label)[0]) and np.array_equal(a["H"], _hess(case, label)[0])
    fz = process.BasisFeaturizer(RH.basis(case))
    x1, x2 = fz.featurize_virials([atoms])[0], fz.featurize_virials([atoms])[0]
    assert max(worst_elementwise(x1[:, k], x2[:, k], rtol=1e-9, floor=1e-11) for k in range(x1.shape[1])) <= 1.0


def test_a_batch_of_a_skewed_a_slab_and_a_wire_description_gives_each_frame_what_it_gets_alone():
    picks = [("bcc_mow", "skew_821"), ("slab_mow", "skew_in_plane_531"), ("wire_mow", "perm_rotation_shift")]
    calc = _calc("bcc_mow")                                      # (Mo / W throughout: one model)
    assert all(list(RH.basis(c).element_list) == list(RH.basis("bcc_mow").element_list) for c, _ in picks)
    frames = [RH.frame(c, l) for c, l in picks]
    vel = [RH.velocities(c, l) for c, l in picks]
    m = [RH.masses(a) for a in frames]
    U, W = calc.site_terms(frames)
    flux = calc.heat_flux(frames, np.concatenate(vel), np.concatenate(m))
    assert [len(u) for u in U] == [16, 16, 36]
    for k, a in enumerate(frames):
        Ua, Wa = calc.site_terms([a])
        fa = calc.heat_flux([a], vel[k], m[k])
        assert np.array_equal(Ua[0], U[k]) and np.array_equal(Wa[0], W[k]) and np.array_equal(fa[0], flux[k]), picks[k]


# ================================================================================================ 3. positions outside the cell
# The frame: the 2 x 2 x 2 Mo/W cell, once with one atom moved by a1 - 2 a3, once with every atom moved by its own lattice vector
# (RH.unwrapped_frames).  The oracle's energy changes under the move (the reference's finite image range, taken around the
# positions as given; tests/test_redescribed_host.py).  uf3_eval and uf3_mc_* follow the reference: they are held to the oracle
# on the SAME unwrapped frame.  uf3_hessian, uf3_site_terms and uf3_heat_flux take nearest images: they do not notice the move,
# and on such a frame they describe the wrapped frame's energy, not what uf3_eval returns there.
UNWRAPPED = ["one_atom", "every_atom"]
_EVAL_ROUTES = {"md": "default", "gather": "gather", "plain": "no_md"}


def _efv(calc, atoms):
    e, f, _, v = calc.evaluate_frames([atoms], virial=True)
    return float(e[0]), f, v[0]


FD_PICKS = [(a, c) for a in (0, 3, 6, 9, 12, 15) for c in range(3)]      # tests/test_gpu_invariance.py
FD_H = (1e-4, 5e-5)                                                      # Richardson pair
FD_TOL = 1e-8                                                            # max |F - F_fd| <= FD_TOL max |F|


@functools.lru_cache(maxsize=None)
def _oracle_gradient(name):
    """Minus the gradient of the ORACLE's energy of the unwrapped frame at FD_PICKS, by Richardson differences (on the CPU, once).
    The oracle's own forces are no reference there: with atoms outside the cell the reference drops ghost-centred 3-body force
    terms, and they differ from the gradient of its energy by 1e-2 of the largest force; the kernels keep those terms (DESIGN.md
    section 7), so their forces are held to the gradient of the energy they share with the oracle."""
    atoms = RH.unwrapped_frames()[name][1]
    ob, coeff = RH.oracle_basis("bcc_mow"), RH.coefficients("bcc_mow")
    out = []
    for a, c in FD_PICKS:
        d = []
        for h in FD_H:
            es = []
            for sgn in (1, -1):
                p = np.asarray(atoms.get_positions(), float).copy()
                p[a, c] += sgn * h
                es.append(O.evaluate(ob, Atoms(numbers=atoms.get_atomic_numbers(), positions=p, cell=atoms.get_cell(), pbc=True),
                                     coeff, forces=False)[0])
            d.append(-(es[0] - es[1]) / (2 * h))
        out.append((4 * d[1] - d[0]) / 3)
    return np.array(out)


def _close_efv(got, want, what, gradient=None):
    """energy and strain derivative against the oracle's; forces against the oracle's, or with ``gradient`` against that"""
    assert abs(got[0] - want[0]) <= EVAL_TOL * abs(want[0]), (what, got[0], want[0])
    assert worst_elementwise(got[2], want[2], rtol=EVAL_TOL, floor=1e-11) <= 1.0, (what, got[2], want[2])
    if gradient is None:
        assert worst_elementwise(got[1], want[1], EVAL_TOL) <= 1.0, what
    else:
        picked = np.array([got[1][a, c] for a, c in FD_PICKS])
        assert np.abs(picked - gradient).max() <= FD_TOL * np.abs(got[1]).max(), (what, np.abs(picked - gradient).max())


@pytest.mark.parametrize("route", list(_EVAL_ROUTES))
@pytest.mark.parametrize("name", UNWRAPPED)
def test_evaluator_follows_the_reference_on_an_unwrapped_frame(name, route, dbg, monkeypatch):
    """uf3_eval on its plain, gather and MD routes: the oracle's energy and strain derivative of the unwrapped frame itself,
    which are not the wrapped frame's, and forces that are minus the gradient of that energy (_oracle_gradient)."""
    env, want = _MD_ROUTES[_EVAL_ROUTES[route]]
    inside, outside = RH.unwrapped_frames()[name]
    basis = dbg.basis(synthetic.notebook_basis(["Mo", "W"]))      # (its device tables live and die with the fixture's context)
    model = ls.WeightedLinearModel(basis)
    model.coefficients = RH.coefficients("bcc_mow").copy()
    ob, coeff = O.OracleBasis(basis), RH.coefficients("bcc_mow")
    for k in env:
        monkeypatch.delenv(k, raising=False)
    plain = calculator.UFCalculator(model, md_skin=0.0)
    for _ in range(2):                                             # (list capacities tuned: the MD route starts from a tuned context)
        for a in (inside, outside):
            plain.evaluate_frames([a], virial=True)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    dbg.launches()
    results = {}
    for key, atoms in (("inside", inside), ("outside", outside)):
        calc = calculator.UFCalculator(model, md_skin=0.5)
        first, second = _efv(calc, atoms), _efv(calc, atoms)
        said = dbg.launches()
        assert said and said[-1]["vir"] == 1, said
        for flag, val in want.items():
            assert said[-1][flag] == val, (route, name, key, said)
        ref = O.evaluate(ob, atoms, coeff, virial=True)
        for got in (first, second):
            _close_efv(got, ref, (route, name, key), _oracle_gradient(name) if key == "outside" else None)
        results[key] = second
    de = results["outside"][0] - results["inside"][0]
    print(f"{route} {name}: E inside {results['inside'][0]:.6f}, outside {results['outside'][0]:.6f}")
    assert abs(de) > 1e-3                                          # the reference's rule, not the nearest-image one


@pytest.mark.parametrize("name", UNWRAPPED)
def test_mc_table_follows_the_evaluator_on_an_unwrapped_frame(name):
    """uf3_mc_delta on the unwrapped frame: differences of evaluator energies of that frame (mc_build_table applies the
    reference's image range to the positions as given, like the walk), which the evaluator test above ties to the oracle."""
    calc = _calc("bcc_mow")
    inside, outside = RH.unwrapped_frames()[name]
    _check_deltas(calc, outside, lambda frames: calc.evaluate_frames(frames, forces=False)[0])
    _check_deltas(calc, outside, _oracle_energies("bcc_mow"))
    swaps, _ = _moves(outside, ["Mo", "W"])
    first, second = [s[0] for s in swaps], [s[1] for s in swaps]
    moved = np.abs(_deltas(calc, outside, "swap", first, second) - _deltas(calc, inside, "swap", first, second)).max()
    print(f"{name}: the largest change of a swap's dE under the move {moved:.3e}")
    assert moved > 1e-3                                            # not the wrapped frame's table


def _inside_cell(atoms):
    frac = np.asarray(atoms.get_positions(), float) @ np.linalg.inv(np.asarray(atoms.get_cell(), float))
    return bool(np.all((frac >= 0) & (frac < 1)))


@pytest.mark.parametrize("name", UNWRAPPED)
def test_hessian_and_site_terms_take_nearest_images(name):
    """Invariant under the move (1e-12 of the largest entry; tests/test_gpu_flux.py::test_lattice_shift).  On the wrapped
    frame sum U is the evaluator's energy and H the derivative of the evaluator's forces (h = 1e-5, 1e-6 of the largest entry:
    tests/test_gpu_harmonic.py::test_device_against_device_force_differences); on the unwrapped frame they still describe the
    wrapped frame, whose energy is not what uf3_eval returns there."""
    calc = _calc("bcc_mow")
    inside, outside = RH.unwrapped_frames()[name]
    vel, m = RH.velocities("bcc_mow", ORIGINAL), RH.masses(inside)
    scale = RH.site_reference("bcc_mow", ORIGINAL)[4]
    U, W, flux = _site("bcc_mow", ORIGINAL)
    H, L, B = _hess("bcc_mow", ORIGINAL)
    Uo, Wo = calc.site_terms([outside])
    fo = calc.heat_flux([outside], vel, m)[0]
    Ho, Lo, Bo, _ = harmonic.hessian(calc, outside, strain=True)
    errs = dict(U=RH.rel(Uo[0], U), W=RH.rel(Wo[0], W), J_conv=RH.rel(fo[0], flux[0]), J_pot=RH.rel(fo[1], flux[1], scale),
                H=RH.rel(Ho, H), mixed=RH.rel(Lo, L), born=RH.rel(Bo, B))
    print(f"{name}: under the move " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12, errs
    e_in, e_out = (float(calc.evaluate_frames([a], forces=False)[0][0]) for a in (inside, outside))
    assert abs(U.sum() - e_in) <= 1e-12 * np.abs(U).sum()
    assert abs(Uo[0].sum() - e_out) > 1e-3                         # sum U is the WRAPPED frame's energy
    pos, n, h = np.asarray(inside.get_positions(), float), len(inside), 1e-5
    frames = []
    for k in range(3 * n):
        for sgn in (1, -1):
            p = pos.copy()
            p[k // 3, k % 3] += sgn * h
            frames.append(Atoms(numbers=inside.get_atomic_numbers(), positions=p, cell=inside.get_cell(), pbc=True))
    assert all(_inside_cell(a) for a in frames)
    f = calc.evaluate_frames(frames)[1].reshape(3 * n, 2, 3 * n)
    Hfd = -(f[:, 0] - f[:, 1]).T / (2 * h)
    err = np.abs(H - Hfd).max() / np.abs(H).max()
    print(f"{name}: H of the wrapped frame against differences of evaluator forces {err:.2e} (bound 1e-6)")
    assert err <= 1e-6


@pytest.mark.parametrize("name", UNWRAPPED)
def test_md_driver_evaluates_the_positions_it_holds(name):
    """MolecularDynamics (NVE, 20 steps, thermo_every = 1) from the wrapped and from the moved frame.  The driver keeps positions
    unwrapped and hands them to the evaluator as they are, so it follows the reference's rule: the step-0 energy and forces of
    each start are uf3_eval's ON THAT FRAME, the energy the oracle's -- those of the moved start lack the interactions the finite
    image range no longer reaches -- and so are the energy and forces at the positions the run ends on.  The two trajectories therefore differ from
    the first step on (deviations: atoms that leave the window around their cell; wrap before a driver starts)."""
    inside, outside = RH.unwrapped_frames()[name]
    calc = _calc("bcc_mow")
    ob, coeff = RH.oracle_basis("bcc_mow"), RH.coefficients("bcc_mow")
    m = {"Mo": RH.MASS[42], "W": RH.MASS[74]}
    vel = RH.velocities("bcc_mow", ORIGINAL)
    records, step0 = {}, {}
    for key, atoms in (("inside", inside), ("outside", outside)):
        with MolecularDynamics(calc, [atoms], 1.0, masses=m) as dyn:
            dyn.set_velocities(vel)
            e, f = float(dyn.get_potential_energies()[0]), dyn.get_forces()
            e_o = O.evaluate(ob, atoms, coeff, forces=False)[0]
            assert abs(e - e_o) <= EVAL_TOL * abs(e_o), (name, key, e, e_o)
            assert worst_elementwise(f, calc.evaluate_frames([atoms])[1], EVAL_TOL) <= 1.0, (name, key)
            step0[key] = (e, f)
            records[key] = dyn.run(20, thermo_every=1)
            end = dyn.get_atoms()[0]
            e1, f1 = float(dyn.get_potential_energies()[0]), dyn.get_forces()
        assert records[key]["potential_energy"].shape[0] == 20
        e_o = O.evaluate(ob, end, coeff, forces=False)[0]
        assert abs(e1 - e_o) <= EVAL_TOL * abs(e_o), (name, key, "after 20 steps", e1, e_o)
        assert worst_elementwise(f1, calc.evaluate_frames([end])[1], EVAL_TOL) <= 1.0, (name, key, "after 20 steps")
    de = step0["outside"][0] - step0["inside"][0]
    df = np.abs(step0["outside"][1] - step0["inside"][1]).max()
    dr = np.abs(records["outside"]["potential_energy"] - records["inside"]["potential_energy"]).max()
    print(f"{name}: step 0 of the moved start against the wrapped one: dE = {de:.4f} eV, max |dF| = {df:.3e} eV/A; the 20 thermo "
          f"records differ by up to {dr:.3e} eV")
    assert abs(de) > 1e-3 and df > 1e-3
