"""Site rows, grades and leverages on re-described frames, the references alone (no GPU): the host rows of tests/_site_rows_ref.py,
the oracle's energy and force rows and ``ls.leverage_reference`` obey every mapping that tests/test_gpu_site_redescribed.py then
asserts of the device -- a description's rows, grades and per-atom force leverages are the original's through its ``src``, its
energy leverage the original's times ``scale**2`` (tests/_util.py: Description).  This pins the frames, the bases, the posteriors
and the cached host rows without a GPU; the device module imports them from here.

Measured on the CPU, asserted at 1e-12 (RH.TOL_HOST):
- host rows of the pinned descriptions (ROWS_HARD) against _flux_ref's U through RH.coefficients 1.7e-15 of max |U|, their
  live-column sums against the oracle's energy row 1.3e-15 of max |x_e|, against the original's rows through ``src`` 2.4e-14 of
  max |B0|;
- symmetry-1 bases (SYM1): a description's rows differ from the mapped original's by 2.5e-2 to 1.8e-1 (7 and 24 entries on the
  one-species basis, 441 to 493 on the two-species one; floor asserted: SYM1_FLOOR = 1e-2), their live-column sums equal the
  oracle's energy row within 4.2e-16.  (On these bases the energy row itself is another one in another description -- the
  energy depends on which image holds an atom, tests/_uneven.py -- so nothing is compared across descriptions but the rows.)
- leverages and grades of the references through the mappings, every description of at most 64 atoms, per case (relative to the
  original's largest; HOST_SPREAD holds each figure with a factor of two or more for another BLAS, and the test holds the
  measurement under it; leverage_bound / grade is 9.7e-13 on the Mo/W bases and 3.2e-12 on the ternary one):
      case       energy x scale^2   force through src   grade through src
      bcc_mow        1.3e-15            2.7e-14             7.4e-15
      slab_mow       8.9e-16            9.7e-15             3.0e-15
      wire_mow       4.8e-16            2.7e-15             1.4e-15
      ternary        2.7e-16            9.4e-15             5.7e-15
- argmax room (the two largest distinct grades, relative to the largest; the same in every pinned description): bcc_mow 4.1e-2,
  slab_mow 8.9e-2, wire_mow 7.4e-2, ternary 1.8e-1, bcc_mow on sym1_binary 1.3e-1; bcc_w_primitive has one atom and no second
  grade: no argmax is asserted there (ARGMAX_CASES leaves it out by name).
- grade samples of the oracle-driven MD restatement (_md_ref with the oracle's forces, NVE, 40 steps of 1 fs from RH.velocities,
  a sample every 5) on bcc_mow original against skew_751_reflection, through ``src``, relative to the sample's largest grade:
  5.8e-15, 6.2e-15, 8.1e-15, 4.7e-15, 6.8e-15, 6.6e-15, 6.3e-15 and, at step 40, 1.6e-10.  These velocities (0.01 A/fs a
  component) carry atoms out of the window of DESIGN.md section 7, by 0.37 A in the cubic cell and by 0.02 A in the skewed one,
  where the reference's finite image range drops terms near the cut-off: the two oracle-driven trajectories themselves are
  4.1e-10 A apart at step 40.  The evaluator follows the reference there, so the device module takes this spread, sample by
  sample (MD_HOST_SPREAD, with a factor of two), as "the references' spread" of its side-by-side comparison.  The largest grade
  sits on atom 13 in every sample with 4.1e-2 to 2.9e-1 of room."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd.regression import least_squares as ls
import _flux_ref as FR
import _site_rows_ref as SR
import _uneven as UN
import test_redescribed_host as RH

ORIGINAL = RH.ORIGINAL
TOL_HOST = RH.TOL_HOST
MAX_ROWS_FEATS = 1326                 # a dense host B beyond this is not feasible (F calls of split_coefficients, a len(c3) x F matrix)
# the descriptions whose host rows are pinned: every RH.HARD one with a notebook basis of at most MAX_ROWS_FEATS columns
ROWS_HARD = [(c, l) for c, l in RH.HARD if c != RH.S8 and RH.basis(c).n_feats <= MAX_ROWS_FEATS]
ROWS_CASES = list(dict.fromkeys(c for c, _ in ROWS_HARD))
# symmetry-1 bases (tests/_uneven.py) on the frames of a case: basis name -> (case, labels)
SYM1 = {"sym1_unary": ("bcc_w_primitive", [ORIGINAL, "conventional", "skew_rotation"]),
        "sym1_binary": ("bcc_mow", [ORIGINAL, "skew_821", "skew_351", "skew_751", "perm_rotation_shift"])}
SYM1_FLOOR = 1e-2                     # max |B' - B0[src]| of every listed description: the tie-break decides columns there
# cases whose leverages the device module compares across descriptions, and what the references alone spread by (docstring)
LEVERAGE_CASES = ["bcc_mow", "slab_mow", "wire_mow", "ternary"]
HOST_SPREAD = {"bcc_mow": dict(energy=3e-15, force=6e-14, grade=2e-14), "slab_mow": dict(energy=2e-15, force=2e-14, grade=6e-15),
               "wire_mow": dict(energy=1e-15, force=6e-15, grade=3e-15), "ternary": dict(energy=1e-15, force=2e-14, grade=2e-14)}
ARGMAX_ROOM = 1e-6
# cases whose frame_argmax the device module asserts through ``src`` (bcc_w_primitive: one atom, every description holds copies
# of it alone, no second grade)
ARGMAX_CASES = ["bcc_mow", "slab_mow", "wire_mow", "ternary"]


# the MD runs of the device module (tests/test_gpu_site_redescribed.py, part 8), restated with the oracle's forces
MD_PAIR = ("bcc_mow", "skew_751_reflection")
MD_STEPS, MD_EVERY, MD_DT = 40, 5, 1.0
MD_MASS = {"Mo": RH.MASS[42], "W": RH.MASS[74]}
MD_HOST_SPREAD = [2e-14] * 7 + [4e-10]     # per sample, relative to the sample's largest grade (docstring)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def host_rows(case, label):
    """Host B [N, F] of one description on its case's notebook basis: computed once, shared, never changed."""
    atoms = RH.frame(case, label)
    assert len(atoms) <= RH.MAX_RESTATED
    return _frozen(SR.site_rows(RH.oracle_basis(case), atoms, RH.basis(case).n_feats))


@functools.lru_cache(maxsize=None)
def sym1_basis(name):
    """One object per name, this module family's own (device tables hang on a basis object)."""
    return {"sym1_unary": UN.sym1_unary, "sym1_binary": UN.sym1_binary}[name]()


@functools.lru_cache(maxsize=None)
def sym1_oracle_basis(name):
    return O.OracleBasis(sym1_basis(name))


@functools.lru_cache(maxsize=None)
def sym1_rows(name, label):
    """Host B of one description of SYM1[name]'s case on the symmetry-1 basis ``name``."""
    return _frozen(SR.site_rows(sym1_oracle_basis(name), RH.frame(SYM1[name][0], label), sym1_basis(name).n_feats))


@functools.lru_cache(maxsize=None)
def posterior(case):
    """A seeded posterior on the case's notebook basis (tests/_site_rows_ref.py: seeded_model) with RH.model's coefficients."""
    model = SR.seeded_model(RH.basis(case))
    model.coefficients = RH.coefficients(case).copy()
    return model


@functools.lru_cache(maxsize=None)
def sym1_posterior(name):
    b = sym1_basis(name)
    model = SR.seeded_model(b)
    coeff = UN.coefficients(b)
    coeff[:len(b.element_list)] = [-0.3, 0.2][:len(b.element_list)]
    model.coefficients = coeff
    return model


@functools.lru_cache(maxsize=None)
def whitening(case):
    """(a copy: the model's own array stays writable for the device layers that wrap it)"""
    return _frozen(posterior(case).whitening().copy())


@functools.lru_cache(maxsize=None)
def sym1_whitening(name):
    return _frozen(sym1_posterior(name).whitening().copy())


def live_columns(basis):
    return np.setdiff1d(np.arange(basis.n_feats), np.asarray(basis.col_idx, dtype=int))


def energy_row(ob, atoms):
    return np.asarray(O.featurize(ob, atoms, forces=False)["xe"], dtype=float)


def room(grades, src=None):
    """(largest - second largest distinct) / largest of a frame's grades; with ``src`` the copies of one original atom count as
    one (their largest).  inf for a frame with a single distinct atom."""
    g = np.asarray(grades, float)
    if src is not None:
        merged = np.full(int(np.max(src)) + 1, -np.inf)
        np.maximum.at(merged, np.asarray(src), g)
        g = merged
    if len(g) < 2:
        return np.inf
    top = np.sort(g)[-2:]
    return float((top[1] - top[0]) / top[1])


# ---- 1. host rows of the pinned descriptions ----------------------------------------------------------------------------------
def test_the_pinned_descriptions_are_what_the_device_module_expects():
    assert ("quinary", "skew_351") not in ROWS_HARD and (RH.S8, ORIGINAL) not in ROWS_HARD
    assert RH.basis("quinary").n_feats == 5675 and RH.basis(RH.S8).n_feats == 8164
    assert {c: RH.basis(c).n_feats for c in ROWS_CASES} == {"bcc_mow": 434, "bcc_w_primitive": RH.basis("bcc_w_primitive").n_feats,
                                                            "slab_mow": 434, "wire_mow": 434, "ternary": 1326}
    assert len(ROWS_HARD) == 11
    assert sym1_basis("sym1_binary").n_feats == 983 and set(sym1_basis("sym1_unary").symmetry.values()) == {1}
    assert 1 in set(sym1_basis("sym1_binary").symmetry.values())
    for name, (case, labs) in SYM1.items():
        assert list(sym1_basis(name).element_list) == list(RH.basis(case).element_list)
        assert all(l == ORIGINAL or RH.description(case, l) is not None for l in labs)


@pytest.mark.parametrize("case,label", ROWS_HARD, ids=[f"{c}-{l}" for c, l in ROWS_HARD])
def test_host_rows_against_site_energies_the_energy_row_and_the_original(case, label):
    atoms, basis, ob = RH.frame(case, label), RH.basis(case), RH.oracle_basis(case)
    B = host_rows(case, label)
    assert B.shape == (len(atoms), basis.n_feats) and not B.flags.writeable
    U = RH.site_reference(case, label)[0]
    err_u = RH.rel(B @ RH.coefficients(case), U)
    x_e, live = energy_row(ob, atoms), live_columns(basis)
    err_e = float(np.abs(B.sum(0) - x_e)[live].max() / np.abs(x_e).max())
    B0 = host_rows(case, ORIGINAL)
    d = RH.description(case, label)
    err_0 = 0.0 if d is None else float(np.abs(B - B0[d.src]).max() / np.abs(B0).max())
    print(f"{case} {label}: host rows, B @ c against U {err_u:.1e}, live-column sums against x_e {err_e:.1e}, against the "
          f"original's rows through src {err_0:.1e}")
    assert max(err_u, err_e, err_0) <= TOL_HOST, (case, label, err_u, err_e, err_0)


# ---- 2. symmetry-1 bases: the tie-break decides columns, and the sum does not see it --------------------------------------------
@pytest.mark.parametrize("name", list(SYM1))
def test_symmetry_1_rows_move_between_descriptions_and_their_sums_do_not(name):
    case, labs = SYM1[name]
    basis, ob = sym1_basis(name), sym1_oracle_basis(name)
    live = live_columns(basis)
    B0 = sym1_rows(name, ORIGINAL)
    for label in labs:
        atoms = RH.frame(case, label)
        B = sym1_rows(name, label)
        x_e = energy_row(ob, atoms)
        err_e = float(np.abs(B.sum(0) - x_e)[live].max() / np.abs(x_e).max())
        assert err_e <= TOL_HOST, (name, label, err_e)
        c = UN.coefficients(basis)
        U = FR.site_terms(ob, atoms, c)[0]
        assert RH.rel(B @ c, U) <= TOL_HOST, (name, label)
        if label == ORIGINAL:
            continue
        d = RH.description(case, label)
        moved = np.abs(B - B0[d.src])
        print(f"{name} on {case} {label}: max |B' - B0[src]| = {moved.max():.2e} in {int((moved > 1e-6).sum())} entries; "
              f"live-column sums against x_e {err_e:.1e}")
        assert moved.max() >= SYM1_FLOOR, (name, label, moved.max())


# ---- 3. leverages and grades of the references through the mappings --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_leverages(case, label):
    """(energy leverage of the oracle's raw energy row, per-atom force leverage of its force rows)"""
    out = O.featurize(RH.oracle_basis(case), RH.frame(case, label))
    w = whitening(case)
    return (float(ls.leverage_reference(out["xe"][None, :], w, 1)[0]),
            _frozen(ls.leverage_reference(out["xf"].reshape(-1, out["xf"].shape[-1]), w, 3)))


@pytest.mark.parametrize("case", LEVERAGE_CASES)
def test_reference_leverages_and_grades_obey_the_mappings(case):
    w = whitening(case)
    qe0, qf0 = _oracle_leverages(case, ORIGINAL)
    g0 = ls.leverage_reference(host_rows(case, ORIGINAL), w, 1)
    worst = dict(energy=0.0, force=0.0, grade=0.0)
    for label in RH.labels(case, RH.MAX_RESTATED)[1:]:
        d = RH.description(case, label)
        assert not d.reference_drops_terms
        qe, qf = _oracle_leverages(case, label)
        worst["energy"] = max(worst["energy"], abs(qe - d.scale ** 2 * qe0) / (d.scale ** 2 * qe0))
        worst["force"] = max(worst["force"], RH.rel(qf, qf0[d.src]))
        if (case, label) in ROWS_HARD:
            worst["grade"] = max(worst["grade"], RH.rel(ls.leverage_reference(host_rows(case, label), w, 1), g0[d.src]))
    bound = ls.leverage_bound(host_rows(case, ORIGINAL), w, 1)
    print(f"{case}: references through the mappings, spread " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items())
          + f"; leverage_bound / grade {float(np.median(bound / g0)):.1e}")
    for k, v in worst.items():
        assert v <= HOST_SPREAD[case][k] <= TOL_HOST, (case, k, v)


# ---- 4. argmax room ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ARGMAX_CASES)
def test_the_largest_grade_of_every_asserted_frame_has_room(case):
    w = whitening(case)
    got = {}
    for c, label in [(case, ORIGINAL)] + [p for p in ROWS_HARD if p[0] == case and p[1] != ORIGINAL]:
        d = RH.description(c, label)
        got[label] = room(ls.leverage_reference(host_rows(c, label), w, 1), None if d is None else d.src)
    print(f"{case}: argmax room " + ", ".join(f"{k} {v:.1e}" for k, v in got.items()))
    assert min(got.values()) >= ARGMAX_ROOM, (case, got)


def test_the_one_atom_cell_has_no_second_grade_and_the_symmetry_1_frame_has_room():
    assert "bcc_w_primitive" not in ARGMAX_CASES and len(RH.frame("bcc_w_primitive", ORIGINAL)) == 1
    g = ls.leverage_reference(sym1_rows("sym1_binary", ORIGINAL), sym1_whitening("sym1_binary"), 1)
    print(f"bcc_mow on sym1_binary: argmax room {room(g):.1e}")
    assert room(g) >= ARGMAX_ROOM
    assert room([3.0, 1.0, 3.0, 2.0], [0, 1, 0, 2]) == pytest.approx(1.0 / 3.0) and room([5.0]) == np.inf


# ---- 5. grade samples along the oracle-driven MD restatement ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def md_reference(label):
    """(grades [n_samples, N] of the wrapped states, positions at the last step, the smallest room inside the image window) of
    the NVE restatement driven by the oracle on one description of MD_PAIR's case."""
    import _driver_cells as DC
    import _md_ref as MR
    from uf3_amd.data.atoms import Atoms
    from uf3_amd.forcefield import md
    from _util import wrapped
    case = MD_PAIR[0]
    assert DC.model_case(case) == case
    a = RH.frame(case, label)
    ora = DC.OracleFrames(case, [a])
    x, v = np.array(a.get_positions(), float), np.array(RH.velocities(case, label), float)
    m, w = md.resolve_masses([a], MD_MASS), whitening(case)
    grades = []
    for _ in range(MD_STEPS // MD_EVERY):
        x, v, _, _ = MR.run(x, v, m, ora.md(), MD_EVERY, MD_DT, 0.0, 0.0, 0)
        state = wrapped(Atoms(numbers=a.get_atomic_numbers(), positions=x, cell=a.get_cell(), pbc=a.get_pbc()))
        grades.append(ls.leverage_reference(SR.site_rows(RH.oracle_basis(case), state, RH.basis(case).n_feats), w, 1))
    return _frozen(np.array(grades)), _frozen(x), DC.window_room(ora.trace, [a], DC.r_cut(case))


def test_md_reference_samples_obey_the_mapping():
    import _driver_cells as DC
    case, label = MD_PAIR
    d = RH.description(case, label)
    (g0, x0, room0), (g1, x1, room1) = md_reference(ORIGINAL), md_reference(label)
    spread = [RH.rel(g1[s], g0[s][d.src]) for s in range(len(g0))]
    rooms = [room(g) for g in g0]
    apart = float(np.abs(DC.Pair(case, label, RH.frame(case, ORIGINAL), d).residual(x1, x0)).max())
    print(f"{case} {label}: oracle-driven MD, grade samples through src " + ", ".join(f"{v:.1e}" for v in spread)
          + f"; window room {room0:.3f} / {room1:.3f} A; positions {apart:.1e} A apart at the end; argmax room "
          + ", ".join(f"{v:.1e}" for v in rooms))
    assert len(spread) == len(MD_HOST_SPREAD) == MD_STEPS // MD_EVERY
    assert all(v <= b for v, b in zip(spread, MD_HOST_SPREAD)), spread
    assert min(rooms) >= ARGMAX_ROOM and all(np.argmax(g1[s]) in np.flatnonzero(d.src == np.argmax(g0[s])) for s in range(len(g0)))
    # the maxima move from sample to sample: a stop threshold between two of them separates them (part 8 d)
    top = g0.max(axis=1)
    assert any(top[s + 1] > top[:s + 1].max() * (1 + ARGMAX_ROOM) for s in range(len(top) - 1)), top
