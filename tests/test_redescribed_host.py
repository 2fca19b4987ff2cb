"""Re-described frames for the Hessian, the site terms, the heat current and the Monte Carlo table, and the references alone on
them (no GPU): the NumPy restatements (_flux_ref, _harmonic_ref) and the oracle obey every mapping that
tests/test_gpu_redescribed.py then asserts of the device -- a description's results are the original's, mapped through its
``src``, ``scale`` and ``Q`` (tests/_util.py: Description) -- on every description of at most 64 atoms.  This pins the frames,
the models and the mappings without a GPU; the device module imports them from here.

Measured on the CPU (max-norm relative to the original's largest entry): site energies 1.3e-14, site virials 4.8e-14, J_conv
5.0e-15, J_pot (relative to the sum of its terms' absolute values) 1.3e-15, Hessian 7.3e-14, sum U - E_oracle 1.2e-13 (the 64-atom
supercell, against the original's largest site energy).  Asserted:
1e-12 (TOL_HOST)."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.regression import least_squares as ls
import _flux_ref as FR
import _harmonic_ref as HR
from _util import basis_from_meta, equivalence_cases, load_case

TOL_HOST = 1e-12
MAX_RESTATED = 64                  # atoms: the restatements walk an explicit supercell term by term
S8 = "case_bcc16_s8"               # eight species, 16 atoms, its own basis
MASS = {1: 1.008, 6: 12.011, 24: 51.996, 28: 58.693, 40: 91.224, 41: 92.906, 42: 95.95, 73: 180.948, 74: 183.84, 78: 195.084,
        92: 238.029}
ORIGINAL = "original"

_EQ = equivalence_cases()
# case -> (the original frame, [Description]); the eight-species capture stands alone
CASES = {name: (base, descs) for name, (_, base, descs) in _EQ.items()}
CASES[S8] = (load_case(S8)[2], [])
# the descriptions held to the restatements directly (and, through the mappings, every other one)
HARD = [("bcc_mow", "skew_821"), ("bcc_mow", "skew_351"), ("bcc_mow", "skew_751"), ("bcc_mow", "skew_751_reflection"),
        ("bcc_mow", "perm_rotation_shift"), ("bcc_w_primitive", ORIGINAL), ("bcc_w_primitive", "skew_rotation"),
        ("slab_mow", "skew_in_plane_531"), ("wire_mow", ORIGINAL), ("wire_mow", "perm_rotation_shift"), ("ternary", "skew_751"),
        ("quinary", "skew_351"), (S8, ORIGINAL)]


def description(case, label):
    """The Description of that name, None for the original."""
    if label == ORIGINAL:
        return None
    return next(d for d in CASES[case][1] if d.label == label)


def frame(case, label):
    return CASES[case][0] if label == ORIGINAL else description(case, label).atoms


def labels(case, cap=None):
    """The original's and every description's label, those of more than ``cap`` atoms left out."""
    return [ORIGINAL] + [d.label for d in CASES[case][1] if cap is None or len(d.atoms) <= cap]


@functools.lru_cache(maxsize=None)
def basis(case):
    if case == S8:
        return basis_from_meta(load_case(S8)[1])
    return synthetic.notebook_basis(list(_EQ[case][0]))


@functools.lru_cache(maxsize=None)
def model(case):
    """Seeded coefficients, normal(0, 0.05), frozen columns zero, unlike one-body terms (tests/test_gpu_mc.py: _mow)."""
    b = basis(case)
    m = ls.WeightedLinearModel(b)
    coeff = np.random.default_rng(31).normal(0, 0.05, b.n_feats)
    coeff[b.col_idx] = 0.0
    n_el = len(b.element_list)
    coeff[:n_el] = np.linspace(-0.3, 0.2, n_el) if n_el > 1 else [-0.3]
    m.coefficients = coeff
    return m


@functools.lru_cache(maxsize=None)
def oracle_basis(case):
    return O.OracleBasis(basis(case))


def coefficients(case):
    return np.asarray(model(case).coefficients, dtype=float)


def masses(atoms):
    return np.array([MASS[int(q)] for q in atoms.get_atomic_numbers()])


@functools.lru_cache(maxsize=None)
def _velocities0(case):
    n = len(CASES[case][0])
    v = np.random.default_rng(sum(map(ord, case))).normal(0, 0.01, (n, 3))
    v.setflags(write=False)
    return v


def velocities(case, label):
    """Seeded velocities of the original, carried to the description: v'[k] = Q v[src[k]]."""
    d = description(case, label)
    return _velocities0(case) if d is None else _velocities0(case)[d.src] @ d.Q.T


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def site_reference(case, label):
    """U, W, J_conv, J_pot and the scale of J_pot (the sum of its terms' absolute values) of one description: the restatement,
    computed once, shared, never changed."""
    atoms = frame(case, label)
    assert len(atoms) <= MAX_RESTATED
    ob, c = oracle_basis(case), coefficients(case)
    U, W = FR.site_terms(ob, atoms, c)
    Jc, Jp, scale = FR.heat_flux(ob, atoms, velocities(case, label), masses(atoms), c, with_scale=True)
    return _frozen(U, W, Jc, Jp, scale)


@functools.lru_cache(maxsize=None)
def hessian_reference(case, label):
    """H, mixed, born of one description: the restatement, computed once."""
    atoms = frame(case, label)
    assert len(atoms) <= MAX_RESTATED
    return _frozen(*HR.hessian(oracle_basis(case), atoms, coefficients(case)))


@functools.lru_cache(maxsize=None)
def oracle_energy(case, label):
    return float(O.evaluate(oracle_basis(case), frame(case, label), coefficients(case), forces=False)[0])


# ---- the mappings: what a description's results must be, given the original's -----------------------------------------------
def rel(got, want, scale=None):
    """max |got - want| relative to the largest |want| (or to ``scale``, entry by entry)"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    return float((np.abs(got - want) / (np.abs(want).max() if scale is None else scale)).max())


@functools.lru_cache(maxsize=None)
def hessian_scales(case):
    """What deviations of H and of the mixed derivative are relative to: the largest |entry| of the original's restatement.  On
    the 1-atom primitive cell both vanish by symmetry in every 1-atom description -- sums of blocks that cancel, rounding noise
    in the restatement and on the device alike -- so there the size of what cancels stands in: the largest entry of H of the
    2-atom conventional cell, where the same force constants are not all folded onto one atom, and for the mixed derivative
    that times (volume per atom)^(1/3), a term of it being a term of H times a length of that order."""
    H0, L0, _ = hessian_reference(case, ORIGINAL)
    if case != "bcc_w_primitive":
        return float(np.abs(H0).max()), float(np.abs(L0).max())
    h = float(np.abs(hessian_reference(case, "conventional")[0]).max())
    a = frame(case, ORIGINAL)
    assert np.abs(H0).max() <= 1e-12 * h
    return h, h * float(abs(np.linalg.det(np.asarray(a.get_cell(), float))) / len(a)) ** (1.0 / 3.0)


def mapped_site_terms(d, U, W):
    """U'[k] = U[src[k]], W'[k] = Q W[src[k]] Q^T"""
    return np.asarray(U)[d.src], np.einsum("ab,kbc,dc->kad", d.Q, np.asarray(W)[d.src], d.Q)


def mapped_flux(d, Jc, Jp, scale):
    """J' = scale Q J; the scale J_pot's rounding is relative to turns with it: a component of Q J is a sum over the components
    of J with the weights |Q|, so its terms' absolute values add up to at most |Q| @ scale (exactly ``scale`` when Q = I)."""
    return d.scale * d.Q @ Jc, d.scale * d.Q @ Jp, d.scale * np.abs(d.Q) @ scale


def folded_hessian(d, H, n0):
    """The original's H from a description's: H0[i, j] = sum over k with src[k] = j of Q^T H'[k_i, k] Q, k_i the first atom with
    src[k_i] = i (every other choice of k_i gives the same rows: ``folded_rows_agree``)."""
    n = len(d.src)
    blocks = np.asarray(H).reshape(n, 3, n, 3).transpose(0, 2, 1, 3)            # [k, k', 3, 3]
    first = np.array([int(np.flatnonzero(d.src == i)[0]) for i in range(n0)])
    rows = np.einsum("ba,ikbc,cd->ikad", d.Q, blocks[first], d.Q)               # Q^T . Q
    out = np.zeros((n0, n0, 3, 3))
    np.add.at(out, (slice(None), d.src), rows)
    return out.transpose(0, 2, 1, 3).reshape(3 * n0, 3 * n0)


def folded_rows_agree(d, H, n0, scale):
    """max over the images k_i of every original atom of the deviation of their folded rows from the first image's, relative to
    ``scale``"""
    n = len(d.src)
    blocks = np.asarray(H).reshape(n, 3, n, 3).transpose(0, 2, 1, 3)
    folded = np.zeros((n, n0, 3, 3))
    np.add.at(folded, (slice(None), d.src), blocks)
    worst = 0.0
    for i in range(n0):
        ks = np.flatnonzero(d.src == i)
        worst = max(worst, float(np.abs(folded[ks] - folded[ks[0]]).max()))
    return worst / scale


def mapped_mixed(d, L):
    """Q = I: mixed'[k] = mixed0[src[k]]"""
    return np.asarray(L).reshape(-1, 3, 6)[d.src].reshape(-1, 6)


def is_identity(Q):
    return np.array_equal(np.asarray(Q), np.eye(3))


# ---- the references obey the mappings ----------------------------------------------------------------------------------------
def test_the_fixtures_are_what_the_device_module_expects():
    for case, label in HARD:
        assert len(frame(case, label)) <= MAX_RESTATED, (case, label)
    assert len(set(frame(S8, ORIGINAL).get_atomic_numbers().tolist())) == 8 and len(frame(S8, ORIGINAL)) == 16
    assert len(set(frame("quinary", "skew_351").get_atomic_numbers().tolist())) == 5
    sizes = {d.label: len(d.atoms) for c in CASES for d in CASES[c][1]}
    assert sizes["supercell_333"] == 432 and sizes["supercell_222_skew_821"] == 128 and sizes["supercell_666"] == 216
    for case in CASES:
        m = masses(CASES[case][0])
        assert len(set(m.tolist())) == len(set(CASES[case][0].get_atomic_numbers().tolist()))      # unequal masses
        c = coefficients(case)
        n_el = len(basis(case).element_list)
        assert len(set(c[:n_el].tolist())) == n_el                                                 # unlike one-body terms


@pytest.mark.parametrize("case", list(CASES))
def test_site_terms_and_flux_of_the_restatement_obey_the_mappings(case):
    U0, W0, Jc0, Jp0, s0 = site_reference(case, ORIGINAL)
    e0 = oracle_energy(case, ORIGINAL)
    worst = dict(U=0.0, W=0.0, J_conv=0.0, J_pot=0.0, sum_U=abs(U0.sum() - e0) / np.abs(U0).max())
    for label in labels(case, MAX_RESTATED)[1:]:
        d = description(case, label)
        U, W, Jc, Jp, _ = site_reference(case, label)
        mU, mW = mapped_site_terms(d, U0, W0)
        mJc, mJp, ms = mapped_flux(d, Jc0, Jp0, s0)
        got = dict(U=rel(U, mU), W=rel(W, mW), J_conv=rel(Jc, mJc), J_pot=rel(Jp, mJp, ms),
                   sum_U=abs(U.sum() - oracle_energy(case, label)) / np.abs(U0).max())
        assert abs(oracle_energy(case, label) - d.scale * e0) <= TOL_HOST * d.scale * np.abs(U0).max(), (case, label)
        for k, v in got.items():
            assert v <= TOL_HOST, (case, label, k, v)
            worst[k] = max(worst[k], v)
    assert worst["sum_U"] <= TOL_HOST, (case, worst)
    print(f"{case}: restatement through the mappings, worst " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("case", list(CASES))
def test_hessian_of_the_restatement_obeys_the_mappings(case):
    H0, L0, B0 = hessian_reference(case, ORIGINAL)
    n0 = len(CASES[case][0])
    sH, sL = hessian_scales(case)
    worst = 0.0
    for label in labels(case, MAX_RESTATED)[1:]:
        d = description(case, label)
        H, L, B = hessian_reference(case, label)
        errs = [rel(folded_hessian(d, H, n0), H0, sH), folded_rows_agree(d, H, n0, sH)]
        if is_identity(d.Q):
            errs += [rel(mapped_mixed(d, L0), L, sL), rel(d.scale * B0, B)]
        assert max(errs) <= TOL_HOST, (case, label, errs)
        worst = max(worst, max(errs))
    print(f"{case}: Hessian restatement through the mappings, worst {worst:.1e}")


# ---- positions outside the cell: what the references do -----------------------------------------------------------------------
def unwrapped_frames():
    """The 2 x 2 x 2 Mo/W cell with (a) one atom moved by a1 - 2 a3 and (b) every atom moved by its own integers(-2, 3) lattice
    vector: name -> (wrapped frame, the same crystal with atoms outside the cell)."""
    base = CASES["bcc_mow"][0]
    cell, pos = np.asarray(base.get_cell(), float), np.asarray(base.get_positions(), float)
    one = pos.copy()
    one[5] += cell[0] - 2 * cell[2]
    shift = np.random.default_rng(41).integers(-2, 3, (len(pos), 3))
    make = lambda p: Atoms(numbers=base.get_atomic_numbers(), positions=p, cell=cell, pbc=True)      # noqa: E731
    return {"one_atom": (base, make(one)), "every_atom": (base, make(pos + shift @ cell))}


@pytest.mark.parametrize("name", ["one_atom", "every_atom"])
def test_the_reference_loses_terms_of_an_atom_outside_its_cell_and_the_restatement_is_no_reference_there(name):
    """The oracle's finite image range is taken around the positions as given: its energy of the moved frame is not the wrapped
    frame's.  _flux_ref walks the oracle's supercell of twice the reach, which covers a wrapped frame's terms only: its site
    energies change under the move too, so it is no reference on an unwrapped frame."""
    inside, outside = unwrapped_frames()[name]
    ob, c = oracle_basis("bcc_mow"), coefficients("bcc_mow")
    e_in, e_out = (O.evaluate(ob, a, c, forces=False)[0] for a in (inside, outside))
    assert abs(e_in - oracle_energy("bcc_mow", ORIGINAL)) == 0.0
    assert abs(e_out - e_in) > 1e-3, (e_in, e_out)
    U_out = FR.site_terms(ob, outside, c)[0]
    assert np.abs(U_out - site_reference("bcc_mow", ORIGINAL)[0]).max() > 1e-3
