"""
The oracle (``oracle/uf3_oracle.c``) on equivalent descriptions of one crystal (``_util.equivalence_cases``): unimodular
re-descriptions of skewed image ranges, supercells, a primitive cell against its conventional cell, permutations, rotations,
reflections and translations, on bulk, slab and wire frames and on two to five species.  Feature rows, energies, forces and
strain derivatives are invariant, or extensive, as the description says; forces are minus the gradient of the energy.

tests/test_gpu_invariance.py holds every kernel route to the same relations: an exception that comes from the reference's own
semantics shows up here, on the CPU, before a kernel is blamed for it.
"""
import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic
from _util import describe, equivalence_cases, worst_elementwise

CASES = equivalence_cases()
TOL = 1e-9                  # rows, energies and forces: relative, entry by entry
H = (1e-4, 5e-5)            # Richardson pair: central differences are O(h^2), (4 D(h/2) - D(h)) / 3 is O(h^4)
FD_TOL = 1e-8               # max |F - F_fd| <= FD_TOL * max |F|


def _coeff(basis, seed):
    coeff = np.random.default_rng(seed).normal(0, 0.05, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    return coeff


def _rows_close(got, want, label):
    assert worst_elementwise(got, want, rtol=TOL, floor=1e-12) <= 1.0, label


def _force_rows_close(got, want, scale, label):
    """force rows of a frame whose rows all vanish by symmetry (the perfect primitive crystal): within 1e-12 of the energy row"""
    if np.abs(want).max() <= 1e-12 * scale:
        assert np.abs(got).max() <= 1e-12 * scale, label
    else:
        _rows_close(got, want, label)


@pytest.mark.parametrize("case", list(CASES))
def test_feature_rows_of_equivalent_descriptions(case):
    els, base, descs = CASES[case]
    ob = O.OracleBasis(synthetic.notebook_basis(els))
    ref = O.featurize(ob, base)
    scale = np.abs(ref["xe"]).max()
    for d in descs:
        got = O.featurize(ob, d.atoms)
        _rows_close(got["xe"], d.xe(ref["xe"]), (case, d.label, "energy row"))
        if not d.reference_drops_terms:
            _force_rows_close(got["xf"], d.xf(ref["xf"]), scale, (case, d.label, "force rows"))


@pytest.mark.parametrize("case", list(CASES))
def test_energy_forces_and_strain_derivative_of_equivalent_descriptions(case):
    els, base, descs = CASES[case]
    basis = synthetic.notebook_basis(els)
    ob, coeff = O.OracleBasis(basis), _coeff(basis, 7)
    e0, f0, v0 = O.evaluate(ob, base, coeff, virial=True)
    for d in descs:
        e, f, v = O.evaluate(ob, d.atoms, coeff, virial=True)
        assert abs(e - d.energy(e0)) <= TOL * abs(d.energy(e0)), (case, d.label, e, d.energy(e0))
        assert worst_elementwise(v, d.virial(v0), rtol=TOL, floor=1e-11) <= 1.0, (case, d.label, v, d.virial(v0))
        if not d.reference_drops_terms:
            want = d.forces(f0)
            if np.abs(want).max() <= 1e-12 * abs(e0):
                assert np.abs(f).max() <= 1e-12 * abs(e0), (case, d.label)
            else:
                assert worst_elementwise(f, want, TOL) <= 1.0, (case, d.label)
            assert np.abs(f.sum(axis=0)).max() <= 1e-11 * max(1.0, np.abs(f).max()), (case, d.label)


def test_the_reference_drops_ghost_centred_terms_on_a_skewed_slab():
    """The one listed exception: on the 3 x 3 x 2 slab re-described by (1 0 / 3 1) the image range [2, 1, 1] no longer holds the
    third atom of every ghost-centred triplet.  Energy row and energy stay invariant; the reference's 3-body force rows and
    forces lose terms.  The kernels keep them: tests/test_gpu_invariance.py holds their force rows and
    forces on this description to the mapped original and to the gradient of the energy instead."""
    els, base, (d,) = CASES["slab_ghost_terms"]
    assert d.reference_drops_terms
    basis = synthetic.notebook_basis(els)
    ob, coeff = O.OracleBasis(basis), _coeff(basis, 7)
    ref, got = O.featurize(ob, base, indices=True), O.featurize(ob, d.atoms, indices=True)
    assert ref["supercell"]["factors"] == [1, 1, 1] and got["supercell"]["factors"] == [2, 1, 1]
    _rows_close(got["xe"], d.xe(ref["xe"]), "energy row")
    assert worst_elementwise(got["xf"], d.xf(ref["xf"])) > 1e3
    e0, f0 = O.evaluate(ob, base, coeff)
    e, f = O.evaluate(ob, d.atoms, coeff)
    assert abs(e - e0) <= TOL * abs(e0)
    assert np.abs(f - d.forces(f0)).max() > 1e-6 * np.abs(f0).max()
    assert np.abs(f.sum(axis=0)).max() > 1e-8                            # (nor do they add up to zero)


def _fd_forces(energy, atoms, picks):
    """Richardson-extrapolated central differences of ``energy(atoms)``: -dE/dx for each (atom, component) in ``picks``"""
    out = []
    for a, c in picks:
        d = []
        for h in H:
            es = []
            for sgn in (1, -1):
                p = atoms.get_positions()
                p[a, c] += sgn * h
                es.append(energy(type(atoms)(numbers=atoms.get_atomic_numbers(), positions=p, cell=atoms.get_cell(),
                                             pbc=atoms.get_pbc())))
            d.append(-(es[0] - es[1]) / (2 * h))
        out.append((4 * d[1] - d[0]) / 3)
    return np.array(out)


FD_PICKS = [(0, 0), (1, 1), (3, 2), (5, 0), (8, 1), (12, 2), (15, 0), (15, 1)]


@pytest.mark.parametrize("case,label", [("bcc_mow", "skew_821"), ("bcc_mow", "skew_751_reflection"), ("slab_mow", "skew_in_plane_531"),
                                        ("wire_mow", "perm_rotation_shift"), ("quinary", "skew_351")])
def test_oracle_forces_are_minus_the_gradient_of_its_energy(case, label):
    els, _, descs = CASES[case]
    atoms = next(d for d in descs if d.label == label).atoms
    basis = synthetic.notebook_basis(els)
    ob, coeff = O.OracleBasis(basis), _coeff(basis, 7)
    _, f = O.evaluate(ob, atoms, coeff)
    fd = _fd_forces(lambda a: O.evaluate(ob, a, coeff, forces=False)[0], atoms, FD_PICKS)
    got = np.array([f[a, c] for a, c in FD_PICKS])
    assert np.abs(got - fd).max() <= FD_TOL * np.abs(f).max(), (got, fd)


def test_energy_row_gradient_is_the_force_rows_on_a_skewed_cell():
    """-d x_e / d r = x_f, the featurizer's relation, on the [8, 2, 1] description"""
    els, _, descs = CASES["bcc_mow"]
    atoms = next(d for d in descs if d.label == "skew_821").atoms
    ob = O.OracleBasis(synthetic.notebook_basis(els))
    xf = O.featurize(ob, atoms)["xf"]
    for a, c in FD_PICKS[::2]:
        d = []
        for h in H:
            rows = []
            for sgn in (1, -1):
                p = atoms.get_positions()
                p[a, c] += sgn * h
                rows.append(O.featurize(ob, type(atoms)(numbers=atoms.get_atomic_numbers(), positions=p, cell=atoms.get_cell(),
                                                        pbc=True), forces=False)["xe"])
            d.append(-(rows[0] - rows[1]) / (2 * h))
        fd = (4 * d[1] - d[0]) / 3
        assert np.abs(fd - xf[a, c]).max() <= FD_TOL * np.abs(xf).max(), (a, c)


def test_descriptions_map_back_to_the_original():
    """the helper itself: a supercell's block 0 is the original atoms (wrapped), a rotation turns positions and cell alike,
    a reflection is accepted, a transform that mixes in an open axis is refused"""
    els, base, descs = CASES["bcc_mow"]
    sc = next(d for d in descs if d.label == "supercell_212")
    assert sc.scale == 4 and len(sc.atoms) == 4 * len(base) and np.array_equal(sc.src[:len(base)], np.arange(len(base)))
    assert np.allclose(sc.atoms.get_positions()[:len(base)], base.get_positions(), atol=1e-12)
    rot = next(d for d in descs if d.label == "perm_rotation_shift")
    g0 = np.asarray(base.get_cell()) @ np.asarray(base.get_cell()).T
    g1 = np.asarray(rot.atoms.get_cell()) @ np.asarray(rot.atoms.get_cell()).T
    assert np.allclose(g0, g1, atol=1e-12)
    v = np.arange(1.0, 7.0)
    assert np.allclose(describe(base, Q=np.diag([-1.0, 1.0, 1.0])).virial(v), v * [1, 1, 1, 1, -1, -1])
    _, slab, _ = CASES["slab_mow"]
    with pytest.raises(AssertionError, match="open axis"):
        describe(slab, U=[[1, 0, 1], [0, 1, 0], [0, 0, 1]])
