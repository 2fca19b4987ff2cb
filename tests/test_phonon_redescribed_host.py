"""A crystal's phonon spectrum does not depend on how the crystal is written down: the host route
(``harmonic.minimum_image_weights`` / ``image_terms`` / ``dynamical_matrices``) on skewed, turned, permuted, shifted, folded and
unwrapped descriptions of one crystal (tests/_phonon_redescribed.py), against the base frame through the mappings.  No GPU.

The nearest images are compared with a search by exhaustion; the spectra use a synthetic short-ranged force-constant function of
the separation vector, so that every difference is the image choice and the phases.

Measured on the CPU, ``max |dlam| / max |lam|`` between a description and its base at mapped q (folded sets included):
compact-to-compact pairs (COMPACT, where the +-2 search was already right) 9.4e-16 to 2.2e-15, so SPECTRUM_BOUND = 16 x 2.2e-15 =
3.5e-14 for every pair; all pairs lie between 7.5e-16 and 2.2e-15.  With the search put back to +-2
(``test_the_old_search_is_seen``) the three skews of the 16-atom cell give, at n_super 1 / 2: skew_821 8.0e-2 / 4.4e-2 with a
chosen image up to 4.0 / 9.7 Angstrom farther than the nearest, skew_351 3.4e-2 / 1.2e-3 (0.2 / 3.0 Angstrom), skew_751 1.0e-1 /
1.2e-2 (6.4 / 15.5 Angstrom): 3e10 to 3e12 times the bound."""
import functools

import numpy as np
import pytest

from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import harmonic
import _phonon_redescribed as P
import test_phonon_host as PH
from test_gpu_phonon import CASES as DEVICE_CASES, EXTRA as DEVICE_EXTRA

COMPACT_WORST = 2.2e-15                    # measured: see the module's docstring
SPECTRUM_BOUND = 16 * COMPACT_WORST
PAIRS = P.all_pairs()
IDS = [f"{f}-{lab}-{na}-{nb}" for f, lab, na, nb in PAIRS]


def _points():
    rng = np.random.default_rng(23)
    special = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0.5], [0.5, 0.5, 0.5], [0.25, 0.25, 0.25], [1.0, 0, 0]], dtype=float)
    return np.concatenate([rng.uniform(-0.5, 0.5, (12, 3)), special])


@functools.lru_cache(maxsize=None)
def _base_rows(frame, n_a):
    a = P.base(frame)
    fc = P.synthetic_rows(a, n_a, n_a * np.asarray(a.get_cell(), float))
    fc.setflags(write=False)
    return fc


def _description_rows(frame, label, n_a, n_b):
    a, d = P.base(frame), P.description(frame, label)
    return P.synthetic_rows(d.atoms, n_b, P.compact_supercell_basis(a, n_a, d))


def _spectrum_gap(frame, label, n_a, n_b):
    """max over q of |lam_B(q') - lam_A(mapped q, folded)| / max |lam_A|"""
    a, d = P.base(frame), P.description(frame, label)
    q_b = _points()
    lam_b = P.host_eigenvalues(_description_rows(frame, label, n_a, n_b), d.atoms, q_b, n_b)
    q_a = P.fold_q(a, d, q_b)
    lam_a = P.host_eigenvalues(_base_rows(frame, n_a), a, q_a.reshape(-1, 3), n_a).reshape(len(q_b), d.scale, -1)
    want = P.folded_union(lam_a)
    assert want.shape == lam_b.shape
    return float((np.abs(lam_b - want).max(axis=1) / P.spectrum_scale(want, q_b)).max())


# ---- the helpers check themselves ------------------------------------------------------------------------------------------------
def test_the_cases_are_the_ones_asked_for():
    have = {(f, lab) for f, lab, _, _ in PAIRS}
    for lab in ("skew_821", "skew_351", "skew_751", "perm_rotation_shift", "skew_751_reflection"):
        assert ("bcc_mow", lab) in have
    assert {("bcc_w_primitive", "skew_rotation"), ("bcc_w_primitive", "folded_222"), ("mow_skew3", "skew_821"),
            ("bcc_mow_unwrapped", "every_atom")} <= have
    assert ("bcc_w_primitive", "folded_222", 4, 2) in PAIRS and ("bcc_w_primitive", "folded_222", 2, 1) in PAIRS
    assert len(P.description("bcc_w_primitive", "folded_222").atoms) == 8
    assert [p[2:] for p in PAIRS if p[:2] == ("bcc_mow", "skew_751")] == [(1, 1), (2, 2)]
    assert [p[2:] for p in PAIRS if p[:2] == ("mow_skew3", "skew_821")] == [(1, 1), (2, 2), (3, 3)]
    outside = P.description("bcc_mow_unwrapped", "every_atom").atoms
    frac = outside.get_positions() @ np.linalg.inv(np.asarray(outside.get_cell(), float))
    assert frac.min() < -1.0 and frac.max() > 2.0                       # several cells outside
    s3 = DEVICE_CASES["mow_skew3"][1]()
    assert np.array_equal(s3.get_positions(), P.skew3().get_positions()) and np.array_equal(s3.get_cell(), P.skew3().get_cell())


def test_same_supercell_predicate():
    prim = P.base("bcc_w_primitive")
    fold = P.description("bcc_w_primitive", "folded_222")
    assert P.same_supercell(prim, 4, fold, 2) and P.same_supercell(prim, 2, fold, 1)
    assert not P.same_supercell(prim, 2, fold, 2) and not P.same_supercell(prim, 3, fold, 2)
    conv = next(d for d in P.equivalence_cases()["bcc_w_primitive"][2] if d.label == "conventional")
    assert not any(P.same_supercell(prim, na, conv, nb) for na in range(1, 5) for nb in range(1, 5))   # bcc against cubic P
    for f, lab, na, nb in PAIRS:
        assert P.same_supercell(P.base(f), na, P.description(f, lab), nb)
    assert P.generates([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0, 0], [3, 1, 0], [-2, 2, 1]])
    assert not P.generates([[2, 0, 0], [0, 1, 0], [0, 0, 1]], np.eye(3)) and not P.generates(np.eye(3), [[2, 0, 0], [0, 1, 0], [0, 0, 1]])


def test_wave_vector_mappings():
    q = _points()
    for f, lab, _, _ in PAIRS:
        a, d = P.base(f), P.description(f, lab)
        k_a = P.map_q(a, d, q) @ np.linalg.inv(np.asarray(a.get_cell(), float)).T
        k_b = q @ np.linalg.inv(np.asarray(d.atoms.get_cell(), float)).T
        assert np.abs(k_a @ d.Q.T - k_b).max() <= 1e-12                      # the same Cartesian vector, turned
        # ... under which every phase exp(2 pi i k . R) of a lattice vector keeps its value: R_B = Q R_A
        R_a = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, -1, 3]]) @ np.asarray(a.get_cell(), float)
        assert np.abs(k_a @ R_a.T - k_b @ (R_a @ d.Q.T).T).max() <= 1e-11
    prim, fold = P.base("bcc_w_primitive"), P.description("bcc_w_primitive", "folded_222")
    got = P.fold_q(prim, fold, q)
    assert got.shape == (len(q), 8, 3)
    want = {tuple(np.round((q[3] + g) / 2.0 % 1.0, 9)) for g in np.ndindex(2, 2, 2)}
    assert {tuple(np.round(r % 1.0, 9)) for r in got[3]} == want
    assert P.fold_q(P.base("bcc_mow"), P.description("bcc_mow", "skew_751"), q).shape == (len(q), 1, 3)


@pytest.mark.parametrize("frame,label,n_a,n_b", PAIRS, ids=IDS)
def test_atom_mapping_and_mapped_rows(frame, label, n_a, n_b):
    """``pair_map`` keeps every separation modulo the supercell lattice, and the synthetic force constants evaluated on the
    description are the base's through ``mapped_rows``: the mapping and the description-free evaluation check each other."""
    a, d = P.base(frame), P.description(frame, label)
    pm = P.pair_map(a, n_a, d, n_b)
    xa, xb = P.supercell_positions(a, n_a), P.supercell_positions(d.atoms, n_b)
    sup_inv = np.linalg.inv(n_a * np.asarray(a.get_cell(), float))
    for i in range(len(d.atoms)):
        assert np.array_equal(np.sort(pm[i]), np.arange(len(xa)))
        assert pm[i, i] == d.src[i]
        f = ((xb - xb[i]) @ d.Q - (xa[pm[i]] - xa[d.src[i]])) @ sup_inv
        assert np.abs(f - np.rint(f)).max() <= 1e-6
    z_a = np.tile(a.get_atomic_numbers(), n_a ** 3)
    z_b = np.tile(d.atoms.get_atomic_numbers(), n_b ** 3)
    assert np.array_equal(z_a[pm], np.broadcast_to(z_b, pm.shape))
    fc_a = _base_rows(frame, n_a)
    fc_b = _description_rows(frame, label, n_a, n_b)
    assert np.abs(fc_b - P.mapped_rows(fc_a, a, n_a, d, n_b)).max() <= 1e-13 * np.abs(fc_a).max()
    # the synthetic function itself: the sum rule, a finite range, and something in it
    assert np.abs(fc_b.sum(axis=1)).max() <= 1e-13 * np.abs(fc_b).max()
    assert (np.abs(fc_b).max(axis=(2, 3)) > 0).sum() >= 2 * len(d.atoms)


def test_synthetic_blocks_are_covariant_and_short_ranged():
    r = np.random.default_rng(3).uniform(-4, 4, (50, 3))
    Q = P.TURN
    got = P.pair_block(r @ Q.T, 1.0, 1.3)
    assert np.abs(got - np.einsum("ab,kbc,dc->kad", Q, P.pair_block(r, 1.0, 1.3), Q)).max() <= 1e-14
    assert np.all(P.pair_block(np.array([[P.RANGE, 0, 0], [0, 0, 0], [5, 5, 5]]), 1, 1) == 0)
    assert np.abs(P.pair_block(np.array([3.0, 0, 0]), 1, 1)).max() > 0.1


def test_brute_force_and_legacy_searches_on_a_known_cell():
    """The 2 Angstrom cubic cell at n_super 2 (tests/test_harmonic_host.py): two images at the face, eight at the corner."""
    atoms = Atoms(numbers=[74], positions=np.zeros((1, 3)), cell=np.eye(3) * 2.0, pbc=True)
    terms, w, worst = P.brute_force_images(atoms, 2, np.eye(3) * 4.0)
    assert worst <= 1.0
    assert (terms[:, 1] == 4).sum() == 2 and (terms[:, 1] == 7).sum() == 8 and (terms[:, 1] == 0).sum() == 1
    assert np.all(w[terms[:, 1] == 7] == 0.125)
    assert terms[terms[:, 1] == 4][:, 2:].tolist() == [[-1, 0, 0], [1, 0, 0]]
    pair, K, mult, examined = P.legacy_nearest_images(np.eye(3) * 4.0, [[2.0, 0, 0], [0.3, 0, 0]])
    assert pair.tolist() == [0, 0, 1] and K.tolist() == [[-1, 0, 0], [0, 0, 0], [0, 0, 0]] and mult.tolist() == [2, 1]
    assert examined.tolist() == [125, 125]


# ---- the fix ---------------------------------------------------------------------------------------------------------------------
def _existing_cells():
    cells = {name: (make(), n) for name, (_, make, _, n) in {**DEVICE_CASES, **DEVICE_EXTRA}.items()}
    for label, atoms, _ in PH._structures():
        for n in (2, 3, 5):
            cells[f"{label}-{n}"] = (atoms, n)
    return cells


@pytest.mark.parametrize("name", list(_existing_cells()))
def test_compact_cells_keep_their_terms_and_examine_no_more_candidates(name, monkeypatch):
    """On every cell of the existing phonon tests: the terms, weights and order are those of the +-2 search, and the helper
    computes the length of at most 125 candidate translations per pair (27 at most, as measured)."""
    atoms, n = _existing_cells()[name]
    terms, w = harmonic.image_terms(atoms, n)
    rows = harmonic.minimum_image_weights(atoms.get_cell(), atoms.get_positions(), n)
    cell = np.asarray(atoms.get_cell(), float)
    sc = P.supercell_positions(atoms, n)
    worst = 0
    for i in range(len(atoms)):
        _, _, _, examined = harmonic.nearest_images(cell * n, sc - sc[i])
        worst = max(worst, int(examined.max()))
    print(f"{name}: at most {worst} candidate translations per pair")
    assert worst <= 125
    monkeypatch.setattr(harmonic, "nearest_images", P.legacy_nearest_images)
    old_terms, old_w = harmonic.image_terms(atoms, n)
    old_rows = harmonic.minimum_image_weights(atoms.get_cell(), atoms.get_positions(), n)
    assert terms.dtype == np.int32 and np.array_equal(terms, old_terms) and np.array_equal(w, old_w)
    for new, old in zip(rows, old_rows):
        assert len(new) == len(old)
        for (R1, w1), (R0, w0) in zip(new, old):
            assert np.array_equal(R1, R0) and w1 == w0


DESCRIBED = sorted({(f, lab, nb) for f, lab, _, nb in PAIRS})


@pytest.mark.parametrize("frame,label,n_b", DESCRIBED, ids=[f"{f}-{lab}-{nb}" for f, lab, nb in DESCRIBED])
def test_image_choice_against_exhaustion(frame, label, n_b):
    """The image sets (ties within 1e-5 included), their order and their weights, from ``image_terms`` and from
    ``minimum_image_weights``, are those of the search by exhaustion, whose range is derived from the covering radius of a compact
    basis and asserted to suffice."""
    a, d = P.base(frame), P.description(frame, label)
    n_a = next(na for f, lab, na, nb in PAIRS if (f, lab, nb) == (frame, label, n_b))
    want, want_w, worst = P.brute_force_images(d.atoms, n_b, P.compact_supercell_basis(a, n_a, d))
    assert worst <= 1.0, worst
    terms, w = harmonic.image_terms(d.atoms, n_b)
    assert terms.dtype == np.int32
    assert terms.shape == want.shape and np.array_equal(terms, want)
    assert np.array_equal(w, want_w)
    cell = np.asarray(d.atoms.get_cell(), float)
    rows = harmonic.minimum_image_weights(cell, d.atoms.get_positions(), n_b)
    R = np.concatenate([r for row in rows for r, _ in row])
    wt = np.concatenate([[x] * len(r) for row in rows for r, x in row])
    assert len(R) == len(want) and np.abs(R - want[:, 2:].astype(float) @ cell).max() <= 1e-9 and np.array_equal(wt, want_w)
    assert sum(len(row) for row in rows) == len(d.atoms) ** 2 * n_b ** 3


def test_atoms_far_outside_their_cell_and_the_int32_limit():
    a = P.skew3()
    cell = np.asarray(a.get_cell(), float)
    terms, w = harmonic.image_terms(a, 2)
    far = np.array([[1000, -2000, 3000], [0, 0, 0], [-70000, 6, 12]])              # whole supercells
    moved = Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions() + far @ cell, cell=cell, pbc=True)
    t2, w2 = harmonic.image_terms(moved, 2)
    # atom j moved by m_j cells, a lattice vector of the supercell: the image of (i, p = (shift, j)) is the same point, so its triple is the old one - m_j + m_i
    # (tied images keep the order of their new triples: compare the records sorted)
    want = np.concatenate([terms[:, :2], terms[:, 2:] - far[terms[:, 1] % 3] + far[terms[:, 0]]], axis=1)
    order = lambda t: t[np.lexsort(t.T[::-1])]                                                      # noqa: E731
    assert np.array_equal(order(t2.astype(np.int64)), order(want)) and np.array_equal(w2, w)
    gone = Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions() + np.array([[3e9, 0, 0], [0, 0, 0], [0, 0, 0]]) @ cell,
                 cell=cell, pbc=True)
    with pytest.raises(ValueError, match="32 bits"):
        harmonic.image_terms(gone, 1)
    with pytest.raises(ValueError, match="finite"):
        harmonic.nearest_images(cell, [[np.nan, 0, 0]])


# ---- the spectrum ----------------------------------------------------------------------------------------------------------------
def test_compact_pairs_measure_the_bound():
    """Where the +-2 search was already right the description's spectrum is the base's to rounding; 16 x the worst of these
    figures is the bound every pair is held to."""
    worst = {}
    for f, lab, na, nb in P.all_pairs(only=P.COMPACT):
        worst[(f, lab, na, nb)] = _spectrum_gap(f, lab, na, nb)
    for k, v in worst.items():
        print(f"compact pair {k}: max |dlam| / max|lam| = {v:.2e}")
    assert len(worst) >= 8
    assert max(worst.values()) <= SPECTRUM_BOUND


@pytest.mark.parametrize("frame,label,n_a,n_b", PAIRS, ids=IDS)
def test_spectrum_does_not_depend_on_the_description(frame, label, n_a, n_b):
    gap = _spectrum_gap(frame, label, n_a, n_b)
    print(f"{frame} {label} n_super {n_a} / {n_b}: max |dlam| / max|lam| = {gap:.2e} (bound {SPECTRUM_BOUND:.1e})")
    assert gap <= SPECTRUM_BOUND


@pytest.mark.parametrize("frame,label", P.SKEWS)
def test_the_old_search_is_seen(frame, label, monkeypatch):
    """With the +-2 search back in place the spectrum test fails on each of the three skews, at every n_super."""
    monkeypatch.setattr(harmonic, "nearest_images", P.legacy_nearest_images)
    a, d = P.base(frame), P.description(frame, label)
    for na, nb in P.n_super_pairs(frame, label):
        gap = _spectrum_gap(frame, label, na, nb)
        terms, _ = harmonic.image_terms(d.atoms, nb)
        want, _, _ = P.brute_force_images(d.atoms, nb, P.compact_supercell_basis(a, na, d))
        cell, pos, n = np.asarray(d.atoms.get_cell(), float), d.atoms.get_positions(), len(d.atoms)

        def nearest(t):                     # per (i, p): the shortest |pos_j + n @ cell - pos_i| among the records t
            dist = np.linalg.norm(pos[t[:, 1] % n] + t[:, 2:].astype(float) @ cell - pos[t[:, 0]], axis=1)
            out = np.full((n, n * nb ** 3), np.inf)
            np.minimum.at(out, (t[:, 0], t[:, 1]), dist)
            return out

        excess = float((nearest(terms) - nearest(want)).max())
        print(f"{frame} {label} n_super {nb}, +-2 search: max |dlam| / max|lam| = {gap:.2e} = {gap / SPECTRUM_BOUND:.1e} x the bound; "
              f"a chosen image up to {excess:.1f} Angstrom farther than the nearest")
        assert gap > SPECTRUM_BOUND and excess > 0.1               # (against the tie tolerance of 1e-5)
        assert terms.shape != want.shape or not np.array_equal(terms, want)
