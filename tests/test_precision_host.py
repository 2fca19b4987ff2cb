"""
The extended-precision harness (tests/_precision.py) on the CPU: the extended build of the oracle, its magnitudes, the recorded
worst ratios of the fp64 oracle (``RHO_O``, which ``GAMMA`` for the kernels follows from), and what the harness sees that the
1e-9 tolerance of the parity tests does not -- four planted defects, each invisible to ``worst_elementwise(..., rtol=1e-9)``.
"""
import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd.representation import bspline
import _precision as P
from _util import worst_elementwise

NAMES = list(P.cases())


def test_extended_build_has_a_64_bit_mantissa():
    assert O.mant_dig() >= 64 and O.mant_dig(extended=False) == 53
    assert np.finfo(np.longdouble).nmant + 1 >= 64


@pytest.mark.parametrize("name", NAMES)
def test_magnitudes_bound_the_values_and_vanish_where_no_term_arrives(name):
    """M >= |value| for every entry; M == 0 exactly where the fp64 oracle's entry is 0.0.  One exception to the converse, by
    exact cancellation and not for want of terms: the lone Mo atom of the 3-atom triclinic cell sees only its own images in the
    Mo-Mo pair block, at +-(lattice vector), and in fp64 one of its force-row entries sums to 0.0 with M = 153 (the extended
    value, of the tiled positions' roundings, is -5e-15).  Such entries must lie in that block and be within the bound."""
    ob, _, val, mag = P.reference(name)
    got = P.fp64_oracle(name)
    for k in P.KINDS:
        v, m, g = np.asarray(val[k]), np.asarray(mag[k]), np.asarray(got[k])
        assert np.all(m.astype(np.longdouble) >= np.abs(v)), (name, k)
        assert not np.any(g[m == 0]), (name, k)
        odd = (g == 0) & (m > 0)
        if name == "triclinic_thin" and k == "xf":
            col = ob.pair_col[ob.pairs.index(("Mo", "Mo"))]
            assert np.all(np.argwhere(odd)[:, 0] == 2) and np.all((np.argwhere(odd)[:, 2] >= col) & (np.argwhere(odd)[:, 2] < col + 18))
            assert np.all(np.abs(v[odd]) <= P.RHO_O[k] * P.U * m[odd])
        else:
            assert not odd.any(), (name, k, int(odd.sum()))


def test_fp64_oracle_stays_within_the_recorded_table():
    """The measurement behind RHO_O, kept honest: the worst ratio of the fp64 build against the extended one, per kind, over all
    cases; the extended values rounded to double agree with the fp64 build within rho_o u M (the same statement, asserted on
    the rounded values); both builds count the same pairs and 3-body list entries."""
    worst = {k: 0.0 for k in P.KINDS}
    for name in NAMES:
        _, _, val, mag = P.reference(name)
        got = P.fp64_oracle(name)
        r = P.ratios(got, name)
        print(f"[precision] fp64 oracle, {name}: {P.fmt(r)}")
        assert set(r) == set(P.KINDS)
        for k in P.KINDS:
            worst[k] = max(worst[k], r[k])
            assert r[k] <= P.RHO_O[k], (name, k, r[k])
            rounded = np.asarray(val[k]).astype(np.float64)
            assert np.all(np.abs(rounded - np.asarray(got[k])) <= P.RHO_O[k] * float(P.U) * np.asarray(mag[k])), (name, k)
        assert np.array_equal(got["pair_cnt"], val["pair_cnt"]) and got["n3_cnt"] == val["n3_cnt"] and got["n3_cnt"] > 0
    print(f"[precision] fp64 oracle, worst over {len(NAMES)} cases: {P.fmt(worst)}")
    for k in P.KINDS:                                   # (the table is the measurement, not a loose cap)
        assert P.RHO_O[k] <= max(2.0 * worst[k], 1.0), (k, worst[k])
        assert P.GAMMA[k] == 16.0 * max(P.RHO_O[k], 1.0)


def test_ratio_counts_every_entry_and_insists_on_exact_zeros():
    t, m = np.array([1.0, 0.0, -2.0]), np.array([1.0, 0.0, 4.0])
    assert P.ratio(t, t, m) == 0.0
    assert P.ratio(t + np.array([2.0 ** -52, 0, 0]), t, m) == 2.0
    assert P.ratio(t + np.array([0, 0, 2.0 ** -51]), t, m) == 1.0
    with pytest.raises(AssertionError):
        P.ratio(t + np.array([0, 1e-300, 0]), t, m)
    with pytest.raises(AssertionError):
        P.ratio(t[:2], t, m)


def test_a_frame_with_a_leg_at_an_untrimmed_end_is_not_clear():
    basis, atoms, _ = P.cases()["cluster"]
    pos = np.asarray(atoms.get_positions()).copy()
    pos[1] = pos[0] + np.array([1.5, 0.0, 0.0])              # (a leg of length r_min of a basis without leading trim)
    moved = type(atoms)(numbers=atoms.get_atomic_numbers(), positions=pos)
    with pytest.raises(AssertionError):
        P.clear_of_discontinuities(basis, moved)
    assert P.clear_of_discontinuities(basis, atoms) > 1e-9


# ------------------------------------------------------------------------------------------------ planted defects
def _unary_triplets(basis, atoms):
    """(trio, L M N, [(r_ij, r_ik, r_jk)]) over the real centres of a one-species frame, legs as the oracle assigns them"""
    trio = basis.interactions_map[3][0]
    seqs = [np.asarray(k, float) for k in basis.knots_map[trio]]
    pos, _, _ = O.supercell(atoms, basis.r_cut)
    rmin3, rmax3 = min(k.min() for k in seqs), max(k.max() for k in seqs[:2])
    out = []
    for i in range(len(atoms)):
        d = np.linalg.norm(pos - pos[i], axis=1)
        nb = np.flatnonzero((d > rmin3) & (d <= rmax3))
        for a in range(len(nb)):
            for b in range(a + 1, len(nb)):
                rjk = np.linalg.norm(pos[nb[a]] - pos[nb[b]])
                if seqs[2][0] <= rjk <= seqs[2][-1]:
                    out.append((d[nb[a]], d[nb[b]], rjk))
    return trio, seqs, np.array(out)


def _leg(basis, seq, r):
    """(first, the four values) of a leg, trimmed functions zero"""
    first, vals, _ = bspline.basis_values(seq, [r])
    first, vals = int(first[0]), vals[0].copy()
    dim = len(seq) - 4
    for q in range(4):
        if not basis.leading_trim[3] <= first + q < dim - basis.trailing_trim[3]:
            vals[q] = 0.0
    return first, vals


def _triplet_grid(basis, seqs, legs):
    grid = np.zeros([len(s) - 4 for s in seqs])
    (il, vl), (im, vm), (iN, vn) = legs
    for x in range(4):
        for y in range(4):
            for w in range(4):
                if vl[x] * vm[y] * vn[w] != 0.0:
                    grid[il + x, im + y, iN + w] += vl[x] * vm[y] * vn[w]
    return grid


def _pair_terms(ob, atoms, p):
    """(i, j, d, bond vector) of the directed pairs of pair block p, the oracle's"""
    basis = ob.basis
    pos, z, _ = O.supercell(atoms, basis.r_cut)
    za, zb = ob.pair_z[p]
    out = []
    for i in range(len(atoms)):
        d = np.linalg.norm(pos - pos[i], axis=1)
        want = zb if z[i] == za else (za if z[i] == zb else -1)
        for j in np.flatnonzero((d > max(ob.pair_rmin[p], 0.0)) & (d < ob.pair_rmax[p]) & (z == want)):
            out.append((i, j, d[j], pos[j] - pos[i]))
    return out


def _report(what, planted, kind, name):
    _, _, val, mag = P.reference(name)
    got = P.fp64_oracle(name)[kind]
    today = worst_elementwise(planted, got, rtol=1e-9)
    seen = P.ratio(planted, val[kind], mag[kind])
    moved = planted != got
    assert moved.any()
    there = P.ratio(planted[moved], np.asarray(val[kind])[moved], np.asarray(mag[kind])[moved])
    print(f"[precision] planted: {what}: worst_elementwise at 1e-9 {today:.3g}, ratio {seen:.3g} (GAMMA {P.GAMMA[kind]:g}; "
          f"over the {int(moved.sum())} entries it moved {there:.3g}, the fp64 oracle's own there "
          f"{P.ratio(got[moved], np.asarray(val[kind])[moved], np.asarray(mag[kind])[moved]):.3g})")
    assert today <= 1.0, (what, today)
    return seen


@pytest.fixture(scope="module")
def unary():
    basis, atoms, _ = P.cases()["w_cap16"]
    trio, seqs, trips = _unary_triplets(basis, atoms)
    ob = P.reference("w_cap16")[0]
    lo = ob.trio_col[0]
    # the restatement reproduces the oracle's 3-body energy columns: the planted terms are terms of these entries
    row = np.zeros(ob.trio_ncol[0])
    for r in trips:
        row += basis.compress_3B(_triplet_grid(basis, seqs, [_leg(basis, s, x) for s, x in zip(seqs, r)]), trio)
    xe = P.fp64_oracle("w_cap16")["xe"]
    assert np.abs(row - xe[lo:lo + len(row)]).max() <= 1e-12 * np.abs(row).max()
    return basis, trio, seqs, trips, lo, xe


def test_planted_leg_values_through_fp32(unary):
    """The four values of one leg of one triplet rounded through np.float32 (a window row that went through fp32 on the host).
    Measured: worst_elementwise 0.057, ratio 6.7e+03 (the fp64 oracle's own on the nine entries it moves: 0.2); against the
    magnitudes widened for the routes that evaluate local pieces (``ratios(..., pieces=True)``) it still reads above GAMMA,
    asserted too."""
    basis, trio, seqs, trips, lo, xe = unary
    legs = [_leg(basis, s, x) for s, x in zip(seqs, trips[0])]
    low = [(legs[0][0], legs[0][1].astype(np.float32).astype(np.float64))] + legs[1:]
    delta = basis.compress_3B(_triplet_grid(basis, seqs, low) - _triplet_grid(basis, seqs, legs), trio)
    planted = xe.copy()
    planted[lo:lo + len(delta)] += delta
    assert _report("one leg's four values through fp32", planted, "xe", "w_cap16") > P.GAMMA["xe"]
    wide = P.ratios({"xe": planted}, "w_cap16", pieces=True)["xe"]
    print(f"[precision] planted: one leg's four values through fp32, piece magnitudes: ratio {wide:.3g}")
    assert wide > P.GAMMA["xe"]


def test_planted_term_scaled(unary):
    """One term scaled by 1 + 1e-11, in two entries.  (i) A pair force-row entry of atom 0 (W, 16-atom cell), a sum of the few
    bonds whose distance lies in one function's support: the bond's term 2 B'(d) cos scaled.  Measured: worst_elementwise
    0.46, ratio 374 -- asserted above GAMMA (32).  (ii) One triplet's largest product of three leg values in a 3-body column of
    the energy row, a sum of about 1700 such products: worst_elementwise 1.2e-05, ratio 1.9 -- BELOW GAMMA (24): 1e-11 of one
    term in thousands is below the entry's own rounding, and no fp64 comparison can see it.  Reported, asserted only to move
    the entry."""
    basis, trio, seqs, trips, lo, xe = unary
    name = "w_cap16"
    ob = P.reference(name)[0]
    xf = P.fp64_oracle(name)["xf"]
    knots = np.asarray(basis.knots_map[ob.pairs[0]], float)
    _, _, d, vec = [t for t in _pair_terms(ob, P.cases()[name][1], 0) if t[0] == 0][0]
    first, _, der = bspline.basis_values(knots, [d])
    q = int(np.argmax(np.abs(der[0])))
    planted = xf.copy()
    planted[0, :, ob.pair_col[0] + first[0] + q] += 1e-11 * 2.0 * der[0, q] * vec / d
    assert _report("one bond's term of a pair force-row entry scaled by 1 + 1e-11", planted, "xf", name) > P.GAMMA["xf"]
    grid = _triplet_grid(basis, seqs, [_leg(basis, s, x) for s, x in zip(seqs, trips[0])])
    one = np.zeros_like(grid)
    one.flat[np.argmax(grid)] = grid.max()
    delta = basis.compress_3B(one * 1e-11, trio)
    planted = xe.copy()
    planted[lo:lo + len(delta)] += delta
    assert _report("one product of a 3-body energy column scaled by 1 + 1e-11", planted, "xe", name) > 0.0


def test_planted_smallest_term_removed():
    """The smallest term of a pair column of the energy row removed, where it is >= 1e-11 of the entry and still invisible at
    1e-9: every such (column, term) of the 54-atom Mo/W cell is planted in turn, and every one must show.  Measured: 3
    terms (5.6e-11 of 2.98, 2.4e-09 of 56.6, 1.4e-08 of 130), worst_elementwise at most 0.11, ratio at least 4.0e+03."""
    name = "mow_cap16"
    ob = P.reference(name)[0]
    _, atoms, _ = P.cases()[name]
    xe = P.fp64_oracle(name)["xe"]
    seen, n = np.inf, 0
    for p in range(len(ob.pairs)):
        knots = np.asarray(ob.basis.knots_map[ob.pairs[p]], float)
        d = np.array([t[2] for t in _pair_terms(ob, atoms, p)])
        first, vals, _ = bspline.basis_values(knots, d)
        cols = np.zeros((len(d), len(knots) - 4))
        for q in range(4):
            cols[np.arange(len(d)), first + q] = vals[:, q]
        cols = cols[:, :len(knots) - 4 - ob.basis.trailing_trim[2]]
        lo = ob.pair_col[p]
        assert np.abs(cols.sum(0) - xe[lo:lo + cols.shape[1]]).max() <= 1e-12 * xe.max()
        for b in range(cols.shape[1]):
            t = cols[:, b]
            t = t[t > 0]
            if len(t) > 1 and 1e-11 * xe[lo + b] <= t.min() <= 0.9 * (1e-9 * xe[lo + b] + 1e-12 * np.abs(xe).max()):
                planted = xe.copy()
                planted[lo + b] -= t.min()
                seen = min(seen, _report(f"smallest term ({t.min():.2e} of {xe[lo + b]:.3g}) removed", planted, "xe", name))
                n += 1
    assert n >= 1, n
    assert seen > P.GAMMA["xe"], seen


def test_planted_reciprocal_a_newton_step_short():
    """1 / r of one bond (atom 0's first, W-W block) from a 24-bit estimate and ONE Newton step, in the pair force rows of atom
    0: the relative error of the reciprocal is the estimate's squared, at most 2^-48 = 3.6e-15 = 32 u.  Measured:
    worst_elementwise 6e-05; over the 12 entries the bond reaches the ratio is 0.37 where the fp64 oracle's own is 0.38, and
    with the same reciprocal on every bond of the atom 1.09 against 0.97 (the frame's worst, 1.15, lies elsewhere) -- BELOW
    GAMMA (32), and not told from rounding at all: 32 u on a cosine whose term is a fraction of M is what any fp64 evaluation
    may leave.  The harness does not see a reciprocal one step short of a 24-bit estimate; it would see one two steps short
    (2^-24: the 1e-9 tolerance does not).  Asserted as found, so that a change of the harness that alters it shows."""
    name = "w_cap16"
    ob = P.reference(name)[0]
    _, atoms, _ = P.cases()[name]
    xf = P.fp64_oracle(name)["xf"]
    knots = np.asarray(ob.basis.knots_map[ob.pairs[0]], float)
    bonds = [t for t in _pair_terms(ob, atoms, 0) if t[0] == 0]
    lo, nb = ob.pair_col[0], len(knots) - 4 - ob.basis.trailing_trim[2]

    def planted(which):
        out = xf.copy()
        for _, _, d, vec in which:
            y = np.float64(np.float32(1.0 / d))
            y = y * (2.0 - d * y)
            first, _, der = bspline.basis_values(knots, [d])
            for q in range(4):
                if first[0] + q < nb:
                    out[0, :, lo + first[0] + q] += 2.0 * der[0, q] * vec * (y - 1.0 / d)
        return out

    one = _report("1/r of one bond, 24-bit estimate + one Newton step", planted(bonds[:1]), "xf", name)
    every = _report("1/r of every bond of an atom, 24-bit estimate + one step", planted(bonds), "xf", name)
    assert one < P.GAMMA["xf"] and every < P.GAMMA["xf"]      # (the finding above; a harness that began to see it would say so here)
