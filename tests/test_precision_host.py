"""
The extended-precision harness (tests/_precision.py) on the CPU: the extended build of the oracle, its magnitudes, the recorded
worst ratios of the fp64 oracle (``RHO_O``, which ``GAMMA`` for the kernels follows from), and what the harness sees that the
1e-9 tolerance of the parity tests does not -- four planted defects, each invisible to ``worst_elementwise(..., rtol=1e-9)``.
The second half does the same for the second-derivative and per-centre kinds (``P.KINDS_D2``: the oracle's ``hessian_x``,
``site_terms_x``, ``site_rows_x``): magnitudes, the recorded table, cross-checks against the three NumPy restatements at the
tolerances of the GPU tests that use them, and five planted defects invisible at 1e-10 of the array's largest entry.
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


# ================================================================================================ second derivatives, site terms
# Hessian, mixed and Born terms (oracle.hessian_x), site energies, site virials and the heat current's per-centre shares
# (oracle.site_terms_x), site rows (oracle.site_rows_x): the kinds P.KINDS_D2.
def _tensor_to_voigt(t):
    return np.array([t[0, 0], t[1, 1], t[2, 2], t[1, 2], t[0, 2], t[0, 1]])


def test_second_derivative_kinds_move_no_case():
    """Every case has 3-body trims of 0 or 3 at either end, so the leg ends that are steps for the second-derivative kinds are
    the ones that are steps for the values: the same clearance, asserted and not assumed."""
    for name in NAMES:
        basis, atoms, _ = P.cases()[name]
        assert int(basis.leading_trim[3]) in (0, 3) and int(basis.trailing_trim[3]) in (0, 3), name
        assert P.clear_of_discontinuities(basis, atoms, second=True) == P.clear_of_discontinuities(basis, atoms), name
    # a leading trim of 1 or 2: the kept functions vanish at the leading end, their second derivatives do not.  (A third leg that
    # begins above the list range's lower end, so that the leg end is not a step of the list itself.)
    from uf3_amd.data import composition
    from uf3_amd.data.atoms import Atoms
    cs = composition.ChemicalSystem(["W"], 3)
    pair, trio = cs.interactions_map[2][0], cs.interactions_map[3][0]
    atoms = Atoms(numbers=[74, 74, 74], positions=[[0, 0, 0], [1.5, 1.0, 0], [1.5, -1.0, 0]])      # r_jk = 2.0 exactly
    for lead in (0, 1, 2, 3):
        basis = bspline.BSplineBasis(cs, r_min_map={pair: 0.001, trio: [1.5, 1.5, 2.0]}, r_max_map={pair: 5.5, trio: [3.5, 3.5, 7.0]},
                                     resolution_map={pair: 15, trio: [6, 6, 12]}, leading_trim={2: 0, 3: lead},
                                     trailing_trim={2: 3, 3: 3})
        for second in (False, True):
            if lead == 0 or (second and lead < 3):
                with pytest.raises(AssertionError):
                    P.clear_of_discontinuities(basis, atoms, second=second)
            else:
                assert P.clear_of_discontinuities(basis, atoms, second=second) > 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_d2_magnitudes_bound_the_values_and_vanish_where_no_term_arrives(name):
    """M >= |value|; M == 0 exactly where no term arrives, and there the fp64 build's entry is exactly 0.0: an H block between
    two atoms that share no term (farther apart than any pair range and with no common triplet), the site-row columns of a
    species an atom never meets.  H's extended value is symmetric and its rows sum to zero, each within u M."""
    basis, atoms, _ = P.cases()[name]
    ob, _, val, mag = P.reference(name)
    n = len(atoms)
    for kind in P.KINDS_D2:
        got = P.fp64_oracle_d2(name, kind)[kind]
        v, m = np.asarray(val[kind]), np.asarray(mag[kind])
        assert np.all(m.astype(np.longdouble) >= np.abs(v)), (name, kind)
        assert not np.any(got[m == 0]) and not np.any(v[m == 0]), (name, kind)
    H, MH = np.asarray(val["H"]), np.asarray(mag["H"]).astype(np.longdouble)
    assert np.all(np.abs(H - H.T) <= P.U * np.maximum(MH, MH.T)), name
    # (the sum over the column atoms' blocks; its bound is the sum of the entries' own)
    sums, bound = H.reshape(3 * n, n, 3).sum(axis=1), MH.reshape(3 * n, n, 3).sum(axis=1)
    assert np.all(np.abs(sums) <= P.U * bound), (name, float(np.max(np.abs(sums) / (P.U * bound))))
    # a block between two atoms with no common term has M == 0: no image of one within the longest pair range of the other, nor
    # within a centre leg's range (centre and neighbour), nor within what two neighbours of one centre can be apart (twice a
    # centre leg, and no more than the third leg's range)
    pos, _, _ = O.supercell(atoms, O.supercell_radius(ob, atoms) + 2.0 * float(basis.r_cut))
    rmax3 = max((float(np.max(k)) for t in ob.trios for k in basis.knots_map[t][:2]), default=0.0)
    rmax_n = max((float(np.max(basis.knots_map[t][2])) for t in ob.trios), default=0.0)
    reach = max(float(np.max(ob.pair_rmax)), rmax3, min(2.0 * rmax3, rmax_n))
    blocks = MH.reshape(n, 3, n, 3).max(axis=(1, 3))
    par = np.arange(len(pos)) % n
    empty = 0
    for i in range(n):
        d = np.linalg.norm(pos - pos[i], axis=1)
        near = np.zeros(n, bool)
        near[par[d <= reach * (1 + 1e-12)]] = True
        assert not blocks[i, ~near].any(), (name, i)
        empty += int((~near).sum())
    print(f"[precision] {name}: {empty} of {n * n} blocks of H between atoms that share no term, {int((blocks == 0).sum())} with M == 0")
    if name in ("mow_cap16", "uneven_lead3", "w16_sym3"):
        assert empty > 0, name
    # site rows: the pair and 3-body columns of a species that an atom never meets, within the longest range, stay empty
    b, Mb = np.asarray(val["b"]), np.asarray(mag["b"])
    z = np.asarray(atoms.get_atomic_numbers())
    for i in range(n):
        assert np.array_equal(np.flatnonzero(Mb[i, :len(ob.species_z)]), [list(ob.species_z).index(z[i])])
        for p, (za, zb) in enumerate(ob.pair_z):
            if z[i] not in (za, zb):
                lo = ob.pair_col[p]
                assert not Mb[i, lo:lo + ob.pair_nk[p] - 4].any() and not b[i, lo:lo + ob.pair_nk[p] - 4].any(), (name, i, p)
        for t, (zc, _, _) in enumerate(ob.trio_z):
            if z[i] != zc:
                lo = ob.trio_col[t]
                assert not Mb[i, lo:lo + ob.trio_ncol[t]].any(), (name, i, t)


def test_fp64_oracle_stays_within_the_recorded_table_d2():
    """The measurement behind RHO_O for the kinds of KINDS_D2: the worst ratio of the fp64 build against the extended one over
    all cases.  Also: sum_i b_i is the extended energy row, sum_i U_i the extended energy, and the symmetrised sum_i W_i the
    extended strain derivative, each within a few u M of the entry -- on every case whose atoms lie inside their cell, the frames
    on which both descriptions mean the same frame."""
    worst = {k: 0.0 for k in P.KINDS_D2}
    for name in NAMES:
        basis, atoms, _ = P.cases()[name]
        ob, coeff, val, mag = P.reference(name)
        r = {}
        for kind in ("H", "U", "b"):
            r.update(P.ratios(P.fp64_oracle_d2(name, kind), name))
        print(f"[precision] fp64 oracle, {name}: {P.fmt(r)}")
        assert set(r) == set(P.KINDS_D2)
        for k in P.KINDS_D2:
            worst[k] = max(worst[k], r[k])
            assert r[k] <= P.RHO_O[k], (name, k, r[k])
        if O.supercell_radius(ob, atoms) == basis.r_cut:
            rows_v, rows_m = O.site_rows_x(ob, atoms)
            live = np.asarray(mag["xe"]) > 0
            assert np.array_equal(np.asarray(rows_v["xe"]), np.asarray(val["xe"]))     # (the same walk, the same order)
            assert not np.asarray(rows_v["xe"])[np.asarray(basis.col_idx, dtype=int)].any()
            sums = {"b": P.ratio(np.asarray(val["b"]).sum(0)[live], np.asarray(val["xe"])[live], np.asarray(mag["xe"])[live]),
                    "U": P.ratio(np.asarray(val["U"]).sum(), val["e"], mag["e"])}
            Ws = np.asarray(val["W"]).sum(0)
            sums["W"] = P.ratio(_tensor_to_voigt(0.5 * (Ws + Ws.T)), val["v"], mag["v"])
            print(f"[precision] sums over centres against the frame's, {name}: {P.fmt(sums)}")
            assert max(sums.values()) <= 4.0, (name, sums)
    print(f"[precision] fp64 oracle, worst over {len(NAMES)} cases: {P.fmt(worst)}")
    for k in P.KINDS_D2:
        assert P.RHO_O[k] <= max(2.0 * worst[k], 1.0), (k, worst[k])
        assert P.GAMMA[k] == 16.0 * max(P.RHO_O[k], 1.0)


# ------------------------------------------------------------------------------------------------ cross-checks
def _harmonic_cases():
    import test_gpu_harmonic as TH
    return TH._cases()


@pytest.mark.parametrize("label", [c[0] for c in _harmonic_cases()])
def test_hessian_entry_against_the_numpy_restatement(label):
    """oracle.hessian_x (fp64 build) against _harmonic_ref.hessian on the frames of tests/test_gpu_harmonic.py, at that test's
    tolerance (1e-10 of each array's largest entry): two references written from different descriptions."""
    import _harmonic_ref as HR
    _, model, atoms = [c for c in _harmonic_cases() if c[0] == label][0]
    m = model()
    ob, coeff = O.OracleBasis(m.bspline_config), np.asarray(m.coefficients, dtype=float)
    ref = dict(zip(("H", "mixed", "born"), HR.hessian(ob, atoms, coeff)))
    got, _ = O.hessian_x(ob, atoms, coeff, extended=False)
    for k in ("H", "mixed", "born"):
        err = np.abs(got[k] - ref[k]).max()
        print(f"[precision] hessian_x against _harmonic_ref, {label}: {k} {err / np.abs(ref[k]).max():.3g} of the largest entry")
        assert err <= 1e-10 * np.abs(ref[k]).max(), (label, k)


@pytest.mark.parametrize("label", ["w16", "w2", "nexe4", "w16_2and3", "cluster13", "w1", "w65", "mow16"])
def test_site_terms_entry_against_the_numpy_restatement(label):
    """oracle.site_terms_x (fp64 build) against _flux_ref on the frames of tests/test_gpu_flux.py, at that test's tolerances:
    U and W at 1e-10 of the largest magnitude, the frame's J_pot (the sum of the per-centre shares) at 1e-10 of the sum of its
    terms' absolute values."""
    import test_gpu_flux as TF
    model, make, seed = TF.FRAMES[label]
    m, atoms = TF._model(model), make()
    rU, rW, _, rJp, scale = TF._reference(label)
    got, _ = O.site_terms_x(O.OracleBasis(m.bspline_config), atoms, np.asarray(m.coefficients, dtype=float), TF._vel(atoms, seed),
                            extended=False)
    assert np.abs(got["U"] - rU).max() <= TF.RTOL * np.abs(rU).max()
    assert np.abs(got["W"] - rW).max() <= TF.RTOL * np.abs(rW).max()
    assert np.all(np.abs(got["jp"].sum(0) - rJp) <= TF.RTOL * scale)


@pytest.mark.parametrize("name", ["unary", "mow", "uneven", "sym1", "cluster", "pairs"])
def test_site_rows_entry_against_the_numpy_restatement(name):
    """oracle.site_rows_x (fp64 build) against _site_rows_ref on the cases of tests/test_gpu_site_grade.py, at that test's
    tolerance (1e-10 of the largest |B|)."""
    import _site_rows_ref as SR
    basis, atoms = SR.case(name)
    B = SR.reference(name)
    got, _ = O.site_rows_x(O.OracleBasis(basis), atoms, extended=False)
    assert np.abs(got["b"] - B).max() <= 1e-10 * np.abs(B).max()


# ------------------------------------------------------------------------------------------------ planted defects (KINDS_D2)
def _report_d2(what, planted, kind, name):
    """as _report, against today's tolerance for these kinds: 1e-10 of the array's largest entry"""
    _, _, val, mag = P.reference(name)
    got = P.fp64_oracle_d2(name, kind)[kind]
    today = float(np.abs(planted - got).max() / (1e-10 * np.abs(got).max()))
    seen = P.ratio(planted, val[kind], mag[kind])
    moved = planted != got
    assert moved.any()
    v, m = np.asarray(val[kind])[moved], np.asarray(mag[kind])[moved]
    print(f"[precision] planted: {what}: error over (1e-10 max|{kind}|) {today:.3g}, ratio {seen:.3g} (GAMMA {P.GAMMA[kind]:g}; "
          f"over the {int(moved.sum())} entries it moved {P.ratio(planted[moved], v, m):.3g}, the fp64 oracle's own there "
          f"{P.ratio(got[moved], v, m):.3g})")
    assert today <= 1.0, (what, today)
    return seen


def _unary_terms(name):
    """The terms of the Hessian of a 16-atom W cell, restated with scipy's B-splines over the oracle's supercell
    (_harmonic_ref's walk: one species, so the lower supercell index takes leg l): pair terms (i, parent j, d, g, k) and triplet
    terms (i, parent j, parent k, d [3, 3], the legs' values and derivatives nu = 0, 1, 2, the coefficient grid).  Their sum
    reproduces the fp64 oracle's H: the planted terms are terms of these entries."""
    import _harmonic_ref as HR
    basis, atoms, _ = P.cases()[name]
    assert len(P.reference(name)[0].trios) == 1
    ob, coeff, _, _ = P.reference(name)
    _, c2, c3 = O.split_coefficients(ob, coeff)
    n = len(atoms)
    pk = np.asarray(basis.knots_map[ob.pairs[0]], float)
    tk = [np.asarray(k, float) for k in basis.knots_map[ob.trios[0]]]
    G = c3.reshape(ob.grid_shapes[0])
    pos, _, _ = O.supercell(atoms, O.supercell_radius(ob, atoms))
    pairs, trips = [], []
    for i in range(n):
        d = pos - pos[i]
        r = np.linalg.norm(d, axis=1)
        for j in np.flatnonzero((r > max(ob.pair_rmin[0], 0.0)) & (r < ob.pair_rmax[0])):
            pairs.append((i, j % n, d[j].copy(), float(c2 @ HR._basis(pk, r[j], 1)[0]), float(c2 @ HR._basis(pk, r[j], 2)[0])))
        nb = np.flatnonzero((r > tk[0][0]) & (r <= max(tk[0][-1], tk[1][-1])))
        for x in range(len(nb)):
            for y in range(x + 1, len(nb)):
                j, k = nb[x], nb[y]
                dv = np.array([d[j], d[k], d[k] - d[j]])
                rr = np.linalg.norm(dv, axis=1)
                if all(tk[q][0] < rr[q] < tk[q][-1] for q in range(3)):
                    bv = [[np.nan_to_num(HR._basis(tk[q], rr[q], nu)[0]) for nu in range(3)] for q in range(3)]
                    trips.append((i, j % n, k % n, dv, bv))
    return n, pairs, trips, G


def _restated_H(name):
    """(n, pairs, trips, G, the fp64 oracle's H, per triplet its block between its two neighbours or None): the restatement's sum
    reproduces the oracle's H -- the planted terms are terms of these entries"""
    import _harmonic_ref as HR
    n, pairs, trips, G = _unary_terms(name)
    H = P.fp64_oracle_d2(name, "H")["H"]
    total, blocks = np.zeros_like(H), []
    L, B = np.zeros((3 * n, 6)), np.zeros((6, 6))
    for i, pj, d, g, k in pairs:
        HR._add(total, L, B, [i, pj], [(0, 1)], d[None], np.array([g]), np.array([[k]]))
    for term in trips:
        Ht = _triplet_H(n, term, G)
        total += Ht
        i, pj, pk_, _, _ = term
        blocks.append(Ht[3 * pj:3 * pj + 3, 3 * pk_:3 * pk_ + 3].copy() if len({i, pj, pk_}) == 3 else None)
    assert np.abs(total - H).max() <= 1e-12 * np.abs(H).max()
    return n, pairs, trips, G, H, blocks


def _leg_space(G, bv):
    c = lambda a, b, d: float(np.einsum("abc,a,b,c->", G, bv[0][a], bv[1][b], bv[2][d]))           # noqa: E731
    g = np.array([c(1, 0, 0), c(0, 1, 0), c(0, 0, 1)])
    K = np.array([[c(2, 0, 0), c(1, 1, 0), c(1, 0, 1)], [c(1, 1, 0), c(0, 2, 0), c(0, 1, 1)], [c(1, 0, 1), c(0, 1, 1), c(0, 0, 2)]])
    return g, K


def _triplet_H(n, term, G, bv=None):
    import _harmonic_ref as HR
    i, pj, pk_, dv, bv0 = term
    g, K = _leg_space(G, bv0 if bv is None else bv)
    H, L, B = np.zeros((3 * n, 3 * n)), np.zeros((3 * n, 6)), np.zeros((6, 6))
    HR._add(H, L, B, [i, pj, pk_], [(0, 1), (0, 2), (1, 2)], dv, g, K)
    return H


def test_planted_hessian_defects():
    """Three defects planted into the fp64 oracle's H of a 16-atom W cell ((a), (b): the bcc cell at a = 3.165 A; (c): the one at
    a = 4.0 A, whose first shell at 3.46 A lies next to the end of the centre legs at 3.5 A: triplets with tiny blocks), each
    invisible at 1e-10 max|H| and each above GAMMA:
    (a) the second derivatives of one triplet's three legs rounded through np.float32;
    (b) the g (I - uu^T) / r part of one far pair bond's blocks scaled by 1 + 1e-7: of the bonds beyond 5.0 A (r_max = 5.5) the one
        with the largest gradient.  (On the very farthest bond, r = 5.4992, g = -1.6e-07 is 1e-7 of the entry's M and the defect
        reads 0.06: below any fp64 evaluation's own rounding.);
    (c) one triplet's contribution to the block between its two neighbours removed -- the block a row atom reaches through the
        neighbour-slot walk, what a failed reverse-shift lookup loses -- for the triplet whose such block is the largest that
        today's tolerance still does not see.
    Measured figures are printed by _report_d2."""
    name = "w_cap16"
    n, pairs, trips, G, H, _ = _restated_H(name)
    limit = 1e-10 * np.abs(H).max()
    # (a): of the triplets of centre 0, the one this moves most while today's tolerance still does not see it
    pick = None
    for term in [t for t in trips if t[0] == 0]:
        low = [[q[0], q[1], q[2].astype(np.float32).astype(np.float64)] for q in term[4]]
        delta = _triplet_H(n, term, G, low) - _triplet_H(n, term, G)
        size = np.abs(delta).max()
        if 0 < size <= 0.9 * limit and (pick is None or size > pick[0]):
            pick = (size, delta)
    assert pick is not None
    planted = H + pick[1]
    assert _report_d2("one triplet's leg second derivatives through fp32", planted, "H", name) > P.GAMMA["H"]
    # (b)
    far = [t for t in pairs if np.linalg.norm(t[2]) > 5.0]        # (the two outermost shells of the bcc cell: 5.25 and 5.48 A)
    i, pj, d, g, k = max(far, key=lambda t: abs(t[3]))
    r = np.linalg.norm(d)
    blk = 1e-7 * g * (np.eye(3) - np.outer(d, d) / r ** 2) / r
    planted = H.copy()
    for s, t, sign in ((i, i, 1), (pj, pj, 1), (i, pj, -1), (pj, i, -1)):
        planted[3 * s:3 * s + 3, 3 * t:3 * t + 3] += sign * blk
    print(f"[precision] (the far bond: r = {r:.4f} of r_max = 5.5, g = {g:.3g}, k = {k:.3g})")
    assert _report_d2("g (I - uu^T) / r of one far pair bond scaled by 1 + 1e-7", planted, "H", name) > P.GAMMA["H"]
    # (c)
    name = "w_sparse_generic"
    n, pairs, trips, G, H, blocks = _restated_H(name)
    limit, best = 1e-10 * np.abs(H).max(), None
    for term, blk in zip(trips, blocks):
        size = 0.0 if blk is None else np.abs(blk).max()
        if 0 < size <= 0.9 * limit and (best is None or size > best[0]):
            best = (size, term[1], term[2], blk)
    assert best is not None
    size, pj, pk_, blk = best
    planted = H.copy()
    planted[3 * pj:3 * pj + 3, 3 * pk_:3 * pk_ + 3] -= blk
    print(f"[precision] (the removed block's largest entry: {size:.3g} of max|H| = {np.abs(H).max():.3g})")
    assert _report_d2("one triplet's block between its two neighbours removed", planted, "H", name) > P.GAMMA["H"]


def test_planted_site_virial_component_scaled():
    """(d) One component of a surface atom's site virial scaled by 1 + 1e-8: on the open cluster, the largest component of any
    atom that is still below 0.9 % of max|W|, so that today's 1e-10 max|W| does not see it."""
    name = "cluster"
    W = P.fp64_oracle_d2(name, "W")["W"]
    small = np.where(np.abs(W) <= 0.009 * np.abs(W).max(), np.abs(W), 0.0)
    at = np.unravel_index(np.argmax(small), W.shape)
    assert small[at] > 0
    planted = W.copy()
    planted[at] *= 1.0 + 1e-8
    print(f"[precision] (component {at}: {W[at]:.3g} of max|W| = {np.abs(W).max():.3g})")
    assert _report_d2("one component of one atom's site virial scaled by 1 + 1e-8", planted, "W", name) > P.GAMMA["W"]


def test_planted_site_row_smallest_term_removed():
    """(e) The smallest term of a site-row entry removed: over every atom and pair column of the 54-atom Mo/W cell, every smallest
    term that today's 1e-10 max|b| does not see and that is at least 1e-13 of its entry is planted in turn; all must show."""
    name = "mow_cap16"
    ob = P.reference(name)[0]
    _, atoms, _ = P.cases()[name]
    b = P.fp64_oracle_d2(name, "b")["b"]
    seen, count = np.inf, 0
    for p in range(len(ob.pairs)):
        knots = np.asarray(ob.basis.knots_map[ob.pairs[p]], float)
        lo, nb = ob.pair_col[p], len(knots) - 4
        terms = _pair_terms(ob, atoms, p)
        for i in sorted({t[0] for t in terms}):
            d = np.array([t[2] for t in terms if t[0] == i])
            first, vals, _ = bspline.basis_values(knots, d)
            cols = np.zeros((len(d), nb))
            for q in range(4):
                cols[np.arange(len(d)), first + q] = vals[:, q]
            assert np.abs(cols.sum(0) - b[i, lo:lo + nb]).max() <= 1e-12 * np.abs(b).max()
            for c in range(nb):
                t = cols[:, c]
                t = t[t > 0]
                if len(t) > 1 and 1e-13 * b[i, lo + c] <= t.min() <= 0.9e-10 * np.abs(b).max():
                    planted = b.copy()
                    planted[i, lo + c] -= t.min()
                    seen = min(seen, _report_d2(f"smallest term ({t.min():.2e} of {b[i, lo + c]:.3g}) of a site-row entry removed",
                                                planted, "b", name))
                    count += 1
    assert count >= 1, count
    assert seen > P.GAMMA["b"], seen
