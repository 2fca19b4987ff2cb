"""
The Monte Carlo kind of the extended-precision harness (tests/_precision.py, kind ``dE``) on the CPU: the oracle entry
``oracle.mc_delta_x`` (uf3_oracle.c: uf3o_mc_delta_x -- the evaluator's own term loop with a sink that keeps the terms a move
touches), its magnitude M, the recorded worst ratio of the fp64 entry (``RHO_O["dE"]``, which ``GAMMA["dE"]`` for mc_delta
follows from), and what the bound sees that ``1e-9 max(1, |E_frame|)`` of the Monte Carlo parity tests does not: five planted
defects of mc_delta's own bookkeeping, each far below that tolerance.

The extended differences of all cases are computed once (``P.mc_reference``, about a minute in all) and shared.
"""
import numpy as np
import pytest

from oracle import oracle as O
import _precision as P
from _on_knots import with_numbers

NAMES = list(P.mc_cases())
SMALL = [k for k in NAMES if k not in ("dense432", "thin16_r3", "thin16_r4", "limit512")]     # (cheap whole-frame energies)
U = float(P.U)


def _after(atoms, ob, i, second, mode):
    """the frame after the move"""
    z = np.asarray(atoms.get_atomic_numbers()).copy()
    if mode == "swap":
        z[i], z[second] = z[second], z[i]
    else:
        z[i] = O._Z[second]
    return with_numbers(atoms, z)


def test_fp64_entry_stays_within_the_recorded_table():
    """The measurement behind RHO_O["dE"], kept honest: the fp64 build's entry against the extended one over every move of every
    case, both modes; the magnitudes of both builds agree; null moves are exactly (0, 0) in both."""
    worst = 0.0
    for name in NAMES:
        _, atoms, _, _ = P.mc_cases()[name]
        for mode in P.MC_MODES:
            ref = P.mc_reference(name, mode)
            got, m64 = O.mc_delta_x(ref["ob"], atoms, ref["coeff"], ref["i"], ref["second"], mode, extended=False)
            r = P.ratio(got, ref["dE"], ref["M"])
            print(f"[precision] fp64 oracle mc_delta {mode}, {name}: dE {r:.3g}")
            worst = max(worst, r)
            assert r <= P.RHO_O["dE"], (name, mode, r)
            assert np.all(np.abs(m64 - ref["M"]) <= 1e-12 * ref["M"])
            null = np.array([lab == "null" for lab in ref["label"]])
            assert null.any() and not np.any(ref["dE"][null]) and not np.any(ref["M"][null]) and not np.any(got[null])
            assert np.all(ref["M"][~null] > 0) and np.all(ref["M"].astype(np.longdouble) >= np.abs(ref["dE"]))
    print(f"[precision] fp64 oracle mc_delta, worst over {len(NAMES)} cases: dE {worst:.3g}")
    assert P.RHO_O["dE"] <= max(2.0 * worst, 1.0)             # (the table is the measurement, not a loose cap)
    assert P.GAMMA["dE"] == 16.0 * max(P.RHO_O["dE"], 1.0)


@pytest.mark.parametrize("name", SMALL)
def test_difference_of_touched_terms_is_the_difference_of_two_energies(name):
    """In the extended build |dE - (E_x(z') - E_x(z))| <= u (M_e(z) + M_e(z')) -- the two whole energies carry the untouched
    terms' roundings, dE does not -- and M_dE <= M_e(z) + M_e(z'), strictly smaller on a frame of more than 16 atoms: the
    untouched terms are in neither dE nor M.  Three live moves of each mode."""
    _, atoms, _, _ = P.mc_cases()[name]
    for mode in P.MC_MODES:
        ref = P.mc_reference(name, mode)
        e0, m0 = O.evaluate_x(ref["ob"], atoms, ref["coeff"], virial=False, forces=False)
        live = [k for k, lab in enumerate(ref["label"]) if lab != "null"]
        for k in live[:: max(1, len(live) // 3)][:3]:
            e1, m1 = O.evaluate_x(ref["ob"], _after(atoms, ref["ob"], int(ref["i"][k]), ref["second"][k], mode), ref["coeff"],
                                  virial=False, forces=False)
            bound = P.U * (np.longdouble(m0["e"]) + m1["e"])
            err = abs(ref["dE"][k] - (e1["e"] - e0["e"]))
            assert err <= bound, (name, mode, k, float(err), float(bound))
            assert ref["M"][k] <= m0["e"] + m1["e"]
            if len(atoms) > 16:
                assert ref["M"][k] < 0.9 * (m0["e"] + m1["e"]), (name, mode, k, ref["M"][k], m0["e"] + m1["e"])


def test_untouched_terms_stay_out_of_the_magnitude_on_the_large_frames():
    """The same strict inequality where it matters most: 288 and 432 atoms (the whole-frame magnitudes from the fp64 build, which
    agree with the extended ones to rounding)."""
    for name in ("mow288", "dense432"):
        _, atoms, _, _ = P.mc_cases()[name]
        ref = P.mc_reference(name, "swap")
        k = ref["label"].index("three_body")
        m0 = O.evaluate_x(ref["ob"], atoms, ref["coeff"], virial=False, forces=False, extended=False)[1]["e"]
        m1 = O.evaluate_x(ref["ob"], _after(atoms, ref["ob"], int(ref["i"][k]), ref["second"][k], "swap"), ref["coeff"],
                          virial=False, forces=False, extended=False)[1]["e"]
        print(f"{name}: M_dE {ref['M'][k]:.4g}, M_e(z) + M_e(z') {m0 + m1:.4g}")
        assert ref["M"][k] < 0.5 * (m0 + m1)


@pytest.mark.parametrize("name", ["mow_cap16", "bcc24_s8", "triclinic_thin", "thin16_r3"])
def test_swap_is_symmetric_bit_for_bit(name):
    """swap (i, j) and swap (j, i): the same T, the same species afterwards, the same bits -- in both builds"""
    _, atoms, _, _ = P.mc_cases()[name]
    ref = P.mc_reference(name, "swap")
    keep = [k for k, lab in enumerate(ref["label"]) if lab != "null"][:2 if name == "thin16_r3" else 12]
    i, j = ref["i"][keep], np.array([ref["second"][k] for k in keep])
    for extended in (True, False):
        a, ma = O.mc_delta_x(ref["ob"], atoms, ref["coeff"], i, j, "swap", extended=extended)
        b, mb = O.mc_delta_x(ref["ob"], atoms, ref["coeff"], j, i, "swap", extended=extended)
        assert np.array_equal(a, b) and np.array_equal(ma, mb) and np.all(ma > 0)
        if extended:
            assert np.array_equal(a, ref["dE"][keep]) and np.array_equal(ma, ref["M"][keep])


def test_null_moves_are_exactly_zero():
    _, atoms, _, _ = P.mc_cases()["bcc24_s8"]
    ref = P.mc_reference("bcc24_s8", "swap")
    z = np.asarray(atoms.get_atomic_numbers())
    n = len(z)
    same = [(i, j) for i in range(n) for j in range(n) if z[i] == z[j]]
    dE, M = O.mc_delta_x(ref["ob"], atoms, ref["coeff"], [m[0] for m in same], [m[1] for m in same], "swap")
    assert len(same) >= n and not dE.any() and not M.any()
    dE, M = O.mc_delta_x(ref["ob"], atoms, ref["coeff"], np.arange(n), [int(q) for q in z], "transmute")
    assert not dE.any() and not M.any()


# ------------------------------------------------------------------------------------------------ planted defects
LOOSE = 1e-9                  # what tests/test_gpu_mc.py and its siblings hold an energy difference to, times max(1, |E_frame|)
LEG_END, PAIR_END = 3.5, 5.5  # the upper end of a centre leg and the pair r_max of the notebook basis (trailing trim 3)


def _edge_frame():
    """A frame that HAS small terms -- which an ordinary rattled lattice has not: its smallest term is of the order of 1e-5 eV,
    and a Monte Carlo parity test at 1e-9 would see one go missing.  The 54-atom Mo-W cell of ``mow_cap16`` is dilated until the
    second shell stands at the end of the centre legs, with one bond (i, m) 2e-4 A inside it: every term that holds that leg
    carries the factor ((3.5 - r) / 0.333)^3 = 2e-10 of the last kept function of a leg trimmed by 3.  Then one atom q of i's
    fourth shell is drawn towards i until their distance is 5e-4 A inside the pair r_max (factor (5e-4 / 0.367)^3 = 3e-9).
    j is an atom of the other species in i's 3-body range that is no neighbour of m.  -> (basis, atoms, i, j, m, q)"""
    basis, atoms, _, _ = P.mc_cases()["mow_cap16"]
    pos, cell, z = np.asarray(atoms.get_positions()).copy(), np.asarray(atoms.get_cell()).copy(), np.asarray(atoms.get_atomic_numbers())
    i = 0

    def images(p, c):
        sh = np.array([[a, b, d] for a in (-1, 0, 1) for b in (-1, 0, 1) for d in (-1, 0, 1)], dtype=float) @ c
        v = p[None, :, :] + sh[:, None, :] - p[i]
        return v, np.linalg.norm(v, axis=-1)                   # [27, N, 3], [27, N]
    _, d = images(pos, cell)
    dm = d.min(0)
    m = int(np.argmin(np.abs(dm - 3.165)))
    s = (LEG_END - 2e-4) / dm[m]
    pos, cell = pos * s, cell * s
    v, d = images(pos, cell)
    near3 = lambda a: np.linalg.norm((pos[None, :, :] + (np.array([[x, y, w] for x in (-1, 0, 1) for y in (-1, 0, 1) for w in (-1, 0, 1)],
                                                                 dtype=float) @ cell)[:, None, :] - pos[a]), axis=-1).min(0)
    j = next(int(k) for k in np.argsort(d.min(0)) if z[k] != z[i] and 1.5 < d.min(0)[k] < 3.3 and near3(m)[k] > LEG_END + 0.3)
    img, q = next((int(a), int(b)) for a, b in zip(*np.nonzero((d > 5.6) & (d < 6.0))) if b not in (i, j, m) and near3(b)[m] > PAIR_END + 0.5)
    pos[q] -= v[img, q] / d[img, q] * (d[img, q] - (PAIR_END - 5e-4))
    frame = type(atoms)(numbers=z, positions=pos, cell=cell, pbc=True)
    P.clear_of_discontinuities(basis, frame)
    return basis, frame, i, j, m, q


@pytest.fixture(scope="module")
def terms():
    """The swap (i, j) of ``_edge_frame`` as the fp64 entry's own terms: dict(t: the records as a dict of columns, sign: +1 for
    the new species' pass and -1 for the old, T: the two atoms, m, q: the far centre and the far pair partner, ref: (dE_x, M),
    E: the frame's energy)."""
    basis, atoms, i, j, m, q = _edge_frame()
    ob, coeff = O.OracleBasis(basis), P.coefficients(basis)
    dE_x, M = O.mc_delta_x(ob, atoms, coeff, [i], [j], "swap")
    dE64, M64, rec = O.mc_terms_x(ob, atoms, coeff, i, j, "swap")
    t = {f: rec[:, k] for k, f in enumerate(O.MC_TERM_FIELDS)}
    e = O.evaluate(ob, atoms, coeff, forces=False)[0]
    return {"t": t, "sign": np.where(t["pass"] == 1, 1.0, -1.0), "T": (i, j), "m": m, "q": q, "ref": (dE_x[0], M[0]), "E": e,
            "dE64": dE64, "z": np.asarray(atoms.get_atomic_numbers())}


def _host_sum(terms, value=None, weight=None):
    """the move's energy difference as an fp64 NumPy sum of its terms (optionally with changed values or weights)"""
    v = terms["t"]["value"] if value is None else value
    w = terms["sign"] if weight is None else weight
    return float(np.sum(w * v))


def _same_triplet(t, q):
    """the records of both passes that hold the triplet of record q: the same centre and the same three lengths (the legs l and
    m may change places between the passes, with the species)"""
    lo, hi = np.minimum(t["r_ij"], t["r_ik"]), np.maximum(t["r_ij"], t["r_ik"])
    return np.flatnonzero((t["kind"] == 3) & (t["centre"] == t["centre"][q]) & (t["distance"] == t["distance"][q]) &
                          (lo == lo[q]) & (hi == hi[q]))


def _far_centre_triplet(terms):
    """the first triplet (new pass) of the far centre m: it holds the leg (m, i) that ends 2e-4 A inside the leg's range"""
    t, (i, j) = terms["t"], terms["T"]
    own = np.flatnonzero((t["kind"] == 3) & (t["pass"] == 1) & (t["centre"] == terms["m"]))
    legs_to_T = np.concatenate([t["r_ij"][own][np.isin(t["p1"][own], (i, j))], t["r_ik"][own][np.isin(t["p2"][own], (i, j))]])
    assert len(own) and np.all(legs_to_T > LEG_END - 3e-4)    # (every touched term of m holds the long leg; j is no neighbour of m)
    return int(own[0])


def _defects(terms):
    """name -> the fp64 host sum with the defect planted.  Each is chosen by a rule on the geometry, never by its effect."""
    t, sign, (i, j), z = terms["t"], terms["sign"], terms["T"], terms["z"]
    out = {}
    # 1. one triplet of a far affected centre is missing (from both passes, as a kernel that skips it would)
    q = _far_centre_triplet(terms)
    w = sign.copy()
    w[_same_triplet(t, q)] = 0.0
    out["triplet of a far centre removed"] = _host_sum(terms, weight=w)
    # 2. weight 1 for 2 on the pair entry of i that lies nearest its r_max, its partner outside T: one of the two directed terms
    #    of that bond is missing
    from_i = (t["kind"] == 2) & (t["centre"] == i) & (t["p1"] != i) & (t["p1"] != j)
    d_far = np.where(from_i, t["distance"], -1.0).max()
    assert PAIR_END - 6e-4 < d_far < PAIR_END - 4e-4 and np.all(t["p1"][from_i & (t["distance"] == d_far)] == terms["q"])
    w = sign.copy()
    w[from_i & (t["distance"] == d_far)] = 0.0
    assert np.sum(from_i & (t["distance"] == d_far)) == 2                            # one record a pass
    out["weight 1 for 2 on a pair entry near r_max"] = _host_sum(terms, weight=w)
    # 3. legs l and m exchanged on the triplet of centre i whose partners have equal species and whose centre legs differ most
    same = (t["kind"] == 3) & (t["centre"] == i) & (t["pass"] == 1) & (z[t["p1"].astype(int)] == z[t["p2"].astype(int)]) \
        & (t["p1"] != j) & (t["p2"] != j)
    q = int(np.argmax(np.where(same, np.abs(t["r_ij"] - t["r_ik"]), -1.0)))
    v = t["value"].copy()
    both = _same_triplet(t, q)
    v[both] = t["legs_exchanged"][both]
    out["l and m legs exchanged, equal partner species"] = _host_sum(terms, value=v)
    # 4. the far centre of 1. counted twice: all its touched triplets once more
    far = t["centre"][_far_centre_triplet(terms)]
    w = sign.copy()
    w[(t["kind"] == 3) & (t["centre"] == far)] *= 2.0
    out["a far centre counted twice"] = _host_sum(terms, weight=w)
    # 5. one leg length through fp32: the triplet of centre i with the shortest l leg (its strongest bond), in both passes
    own = (t["kind"] == 3) & (t["centre"] == i) & (t["pass"] == 1)
    q = int(np.argmin(np.where(own, t["r_ij"], np.inf)))
    v = t["value"].copy()
    both = _same_triplet(t, q)
    v[both] = t["leg_fp32"][both]
    out["one leg length through fp32"] = _host_sum(terms, value=v)
    return out


# Whether the bound reads each planted defect above GAMMA, recorded as found (never tuned); the figures of 2026-10-20:
#   weight 1 for 2 on the pair entry near r_max    changes dE by 6.7e-12 eV, ratio 218     seen
#   the far centre counted twice                   4.4e-12 eV, ratio 143                   seen
#   one leg length through fp32                    3.5e-09 eV, ratio 1.1e5                 seen
#   one triplet of the far centre removed          1.2e-14 eV, ratio 0.40                  NOT seen
#   l and m legs exchanged, equal partner species  0 eV, ratio of the clean sum            NOT seen
# The lone triplet is not seen because it is smaller than u M itself (1.3e-13 eV here): with its leg 2e-4 A inside the range it
# carries 2e-10 of an ordinary term, below the rounding of ANY fp64 sum of the move's terms, so no test of dE can miss it to the
# chain's harm either; the thirteen touched triplets of the same centre together (counted twice) are seen.  The exchanged legs
# cannot be seen by any bound on dE: a trio whose two neighbour species are equal has legs l and m on the same knots and a
# coefficient grid that is symmetric in them (the basis folds it so: symmetry 2), so the exchanged triplet has the same value.
# mc_delta's "lower (species, supercell index) is leg l" is therefore not observable through dE where the species are equal;
# where they differ, an exchange selects another trio and is seen like any wrong term.
SEEN = {"triplet of a far centre removed": False, "weight 1 for 2 on a pair entry near r_max": True,
        "l and m legs exchanged, equal partner species": False, "a far centre counted twice": True,
        "one leg length through fp32": True}


def test_host_sum_of_the_terms_is_within_the_bound(terms):
    """the fp64 NumPy sum of the entry's own terms (another order of additions than the entry's) lies within GAMMA u M, and
    the records are complete: they sum to the entry's dE"""
    dE_x, M = terms["ref"]
    r = P.ratio(_host_sum(terms), dE_x, M)
    print(f"[precision] fp64 host sum of {len(terms['sign'])} terms, edge_frame: dE {r:.3g}")
    assert r <= P.GAMMA["dE"]
    assert abs(_host_sum(terms) - terms["dE64"]) <= P.GAMMA["dE"] * U * M
    assert set(np.unique(terms["t"]["kind"])) == {1.0, 2.0, 3.0}
    assert np.isclose(np.sum(terms["t"]["magnitude"]), M, rtol=1e-12, atol=0.0)


def test_planted_defects_hide_below_1e_9_and_read_above_gamma(terms):
    """Each defect changes dE by less than 1e-9 max(1, |E_frame|) -- no Monte Carlo parity test could see it -- and, but for
    the two explained at SEEN (the lone triplet, 1.2e-14 eV at ratio 0.40; the exchanged legs, exactly 0), reads above
    GAMMA["dE"]."""
    dE_x, M = terms["ref"]
    clean = _host_sum(terms)
    loose = LOOSE * max(1.0, abs(terms["E"]))
    seen, change = {}, {}
    for name, bad in _defects(terms).items():
        r = P.ratio(bad, dE_x, M)
        seen[name] = r > P.GAMMA["dE"]
        print(f"[precision] planted mc_delta defect, {name}: changes dE by {abs(bad - clean):.3e} (1e-9 tolerance {loose:.1e}), "
              f"ratio {r:.4g} (GAMMA {P.GAMMA['dE']:g}): {'seen' if seen[name] else 'NOT seen'}")
        change[name] = abs(bad - clean)
    assert all(c < loose for c in change.values()), (change, loose)
    assert seen == SEEN, seen
