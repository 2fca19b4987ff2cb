"""The bases and frames of tests/_on_knots.py do what tests/test_gpu_on_knots.py needs of them: every distance that comes near a
knot is exact in every formulation, every knot of every sequence is met, the untrimmed leading edge is a jump of order one in
the oracle's rows, and the references that test holds the kernels to agree with each other there.  No GPU.

Bounds between the references, as in tests/test_uneven_legs_host.py: 1e-11 of the quantity's largest magnitude (fp64 sums taken
in different orders, two independent B-spline codes); differences of forces 1e-6 of the largest entry.  On a knot the energy's
third derivative jumps by J, and a central difference of forces with step h carries J h / 4 on top of the h^2 term: the
differences are taken at h and h / 2 and extrapolated (2 D(h / 2) - D(h)), which removes the term linear in h."""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
import _flux_ref as FR
import _harmonic_ref as HR
import _on_knots as K
import _site_rows_ref as SR
from _util import tensor_to_voigt

RTOL = 1e-11                 # tests/test_uneven_legs_host.py
FD_TOL = 1e-6                # tests/test_uneven_legs_host.py
REACH = 8.0


@functools.lru_cache(maxsize=None)
def _ob(name):
    return O.OracleBasis(K.basis(name))


def _coeff(name):
    return K.coefficients(K.basis(name))


def _all_frames(name):
    return K.probe_frames(name) + K.crystals(name) + K.small_frames(name)[:1] + K.small_frames(name)[2:]


# ------------------------------------------------------------------------------------------------ 1. exactness
def _fl(x):
    return Fraction(float(x))            # (Fraction -> float rounds to nearest: one rounding of the exact value)


def _roots(d):
    """r of the exact difference vector d (three doubles) by the unfused sum in cdist's order, by fused sums in two orders, and
    the exact root if it is a double (else None)"""
    x, y, z = (Fraction(float(c)) for c in d)
    unfused = float(np.sqrt(float(_fl(_fl(_fl(x * x) + _fl(y * y)) + _fl(z * z)))))
    fused_a = float(np.sqrt(float(_fl(z * z + _fl(y * y + _fl(x * x))))))
    fused_b = float(np.sqrt(float(_fl(x * x + _fl(y * y + _fl(z * z))))))
    s = x * x + y * y + z * z
    num, den = s.numerator, s.denominator
    exact = None
    rn, rd = math.isqrt(num), math.isqrt(den)
    if rn * rn == num and rd * rd == den and Fraction(float(Fraction(rn, rd))) == Fraction(rn, rd):
        exact = float(Fraction(rn, rd))
    return unfused, fused_a, fused_b, exact


def _sum_is_exact(a, b):
    """a + b carries no rounding error, entry by entry (Knuth's TwoSum: the error term of a double addition, itself exact)"""
    s = a + b
    bb = s - a
    return ((a - (s - bb)) + (b - bb)) == 0.0


def _neighbour_differences(atoms):
    """Every difference p_j + shift - p_i within REACH, over all images, as (sorted |components| [U, 3] without repeats, how
    often each occurs); asserts on the way that the float arithmetic forms each of them without rounding, whichever way the
    image shift is applied."""
    pos = np.asarray(atoms.get_positions(), dtype=float)
    edge = np.diag(np.asarray(atoms.get_cell(), dtype=float))
    pj, pi = pos[None, :, :], pos[:, None, :]
    d0 = pj - pi
    if np.all(edge >= 2 * REACH):                                        # one image of j can be within reach of i: the nearest
        shifts = [-edge * np.round(d0 / edge)]
    else:
        n_img = [int(np.ceil(REACH / e)) for e in edge]
        shifts = [np.array(m, dtype=float) * edge + 0.0 * d0 for m in itertools.product(*[range(-m, m + 1) for m in n_img])]
    found = []
    for s in shifts:
        a = d0 + s                                                       # (p_j - p_i) + s
        up = pj + s
        b = up - pi                                                      # (p_j + s) - p_i
        r = np.sqrt((a * a).sum(axis=2))
        near = (r < REACH) & (r > 0)
        exact = (_sum_is_exact(pj, -pi) & _sum_is_exact(d0, s) & _sum_is_exact(pj, s) & _sum_is_exact(up, -pi)).all(axis=2)
        assert np.all(exact[near]) and np.array_equal(a[near], b[near])
        found.append(np.sort(np.abs(a[near]), axis=1))
    return np.unique(np.concatenate(found), axis=0, return_counts=True)


@pytest.mark.parametrize("name", K.BASES)
def test_exactness(name):
    """Every neighbour difference within 8 A is computed without rounding, whichever way the image shift is applied -- so the
    difference of two centre-relative vectors is the direct difference too (a triplet's r_jk is at most 7 A) -- and its length
    is either an exactly representable root that the unfused and the fused sums both return, or more than 1e-3 from every knot."""
    knots = K.all_knots(K.basis(name))
    checked = {}
    n_exact = n_clear = 0
    for atoms in _all_frames(name):
        for d, count in zip(*_neighbour_differences(atoms)):
            key = tuple(float(c) for c in d)
            if key not in checked:
                unfused, fused_a, fused_b, exact = _roots(d)
                near = float(np.min(np.abs(knots - unfused))) <= K.CLEAR
                if near:
                    assert exact is not None and unfused == fused_a == fused_b == exact, (key, unfused, fused_a, fused_b, exact)
                checked[key] = near
            n_exact += int(count) * checked[key]
            n_clear += int(count) * (not checked[key])
    print(f"{name}: {n_exact} neighbour differences on or within 2 DELTA of a knot (all exact), {n_clear} clear of every knot")
    assert n_exact > 0 and n_clear > 0


# ------------------------------------------------------------------------------------------------ 2. coverage
def _probe_legs(name, chunk, k):
    """exact squared lengths (Fractions) of the legs of probe k as its frame holds it: pairs (r,), triplets (r_ij, r_ik, r_jk)"""
    atoms = K.probe_frames(name)[chunk]
    pos = np.asarray(atoms.get_positions(), dtype=float)
    edge = float(np.asarray(atoms.get_cell())[0, 0])
    idx = K.probe_atoms(name, chunk, k)

    def d2(a, b):
        out = Fraction(0)
        for c in range(3):
            d = Fraction(float(pos[b, c])) - Fraction(float(pos[a, c]))
            d -= Fraction(edge) * round(d / Fraction(edge))
            out += d * d
        return out
    if len(idx) == 2:
        return (d2(idx[0], idx[1]),)
    return d2(idx[0], idx[1]), d2(idx[0], idx[2]), d2(idx[1], idx[2])


@pytest.mark.parametrize("name", K.BASES)
def test_coverage(name):
    """Every distinct knot of every pair sequence and of every leg of every trio -- r_min2, r_max2, each trio's own t0 and tlast
    among them -- is met at q = -1, 0, +1 by a probe whose stored coordinates give that leg exactly knot + q DELTA and whose
    other two legs lie strictly inside their supports.  The one exception is geometry: a leg-n knot at or beyond tlast_l +
    tlast_m closes no triangle with shorter centre legs; it is met by the collinear probe with both centre legs on their last
    knots."""
    b = K.basis(name)
    met = set()
    through_a_face = 0
    for chunk, plist in enumerate(K.probe_chunks(name)):
        frame = K.probe_frames(name)[chunk]
        assert len(frame) <= 1500
        z = np.asarray(frame.get_atomic_numbers())
        pos = np.asarray(frame.get_positions())
        for k, pr in enumerate(plist):
            kind, inter, leg, t, q = pr.hit
            idx = K.probe_atoms(name, chunk, k)
            assert tuple(z[idx]) == pr.z
            through_a_face += bool(np.ptp(pos[idx], axis=0).max() > 0.5 * K.EDGE and kind in ("leg", "collinear") and q in (-1, 0, 1))
            if kind not in ("pair", "leg", "collinear"):
                continue
            legs2 = _probe_legs(name, chunk, k)
            target = Fraction(float(t)) + q * Fraction(K.DELTA)
            if kind == "pair":
                assert legs2[0] == target * target, pr
                met.add((inter, None, t, q))
                continue
            seqs = [np.asarray(s, dtype=float) for s in b.knots_map[inter]]
            r = [float(np.sqrt(float(v))) for v in legs2]
            if kind == "leg":
                assert legs2[leg] == target * target, pr
                others = [x for x in range(3) if x != leg]
                assert all(seqs[x][0] < r[x] < seqs[x][-1] for x in others), (pr, r)
                assert all(np.min(np.abs(seqs[x] - r[x])) > K.CLEAR for x in others), (pr, r)
                met.add((inter, leg, t, q))
                if leg == 0 and inter[1] == inter[2] and np.array_equal(seqs[0], seqs[1]):
                    met.add((inter, 1, t, q))                              # (one sequence, one species: either neighbour)
            elif legs2[2] == target * target and t >= seqs[0][-1] + seqs[1][-1]:
                assert r[0] == seqs[0][-1] + (q * K.DELTA) and r[1] == seqs[1][-1]
                met.add((inter, 2, t, q))
    n = 0
    for key, seq in K.sequences(b).items():
        inter, leg = (key, None) if leg_free(key) else key
        for t in np.unique(seq):
            for q in (-1, 0, 1):
                assert (inter, leg, float(t), q) in met, (name, inter, leg, t, q)
                n += 1
    print(f"{name}: {n} (sequence, knot, q) cases met, the {2 * len(K.sequences(b))} sequence ends among them; "
          f"{through_a_face} on-knot triplets meet through a cell face")
    assert through_a_face >= 10


def leg_free(key):
    """a pair's key"""
    return len(key) == 2 and isinstance(key[0], str)


# ------------------------------------------------------------------------------------------------ 3. the probes bite
def _row_move(name, hit0):
    """largest change of any column of the oracle's energy row when the probe made for ``hit0`` (q = 0) goes to q = +1"""
    ps = {p.hit: p for p in K.probes(name)}
    rows = [O.featurize(_ob(name), K.single_probe_frame(ps[hit0[:4] + (q,)]), forces=False)["xe"] for q in (0, 1)]
    return float(np.abs(rows[1] - rows[0]).max())


@pytest.mark.parametrize("name", K.BASES)
def test_the_probes_bite(name):
    """Across one DELTA: a pair at r_min2 (leading trim 0 on every basis) and, with lead3 = 0, a triplet whose r_jk crosses leg
    n's first knot or whose r_ij crosses the trio's own first knot of leg l (on grid_binary: above the list's r_min3) move a
    column of the oracle's energy row by at least 1 where the three atoms are of one species (and by at least 0.5 where only
    one of them is a centre of that trio); with lead3 = 3 the same triplets move it by less than 1e-9."""
    b = K.basis(name)
    for p in b.interactions_map[2]:
        move = _row_move(name, ("pair", p, None, float(b.knots_map[p][0]), 0))
        print(f"{name} pair {p} across r_min2: {move:.3g}")
        assert move >= 1.0
    rmin3 = min(float(b.knots_map[t][0][0]) for t in b.interactions_map[3])
    own = 0
    for t in b.interactions_map[3]:
        # one species: the three atoms are centres of one trio and feed one column, 3 x 0.82^2; else one centre does, 0.82^2
        floor = 1.0 if len(set(t)) == 1 else 0.5
        for leg in (2, 0):
            t0 = float(b.knots_map[t][leg][0])
            move = _row_move(name, ("bite", t, leg, t0, 0))
            bound = f"at least {floor}" if K.lead3(name) == 0 else "below 1e-9"
            print(f"{name} trio {t} leg {'lmn'[leg]} across its first knot {t0}: {move:.3g} ({bound})")
            assert (move >= floor) if K.lead3(name) == 0 else (move < 1e-9), (t, leg, move)
            own += leg == 0 and t0 > rmin3 and floor == 1.0
    if name == "grid_binary":
        assert own >= 1                          # (W-W-W: its legs l, m begin at 1.75, the list at 1.5)
        assert any(float(b.knots_map[t][0][-1]) < max(float(b.knots_map[u][q][-1]) for u in b.interactions_map[3] for q in (0, 1))
                   for t in b.interactions_map[3])


# ------------------------------------------------------------------------------------------------ 4. the references agree
@pytest.mark.parametrize("name,which", K.SMALL_CASES)
def test_references_agree_on_energy_forces_virial_and_rows(name, which):
    """_flux_ref's site terms and term forces, _site_rows_ref's rows and _harmonic_ref's Hessian against the oracle on the small
    probe frame (0), the 16-atom crystal (1) and, with one species, that crystal with a vacancy (2)."""
    ob, coeff = _ob(name), _coeff(name)
    a = K.small_frames(name)[which]
    n = len(a)
    assert n <= 36
    e_o, f_o, v_o = O.evaluate(ob, a, coeff, virial=True)
    Us, W = FR.site_terms(ob, a, coeff)
    assert abs(Us.sum() - e_o) <= RTOL * max(1.0, np.abs(Us).sum())
    Ws = W.sum(axis=0)
    assert np.abs(tensor_to_voigt(0.5 * (Ws + Ws.T)) - v_o).max() <= RTOL * np.abs(v_o).max()
    f_t = FR.term_forces(ob, a, coeff)
    scale = np.abs(f_t).max()                                       # (tests/test_uneven_legs_host.py)
    if which == 1 and K.forces_vanish(name, 0):
        # the perfect one-species crystal alone: every force is a sum of terms that cancel, relative to the largest sum of their sizes
        size = np.zeros(n)
        for i, _, slots in FR.terms(ob, a, coeff)[1]:
            for p, _, g in slots:
                size[p] += np.abs(g).max()
                size[i] += np.abs(g).max()
        assert scale < 1e-12 * size.max()
        scale = size.max()
    assert np.abs(f_o - f_t).max() <= RTOL * scale
    B = SR.site_rows(ob, a, K.basis(name).n_feats)
    assert np.abs(B @ coeff - Us).max() <= RTOL * np.abs(Us).max()
    x_e = O.featurize(ob, a, forces=False)["xe"]
    live = np.setdiff1d(np.arange(len(x_e)), np.asarray(K.basis(name).col_idx, dtype=int))
    assert np.abs(B.sum(axis=0) - x_e)[live].max() <= RTOL * np.abs(x_e).max()
    H, L, Bn = HR.hessian(ob, a, coeff)
    scale = np.abs(H).max()
    assert scale > 0 and np.abs(H - H.T).max() <= RTOL * scale
    assert np.abs(H.reshape(3 * n, n, 3).sum(axis=1)).max() <= RTOL * scale * n          # (a rigid shift moves no force)
    print(f"{name} frame {which}: {n} atoms, E = {e_o:.6f}, max |F| = {np.abs(f_o).max():.3e}, max |H| = {scale:.3e}")


@pytest.mark.parametrize("name", K.BASES)
def test_restated_hessian_is_the_derivative_of_the_oracle_s_forces_on_knots(name):
    """four atoms of the crystal (1 x 1 x 2 cells, a = 3.0: every atom neighbours its own images, shells on knots)"""
    ob, coeff = _ob(name), _coeff(name)
    a = K._crystal("bcc", 3.0, (1, 1, 2), K.numbers_of(name), 64)
    n = len(a)
    H = HR.hessian(ob, a, coeff)[0]
    pos = np.asarray(a.get_positions(), dtype=float)

    def diff(h):
        D = np.zeros((3 * n, 3 * n))
        for k in range(3 * n):
            f_pm = []
            for sgn in (1, -1):
                p = pos.copy()
                p[k // 3, k % 3] += sgn * h
                f_pm.append(O.evaluate(ob, K.displaced(a, p), coeff)[1].ravel())
            D[:, k] = -(f_pm[0] - f_pm[1]) / (2 * h)
        return D
    Hfd = 2.0 * diff(1e-5) - diff(2e-5)
    err = np.abs(H - Hfd).max() / np.abs(H).max()
    print(f"{name}: restated Hessian against extrapolated differences of the oracle's forces {err:.2e}")
    assert err <= FD_TOL


LEAD0_BASES = [name for name in K.BASES if K.lead3(name) == 0]


@pytest.mark.parametrize("name", LEAD0_BASES)
def test_restated_hessian_counts_a_triplet_one_step_inside_its_first_knot(name):
    """_harmonic_ref's masks against the oracle where it matters: one probe alone with r_jk = t0_n + 2^-42 A, the other legs 1/64 A
    above their first knots, leading trim 0.  The triplet's term is of order one and exists on this side only, so differences
    cannot straddle the point: the column of H for moving k along j -> k (r_jk grows, the term stays) is held to the second-order
    one-sided difference (-3 f(0) + 4 f(h) - f(2 h)) / 2 h of the oracle's forces, h = 2e-5, within the 1e-6 of the largest entry
    that tests/test_uneven_legs_host.py gives differences of forces (the h^2 term and eps |f| / h are both far below it).  The
    restatement of the probe at q = 0 leaves the triplet out, as it must; held to the same differences it is off by order one,
    which is asserted too: a restatement with the mask on the wrong side would not pass."""
    b = K.basis(name)
    ob, coeff = _ob(name), _coeff(name)
    trio = b.interactions_map[3][0]
    by_hit = {p.hit: p for p in K.probes(name)}
    t0 = float(b.knots_map[trio][2][0])
    inside, on = (K.single_probe_frame(by_hit[("bite", trio, 2, t0, q)]) for q in (1, 0))
    pos = np.asarray(inside.get_positions(), dtype=float)
    d = pos[2] - pos[1]
    axis = int(np.argmax(np.abs(d)))
    assert np.count_nonzero(d) == 1 and d[axis] == t0 + K.DELTA          # (j -> k lies along an axis, one step inside)
    h = 2e-5
    f = []
    for m in range(3):
        p = pos.copy()
        p[2, axis] += m * h
        f.append(O.evaluate(ob, K.displaced(inside, p), coeff)[1].ravel())
    column = -(-3.0 * f[0] + 4.0 * f[1] - f[2]) / (2 * h)
    H_in, H_on = (HR.hessian(ob, a, coeff)[0] for a in (inside, on))
    err = np.abs(H_in[:, 6 + axis] - column).max() / np.abs(H_in).max()
    off = np.abs(H_on[:, 6 + axis] - column).max() / np.abs(H_in).max()
    print(f"{name}: H column one step inside t0 against one-sided differences {err:.2e} (bound {FD_TOL:.0e}); "
          f"the q = 0 restatement, which leaves the triplet out, is {off:.2e} off")
    assert err <= FD_TOL and off > 1e-3


def test_a_swap_s_energy_difference_follows_the_site_terms_on_the_small_frames():
    """What tests/test_gpu_on_knots.py holds mc.delta_energy to is the difference of two oracle energies.  Here one swap of unlike
    atoms on each of grid_binary's small frames, which moves triplets across the trios' own leg ends, is held to the difference
    of _flux_ref's site-term sums.  (_mc_ref itself has no energies of its own: it is driven by whatever energies it is given.)"""
    name = "grid_binary"
    ob, coeff = _ob(name), _coeff(name)
    zs = np.array(K.numbers_of(name))
    for a in K.small_frames(name):
        z = np.asarray(a.get_atomic_numbers())
        i, j = int(np.flatnonzero(z == zs[0])[0]), int(np.flatnonzero(z == zs[1])[0])
        zz = z.copy()
        zz[i], zz[j] = z[j], z[i]
        after = K.with_numbers(a, zz)
        e0 = O.evaluate(ob, a, coeff, forces=False)[0]
        de_o = O.evaluate(ob, after, coeff, forces=False)[0] - e0
        de_t = FR.site_terms(ob, after, coeff)[0].sum() - FR.site_terms(ob, a, coeff)[0].sum()
        assert abs(de_o) > 1e-6 and abs(de_o - de_t) <= RTOL * max(1.0, abs(e0))
