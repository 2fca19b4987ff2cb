"""
The extended-precision harness: feature rows, energies, forces and strain derivatives against the oracle's extended build
(``oracle/libuf3oracle_x.so``: the oracle's own source with ``long double`` values and fp64 decisions), entry by entry, in units
of the entry's own first-order error bound.

``ratio(got, truth, M)`` is ``max |got - truth| / (u M)`` with ``u = 2**-53`` and M the magnitude the extended oracle returns
beside every entry (uf3_oracle.c: the sum over the entry's terms of the term with absolute values taken wherever it takes signs,
plus its sensitivity to a relative rounding of each of its distances).  No entry is left out; an entry whose M is 0 has no
term at all and must be exactly 0.

The bound.  ``RHO_O`` records, per kind of output, the worst ratio of the **fp64 oracle** against the extended one over
``CASES`` -- measured on the CPU, kept honest by tests/test_precision_host.py.  A device result passes at
``GAMMA[kind] = 16 max(rho_o, 1)``: the margin of 16 covers what the kernels legitimately do differently from Cox-de Boor on
tiled positions (local cubic pieces, FMA contraction, ``fast_rcp`` and ``norm3_leg`` at about an ulp each, another order of
summation), each a bounded number of extra roundings per term.  The bound is never derived from a device result.

The second-derivative and per-centre kinds -- ``H``, ``mixed``, ``born`` (k_hessian; ``oracle.hessian_x``), ``U``, ``W``, ``jp``
(k_flux_site_terms; ``oracle.site_terms_x``) and ``b`` (k_site_rows; ``oracle.site_rows_x``) -- are held in the same way, by the
same rule: ``reference(name)`` computes them on first use.  Those three kernels describe the frame with every atom counted as
its image inside the cell, and so do these oracle entries (``oracle.supercell_radius``).

Monte Carlo energy differences -- kind ``dE`` (mc_delta through k_mc_delta and k_mc_trials; ``oracle.mc_delta_x``) -- have
cases and moves of their own (``mc_cases``, ``mc_moves``, ``mc_reference`` at the end of this file) and the same rule.

One documented design choice is not a bounded number of roundings per term: the launches that evaluate leg functions from
local cubic pieces in powers of ``x - t_i`` (k_featurize3, the grouped matrix-core launch) carry Horner's absolute error on
values that are themselves tiny.  For those routes alone M is the oracle's widened one (``ratios(..., pieces=True)``;
uf3_oracle.c: piece_abs holds the derivation); GAMMA is the same.
"""
import functools
import json

import numpy as np

from oracle import oracle as O
from uf3_amd import synthetic
from uf3_amd.data import composition
from uf3_amd.data.atoms import Atoms
from uf3_amd.representation import bspline
from _on_knots import coefficients
from _util import SPECIES_CASES, basis_from_meta, load_case
from test_feat3_pad_clamp import CELLS, ELEMENTS, _basis as clamp_basis, _frame as clamp_frame

U = np.longdouble(2.0) ** -53
KINDS = ("xe", "xf", "xv", "e", "f", "v")        # energy rows, force rows, virial rows; energies, forces, virials
# Hessian, mixed position / strain derivatives, clamped-ion strain term; site energies, site virials, each centre's share of J_pot;
# site rows
KINDS_D2 = ("H", "mixed", "born", "U", "W", "jp", "b")

# Worst ratio of the fp64 oracle (libuf3oracle.so) against the extended build over CASES, per kind, as printed by
# tests/test_precision_host.py::test_fp64_oracle_stays_within_the_recorded_table.  Measured 2026-10-20 (x86-64, gcc -O2
# -ffp-contract=off, 80-bit long double): xe 1.33, xf 1.77, xv 1.35, e 0.529, f 0.252, v 0.349 -- recorded rounded up.
RHO_O = {"xe": 1.5, "xf": 2.0, "xv": 1.5, "e": 0.6, "f": 0.3, "v": 0.4}
# The same for KINDS_D2, as printed by tests/test_precision_host.py::test_fp64_oracle_stays_within_the_recorded_table_d2.
# Measured 2026-10-20 (the same build): H 0.968, mixed 0.308, born 0.243, U 0.175, W 0.378, jp 0.253, b 1.66 -- recorded rounded up.
RHO_O.update({"H": 1.0, "mixed": 0.4, "born": 0.3, "U": 0.2, "W": 0.4, "jp": 0.3, "b": 2.0})
GAMMA = {k: 16.0 * max(v, 1.0) for k, v in RHO_O.items()}


def ratio(got, truth, M):
    """max |got - truth| / (u M) over ALL entries, in np.longdouble.  Where M == 0 no term reaches the entry: ``got`` must be
    exactly zero there (asserted), and the entry counts with ratio 0."""
    got = np.asarray(got, dtype=np.longdouble)
    truth = np.asarray(truth, dtype=np.longdouble)
    M = np.asarray(M, dtype=np.longdouble)
    assert got.shape == truth.shape == M.shape, (got.shape, truth.shape, M.shape)
    assert np.all(np.isfinite(got)) and np.all(M >= 0)
    none = M == 0
    assert not np.any(got[none]), "an entry no term reaches is not exactly zero"
    if not got.size:
        return 0.0
    err = np.abs(got - truth)
    return float((np.where(none, 0, err) / np.where(none, 1, U * M)).max())


# ------------------------------------------------------------------------------------------------ frames clear of steps
def clear_of_discontinuities(basis, atoms, eps=1e-9, second=False):
    """No distance of the frame lies within ``eps`` of a point where the rows are discontinuous in it: a pair ``r_min`` or
    ``r_max``, the ends of the 3-body list range, and an end of a leg (centre legs and ``r_jk``) whose kept functions do not
    vanish there -- an untrimmed leading end, or a trailing end trimmed by fewer than 3.  (Interior knots need no clearance: a
    cubic spline is C2 there.)  ``second``: for the second-derivative kinds (H, mixed, born) a leg end is a step wherever a kept
    function's SECOND derivative does not vanish there: a leading or a trailing end trimmed by fewer than 3 (at an end knot of
    multiplicity 4 the q-th function from the end vanishes like the q-th power of the distance from it).  A pair ``r_max``
    trimmed by 3 is no step for them either; ``r_min`` and ``r_max`` are cleared as steps in any case.
    Returns the smallest clearance found; raises AssertionError otherwise."""
    ob = O.OracleBasis(basis)
    pos, _, _ = O.supercell(atoms, basis.r_cut)
    n = len(atoms)
    d = np.linalg.norm(pos[None, :, :] - pos[:n, None, :], axis=-1)
    pair_d = d[d > 0]
    steps2 = sorted({max(float(v), 0.0) for v in ob.pair_rmin} | {float(v) for v in ob.pair_rmax})
    clear = min([np.abs(pair_d - s).min() for s in steps2] + [np.inf]) if pair_d.size else np.inf
    assert clear > eps, ("pair distance at a pair cut-off", clear)
    if basis.degree < 3 or not ob.trios:
        return float(clear)
    seqs = [[np.asarray(k, float) for k in basis.knots_map[t]] for t in ob.trios]
    rmin3 = max(min(k.min() for ks in seqs for k in ks), 0.0)
    rmax3 = max(k.max() for ks in seqs for k in ks[:2])
    c = min(np.abs(pair_d - rmin3).min(), np.abs(pair_d - rmax3).min())
    assert c > eps, ("distance at an end of the 3-body list range", c)
    clear = min(clear, c)
    lead, trail = int(basis.leading_trim[3]), int(basis.trailing_trim[3])
    ends = set()
    for ks in seqs:
        for k in ks:
            if lead == 0 or (second and lead < 3):
                ends.add(float(k[0]))
            if trail < 3:
                ends.add(float(k[-1]))
    if not ends:
        return float(clear)
    legs = [pair_d[pair_d <= rmax3 * (1 + 1e-6)]]
    for i in range(n):
        nb = np.flatnonzero((d[i] > 0) & (d[i] <= rmax3 * (1 + 1e-6)))
        if len(nb) > 1:
            x = pos[nb]
            legs.append(np.linalg.norm(x[:, None] - x[None], axis=-1)[np.triu_indices(len(nb), 1)])
    legs = np.concatenate(legs)
    c = min(np.abs(legs - e).min() for e in ends)
    assert c > eps, ("leg at an end whose kept functions do not vanish", c)
    return float(min(clear, c))


# ------------------------------------------------------------------------------------------------ the cases
def _uneven_basis(lead):
    """the knot sequences of test_bond_factorised_launch_with_non_uniform_knot_sequences (tests/test_gpu_parity.py)"""
    def clamped(lo, hi, n_int, power):
        inner = lo + (hi - lo) * np.linspace(0.0, 1.0, n_int + 1) ** power
        return np.concatenate([[lo] * 3, inner, [hi] * 3])

    cs = composition.ChemicalSystem(['Mo', 'W'], 3)
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    knots = {p: clamped(0.001, 5.5, 15, 1.3) for p in pairs}
    for t in trios:
        knots[t] = [clamped(1.5, 3.5, 6, 1.5), clamped(1.5, 7.0, 12, 0.75)]
    return bspline.BSplineBasis(cs, knots_map=knots, leading_trim={2: 0, 3: lead}, trailing_trim={2: 3, 3: 3})


def _resolution_basis(res3, elements=('Mo', 'W')):
    """kept windows of (res - 3) bins a centre leg: [5, 5, 10] -> 2 x 2 x 7, [7, 7, 14] -> 4 x 4 x 11 (two rounds of positions),
    [8, 8, 16] -> 5 x 5 x 13 (three)"""
    cs = composition.ChemicalSystem(list(elements), 3)
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    return bspline.BSplineBasis(
        cs, r_min_map={**{p: 0.001 for p in pairs}, **{t: [1.5, 1.5, 1.5] for t in trios}},
        r_max_map={**{p: 5.5 for p in pairs}, **{t: [3.5, 3.5, 7.0] for t in trios}},
        resolution_map={**{p: 15 for p in pairs}, **{t: list(res3) for t in trios}},
        leading_trim={2: 0, 3: 3}, trailing_trim={2: 3, 3: 3})


def _mixed_boundary_frames():
    """the cluster, the slab with atoms outside its cell and the 3-atom triclinic cell thinner than the cut-off of
    test_ragged_batch_mixed_boundary_conditions (tests/test_gpu_parity.py), drawn as there"""
    rng = np.random.default_rng(3)
    cell = np.array([[4.1, 0.3, 0.0], [-0.5, 3.9, 0.2], [0.4, -0.3, 4.4]])
    cluster = Atoms(numbers=rng.choice([42, 74], 9), positions=rng.uniform(0, 5.5, (9, 3)))
    slab = Atoms(numbers=rng.choice([42, 74], 12), positions=rng.uniform(-1, 7, (12, 3)),
                 cell=np.diag([6.3, 6.9, 20.0]), pbc=[True, True, False])
    thin = Atoms(numbers=rng.choice([42, 74], 3), positions=rng.uniform(0, 4, (3, 3)), cell=cell, pbc=True)
    return cluster, slab, thin


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (basis, atoms, what the case is for): the smallest cells that reach every kernel instance.  Every frame is
    asserted clear of discontinuities where its reference is made (``reference``)."""
    out = {}
    for name, lattice, reps, a, numbers, seed, r3, _, cap in CELLS:
        if name in ("mow_cap16_r4", "mow_dilated_cap16"):          # (slot coverage of the pad clamp: the same instance)
            continue
        out[name] = (clamp_basis([ELEMENTS[z] for z in sorted(numbers)], r3), clamp_frame(lattice, reps, a, numbers, seed),
                     f"3 x 9 windows, list capacity {cap}")
    mow54 = clamp_frame("bcc", (3, 3, 3), 3.165, [42, 74], 300)
    out["mow_lead0"] = (clamp_basis(["Mo", "W"], 3.5, lead3=0), mow54, "6 x 12 windows, three rounds, F = 1798")
    out["mow_2x7"] = (_resolution_basis([5, 5, 10]), mow54, "2 x 7 windows (the reference's default 3-body resolution)")
    out["mow_4x11"] = (_resolution_basis([7, 7, 14]), mow54, "4 x 11 windows, two rounds")
    out["w_5x13"] = (_resolution_basis([8, 8, 16], ('W',)), clamp_frame("bcc", (3, 3, 3), 3.165, [74], 303),
                     "5 x 13 windows, three rounds")
    uneven = synthetic.lattice_frame("bcc", (3, 3, 4), 3.165, [42, 74], 87, rattle=0.15)
    out["uneven_lead3"] = (_uneven_basis(3), uneven, "uneven knot sequences")
    out["uneven_lead0"] = (_uneven_basis(0), uneven, "uneven knot sequences, no leading trim")
    _, meta, atoms = load_case("case_bcc24_s4")
    assert sorted(set(atoms.get_atomic_numbers().tolist())) == SPECIES_CASES["case_bcc24_s4"]
    out["bcc24_s4"] = (basis_from_meta(meta), atoms, "four species")
    _, meta, atoms = load_case("case_w16_sym3")             # (trimmed at both ends, as test_matrix_core_and_generic_trio_kernels_agree)
    meta = json.loads(json.dumps(meta))
    meta["basis_kwargs"]["leading_trim"], meta["basis_kwargs"]["trailing_trim"] = {"2": 0, "3": 3}, {"2": 3, "3": 3}
    out["w16_sym3"] = (basis_from_meta(meta), atoms, "three equal legs: the six-fold symmetry fold")
    cluster, slab, thin = _mixed_boundary_frames()
    lead0 = synthetic.notebook_basis(['Mo', 'W'], lead3=0)
    out["triclinic_thin"] = (lead0, thin, "3-atom triclinic cell thinner than the cut-off")
    out["slab_outside"] = (lead0, slab, "slab with atoms outside its cell")
    out["cluster"] = (lead0, cluster, "open cluster")
    return out


def velocities(name):
    """the seeded velocities [N, 3] (Angstrom / fs) the heat current of a case is taken at"""
    n = len(cases()[name][1])
    return np.random.default_rng(1000 + sorted(cases()).index(name)).normal(0.0, 0.01, (n, 3))


_D2_GROUPS = (("H", "mixed", "born"), ("U", "W", "jp"), ("b",))


def _d2(name, ob, coeff, kind, extended=True):
    """(values, magnitudes) of the group of KINDS_D2 that holds ``kind``, from the extended (or the fp64) oracle"""
    basis, atoms, _ = cases()[name]
    if kind in _D2_GROUPS[0]:
        return O.hessian_x(ob, atoms, coeff, strain=True, extended=extended)
    if kind in _D2_GROUPS[1]:
        val, mag = O.site_terms_x(ob, atoms, coeff, velocities(name), extended=extended)
        return {k: val[k] for k in _D2_GROUPS[1]}, {k: mag[k] for k in _D2_GROUPS[1]}
    val, mag = O.site_rows_x(ob, atoms, extended=extended)
    return {"b": val["b"]}, {"b": mag["b"]}


class _Lazy(dict):
    """values (or magnitudes) of a case: the keys of KINDS from the start, a group of KINDS_D2 computed when one of its keys is
    first asked for -- once per case, into both dicts, read-only"""

    def __init__(self, first, fill):
        super().__init__(first)
        self._fill = fill

    def __missing__(self, key):
        if key not in KINDS_D2:
            raise KeyError(key)
        self._fill(key)
        return dict.__getitem__(self, key)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(ob, coefficients, values, magnitudes) of a case from the extended oracle, computed once and shared (read-only): the keys
    of KINDS, rows from ``featurize_x(virial=True)``, e / f / v from ``evaluate_x``; and, computed on first use, the keys of
    KINDS_D2 from ``hessian_x``, ``site_terms_x`` (at ``velocities(name)``) and ``site_rows_x``.  ``magnitudes["pieces"]`` holds
    the row magnitudes widened for the routes that evaluate leg functions from local cubic pieces (``ratios(..., pieces=True)``)."""
    basis, atoms, _ = cases()[name]
    assert len(atoms) <= 130
    clear_of_discontinuities(basis, atoms)
    ob = O.OracleBasis(basis)
    coeff = coefficients(basis)
    val, mag = O.featurize_x(ob, atoms, virial=True)
    ev, em = O.evaluate_x(ob, atoms, coeff, virial=True)
    val.update(ev)
    mag.update(em)
    wide = O.featurize_x(ob, atoms, virial=True, pieces=True)[1]
    for k in ("xe", "xf", "xv"):
        assert np.all(wide[k] >= mag[k]) and np.array_equal(wide[k] == 0, mag[k] == 0)
    mag["pieces"] = wide
    for d in (val, mag, wide):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)

    def fill(kind):
        if kind in _D2_GROUPS[0]:
            clear_of_discontinuities(basis, atoms, second=True)
        v2, m2 = _d2(name, ob, coeff, kind)
        for k in v2:
            v2[k].setflags(write=False)
            m2[k].setflags(write=False)
            dict.__setitem__(val, k, v2[k])
            dict.__setitem__(mag, k, m2[k])

    val, mag = _Lazy(val, fill), _Lazy(mag, fill)
    return ob, coeff, val, mag


def fp64_oracle(name):
    """the fp64 build's results of a case, keys of KINDS (the virial rows from the fp64 build's own ``*_x`` entry)"""
    basis, atoms, _ = cases()[name]
    ob, coeff, _, _ = reference(name)
    rows = O.featurize(ob, atoms)
    e, f, v = O.evaluate(ob, atoms, coeff, virial=True)
    xv = O.featurize_x(ob, atoms, virial=True, extended=False)[0]
    assert np.array_equal(xv["xe"], rows["xe"]) and np.array_equal(xv["xf"], rows["xf"])
    return {"xe": rows["xe"], "xf": rows["xf"], "xv": xv["xv"], "e": e, "f": f, "v": v,
            "pair_cnt": xv["pair_cnt"], "n3_cnt": xv["n3_cnt"]}


def fp64_oracle_d2(name, kind):
    """the fp64 build's results of the group of KINDS_D2 that holds ``kind``"""
    ob, coeff, _, _ = reference(name)
    return _d2(name, ob, coeff, kind, extended=False)[0]


def ratios(got, name, kinds=None, pieces=False):
    """{kind: ratio} of the results ``got`` (a dict with keys of KINDS) of a case against its reference.  ``pieces``: the rows
    come from a route that evaluates the 3-body leg functions from local cubic pieces in powers of the distance from the
    interval's lower knot (k_featurize3, the grouped matrix-core launch), whose absolute error does not shrink with the
    value: M is the oracle's widened one (uf3_oracle.c: piece_abs).  Every other route is held to the plain M."""
    _, _, val, mag = reference(name)
    if pieces:
        mag = {**mag, **mag["pieces"]}
    return {k: ratio(got[k], val[k], mag[k]) for k in (kinds or KINDS + KINDS_D2) if k in got and got[k] is not None}


def fmt(r):
    return ", ".join(f"{k} {v:.3g}" for k, v in r.items())


# ================================================================================================ Monte Carlo energy differences
# kind "dE": mc_delta (uf3_mc.h, through k_mc_delta and k_mc_trials) against oracle.mc_delta_x.  M of a move is the sum of the
# magnitudes of the terms that contain a moved atom, over both species assignments (uf3_oracle.c: mc_worker holds the derivation);
# the terms the move leaves alone are in neither dE nor M.
#
# Worst ratio of the fp64 oracle entry against the extended one over every move of MC_CASES, both modes, as printed by
# tests/test_mc_precision_host.py::test_fp64_entry_stays_within_the_recorded_table.  Measured 2026-10-20 (x86-64, gcc -O2
# -ffp-contract=off, 80-bit long double): dE 0.169 (uneven_lead0, transmute) -- recorded rounded up.  It is far below 1 because M
# adds the magnitudes of several hundred terms as if their roundings all pointed one way, while the oracle's own sum errs like a
# random walk; GAMMA stays at its floor of 16.
RHO_O["dE"] = 0.2
GAMMA["dE"] = 16.0 * max(RHO_O["dE"], 1.0)
MC_MODES = ("swap", "transmute")


def _compressed(reps, a, seed, rattle, numbers=(42, 74)):
    """a bcc cell at a lattice constant far below the physical one: the way to long 3-body lists with few atoms"""
    return synthetic.lattice_frame("bcc", reps, a, list(numbers), seed=seed, rattle=rattle, strain=0.0)


def mc_counts(basis, atoms):
    """From the geometry alone, with the oracle's supercell: ``n3`` [N] entries of every atom's 3-body list, ``in3`` / ``in2``
    [N, N] how many images of atom j lie in atom i's 3-body range / within the largest pair r_max (the device table's two
    lists: uf3_hip.hip mc_build_table)."""
    ob = O.OracleBasis(basis)
    pos, _, _ = O.supercell(atoms, basis.r_cut)
    n = len(atoms)
    in2, in3 = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    r2 = float(ob.pair_rmax.max())
    if basis.degree > 2 and ob.trios:
        seqs = [[np.asarray(k, float) for k in basis.knots_map[t]] for t in ob.trios]
        rmin3, rmax3 = max(min(k.min() for ks in seqs for k in ks), 0.0), max(k.max() for ks in seqs for k in ks[:2])
    else:
        rmin3, rmax3 = 0.0, -1.0
    parent = np.arange(len(pos)) % n
    for i in range(n):
        d = np.linalg.norm(pos - pos[i], axis=1)
        d[i] = -1.0
        np.add.at(in2[i], parent[(d >= 0) & (d < r2)], 1)
        np.add.at(in3[i], parent[(d > rmin3) & (d <= rmax3)], 1)
    return {"n3": in3.sum(1), "in2": in2, "in3": in3}


@functools.lru_cache(maxsize=None)
def limit_frames(target=512):
    """(frame whose longest 3-body list holds exactly ``target`` entries, frame whose longest holds ``target + 1``): a rattled
    16-atom bcc cell of Mo and W (an 8-atom cell and its translate of the other species) scaled as a whole.  Its lattice constant is bisected between a cell whose longest list is
    longer than ``target`` and one where it is not; from that crossing the constant is walked in steps of 2e-6 A to either side
    until each count is met at a constant whose neighbours 1e-7 A away give the same count (a list loses one entry as the cell
    grows -- or two at once, an atom's own image and its mirror image -- so a count can be stepped over: then the next seed).
    The counts of the frames returned are those of ``mc_counts``, and the frames are clear of discontinuities."""
    basis = cases()["mow_lead0"][0]
    rmin3, rmax3 = 1.5, 3.5
    for seed in range(900, 940):
        half = _compressed((2, 2, 1), 1.0, seed, rattle=0.02)
        hc = np.asarray(half.get_cell())
        zh = np.asarray(half.get_atomic_numbers())
        # the 8-atom cell twice along c, atom k + 8 the translate of atom k with the other species: both have the same lists, so
        # the swap of the atom with the longest list and its translate fills the candidate list to its last slot
        unit = Atoms(numbers=np.concatenate([zh, 42 + 74 - zh]), positions=np.concatenate([half.get_positions(), half.get_positions() + hc[2]]),
                     cell=hc * np.array([[1.0], [1.0], [2.0]]), pbc=True)
        p = np.asarray(unit.get_positions())
        shifts = np.array([[x, y, z] for x in range(-6, 7) for y in range(-6, 7) for z in range(-6, 7)], dtype=float) @ np.asarray(unit.get_cell())
        d = np.sort(np.linalg.norm((p[None, :, None, :] + shifts[None, None, :, :]) - p[:, None, None, :], axis=-1).reshape(len(p), -1), axis=1)

        def frame(a):
            return Atoms(numbers=unit.get_atomic_numbers(), positions=p * a, cell=np.asarray(unit.get_cell()) * a, pbc=True)

        def longest(a):                                   # (the unit cell's sorted distances, the range scaled instead)
            return max(int(np.searchsorted(row, rmax3 / a, side="right") - np.searchsorted(row, rmin3 / a, side="right")) for row in d)
        lo, hi = 0.80, 0.95                               # longest(lo) > target >= longest(hi)
        assert longest(lo) > target + 1 and longest(hi) < target
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if longest(mid) > target else (lo, mid)
        found = {}
        for a in np.concatenate([hi + 2e-6 * np.arange(1, 2000), lo - 2e-6 * np.arange(1, 2000)]):
            c = longest(float(a))
            if c in (target, target + 1) and c not in found and longest(a - 1e-7) == c == longest(a + 1e-7):
                f = frame(float(a))
                try:
                    clear_of_discontinuities(basis, f)
                except AssertionError:
                    continue
                if int(mc_counts(basis, f)["n3"].max()) == c:
                    found[c] = f
            if len(found) == 2:
                return found[target], found[target + 1]
    raise AssertionError("no seed gives both counts")


@functools.lru_cache(maxsize=None)
def mc_cases():
    """name -> (basis, atoms, what it is for, most moves of a mode).  The evaluator cases of ``cases()``, a 2-body model, the
    three-equal-legs basis made binary, eight species, and the shapes that reach mc_delta's structural edges (host-side counts:
    tests/test_gpu_precision_mc.py asserts each before the device is touched)."""
    from test_gpu_species import ELEMENTS as SPECIES_ELEMENTS, _all_species_frame, _z
    out = {}
    for name in ("mow_cap16", "mow_cap32", "mow_lead0", "uneven_lead3", "uneven_lead0", "triclinic_thin", "cluster", "slab_outside",
                 "bcc24_s4"):
        basis, atoms, what = cases()[name]
        out[name] = (basis, atoms, what, 100)
    # three equal legs made binary: Mo-Mo-Mo and W-W-W keep the six-fold fold, Mo-W-W and W-Mo-Mo fold l <-> m, the others none
    _, meta, w16 = load_case("case_w16_sym3")
    cs = composition.ChemicalSystem(["Mo", "W"], 3)
    kw = meta["basis_kwargs"]
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    sym3 = bspline.BSplineBasis(
        cs, r_min_map={**{p: kw["r_min_map"]["W-W"] for p in pairs}, **{t: kw["r_min_map"]["W-W-W"] for t in trios}},
        r_max_map={**{p: kw["r_max_map"]["W-W"] for p in pairs}, **{t: kw["r_max_map"]["W-W-W"] for t in trios}},
        resolution_map={**{p: kw["resolution_map"]["W-W"] for p in pairs}, **{t: kw["resolution_map"]["W-W-W"] for t in trios}},
        leading_trim={2: 0, 3: 3}, trailing_trim={2: 3, 3: 3})
    assert sorted(sym3.symmetry.values()) == [1, 1, 2, 2, 3, 3]
    z = np.random.default_rng(16).permutation(np.resize([42, 74], len(w16)))
    out["w16_sym3_binary"] = (sym3, Atoms(numbers=z, positions=w16.get_positions(), cell=w16.get_cell(), pbc=w16.get_pbc()),
                              "three equal legs, two species: symmetry folds 3, 2 and 1 in one basis", 100)
    cs2 = composition.ChemicalSystem(["Mo", "W"], 2)
    two = bspline.BSplineBasis(cs2, r_min_map={p: 0.001 for p in cs2.interactions_map[2]}, r_max_map={p: 5.5 for p in cs2.interactions_map[2]},
                               resolution_map={p: 15 for p in cs2.interactions_map[2]}, leading_trim={2: 0}, trailing_trim={2: 3})
    out["mow_2body"] = (two, cases()["mow_lead0"][1], "a 2-body model: T = 0, no candidate list", 100)
    els = SPECIES_ELEMENTS[8]
    out["bcc24_s8"] = (synthetic.notebook_basis(els), _all_species_frame(_z(els), (2, 2, 3), 3.165, 68),
                       "eight species: every row of trio_of, seven transmutations an atom", 100)
    mow = cases()["mow_lead0"][0]                             # 3-body range (1.5, 3.5], pair range 5.5: one object for the shapes below
    out["mow288"] = (mow, synthetic.lattice_frame("bcc", (6, 6, 4), 3.165, [42, 74], seed=288, rattle=0.05, strain=0.0),
                     "288 atoms: the strided species load, atoms past 255", 60)
    out["dense432"] = (mow, _compressed((6, 6, 6), 1.34, 432, rattle=0.03),
                       "compressed bcc 6 x 6 x 6: candidate lists past one round, more than 200 distinct centres", 4)
    out["thin16_r3"] = (mow, _compressed((2, 2, 2), 1.03, 163, rattle=0.02),
                        "16 atoms, cell of 2 A against a reach of 7: n_c past 512, every atom dozens of times", 1)
    out["thin16_r4"] = (mow, _compressed((2, 2, 2), 0.93, 164, rattle=0.02), "the same, n_c past 768", 1)
    out["limit512"] = (mow, limit_frames()[0], "longest 3-body list exactly 512: n_c = 1026, pair index 130815", 1)
    return out


MC_CLASSES = ("three_body", "pair_only", "apart", "images")


def mc_move_classes(basis, atoms):
    """{class: [(i, j)]} of every ordered pair of unlike atoms, from the geometry: j in i's 3-body range; in pair range only; in
    neither; met through two or more periodic images (or i among its own neighbours)."""
    c = mc_counts(basis, atoms)
    z = np.asarray(atoms.get_atomic_numbers())
    out = {k: [] for k in MC_CLASSES}
    for i in range(len(z)):
        for j in range(len(z)):
            if z[i] == z[j]:
                continue
            if c["in3"][i, j] > 0:
                out["three_body"].append((i, j))
            elif c["in2"][i, j] > 0:
                out["pair_only"].append((i, j))
            else:
                out["apart"].append((i, j))
            if c["in2"][i, j] >= 2 or c["in2"][i, i] > 0:
                out["images"].append((i, j))
    return out


@functools.lru_cache(maxsize=None)
def mc_moves(name, mode):
    """The chosen moves of a case: ``(i, second, label)`` lists.  Swaps: as many of every class of ``mc_move_classes`` as the
    case's budget allows (seeded), then the null moves: i == j and like species.  Transmutations: chosen atoms (the first of the
    chosen swaps' atoms) to every other species of the basis, then to their own."""
    basis, atoms, _, budget = mc_cases()[name]
    z = np.asarray(atoms.get_atomic_numbers())
    rng = np.random.default_rng(1 + sorted(mc_cases()).index(name))
    classes = mc_move_classes(basis, atoms)
    chosen = []
    if name == "limit512":                                    # the atom with the longest list and its translate (limit_frames)
        k = int(np.argmax(mc_counts(basis, atoms)["n3"])) % 8
        chosen.append((k, k + 8, "last_slot"))
    for k in MC_CLASSES:
        pool = classes[k]
        if budget < 4 and set(pool) & {m[:2] for m in chosen}:  # (a dear frame: one move may stand for several classes)
            continue
        take = rng.choice(len(pool), min(len(pool), max(1, budget // 4)), replace=False) if pool else []
        chosen += [(int(pool[q][0]), int(pool[q][1]), k) for q in take]
    if name == "mow288":                                      # (at least a third of the moves reach past atom 255)
        high = [m for k in MC_CLASSES for m in classes[k] if max(m) >= 256]
        take = rng.choice(len(high), min(len(high), budget // 2), replace=False)
        chosen += [(int(high[q][0]), int(high[q][1]), "past_255") for q in take]
    if mode == "swap":
        like = [(i, j) for i in range(len(z)) for j in range(len(z)) if i != j and z[i] == z[j]]
        nulls = [(i, i, "null") for i in sorted({m[0] for m in chosen})[:3] or [0]]
        nulls += [(int(like[q][0]), int(like[q][1]), "null") for q in (rng.choice(len(like), min(len(like), 3), replace=False) if like else [])]
        return tuple(chosen + nulls)
    els = list(basis.chemical_system.element_list)
    sym = {composition.atomic_numbers[e]: e for e in els}
    atoms_chosen = list(dict.fromkeys([m[0] for m in chosen] + [m[1] for m in chosen] + list(range(len(z)))))
    n_atoms = max(1, min(len(z), budget // max(1, len(els) - 1)))
    if name == "mow288":
        atoms_chosen = [a for a in atoms_chosen if a >= 256][:n_atoms // 2] + atoms_chosen
    out = []
    for a in atoms_chosen[:n_atoms]:
        out += [(int(a), e, "transmute") for e in els if e != sym[int(z[a])]]
    out += [(int(a), sym[int(z[a])], "null") for a in atoms_chosen[:3]]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mc_reference(name, mode):
    """The chosen moves of a case with their extended dE and M, computed once and shared (read-only): dict(i, second, label, dE,
    M, ob, coeff).  The frame is asserted clear of discontinuities: the clearance is a property of the geometry and holds for
    both species assignments of every move."""
    basis, atoms, _, _ = mc_cases()[name]
    clear_of_discontinuities(basis, atoms)
    ob = O.OracleBasis(basis)
    coeff = coefficients(basis)
    moves = mc_moves(name, mode)
    i = np.array([m[0] for m in moves], dtype=np.int64)
    second = [m[1] for m in moves]
    dE, M = O.mc_delta_x(ob, atoms, coeff, i, second, mode)
    for a in (i, dE, M):
        a.setflags(write=False)
    return {"i": i, "second": second, "label": [m[2] for m in moves], "dE": dE, "M": M, "ob": ob, "coeff": coeff}
