"""Bases whose knots are binary fractions and frames whose distances fall on them exactly: shared by tests/test_on_knots_host.py
and tests/test_gpu_on_knots.py.

Every knot is a multiple of 2^-10 and every probe atom sits at (site of a cubic grid) + (a binary fraction) + q DELTA with
DELTA = 2^-42 and q in -2 .. 2, inside a periodic cell whose edges are multiples of 16 A.  So the distances that are meant to
fall on a knot (or one, two DELTA to either side of it) are exactly representable, through a cell face too, and every
formulation of the distance returns the same double (tests/test_on_knots_host.py::test_exactness): which side of a knot a kernel
puts such a distance on is then a property of the kernel.

- ``grid_notebook_lead0/3``, ``grid_wide``, ``grid_binary``, ``grid_nonuniform_lead0/3``: the bases (``basis(name)``).
- ``probe_frames(name)``: isolated pairs and triplets, 16 A apart, one for every knot of every sequence and every q
  (``probes(name)``: each records what it was made to hit).
- ``crystals(name)``: unrattled, unstrained bcc (a = 3.0) and simple cubic (a = 1.75) cells whose shells fall on knots.
- ``small_frames(name)``: a dozen probes in a 32 x 32 x 48 A cell holding both discontinuities of the untrimmed leading edge,
  the 16-atom crystal and, with one species, that crystal with a vacancy: small enough for the NumPy restatements."""
import collections
import functools
import itertools

import numpy as np

from uf3_amd.data import composition
from uf3_amd.data.atoms import Atoms
from uf3_amd.data.composition import atomic_numbers
from uf3_amd.representation import bspline

DELTA = 2.0 ** -42
QS = (-2, -1, 0, 1, 2)
SPACING = 16.0
EDGE = 128.0                  # 8^3 sites a frame
ORIGIN = 1.0                  # the first layer of sites lies 1 A off the cell faces: its probes meet through a face
CLEAR = 1e-3                  # what an inexact distance keeps from every knot
MAX_PROBES = 500              # a frame: at most 1500 atoms

BASES = ["grid_notebook_lead0", "grid_notebook_lead3", "grid_wide", "grid_binary", "grid_nonuniform_lead0", "grid_nonuniform_lead3"]


def _clamped(inner):
    inner = [float(x) for x in inner]
    return np.array([inner[0]] * 3 + inner + [inner[-1]] * 3)


# leg ranges and resolutions of grid_binary, every knot on the 0.25 grid: l != m where the neighbour species differ; the 3-body
# list range is [1.5, 3.5], and Mo-W-W, W-Mo-W (l) and W-W-W begin above it and end below it
_BINARY_PAIRS = {("Mo", "Mo"): (1.0, 5.5, 18), ("Mo", "W"): (0.75, 5.25, 18), ("W", "W"): (1.25, 5.0, 15)}
_BINARY_TRIOS = {("Mo", "Mo", "Mo"): ([1.5, 1.5, 1.5], [3.0, 3.0, 5.5], [6, 6, 16]),
                 ("Mo", "Mo", "W"): ([1.75, 1.5, 1.75], [3.25, 3.5, 6.0], [6, 8, 17]),
                 ("Mo", "W", "W"): ([2.0, 2.0, 1.5], [3.25, 3.25, 5.5], [5, 5, 8]),
                 ("W", "Mo", "Mo"): ([1.5, 1.5, 2.0], [3.5, 3.5, 6.0], [4, 4, 16]),
                 ("W", "Mo", "W"): ([2.0, 1.75, 1.5], [3.0, 3.25, 5.0], [4, 6, 14]),
                 ("W", "W", "W"): ([1.75, 1.75, 1.75], [3.25, 3.25, 5.75], [6, 6, 16])}
# grid_nonuniform: unequal spacings on the 2^-3 grid (the interval guess from one spacing is wrong for most distances)
_NONUNIFORM_PAIR = [1.0, 1.25, 1.5, 1.875, 2.25, 2.5, 3.0, 3.375, 3.75, 4.0, 4.5, 4.75, 5.0, 5.25, 5.5]
_NONUNIFORM_L = [1.5, 1.75, 2.125, 2.375, 2.75, 3.125, 3.5]
_NONUNIFORM_N = [1.5, 1.75, 2.25, 2.625, 3.0, 3.5, 4.0, 4.375, 4.75, 5.25, 5.75, 6.5, 7.0]


@functools.lru_cache(maxsize=None)
def basis(name):
    """one object per name (device tables hang on it)"""
    if name.startswith("grid_notebook") or name == "grid_wide":
        cs = composition.ChemicalSystem(["W"], 3)
        p, t = ("W", "W"), ("W", "W", "W")
        hi, res = ([3.5, 3.5, 7.0], [8, 8, 22]) if name == "grid_wide" else ([3.0, 3.0, 6.0], [6, 6, 12])
        lead3 = 0 if name == "grid_wide" else int(name[-1])
        return bspline.BSplineBasis(cs, r_min_map={p: 1.0, t: [1.5, 1.5, 1.5]}, r_max_map={p: 5.5, t: hi},
                                    resolution_map={p: 18, t: res}, leading_trim={2: 0, 3: lead3}, trailing_trim={2: 3, 3: 3})
    if name == "grid_binary":
        cs = composition.ChemicalSystem(["Mo", "W"], 3)
        rmin = {**{p: v[0] for p, v in _BINARY_PAIRS.items()}, **{t: v[0] for t, v in _BINARY_TRIOS.items()}}
        rmax = {**{p: v[1] for p, v in _BINARY_PAIRS.items()}, **{t: v[1] for t, v in _BINARY_TRIOS.items()}}
        res = {**{p: v[2] for p, v in _BINARY_PAIRS.items()}, **{t: v[2] for t, v in _BINARY_TRIOS.items()}}
        return bspline.BSplineBasis(cs, r_min_map=rmin, r_max_map=rmax, resolution_map=res,
                                    leading_trim={2: 0, 3: 0}, trailing_trim={2: 3, 3: 3})
    if name.startswith("grid_nonuniform"):
        cs = composition.ChemicalSystem(["W"], 3)
        knots = {("W", "W"): _clamped(_NONUNIFORM_PAIR), ("W", "W", "W"): [_clamped(_NONUNIFORM_L), _clamped(_NONUNIFORM_N)]}
        return bspline.BSplineBasis(cs, knots_map=knots, leading_trim={2: 0, 3: int(name[-1])}, trailing_trim={2: 3, 3: 2})
    raise KeyError(name)


def lead3(name):
    return int(basis(name).leading_trim[3])


def coefficients(b, seed=18):
    """seeded model coefficients, the frozen ones zero (tests/test_gpu_virial.py::_model)"""
    coeff = np.random.default_rng(seed).normal(0, 0.05, b.n_feats)
    coeff[np.asarray(b.col_idx, dtype=int)] = 0.0
    return coeff


def sequences(b):
    """{pair: knots, (trio, leg): knots} of a basis, as float arrays"""
    out = {p: np.asarray(b.knots_map[p], dtype=float) for p in b.interactions_map[2]}
    for t in b.interactions_map[3]:
        for q in range(3):
            out[(t, q)] = np.asarray(b.knots_map[t][q], dtype=float)
    return out


def all_knots(b):
    return np.unique(np.concatenate(list(sequences(b).values())))


# ------------------------------------------------------------------------------------------------ probes
# z: atomic numbers (centre, j[, k]); off: the neighbours' offsets from the centre before the axes are turned; hit: what the
# probe was made for: (kind, interaction, leg or None, knot, q)
Probe = collections.namedtuple("Probe", "z off hit")


def _clear(r, knots):
    return float(np.min(np.abs(np.asarray(knots) - r))) > CLEAR


def _inside(r, seq):
    return seq[0] < r < seq[-1]


def _off_grid(seq):
    """distances strictly inside a leg's support, 1/16 off the 2^-3 grid every knot lies on"""
    return np.arange(seq[0] + 0.0625, seq[-1], 0.125)


def _pair_probes(b):
    out = []
    for p in b.interactions_map[2]:
        z = tuple(atomic_numbers[e] for e in p)
        for t in np.unique(np.asarray(b.knots_map[p], dtype=float)):
            for q in QS:
                out.append(Probe(z, ((t + q * DELTA, 0.0, 0.0),), ("pair", p, None, float(t), q)))
    return out


def _leg_probes(b):
    """For every knot of every leg of every trio a triplet with that leg on the knot (+ q DELTA) and the other two legs
    strictly inside their supports, off every knot of the basis: collinear (the neighbours either side of the centre: r_jk is
    the exact sum), else a right angle at the centre or at j, else an isosceles triangle over r_jk."""
    avoid = all_knots(b)
    out = []
    for trio in b.interactions_map[3]:
        z = tuple(atomic_numbers[e] for e in trio)
        kl, km, kn = (np.asarray(s, dtype=float) for s in b.knots_map[trio])
        same_lm = len(kl) == len(km) and np.array_equal(kl, km)
        for leg, seq in enumerate((kl, km, kn)):
            if leg == 1 and same_lm and trio[1] == trio[2]:
                continue                                     # (either neighbour may take leg l: leg 0's probes are these)
            for t in np.unique(seq):
                shape = _shape_for(leg, float(t), kl, km, kn, avoid)
                if leg == 2 and t >= kl[-1] + km[-1]:
                    assert shape is None                     # (no triangle: only _product_probes' a = tlast_l, b = tlast_m get there)
                    continue
                assert shape is not None, (trio, leg, t)
                for q in QS:
                    out.append(Probe(z, shape(q * DELTA), ("leg", trio, leg, float(t), q)))
    return out


def _shape_for(leg, t, kl, km, kn, avoid):
    """q DELTA -> ((j offset), (k offset)), or None"""
    if leg in (0, 1):
        own, other = (kl, km) if leg == 0 else (km, kl)
        for b_ in _off_grid(other):
            for kind in ("opposite", "right"):
                rn = t + b_ if kind == "opposite" else float(np.hypot(t, b_))
                if _inside(rn, kn) and _clear(rn, avoid):
                    second = (-b_, 0.0, 0.0) if kind == "opposite" else (0.0, b_, 0.0)
                    if leg == 0:
                        return lambda d, s=second: ((t + d, 0.0, 0.0), s)
                    return lambda d, s=second: (s, (t + d, 0.0, 0.0))
        return None
    for a in _off_grid(kl):                                  # collinear: r_jk = a + b
        b_ = t - a
        if _inside(b_, km) and _clear(b_, avoid):
            return lambda d, a=a, b_=b_: ((a + d, 0.0, 0.0), (-b_, 0.0, 0.0))
    for a in _off_grid(kl):                                  # right angle at j: r_jk = t along y, r_ik irrational
        rm = float(np.hypot(a, t))
        if _inside(rm, km) and _clear(rm, avoid):
            return lambda d, a=a: ((a, 0.0, 0.0), (a, t + d, 0.0))
    for a in np.arange(0.0625, 4.0, 0.0625):                 # isosceles over r_jk = t
        r = float(np.hypot(a, 0.5 * t))
        if _inside(r, kl) and _inside(r, km) and _clear(r, avoid):
            return lambda d, a=a: ((a, -0.5 * t, 0.0), (a, 0.5 * t + d, 0.0))
    return None


def _product_probes(b):
    """Collinear triplets with BOTH centre legs on knots: j at +(a + q DELTA), k at -b for a, b over the knots of legs l and m
    (r_jk = a + b + q DELTA exactly; q = -1, 0, 1 on a basis of several trios), and j, k on one side (r_jk = b - a + q DELTA; q = 0 only unless b - a is a knot of leg n).
    The trios are cycled through the (a, b) pairs: every trio meets every pair of its own knots."""
    out = []
    for trio in b.interactions_map[3]:
        z = tuple(atomic_numbers[e] for e in trio)
        kl, km, kn = (np.unique(np.asarray(s, dtype=float)) for s in b.knots_map[trio])
        for a, b_ in itertools.product(kl, km):
            for q in (QS if len(b.interactions_map[3]) == 1 else (-1, 0, 1)):
                out.append(Probe(z, ((a + q * DELTA, 0.0, 0.0), (-b_, 0.0, 0.0)), ("collinear", trio, None, float(a + b_), q)))
            if b_ > a:
                for q in (QS if np.any(kn == b_ - a) else (0,)):
                    out.append(Probe(z, ((a, 0.0, 0.0), (b_ + q * DELTA, 0.0, 0.0)), ("same_side", trio, None, float(b_ - a), q)))
    return out


def _bite_probes(b):
    """The leading edge where it jumps most: leg n (and leg l, and leg m where it has a sequence of its own) on its first knot
    + q DELTA with the other two legs 1/64 A above THEIR first knots, where the first basis function of an untrimmed edge is
    still (1 - 1/16)^3 = 0.82 at the widest knot spacing used here (0.25).  The on-knot leg lies along an axis (exact); the
    other two are irrational and clear of every knot."""
    avoid = all_knots(b)
    out = []
    for trio in b.interactions_map[3]:
        z = tuple(atomic_numbers[e] for e in trio)
        kl, km, kn = (np.asarray(s, dtype=float) for s in b.knots_map[trio])
        for leg in (2, 0, 1):
            if leg == 1 and np.array_equal(kl, km) and trio[1] == trio[2]:
                continue
            t = float((kl, km, kn)[leg][0])
            ra, rb = (float(s[0]) + 1.0 / 64 for x, s in enumerate((kl, km, kn)) if x != leg)
            if leg == 2:                                     # j = (x, y), k = (x, y + t): r_ij = ra, r_ik = rb
                y = (rb * rb - ra * ra - t * t) / (2 * t)
                x = np.sqrt(ra * ra - y * y)
                x, y = np.round(x * 256) / 256, np.round(y * 256) / 256
                shape, legs = (lambda d, x=x, y=y, t=t: ((x, y, 0.0), (x, y + t + d, 0.0))), (np.hypot(x, y), np.hypot(x, y + t))
            else:                                            # the on-knot neighbour at (t, 0), the other at (u, v): r = ra, r_jk = rb
                u = (ra * ra - rb * rb + t * t) / (2 * t)
                v = np.sqrt(ra * ra - u * u)
                u, v = np.round(u * 256) / 256, np.round(v * 256) / 256
                if leg == 0:
                    shape = lambda d, u=u, v=v, t=t: ((t + d, 0.0, 0.0), (u, v, 0.0))
                else:
                    shape = lambda d, u=u, v=v, t=t: ((u, v, 0.0), (t + d, 0.0, 0.0))
                legs = (np.hypot(u, v), np.hypot(u - t, v))
            others = [s for x, s in enumerate((kl, km, kn)) if x != leg]
            assert all(s[0] + 0.01 < r < s[0] + 0.02 and _clear(r, avoid) for r, s in zip(legs, others)), (trio, leg, legs)
            for q in QS:
                out.append(Probe(z, shape(q * DELTA), ("bite", trio, leg, t, q)))
    return out


_TRIANGLES = ((1.5, 2.0, 2.5), (2.25, 3.0, 3.75))


def _pythagorean_probes(b):
    """all three legs on the 0.25 grid (q = 0 only: off it the third leg is no double), each side in turn across from the centre"""
    out = []
    for trio in b.interactions_map[3]:
        z = tuple(atomic_numbers[e] for e in trio)
        for p, s, h in _TRIANGLES:
            for x, y in ((p, s), (s, p)):
                out.append(Probe(z, ((x, 0.0, 0.0), (0.0, y, 0.0)), ("pythagorean", trio, None, h, 0)))       # r_jk = h
                out.append(Probe(z, ((x, 0.0, 0.0), (x, y, 0.0)), ("pythagorean", trio, None, y, 0)))         # r_jk = y, r_ik = h
                out.append(Probe(z, ((x, y, 0.0), (x, 0.0, 0.0)), ("pythagorean", trio, None, y, 0)))         # r_jk = y, r_ij = h
    return out


@functools.lru_cache(maxsize=None)
def probes(name):
    b = basis(name)
    return tuple(_pair_probes(b) + _leg_probes(b) + _bite_probes(b) + _pythagorean_probes(b) + _product_probes(b))


def _place(plist, cells, site_of):
    """Atoms of the probes, probe k at site ``site_of(k)`` of a grid SPACING apart in a cell of ``cells`` sites a side, its axes
    turned k times (x -> y -> z), every atom folded into the cell."""
    pos, z = [], []
    edge = np.asarray(cells, dtype=float) * SPACING
    for k, pr in enumerate(plist):
        site = ORIGIN + SPACING * np.asarray(site_of(k), dtype=float)
        pos.append(site)
        for off in pr.off:
            pos.append(site + np.roll(np.asarray(off, dtype=float), k % 3))
        z += list(pr.z)
    pos = np.array(pos)
    pos = np.where(pos < 0.0, pos + edge, pos)
    assert np.all((pos >= 0.0) & (pos < edge))
    return Atoms(numbers=np.array(z), positions=pos, cell=np.diag(edge), pbc=True)


def _frame_of(plist):
    n = int(EDGE / SPACING)
    assert len(plist) <= n ** 3
    return _place(plist, (n, n, n), lambda k: (k % n, (k // n) % n, k // (n * n)))


@functools.lru_cache(maxsize=None)
def probe_chunks(name):
    """the probes of a basis in frames of at most MAX_PROBES"""
    ps = probes(name)
    return tuple(ps[k:k + MAX_PROBES] for k in range(0, len(ps), MAX_PROBES))


@functools.lru_cache(maxsize=None)
def probe_frames(name):
    return tuple(_frame_of(chunk) for chunk in probe_chunks(name))


def probe_atoms(name, chunk, k):
    """indices of the atoms of probe k of a chunk in its frame"""
    start = sum(len(p.z) for p in probe_chunks(name)[chunk][:k])
    return list(range(start, start + len(probe_chunks(name)[chunk][k].z)))


@functools.lru_cache(maxsize=None)
def walk_frames(name):
    """Three frames of the same atoms: every probe of the basis made for q = -1 (at most MAX_PROBES of them), then the same
    probes at q = 0 and at q = +1: a walk of two steps of DELTA across every knot at once."""
    by_hit = {p.hit: p for p in probes(name)}
    minus = [p for p in probes(name) if p.hit[4] == -1][:MAX_PROBES]
    return tuple(_frame_of([by_hit[p.hit[:4] + (q,)] for p in minus]) for q in (-1, 0, 1))


def single_probe_frame(pr):
    """one probe alone in a 32 A cell"""
    return _place([pr], (2, 2, 2), lambda k: (0, 0, 0))


# ------------------------------------------------------------------------------------------------ crystals
def _crystal(kind, a, reps, numbers, seed):
    """unrattled, unstrained; the sites a quarter of the lattice constant off the cell's faces; species in equal shares, shuffled"""
    base = np.array({"bcc": [[0, 0, 0], [.5, .5, .5]], "sc": [[0, 0, 0]]}[kind])
    grid = np.stack(np.meshgrid(*[np.arange(r) for r in reps], indexing="ij"), axis=-1).reshape(-1, 1, 3)
    pos = ((grid + base[None]) * a).reshape(-1, 3) + 0.25 * a
    z = np.random.default_rng(seed).permutation(np.resize(np.asarray(numbers), len(pos)))
    return Atoms(numbers=z, positions=pos, cell=np.diag(np.asarray(reps, dtype=float) * a), pbc=True)


def numbers_of(name):
    return [atomic_numbers[e] for e in basis(name).chemical_system.element_list]


def _without(atoms, k):
    keep = np.arange(len(atoms)) != k
    return Atoms(numbers=np.asarray(atoms.get_atomic_numbers())[keep], positions=np.asarray(atoms.get_positions())[keep],
                 cell=atoms.get_cell(), pbc=atoms.get_pbc())


@functools.lru_cache(maxsize=None)
def crystals(name):
    """bcc a = 3.0 (shells at 3.0 and 6.0 on knots, the rest irrational) in 2 x 2 x 2 and 3 x 3 x 3 cells; on grid_wide also
    simple cubic a = 1.75, 3 x 3 x 3 (shells at 1.75, 3.5, 5.25, 7.0: on knots and on r_max3, collinear).  With one species every
    force and every force row of these vanishes by symmetry, so the one-species bases also get the 3 x 3 x 3 bcc cell with a
    vacancy: the same shells, forces of order one."""
    z = numbers_of(name)
    out = (_crystal("bcc", 3.0, (2, 2, 2), z, 61), _crystal("bcc", 3.0, (3, 3, 3), z, 62))
    if name == "grid_wide":
        out += (_crystal("sc", 1.75, (3, 3, 3), z, 63),)
    return out + (_without(out[1], 7),) if len(z) == 1 else out


def forces_vanish(name, k):
    """crystal k of the basis is a perfect one-species lattice"""
    return len(numbers_of(name)) == 1 and k < len(crystals(name)) - 1


# ------------------------------------------------------------------------------------------------ small frames
@functools.lru_cache(maxsize=None)
def small_probes(name):
    """A dozen probes: for the first pair and the first and last trio, the pair at r_min2 and the triplets with leg n, then leg l,
    on their first knot at q = 0 and q = +1 (both discontinuities of an untrimmed leading edge, either side), a triplet on an
    inner knot of leg n, one on the largest knot of leg n that a triangle reaches, and Pythagorean triangles."""
    b = basis(name)
    ps = probes(name)
    pairs, trios = b.interactions_map[2], b.interactions_map[3]
    want = []
    for q in (0, 1):
        want.append(("pair", pairs[0], None, float(b.knots_map[pairs[0]][0]), q))
        for trio in (trios[0], trios[-1]):
            want.append(("bite", trio, 2, float(b.knots_map[trio][2][0]), q))
    for q in (0, 1):
        want.append(("bite", trios[-1], 0, float(b.knots_map[trios[-1]][0][0]), q))
    want.append(("leg", trios[0], 2, float(np.unique(b.knots_map[trios[0]][2])[3]), 0))
    want.append(max((p.hit for p in ps if p.hit[:3] == ("leg", trios[0], 2) and p.hit[4] == -1), key=lambda h: h[3]))
    out = [next(p for p in ps if p.hit == w) for w in want]
    out += [p for p in ps if p.hit[0] == "pythagorean" and p.hit[1] == trios[0]][:2]
    assert len(out) == 12
    return tuple(out)


@functools.lru_cache(maxsize=None)
def small_frames(name):
    """(the dozen probes in a 32 x 32 x 48 A cell: at most 36 atoms, the 16-atom crystal[, that crystal with a vacancy]).  The
    third frame comes with the one-species bases, on whose perfect crystal forces and the Hessian's mixed term vanish: it
    gives those the magnitude their terms have when they do not cancel."""
    ps = small_probes(name)
    out = _place(ps, (2, 2, 3), lambda k: (k % 2, (k // 2) % 2, k // 4)), crystals(name)[0]
    return out + (_without(out[1], 7),) if len(numbers_of(name)) == 1 else out


SMALL_CASES = [(name, which) for name in BASES for which in range(3 if "binary" not in name else 2)]


def displaced(atoms, pos):
    return Atoms(numbers=atoms.get_atomic_numbers(), positions=pos, cell=atoms.get_cell(), pbc=atoms.get_pbc())


def with_numbers(atoms, z):
    return Atoms(numbers=np.asarray(z), positions=atoms.get_positions(), cell=atoms.get_cell(), pbc=atoms.get_pbc())
