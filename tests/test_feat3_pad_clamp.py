"""
k_featurize3's neighbour role, 3-row windows: a lane whose n slot lies outside a staged record's four functions reads the
record's own 16-byte pad, which is kept zero, instead of selecting the address of a quad of zeros (``min`` in place of compare
and select: uf3_feat3.h).  What can go wrong with that, at the smallest shapes where it can:

- the pads are dirty when a neighbour role begins (the centre role's records and the fold's dump lie over them): cells in
  which every atom runs centre roles and folds in front of neighbour roles, energy + force rows and force rows alone;
- a record's first n slot decides which lanes land on the pad -- below the window (the offset wraps), above it (>= 128) --:
  records with every first slot 0 ... 5 of the 9-slot window occur (asserted from the geometry);
- every instance with a 3-row window: list capacity 16, 24, 32 and the generic one (a context's first call, sparse cells);
- nothing outlives a role: a frame alone and as the last of a batch, bit for bit;
- the wide windows have no pad and keep the quad of zeros: one 6 x 12 basis against the oracle.

Tolerance: that of the three-way test of the trio kernels (test_gpu_parity.py), 1e-9 relative against the oracle.
"""
import itertools
import re

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic, _lib
from uf3_amd.representation import process
from _util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-9
R_MIN = 1.5         # lower end of every 3-body leg of the bases below
ELEMENTS = {74: "W", 42: "Mo"}


def _basis(elements, r3, lead3=3):
    """The notebook basis (3 x 3 x 9 kept bins per trio at ``lead3`` = 3, 6 x 6 x 12 at 0) with the centre legs cut at ``r3``."""
    cs = synthetic.composition.ChemicalSystem(list(elements), 3)
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    return synthetic.bspline.BSplineBasis(
        cs, r_min_map={**{p: 0.001 for p in pairs}, **{t: [R_MIN, R_MIN, R_MIN] for t in trios}},
        r_max_map={**{p: 5.5 for p in pairs}, **{t: [r3, r3, 2 * r3] for t in trios}},
        resolution_map={**{p: 15 for p in pairs}, **{t: [6, 6, 12] for t in trios}}, leading_trim={2: 0, 3: lead3}, trailing_trim={2: 3, 3: 3})


def _neighbour_roles(atoms, basis, r3):
    """From the geometry alone: the 3-body list length of every atom, the number of valid neighbour-role records of every atom
    (all its roles together) and the set of first n slots those records have.  A record is a pair (e, k), e a 3-body neighbour
    of m and k one of e, k not m itself, |m -> k| inside leg n; its four functions are those of the knot interval (t_j, t_j+1]
    that holds |m -> k|, and its first slot is j less the leading trim, held inside the window (uf3_feat3.h: sbn)."""
    pos = np.asarray(atoms.get_positions(), float)
    cell = np.asarray(atoms.get_cell(), float).reshape(3, 3)
    n = len(pos)
    trio = basis.chemical_system.interactions_map[3][0]
    knots = np.asarray(basis.knots_map[trio][2], float)
    lead, trail = basis.leading_trim[3], basis.trailing_trim[3]
    ext_n = len(knots) - 4 - lead - trail
    span = [int(np.ceil(r3 * np.linalg.norm(np.linalg.inv(cell)[:, k]))) for k in range(3)]
    shifts = np.array(list(itertools.product(*[range(-s, s + 1) for s in span]))) @ cell
    lists = []
    for m in range(n):
        d = (pos[None, :, :] + shifts[:, None, :] - pos[m]).reshape(-1, 3)
        r = np.linalg.norm(d, axis=1)
        keep = np.flatnonzero((r > R_MIN) & (r < r3))
        lists.append((keep % n, d[keep]))
    records, slots = np.zeros(n, int), set()
    for m in range(n):
        for e, de in zip(*lists[m]):
            rn = np.linalg.norm(de + lists[e][1], axis=1)           # 0 where k is m itself
            rn = rn[(rn > R_MIN) & (rn < 2 * r3)]
            records[m] += len(rn)
            j = np.searchsorted(knots, rn, side="left") - 1 - 3     # knot interval, counted from the leg's lower end
            slots.update(np.clip(j - lead, 0, max(ext_n - 4, 0)).tolist())
    return np.array([len(l[0]) for l in lists]), records, slots


def _frame(lattice, reps, a, numbers, seed):
    return synthetic.lattice_frame(lattice, reps, a, numbers, seed=seed, rattle=0.03, strain=0.0)


def _check(fz, atoms, ref, capfd, calls=2):
    """Energy + force rows and force rows alone against the oracle, ``calls`` times (a context's first force call runs the generic
    instance at the estimated capacity, the next one the instance of the tuned capacity).  Returns what the launches of every
    call said."""
    said = []
    for call in range(calls):
        capfd.readouterr()
        x_e, x_f, _ = fz.featurize_frames([atoms])
        _, x_f_only, _ = fz.featurize_frames([atoms], energy=False)
        said.append(capfd.readouterr().err)
        err_e, err_f = rel_err(x_e[0], ref["xe"]), rel_err(x_f.reshape(ref["xf"].shape), ref["xf"])
        err_fo = rel_err(x_f_only.reshape(ref["xf"].shape), ref["xf"])
        print(f"call {call}: rel err energy row {err_e:.2e}, force rows {err_f:.2e}, force rows alone {err_fo:.2e}")
        assert err_e < TOL and err_f < TOL and err_fo < TOL, (call, err_e, err_f, err_fo)
    return said


def _fresh(basis, monkeypatch):
    monkeypatch.setenv("UF3_DEBUG_LDS", "1")                      # (read when the context is made: the launches say what they are)
    monkeypatch.setattr(_lib, "_contexts", {})                    # (a context of its own: capacities are a context's grow-only memory)
    fz = process.BasisFeaturizer(basis)
    assert fz._dev()[1].featurizer_modes & 0x1000                 # the bond-factorised launch serves this basis
    return fz


# (name, lattice, repetitions, lattice constant, atomic numbers, seed, cut-off of the centre legs, longest list, list capacity the
# tuned call's instance is laid out for -- 16, 24 and 32 are instances of their own, every other value runs the generic one)
CELLS = [
    ("mow_cap16", "bcc", (3, 3, 3), 3.165, [42, 74], 300, 3.5, 14, 16),
    ("w_cap16", "bcc", (2, 2, 2), 3.165, [74], 300, 3.5, 14, 16),
    ("mow_cap16_r4", "bcc", (3, 3, 3), 3.165, [42, 74], 300, 4.0, 14, 16),
    ("mow_dilated_cap16", "bcc", (3, 3, 3), 3.55, [42, 74], 300, 3.5, 11, 16),
    ("mow_cap24", "fcc", (2, 2, 3), 3.9, [42, 74], 301, 4.0, 18, 24),
    ("mow_cap32", "bcc", (3, 3, 3), 3.165, [42, 74], 300, 4.6, 26, 32),
    ("w_sparse_generic", "bcc", (2, 2, 2), 4.0, [74], 302, 3.5, 8, 8),
]
# the W/Mo bcc cells of capacity 16 between them: the undistorted lattice puts |m -> k| on a few shells only, a longer leg n
# and a dilated copy move the shells over the knot intervals the first cell misses
SLOT_CELLS = ("mow_cap16", "mow_cap16_r4", "mow_dilated_cap16")


def test_records_with_every_first_slot_occur():
    """The cells of test_pad_clamp_against_oracle stage neighbour-role records whose four functions start at every slot 0 ... 5
    of the 9-slot window: every lane is below, inside (both halves) and above some record's window -- on the instance of capacity
    16 (three cells between them), of 24 and of 32 (one cell each)."""
    have = {16: set(), 24: set(), 32: set()}
    for name, lattice, reps, a, numbers, seed, r3, longest, cap in CELLS:
        if cap not in have or (cap == 16 and name not in SLOT_CELLS):
            continue
        atoms = _frame(lattice, reps, a, numbers, seed)
        _, _, slots = _neighbour_roles(atoms, _basis([ELEMENTS[z] for z in sorted(numbers)], r3), r3)
        print(name, "first slots", sorted(slots))
        have[cap] |= slots
    for cap, slots in have.items():
        assert slots == set(range(6)), (cap, sorted(slots))


@pytest.mark.parametrize("name,lattice,reps,a,numbers,seed,r3,longest,cap", CELLS, ids=[c[0] for c in CELLS])
def test_pad_clamp_against_oracle(name, lattice, reps, a, numbers, seed, r3, longest, cap, monkeypatch, capfd):
    atoms = _frame(lattice, reps, a, numbers, seed)
    basis = _basis([ELEMENTS[z] for z in sorted(numbers)], r3)
    fz = _fresh(basis, monkeypatch)
    ref = O.featurize(O.OracleBasis(basis), atoms)
    first, tuned = _check(fz, atoms, ref, capfd)
    # every atom has a list (centre roles, folds) and neighbour-role records: its neighbour roles find the pads written over
    lengths, records, _ = _neighbour_roles(atoms, basis, r3)
    ij = fz.product_n3_indices(atoms)
    assert np.array_equal(np.bincount(ij[:, 0], minlength=len(atoms)), lengths) and lengths.max() == longest
    assert lengths.min() >= 2 and records.min() > 0, (lengths.min(), records.min())
    assert (longest + 7) // 8 * 8 == cap
    assert tuned.count(f", cap {cap} (lists") == 2 and "window 3 x 9, 1 round(s)" in tuned, tuned   # with and without energy rows
    if name == "mow_cap24":
        # the context's very first call: lists longer than 16 at an estimated capacity that is none of the constants -- the generic
        # instance (the call tunes the capacity: the force rows alone behind it ran at 24 already)
        est = {int(c) for c in re.findall(r", cap (\d+) \(lists \d+ apart\), selection 2", first)}
        assert est - {16, 24, 32}, first
    _lib.drop_device_basis(basis)


@pytest.mark.parametrize("energy", [True, False], ids=["energy_and_forces", "forces_alone"])
def test_frame_alone_and_as_last_of_a_batch_bit_for_bit(energy, monkeypatch):
    """The pads are written where a role begins, not carried: the last frame's force rows do not depend on what ran before."""
    frames = [_frame("bcc", (3, 3, 3), 3.165, [42, 74], 310 + k) for k in range(4)]
    basis = _basis(["Mo", "W"], 3.5)
    fz = _fresh(basis, monkeypatch)
    fz.featurize_frames(frames, energy=energy)                    # (the capacity settles)
    _, xf_batch, off = fz.featurize_frames(frames, energy=energy)
    _, xf_alone, _ = fz.featurize_frames(frames[-1:], energy=energy)
    last = np.ascontiguousarray(xf_batch[off[-2]:off[-1]])
    assert last.shape == xf_alone.shape and np.abs(xf_alone).max() > 0
    assert np.array_equal(last.view(np.uint64), np.ascontiguousarray(xf_alone).view(np.uint64))
    _lib.drop_device_basis(basis)


def test_wide_windows_keep_the_quad_of_zeros(monkeypatch, capfd):
    """No leading trim: 6 x 12 windows, three rounds of positions, records without a pad -- the select against the quad of zeros."""
    atoms = _frame("bcc", (3, 3, 3), 3.165, [42, 74], 300)
    basis = _basis(["Mo", "W"], 3.5, lead3=0)
    fz = _fresh(basis, monkeypatch)
    ref = O.featurize(O.OracleBasis(basis), atoms)
    said = _check(fz, atoms, ref, capfd)[-1]
    assert "uf3 featurize3: " in said and "window 6 x 12, 3 round(s)" in said, said
    _lib.drop_device_basis(basis)
