"""
k_featurize3's run boundary (uf3_feat3.h): stage 2 -- the flush of a fixed bond's W sums into the rows of
the window -- writes its second chain under half-wave masks instead of multiplying selected zeros, broadcasts W_plain with one
copy per dword (the sum it clobbers is zeroed right after), and the stage-1 trip and its tails of 3, 2 and 1 records sum into
the same registers.  What can go wrong with that, at the smallest shapes where it can:

- the energy lanes (upper half, second chain) pick up neighbour-role terms: the energy row against the oracle, on its own;
- a clobbered sum survives into the next run, or a tail body of some count sums into the wrong pair: runs of every length --
  every tail behind zero, one, two and three full trips -- in both roles (counted from the geometry and asserted);
- a run that continues across a pass of the stage or a step of 64 items is flushed or zeroed in between: neighbour roles of
  more than 64 items whose runs all have 13 records;
- empty runs, transposed blocks and blocks an atom only zeroes: three species;
- every instance: list capacity 16, 24, 32 and the generic one, with and without the energy row, and a 6 x 12 window (the wide
  windows flush per live round).

Tolerance: that of the three-way test of the trio kernels (test_gpu_parity.py), 1e-9 relative against the oracle.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic, _lib
from uf3_amd.representation import process
from _util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-9
R_MIN = 1.5         # lower end of every 3-body leg of the bases below
ELEMENTS = {23: "V", 42: "Mo", 74: "W"}


def _basis(elements, r3, lead3=3):
    """The notebook basis (3 x 3 x 9 kept bins per trio at ``lead3`` = 3, 6 x 6 x 12 at 0) with the centre legs cut at ``r3``."""
    cs = synthetic.composition.ChemicalSystem(list(elements), 3)
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    return synthetic.bspline.BSplineBasis(
        cs, r_min_map={**{p: 0.001 for p in pairs}, **{t: [R_MIN, R_MIN, R_MIN] for t in trios}},
        r_max_map={**{p: 5.5 for p in pairs}, **{t: [r3, r3, 2 * r3] for t in trios}},
        resolution_map={**{p: 15 for p in pairs}, **{t: [6, 6, 12] for t in trios}}, leading_trim={2: 0, 3: lead3}, trailing_trim={2: 3, 3: 3})


def _frame(lattice, reps, a, numbers, seed):
    return synthetic.lattice_frame(lattice, reps, a, numbers, seed=seed, rattle=0.03, strain=0.0)


def _runs(atoms, basis, r3, transpose=True):
    """From the geometry alone, the way test_feat3_pad_clamp._neighbour_roles counts records: the lengths of the runs stage 1
    sums between two flushes, and the items of every neighbour role.

    A neighbour-role run is a fixed bond (m, e) in a trio block (c; a, b): e a 3-body neighbour of m of species c, m of species a
    or b; its records are the neighbours k of e of the block's other species, k not m itself, |m -> k| inside leg n.  Its role's
    items are all neighbours of that species of all such e, valid or not (64 a step).  A centre-role run is a fixed bond (m, f)
    of an atom m of species c: f of one neighbour species, its records the partners g of the other (of the same species: those
    behind f in the list), |f -> g| inside leg n; f is of species a, except that an atom of species b != a fixes the bond on leg
    m instead (the kernel's transposed blocks; ``transpose`` = False counts every block with f of species a).  Returns
    (neighbour-role lengths, centre-role lengths, items per role), runs without a record included."""
    pos = np.asarray(atoms.get_positions(), float)
    cell = np.asarray(atoms.get_cell(), float).reshape(3, 3)
    sym = atoms.get_chemical_symbols()
    n = len(pos)
    span = [int(np.ceil(r3 * np.linalg.norm(np.linalg.inv(cell)[:, k]))) for k in range(3)]
    shifts = np.array(list(itertools.product(*[range(-s, s + 1) for s in span]))) @ cell
    lists = []
    for m in range(n):
        d = (pos[None, :, :] + shifts[:, None, :] - pos[m]).reshape(-1, 3)
        r = np.linalg.norm(d, axis=1)
        keep = np.flatnonzero((r > R_MIN) & (r < r3))
        lists.append((keep % n, d[keep]))
    inside = lambda rn: (rn > R_MIN) & (rn < 2 * r3)
    nbr, cen, items = [], [], []
    for c, a, b in basis.chemical_system.interactions_map[3]:
        for m in range(n):
            idx, d = lists[m]
            spec = np.array([sym[j] for j in idx])
            if sym[m] in (a, b):
                other = b if sym[m] == a else a
                role = 0
                for e, de in zip(idx[spec == c], d[spec == c]):
                    ke, dk = lists[e]
                    sel = np.array([sym[j] == other for j in ke], bool)
                    rn = np.linalg.norm(de + dk[sel], axis=1)        # 0 where k is m itself
                    nbr.append(int(inside(rn).sum()))
                    role += int(sel.sum())
                if (spec == c).any():
                    items.append(role)
            if sym[m] == c:
                fs, gs = (b, a) if (transpose and a != b and sym[m] == b) else (a, b)
                df, dg = d[spec == fs], d[spec == gs]
                for fi in range(len(df)):
                    part = dg[fi + 1:] if a == b else dg
                    cen.append(int(inside(np.linalg.norm(part - df[fi], axis=1)).sum()))
    return np.array(nbr), np.array(cen), np.array(items)


def _check(fz, atoms, ref, capfd, calls=2):
    """Energy + force rows and force rows alone (the instance without the energy row) against the oracle, ``calls`` times (a
    context's first force call runs the generic instance at the estimated capacity, the next one the instance of the tuned
    capacity).  Returns what the launches of every call said."""
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


# (name, lattice, repetitions, lattice constant, atomic numbers, seed, cut-off of the centre legs, leading trim, list capacity the
# tuned call's instance is laid out for -- 16, 24 and 32 are instances of their own, every other value runs the generic one)
CELLS = {
    "mow": ("bcc", (3, 3, 3), 3.165, [42, 74], 300, 3.5, 3, 16),
    "w": ("bcc", (2, 2, 2), 3.165, [74], 300, 3.5, 3, 16),
    "vmow": ("bcc", (3, 3, 3), 3.165, [23, 42, 74], 300, 3.5, 3, 16),
    "mow_cap24": ("fcc", (2, 2, 3), 3.9, [42, 74], 301, 4.0, 3, 24),
    "mow_cap32": ("bcc", (3, 3, 3), 3.165, [42, 74], 300, 4.6, 3, 32),
    "w_sparse_generic": ("bcc", (2, 2, 2), 4.0, [74], 302, 3.5, 3, 8),
    "mow_wide": ("bcc", (3, 3, 3), 3.165, [42, 74], 300, 3.5, 0, 16),
}


@functools.lru_cache(maxsize=None)
def _cell_frame(name):
    lattice, reps, a, numbers, seed, r3, lead3, _ = CELLS[name]
    return _frame(lattice, reps, a, numbers, seed), _basis([ELEMENTS[z] for z in sorted(numbers)], r3, lead3), r3


@functools.lru_cache(maxsize=None)
def _cell(name):
    """(atoms, basis, oracle rows) of a cell: made once, shared, never written to."""
    atoms, basis, _ = _cell_frame(name)
    ref = O.featurize(O.OracleBasis(basis), atoms)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return atoms, basis, ref


def test_runs_of_every_length_occur():
    """The run lengths the three cells of capacity 16 were chosen for, recounted from the geometry."""
    got = {}
    for name in ("mow", "w", "vmow"):
        atoms, basis, r3 = _cell_frame(name)
        got[name] = _runs(atoms, basis, r3)
        nbr, cen, items = got[name]
        print(name, "neighbour-role runs", np.bincount(nbr).tolist(), "centre-role runs", np.bincount(cen).tolist(),
              "items per neighbour role", items.min(), "...", items.max())
    # W/Mo: every tail body (3, 2, 1, none) behind zero, one and two full trips, in both roles
    # (centre role: 0 ... 12 with the fixed bond always on leg l; the blocks the kernel transposes bring that to 0 ... 11 in this
    # cell, which still ends in every tail behind two trips -- three full trips and more are the W cell's, below)
    nbr, cen, _ = got["mow"]
    assert set(range(1, 13)) <= set(nbr.tolist()) and set(range(0, 12)) <= set(cen.tolist())
    atoms, basis, _ = _cell_frame("mow")
    assert set(range(0, 13)) <= set(_runs(atoms, basis, CELLS["mow"][5], transpose=False)[1].tolist())
    # W: 13 records in every neighbour-role run, and every role takes more than one step of 64 items -- its runs continue across
    # the passes of the stage (29 records) and across the step
    nbr, cen, items = got["w"]
    assert set(nbr.tolist()) == {13} and items.min() > 64 and set(cen.tolist()) == set(range(0, 14))
    # V/Mo/W: empty runs among short ones (three species: transposed blocks, blocks an atom takes no part in and only zeroes)
    nbr, cen, _ = got["vmow"]
    assert int((nbr == 0).sum()) == 19 and set(nbr.tolist()) == set(range(0, 11))


@pytest.mark.parametrize("name", list(CELLS))
def test_flush_against_oracle(name, monkeypatch, capfd):
    atoms, basis, ref = _cell(name)
    lead3, cap = CELLS[name][6], CELLS[name][7]
    fz = _fresh(basis, monkeypatch)
    first, tuned = _check(fz, atoms, ref, capfd)
    window = "window 3 x 9, 1 round(s)" if lead3 else "window 6 x 12, 3 round(s)"
    assert tuned.count(f", cap {cap} (lists") == 2 and window in tuned, tuned       # with and without energy rows
    assert "uf3 featurize3: " in first
    _lib.drop_device_basis(basis)


def test_energy_row_of_the_ternary_cell(monkeypatch):
    """The energy row comes from the centre role alone: on its own against the oracle (force rows can be right while the upper
    half's second chain took neighbour-role terms), entry by entry against the row's largest."""
    atoms, basis, ref = _cell("vmow")
    fz = _fresh(basis, monkeypatch)
    for call in range(2):
        x_e, _, _ = fz.featurize_frames([atoms])
        err = rel_err(x_e[0], ref["xe"])
        print(f"call {call}: rel err energy row {err:.2e}, largest entry {np.abs(ref['xe']).max():.3e}")
        assert np.abs(ref["xe"]).max() > 1.0 and err < TOL, (call, err)
    _lib.drop_device_basis(basis)


@pytest.mark.parametrize("energy", [True, False], ids=["energy_and_forces", "forces_alone"])
def test_frame_alone_and_as_last_of_a_batch_bit_for_bit(energy, monkeypatch):
    """No sum outlives its run: the last frame's force rows do not depend on what ran before."""
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
