"""
k_featurize3's 8-byte LDS reads (uf3_feat3.h): the bond values of a neighbour-role trip, the n-leg
values of a centre-role trip, the T3 entries of the flush and the list entries of the walks and the T-table prologue are read
one ds_read_b64 each instead of as two-address pairs, and a three-row window stores a record's third bond value alone.  The
operands, their order and the record layout are the parent's; what could go wrong is a read at a wrong address or a read
taken before its store, at the smallest shapes where either would show:

- runs of every length 1 ... 8 in both roles -- every tail body behind zero and one full trip of four -- on a 6 x 6 x 6
  rattled bcc W/Mo cell (counted from the geometry with test_feat3_flush_diet._runs and asserted), at list capacity 16 and,
  as one frame of a batch whose other frame has lists of more than 32 entries, through the generic instance; with and without
  the energy row;
- lists above 16 entries (the capacity-24 instance) and neighbour roles of more than 64 items: more than one step and pass;
- three species on 4 x 4 x 4: empty runs, transposed blocks and blocks an atom only zeroes;
- one 6 x 12 window on 4 x 4 x 4: the wide instances.

Tolerance: that of the three-way test of the trio kernels (test_gpu_parity.py), 1e-9 relative against the oracle.
"""
import functools
import re

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import _lib
from _util import rel_err
import test_feat3_flush_diet as flush

TOL = flush.TOL
assert TOL == 1e-9

# (lattice, repetitions, lattice constant, atomic numbers, seed, cut-off of the centre legs, leading trim)
CELLS = {
    "mow666": ("bcc", (6, 6, 6), 3.165, [42, 74], 320, 3.5, 3),
    "mow_dense": ("fcc", (3, 3, 3), 2.8, [42, 74], 321, 3.5, 3),       # 12 + 6 + 24 neighbours inside 3.5
    "mow_cap24": flush.CELLS["mow_cap24"][:7],
    "vmow444": ("bcc", (4, 4, 4), 3.165, [23, 42, 74], 322, 3.5, 3),
    "mow444_wide": ("bcc", (4, 4, 4), 3.165, [42, 74], 323, 3.5, 0),
}


@functools.lru_cache(maxsize=None)
def _cell_frame(name):
    lattice, reps, a, numbers, seed, r3, lead3 = CELLS[name]
    return flush._frame(lattice, reps, a, numbers, seed), flush._basis([flush.ELEMENTS[z] for z in sorted(numbers)], r3, lead3), r3


@functools.lru_cache(maxsize=None)
def _cell(name):
    """(atoms, basis, oracle rows) of a cell: made once, shared, never written to."""
    atoms, basis, _ = _cell_frame(name)
    ref = O.featurize(O.OracleBasis(basis), atoms)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return atoms, basis, ref


def _caps(said):
    """(capacity, selection) of every k_featurize3 launch a call announced."""
    return [(int(c), int(s)) for c, s in re.findall(r"uf3 featurize3: lds \d+ B, cap (\d+) \(lists \d+ apart\), selection (\d)", said)]


def test_runs_of_every_length_up_to_two_trips():
    """6 x 6 x 6 W/Mo: both roles contain runs of every length 1 ... 8 -- every tail behind zero and one full trip."""
    atoms, basis, r3 = _cell_frame("mow666")
    assert len(atoms) == 432
    nbr, cen, items = flush._runs(atoms, basis, r3)
    print("neighbour-role runs", np.bincount(nbr).tolist(), "centre-role runs", np.bincount(cen).tolist(),
          "items per neighbour role", items.min(), "...", items.max())
    assert set(range(1, 9)) <= set(nbr.tolist()) and set(range(1, 9)) <= set(cen.tolist())


def test_lists_of_the_other_cells():
    """What the remaining cells were chosen for, from the geometry: lists above 16 entries with neighbour roles above 64 items,
    and empty runs among short ones on three species."""
    atoms, basis, r3 = _cell_frame("mow_cap24")
    nbr, _, items = flush._runs(atoms, basis, r3)
    print("fcc: neighbour-role runs", np.bincount(nbr).tolist(), "items per neighbour role", items.min(), "...", items.max())
    assert items.max() > 64 and nbr.max() > 8
    atoms, basis, r3 = _cell_frame("vmow444")
    nbr, cen, _ = flush._runs(atoms, basis, r3)
    print("three species: neighbour-role runs", np.bincount(nbr).tolist(), "centre-role runs", np.bincount(cen).tolist())
    assert (nbr == 0).any() and (cen == 0).any() and set(range(1, 5)) <= set(nbr.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name,cap,window", [
    ("mow666", 16, "window 3 x 9, 1 round(s)"),
    ("mow_cap24", 24, "window 3 x 9, 1 round(s)"),
    ("vmow444", 16, "window 3 x 9, 1 round(s)"),
    ("mow444_wide", 16, "window 6 x 12, 3 round(s)"),
])
def test_reads_against_oracle(name, cap, window, monkeypatch, capfd):
    """Energy + force rows and force rows alone, on a context's first call (the estimated capacity) and on the tuned one."""
    atoms, basis, ref = _cell(name)
    fz = flush._fresh(basis, monkeypatch)
    first, tuned = flush._check(fz, atoms, ref, capfd)
    print("first call", _caps(first), "tuned call", _caps(tuned))
    assert tuned.count(f", cap {cap} (lists") == 2 and window in tuned, tuned       # with and without energy rows
    assert _caps(first)
    _lib.drop_device_basis(basis)


@pytest.mark.gpu
def test_generic_instance_on_the_large_cell(monkeypatch, capfd):
    """The 6 x 6 x 6 cell through the generic instance (capacity at run time): as one frame of a batch whose other frame has lists
    of more than 32 entries -- the batch's longest list picks the instance for all its atoms."""
    dense, basis_d, ref_d = _cell("mow_dense")
    atoms, basis, ref = _cell("mow666")
    assert CELLS["mow_dense"][5:] == CELLS["mow666"][5:]                            # one basis serves both
    fz = flush._fresh(basis, monkeypatch)
    refs, said = [ref_d, ref], []
    for call in range(2):
        for energy in (True, False):
            capfd.readouterr()
            x_e, x_f, off = fz.featurize_frames([dense, atoms], energy=energy)
            caps = _caps(capfd.readouterr().err)
            errs = []
            for k, r in enumerate(refs):
                rows = np.ascontiguousarray(x_f[off[k]:off[k + 1]]).reshape(r["xf"].shape)
                errs.append(rel_err(rows, r["xf"]))
                if energy:
                    errs.append(rel_err(x_e[k], r["xe"]))
            said.append(f"call {call}, energy rows {energy}: launches {caps}, rel errs {['%.2e' % e for e in errs]}")
            assert max(errs) < TOL, said
    print("\n".join(said))
    # the tuned call: the capacity-16 instance leaves at once (selection 1), the generic one runs at a capacity of its own
    assert len(caps) == 2 and caps[0] == (16, 1) and caps[1][1] == 2 and caps[1][0] > 32, said
    _lib.drop_device_basis(basis)
