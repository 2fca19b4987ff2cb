"""
k_featurize3's chain of dependent loads per atom (uf3_feat3.h): the walk's gathered entry comes with
parent and shift in one load and the self test is a bitwise and of two compares; the atom's own entries, its row of species
offsets and its species byte are asked for before its count is known, the count only masks the stores; a neighbour's row of
species offsets is asked for whole, whatever the species count; a block's fold table comes with its head.  No operand and no
order of summation changed.  What can go wrong with that, at the smallest shapes where it can:

- a self test that compares the parent alone, or mixes the two words up: a 2 x 2 x 2 cell, where a centre's neighbours at +a
  and -a along an axis are ONE atom under two shifts -- alone and as one frame of a batch;
- what a lane at or past the count received reaches LDS or a ballot: lists of 8 ... 14 entries, shorter than their
  predecessor's, and atoms without any neighbour, on a context whose lists lie more than 16 entries apart and hold a denser
  frame's entries -- bit for bit against the same batch on a fresh context;
- a row of species offsets cut short or shifted: one, three, five and eight species (2, 4, 6 and 9 words: one piece, one
  full piece, a second piece begun, two pieces and the remainder) against the oracle and against the matrix-core launches
  (five and eight are the element lists of test_gpu_species.py, which has none of three: V / Mo / W is this file's);
- every instance: capacity 24, the two- and three-round windows, the generic one, each with and without the energy row.

The geometric preconditions are asserted from the geometry alone in unmarked tests.  Tolerance: that of the three-way test of
the trio kernels (test_gpu_parity.py), 1e-9 relative against the oracle.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic, _lib
from uf3_amd.data import composition
from uf3_amd.data.atoms import Atoms
from uf3_amd.representation import process
from _util import rel_err
import test_feat3_flush_diet as flush
import test_feat3_lds_reads as reads
from _precision import _resolution_basis

TOL = flush.TOL
assert TOL == 1e-9
_frame, _basis, _runs, _caps = flush._frame, flush._basis, flush._runs, reads._caps

SPECIES = {1: ['W'], 3: ['V', 'Mo', 'W'], 5: ['V', 'Nb', 'Mo', 'Ta', 'W'], 8: ['H', 'C', 'Ni', 'Zr', 'Mo', 'W', 'Pt', 'U']}


def _lists(atoms, r3):
    """The 3-body neighbours of every atom from the geometry alone: (parent, shift index triple) of every image inside ``r3``."""
    pos = np.asarray(atoms.get_positions(), float)
    cell = np.asarray(atoms.get_cell(), float).reshape(3, 3)
    n = len(pos)
    span = [int(np.ceil(r3 * np.linalg.norm(np.linalg.inv(cell)[:, k]))) for k in range(3)]
    idx = np.array(list(itertools.product(*[range(-s, s + 1) for s in span])))
    shifts = idx @ cell
    out = []
    for m in range(n):
        r = np.linalg.norm(pos[None, :, :] + shifts[:, None, :] - pos[m], axis=2)
        s, j = np.nonzero((r > flush.R_MIN) & (r < r3))
        out.append([(int(p), tuple(idx[q])) for q, p in zip(s, j)])
    return out


def _ref(basis, atoms):
    ref = O.featurize(O.OracleBasis(basis), atoms)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _rows_of(x_f, off, k, ref):
    return np.ascontiguousarray(x_f[off[k]:off[k + 1]]).reshape(ref["xf"].shape)


# ------------------------------------------------------------------------------------------ same parent, other image
@functools.lru_cache(maxsize=None)
def _small():
    """Rattled bcc 2 x 2 x 2 W/Mo, 16 atoms, a = 3.165, centre legs cut at 3.5: (atoms, basis, cut-off)."""
    return _frame("bcc", (2, 2, 2), 3.165, [42, 74], 330), _basis(["Mo", "W"], 3.5), 3.5


@functools.lru_cache(maxsize=None)
def _small_ref():
    atoms, basis, _ = _small()
    return _ref(basis, atoms)


def test_a_list_holds_one_parent_under_two_shifts():
    atoms, _, r3 = _small()
    assert len(atoms) == 16 and set(atoms.get_atomic_numbers().tolist()) == {42, 74}
    twice = 0
    for lst in _lists(atoms, r3):
        by_parent = {}
        for p, s in lst:
            by_parent.setdefault(p, set()).add(s)
        twice += sum(len(v) >= 2 for v in by_parent.values())
    print("(centre, parent) pairs under two or more shifts:", twice)
    assert twice > 0


@pytest.mark.gpu
def test_same_parent_other_image_alone(monkeypatch, capfd):
    atoms, basis, _ = _small()
    fz = flush._fresh(basis, monkeypatch)
    first, tuned = flush._check(fz, atoms, _small_ref(), capfd)
    assert _caps(first) and _caps(tuned), (first, tuned)
    _lib.drop_device_basis(basis)


@pytest.mark.gpu
def test_same_parent_other_image_in_a_batch(monkeypatch, capfd):
    """... as the second frame of a batch whose first is the 6 x 6 x 6 cell: parents are batch-global atom numbers."""
    atoms, basis, _ = _small()
    big, basis_big, ref_big = reads._cell("mow666")
    assert reads.CELLS["mow666"][3:] == ([42, 74], 320, 3.5, 3)                      # one basis serves both
    fz = flush._fresh(basis, monkeypatch)
    refs = [ref_big, _small_ref()]
    for call in range(2):
        for energy in (True, False):
            x_e, x_f, off = fz.featurize_frames([big, atoms], energy=energy)
            errs = [rel_err(_rows_of(x_f, off, k, r), r["xf"]) for k, r in enumerate(refs)]
            if energy:
                errs += [rel_err(x_e[k], r["xe"]) for k, r in enumerate(refs)]
            print(f"call {call}, energy rows {energy}: rel errs {['%.2e' % e for e in errs]}")
            assert max(errs) < TOL, (call, energy, errs)
    assert _caps(capfd.readouterr().err)
    _lib.drop_device_basis(basis)


# ------------------------------------------------------------------------------------------ stale entries beyond the count
R3_SHORT = 3.3


@functools.lru_cache(maxsize=None)
def _ragged():
    """(frames, basis): rattled bcc 4 x 4 x 4 W/Mo (rattle 0.15 A) and two atoms 6 A apart in a 12 A box; centre legs cut at 3.3."""
    cell = synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, [42, 74], seed=385, rattle=0.15, strain=0.0)
    pair = Atoms(numbers=[42, 74], positions=[[3.0, 6.0, 6.0], [9.0, 6.0, 6.0]], cell=np.eye(3) * 12.0, pbc=True)
    return [cell, pair], _basis(["Mo", "W"], R3_SHORT)


@functools.lru_cache(maxsize=None)
def _ragged_refs():
    frames, basis = _ragged()
    return [_ref(basis, a) for a in frames]


def test_short_ragged_and_empty_lists():
    (cell, pair), _ = _ragged()
    n = np.array([len(lst) for lst in _lists(cell, R3_SHORT)])
    print("list lengths", np.bincount(n).tolist())
    assert n.min() <= 8 and n.max() >= 14 and n.max() <= 16 and (np.diff(n) < 0).any()
    assert [len(lst) for lst in _lists(pair, R3_SHORT)] == [0, 0]


@pytest.mark.gpu
def test_stale_entries_beyond_the_count(monkeypatch, capfd):
    """Dense cell first (the context's capacity grows past 16), then the ragged batch: through the instance laid out for 16 on
    lists further apart, over a denser frame's entries.  Bit for bit the rows of a fresh context."""
    frames, basis = _ragged()
    refs = _ragged_refs()
    dense, basis_d, ref_d = reads._cell("mow_dense")
    fz_d = flush._fresh(basis_d, monkeypatch)
    fz = process.BasisFeaturizer(basis)
    assert fz._dev()[1].featurizer_modes & 0x1000
    for call in range(2):
        x_e, x_f, _ = fz_d.featurize_frames([dense])
        assert rel_err(x_f.reshape(ref_d["xf"].shape), ref_d["xf"]) < TOL and rel_err(x_e[0], ref_d["xe"]) < TOL
    got = {}
    for energy in (True, False):
        capfd.readouterr()
        x_e, x_f, off = fz.featurize_frames(frames, energy=energy)
        caps = _caps(capfd.readouterr().err)
        print(f"energy rows {energy}: launches {caps}")
        # both instances of the device-side selection: the one laid out for 16 runs, the generic one leaves at once
        assert len(caps) == 2 and caps[0] == (16, 1) and caps[1][1] == 2 and caps[1][0] > 32, caps
        got[energy] = (x_e, np.ascontiguousarray(x_f), off)
    _lib.drop_device_basis(basis)
    _lib.drop_device_basis(basis_d)
    fz = flush._fresh(basis, monkeypatch)
    for energy in (True, False):
        fz.featurize_frames(frames, energy=energy)                # (the capacity settles)
        x_e, x_f, off = fz.featurize_frames(frames, energy=energy)
        x_f = np.ascontiguousarray(x_f)
        x_e_old, x_f_old, _ = got[energy]
        assert x_f.shape == x_f_old.shape and np.abs(x_f).max() > 0
        assert np.array_equal(x_f.view(np.uint64), x_f_old.view(np.uint64))
        errs = [rel_err(_rows_of(x_f_old, off, k, r), r["xf"]) for k, r in enumerate(refs)]
        if energy:
            errs += [rel_err(x_e_old[k], r["xe"]) for k, r in enumerate(refs)]
            errs.append(rel_err(x_e, x_e_old))
        print(f"energy rows {energy}: rel errs {['%.2e' % e for e in errs]}")
        assert max(errs) < TOL, (energy, errs)
    # (the two atoms have no neighbour of any kind: their rows are zeros, whatever their lanes received)
    assert not refs[1]["xf"].any() and not _rows_of(x_f_old, off, 1, refs[1]).any()
    _lib.drop_device_basis(basis)


# ------------------------------------------------------------------------------------------ species counts
@functools.lru_cache(maxsize=None)
def _species_case(S):
    """bcc 3 x 3 x 3 (54 atoms), the species dealt round-robin over the sites in a shuffled order (in lattice order no atom of
    the eight-species cell sees all eight); the notebook basis of S species."""
    els = SPECIES[S]
    numbers = [composition.atomic_numbers[e] for e in els]
    base = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [numbers[0]], seed=340 + S, rattle=0.03, strain=0.0)
    z = np.random.default_rng(0).permutation(np.resize(np.asarray(numbers), len(base)))
    atoms = Atoms(numbers=z, positions=base.get_positions(), cell=base.get_cell(), pbc=True)
    return atoms, synthetic.notebook_basis(els), numbers


@pytest.mark.parametrize("S", sorted(SPECIES))
def test_every_species_among_some_atoms_neighbours(S):
    atoms, basis, numbers = _species_case(S)
    z = atoms.get_atomic_numbers()
    assert len(atoms) == 54 and sorted(set(z.tolist())) == sorted(numbers) and len(numbers) == S
    seen = [len({int(z[p]) for p, _ in lst}) for lst in _lists(atoms, 3.5)]
    print("species among an atom's neighbours:", np.bincount(seen).tolist())
    assert max(seen) == S


def _fresh_route(basis, monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("UF3_DEBUG_LDS", "1")
    monkeypatch.setattr(_lib, "_contexts", {})
    _lib.drop_device_basis(basis)
    fz = process.BasisFeaturizer(basis)
    return fz, fz._dev()[1].featurizer_modes


@pytest.mark.gpu
@pytest.mark.parametrize("S", sorted(SPECIES))
def test_species_counts(S, monkeypatch, capfd):
    atoms, basis, _ = _species_case(S)
    ref = _ref(basis, atoms)
    fz, modes = _fresh_route(basis, monkeypatch, UF3_NO_FEAT3="1")
    assert not modes & 0x1000, hex(modes)
    xe_m, xf_m, _ = fz.featurize_frames([atoms])
    assert "uf3 featurize3:" not in capfd.readouterr().err
    monkeypatch.delenv("UF3_NO_FEAT3")
    fz, modes = _fresh_route(basis, monkeypatch)
    assert modes & 0x1000, hex(modes)
    for call in range(2):
        capfd.readouterr()
        x_e, x_f, _ = fz.featurize_frames([atoms])
        _, x_f_only, _ = fz.featurize_frames([atoms], energy=False)
        assert len(_caps(capfd.readouterr().err)) >= 2
        errs = [rel_err(x_e[0], ref["xe"]), rel_err(x_f.reshape(ref["xf"].shape), ref["xf"]),
                rel_err(x_f_only.reshape(ref["xf"].shape), ref["xf"]), rel_err(x_e, xe_m), rel_err(x_f, xf_m)]
        print(f"S = {S}, call {call}: rel err energy row, force rows, force rows alone | against the matrix-core launches: energy "
              f"row, force rows {['%.2e' % e for e in errs]}")
        assert max(errs) < TOL, (S, call, errs)
    _lib.drop_device_basis(basis)


# ------------------------------------------------------------------------------------------ capacities and windows
@pytest.mark.gpu
@pytest.mark.parametrize("name,cap,window", [
    ("mow_cap24", 24, "window 3 x 9, 1 round(s)"),
    ("mow444_wide", 16, "window 6 x 12, 3 round(s)"),
])
def test_capacity_24_and_wide_windows(name, cap, window, monkeypatch, capfd):
    """Energy + force rows and force rows alone, on a context's first call (the generic instance at the estimated capacity) and
    on the tuned one."""
    atoms, basis, ref = reads._cell(name)
    fz = flush._fresh(basis, monkeypatch)
    first, tuned = flush._check(fz, atoms, ref, capfd)
    assert tuned.count(f", cap {cap} (lists") == 2 and window in tuned, tuned
    assert _caps(first)
    _lib.drop_device_basis(basis)


@pytest.mark.gpu
def test_two_round_windows(monkeypatch, capfd):
    """4 x 11 windows, two rounds: the instances in which the atom's own loads differ with the energy row (asked for ahead of
    the count with it, behind the count without: uf3_feat3.h, CH_OWN) -- both through one call pair, at the estimated capacity
    (the generic instance) and at the tuned one."""
    atoms, _, _ = flush._cell_frame("mow")
    basis = _resolution_basis([7, 7, 14])
    fz = flush._fresh(basis, monkeypatch)
    first, tuned = flush._check(fz, atoms, _ref(basis, atoms), capfd)
    window = "window 4 x 11, 2 round(s)"
    assert tuned.count(", cap 16 (lists") == 2 and tuned.count(window) == 2 and window in first, (first, tuned)
    _lib.drop_device_basis(basis)


@pytest.mark.gpu
def test_generic_instance(monkeypatch, capfd):
    """A 3 x 3 x 3 W/Mo cell through the generic instance (capacity at run time), as one frame of a batch whose other frame has
    lists of more than 32 entries; with and without the energy row."""
    dense, basis, ref_d = reads._cell("mow_dense")
    atoms, _, ref = flush._cell("mow")
    assert reads.CELLS["mow_dense"][5:] == flush.CELLS["mow"][5:7]                  # one basis serves both
    fz = flush._fresh(basis, monkeypatch)
    refs = [ref_d, ref]
    for call in range(2):
        for energy in (True, False):
            capfd.readouterr()
            x_e, x_f, off = fz.featurize_frames([dense, atoms], energy=energy)
            caps = _caps(capfd.readouterr().err)
            errs = [rel_err(_rows_of(x_f, off, k, r), r["xf"]) for k, r in enumerate(refs)]
            if energy:
                errs += [rel_err(x_e[k], r["xe"]) for k, r in enumerate(refs)]
            print(f"call {call}, energy rows {energy}: launches {caps}, rel errs {['%.2e' % e for e in errs]}")
            assert max(errs) < TOL, (call, energy, errs)
    assert len(caps) == 2 and caps[0] == (16, 1) and caps[1][1] == 2 and caps[1][0] > 32, caps
    _lib.drop_device_basis(basis)
