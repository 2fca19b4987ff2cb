"""Shared helpers: load golden cases and rebuild the basis / atoms they describe; equivalent descriptions of a frame; the
``dbg`` fixture of the evaluator tests."""
import gc
import json
import os
import re
import sys

import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.data import composition
from uf3_amd.data.atoms import Atoms
from uf3_amd.representation import bspline

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dekey(k):
    return tuple(k.split("-")) if "-" in k else k


def decode_basis_kwargs(kw):
    out = {}
    for name, v in kw.items():
        if isinstance(v, dict):
            if name in ("leading_trim", "trailing_trim"):
                out[name] = {int(a): b for a, b in v.items()}
            else:
                out[name] = {_dekey(a): b for a, b in v.items()}
        else:
            out[name] = v
    return out


def basis_from_meta(meta):
    cs = composition.ChemicalSystem(meta["element_list"], meta["degree"])
    return bspline.BSplineBasis(cs, **decode_basis_kwargs(meta["basis_kwargs"]))


def load_case(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(d["meta"]))
    atoms = None
    if "positions" in d:
        atoms = Atoms(numbers=d["numbers"], positions=d["positions"], cell=d["cell"], pbc=d["pbc"])
    return d, meta, atoms


FEATURE_CASES = ["case_steel", "case_h2o", "case_h2o_lead0", "case_ch4", "case_ch4_lead0",
                 "case_w128_2body", "case_w16", "case_w16_lead0", "case_w54", "case_nexe32",
                 "case_nexe32_lead0", "case_ternary24_slab", "case_w16_sym1", "case_w16_sym3"]
# captures beyond three species (tests/golden/make_species_golden.py): case -> the atomic numbers its frame and basis hold
SPECIES_CASES = {"case_bcc24_s4": [24, 42, 73, 74], "case_bcc16_s8": [1, 6, 28, 40, 42, 74, 78, 92]}


def rel_err(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if a.size else 0.0


def worst_elementwise(a, b, rtol=1e-9, floor=1e-12):
    """north_star's "within 1e-6 relative", literally: max over entries of |a - b| / (rtol |b| + floor max|b|); <= 1 passes.
    Every entry is held to ``rtol`` of ITS OWN magnitude; ``floor`` (relative to the largest entry) only covers entries that
    are sums of cancelling terms around zero.  (``rel_err`` above is the max-norm and lets small columns hide behind large
    ones.)"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if not a.size:
        return 0.0
    return float((np.abs(a - b) / (rtol * np.abs(b) + floor * max(np.abs(b).max(), 1e-300))).max())


# ------------------------------------------------------------------------------------------------
# equivalent descriptions of one crystal (tests/test_oracle_invariance.py, tests/test_gpu_invariance.py)
# ------------------------------------------------------------------------------------------------
VOIGT = [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]


def voigt_to_tensor(v):
    t = np.zeros((3, 3))
    for k, (i, j) in enumerate(VOIGT):
        t[i, j] = t[j, i] = v[k]
    return t


def tensor_to_voigt(t):
    return np.array([t[i, j] for i, j in VOIGT])


def wrap_positions(cell, pos, pbc):
    """``frac -= floor(frac)`` on the periodic axes.  The reference does not wrap (an atom outside its cell keeps only the
    images its finite range reaches), so rows are invariant across descriptions only with every atom inside its cell."""
    cell = np.asarray(cell, float).reshape(3, 3)
    frac = np.asarray(pos, float) @ np.linalg.inv(cell)
    per = np.asarray(pbc, bool)
    frac[:, per] -= np.floor(frac[:, per])
    return frac @ cell


class Description:
    """One description of a frame and how its results map back to the original's.

    Atom k of ``atoms`` is an image of original atom ``src[k]``; the description holds ``scale`` copies of the original
    (a supercell) and is the original rotated by ``Q`` (positions ``x -> Q x``).  So the energy row, energy and strain
    derivative scale by ``scale``, and force rows / forces of atom k are the original's of ``src[k]`` turned by ``Q``."""

    def __init__(self, label, atoms, src, scale, Q, reference_drops_terms=False):
        self.label, self.atoms, self.src, self.scale, self.Q = label, atoms, np.asarray(src), int(scale), np.asarray(Q, float)
        # True: the reference's force rows / forces lose ghost-centred 3-body terms here, so they are not the mapped original's
        self.reference_drops_terms = reference_drops_terms

    def xe(self, xe):
        return self.scale * np.asarray(xe)

    def xf(self, xf):
        return np.einsum("ab,kbf->kaf", self.Q, np.asarray(xf)[self.src])

    def energy(self, e):
        return self.scale * e

    def forces(self, f):
        return np.asarray(f)[self.src] @ self.Q.T

    def virial(self, v):
        return self.scale * tensor_to_voigt(self.Q @ voigt_to_tensor(v) @ self.Q.T)


def describe(atoms, label="", U=None, reps=None, perm=None, Q=None, shift=None, reference_drops_terms=False):
    """An equivalent description of ``atoms`` (whose atoms must lie inside their cell), built in this order:

    - ``reps``: supercell, (n1, n2, n3) or an integer matrix M (new cell ``M @ cell``, |det M| copies); row block 0 holds the
      original atoms, block t the images under the t-th lattice translation, each wrapped into the new cell;
    - ``U``: unimodular re-description, new cell ``U @ cell`` with the positions wrapped and the atom order kept;
    - ``shift``: rigid translation (Cartesian), then a wrap;
    - ``perm``: atom order, new atom k is old atom ``perm[k]``;
    - ``Q``: rotation or reflection (det +-1) of cell and positions alike.

    On a slab or wire M and U must act on the periodic axes only (identity rows and columns on the others).  ``reference_drops_terms``
    marks a description where the reference's finite image range drops 3-body force terms (see equivalence_cases)."""
    cell = np.asarray(atoms.get_cell(), float).reshape(3, 3)
    pos = np.asarray(atoms.get_positions(), float)
    nums = np.asarray(atoms.get_atomic_numbers())
    pbc = np.asarray(atoms.get_pbc(), bool)
    n0 = len(nums)
    src = np.arange(n0)
    scale = 1

    def on_periodic_axes(M):
        M = np.asarray(M)
        for k in np.flatnonzero(~pbc):
            e = np.eye(3, dtype=M.dtype)[k]
            assert np.array_equal(M[k], e) and np.array_equal(M[:, k], e), "transform mixes in an open axis"
        return M

    if reps is not None:
        M = np.diag(reps) if np.ndim(reps) == 1 else np.asarray(reps)
        M = on_periodic_axes(np.rint(M).astype(int))
        scale = int(round(abs(np.linalg.det(M))))
        new = M @ cell
        inv = np.linalg.inv(new)
        span = int(np.abs(M).sum(axis=0).max()) + 1
        rng = [range(-span, span + 1) if p else range(1) for p in pbc]
        # lattice translations of the old cell that fall inside the new one (fractional coordinates in [0, 1)), 0 first
        ts = [np.zeros(3, int)]
        for i in rng[0]:
            for j in rng[1]:
                for k in rng[2]:
                    t = np.array([i, j, k])
                    f = (t @ cell) @ inv
                    f = np.where(np.abs(f - np.rint(f)) < 1e-9, np.rint(f), f)
                    if t.any() and np.all((f >= 0) & (f < 1)):
                        ts.append(t)
        assert len(ts) == scale, (len(ts), scale)
        pos = np.concatenate([pos + t @ cell for t in ts])
        nums, src, cell = np.tile(nums, scale), np.tile(src, scale), new
        pos = wrap_positions(cell, pos, pbc)
    if U is not None:
        U = on_periodic_axes(np.rint(np.asarray(U)).astype(int))
        assert abs(round(np.linalg.det(U))) == 1, U
        cell = U @ cell
        pos = wrap_positions(cell, pos, pbc)
    if shift is not None:
        pos = wrap_positions(cell, pos + np.asarray(shift, float), pbc)
    if perm is not None:
        perm = np.asarray(perm)
        assert np.array_equal(np.sort(perm), np.arange(len(nums)))
        pos, nums, src = pos[perm], nums[perm], src[perm]
    if Q is None:
        Q = np.eye(3)
    Q = np.asarray(Q, float)
    assert np.allclose(Q @ Q.T, np.eye(3), atol=1e-12)
    pos, cell = pos @ Q.T, cell @ Q.T
    return Description(label, Atoms(numbers=nums, positions=pos, cell=cell, pbc=pbc), src, scale, Q, reference_drops_terms)


def rotation(axis, angle):
    """Rodrigues rotation about ``axis`` by ``angle`` radians."""
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def wrapped(atoms):
    """``atoms`` with every position folded into its cell along the periodic axes."""
    return Atoms(numbers=atoms.get_atomic_numbers(), cell=atoms.get_cell(), pbc=atoms.get_pbc(),
                 positions=wrap_positions(atoms.get_cell(), atoms.get_positions(), atoms.get_pbc()))


def bcc_primitive(a, number):
    """The 1-atom primitive bcc cell (rows a/2 (-1, 1, 1), a/2 (1, -1, 1), a/2 (1, 1, -1)); its atom off the origin, so that
    no rotation or re-description leaves it a rounding error outside the cell.  ``CONVENTIONAL @ cell`` is the cubic cell."""
    cell = 0.5 * a * (np.ones((3, 3)) - 2 * np.eye(3))
    return Atoms(numbers=[number], positions=np.array([[0.31, 0.22, 0.13]]) @ cell, cell=cell, pbc=True)


BCC_CONVENTIONAL = np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]])


# unimodular re-descriptions with image ranges `fac` of [8, 2, 1], [3, 5, 1] and [7, 5, 1] on the 2 x 2 x 2 bcc cell at r_cut 5.5:
# bin radii above the bin count, runs that wrap more than once along the fast axis, the 3-body walk's shift test
SKEW_U = {"skew_821": [[1, 0, 0], [3, 1, 0], [-2, 2, 1]],
          "skew_351": [[2, 5, 0], [1, 3, 0], [0, 0, 1]],
          "skew_751": [[1, 0, 0], [0, 1, 0], [7, 5, 1]]}


def equivalence_cases():
    """name -> (elements, original frame, [Description]): the frames whose descriptions the invariance tests compare."""
    from uf3_amd import synthetic
    mow, perm16 = [42, 74], np.random.default_rng(5).permutation(16)
    bcc = wrapped(synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, mow, seed=81))
    turn = rotation([1, 2, 3], 0.7)
    prim = bcc_primitive(3.165, 74)
    slab = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, mow, seed=82)
    slab = wrapped(Atoms(numbers=slab.get_atomic_numbers(), positions=slab.get_positions(), cell=slab.get_cell(),
                         pbc=[True, True, False]))
    wide = synthetic.lattice_frame("bcc", (3, 3, 2), 3.165, mow, seed=86)
    wide = wrapped(Atoms(numbers=wide.get_atomic_numbers(), positions=wide.get_positions(), cell=wide.get_cell(),
                         pbc=[True, True, False]))
    wire = synthetic.lattice_frame("bcc", (2, 3, 3), 3.165, mow, seed=83)
    wire = wrapped(Atoms(numbers=wire.get_atomic_numbers(), positions=wire.get_positions(), cell=wire.get_cell(),
                         pbc=[True, False, False]))
    tern = wrapped(synthetic.lattice_frame("bcc", (2, 2, 2), 3.2, [41, 42, 74], seed=84))
    quin = wrapped(synthetic.lattice_frame("bcc", (2, 2, 2), 3.2, [24, 41, 42, 73, 74], seed=85))
    return {
        "bcc_mow": (["Mo", "W"], bcc, [describe(bcc, k, U=U) for k, U in SKEW_U.items()] + [
            describe(bcc, "supercell_212", reps=(2, 1, 2)),
            describe(bcc, "supercell_222_skew_821", reps=(2, 2, 2), U=SKEW_U["skew_821"]),
            describe(bcc, "supercell_333", reps=(3, 3, 3)),
            describe(bcc, "perm_rotation_shift", perm=perm16, Q=turn, shift=[1.1, -0.4, 2.2]),
            describe(bcc, "skew_751_reflection", U=SKEW_U["skew_751"], Q=np.diag([1.0, -1.0, 1.0]) @ turn)]),
        "bcc_w_primitive": (["W"], prim, [
            describe(prim, "conventional", reps=BCC_CONVENTIONAL),
            describe(prim, "supercell_666", reps=(6, 6, 6)),
            describe(prim, "skew_rotation", U=[[1, 0, 0], [2, 1, 0], [-1, 3, 1]], Q=turn)]),
        "slab_mow": (["Mo", "W"], slab, [
            describe(slab, "skew_in_plane_531", U=[[3, 1, 0], [5, 2, 0], [0, 0, 1]]),
            describe(slab, "supercell_211_rotation", reps=(2, 1, 1), Q=turn),
            describe(slab, "perm_shift", perm=np.random.default_rng(6).permutation(len(slab)), shift=[0.7, 2.5, -1.0])]),
        # (the reference's semantics, not a symmetry: in this description its image range, [2, 1, 1], no longer holds the third
        # atom of every ghost-centred triplet, and its 3-body force rows and forces lose those terms.  Energy rows, energies and
        # strain derivatives stay invariant.  The kernels keep the terms -- a listed deviation, DESIGN.md section 7 -- so their
        # force rows and forces are the mapped original's and minus the gradient of the energy, not the oracle's.)
        "slab_ghost_terms": (["Mo", "W"], wide, [
            describe(wide, "skew_in_plane_131", U=[[1, 0, 0], [3, 1, 0], [0, 0, 1]], reference_drops_terms=True)]),
        "wire_mow": (["Mo", "W"], wire, [
            describe(wire, "supercell_311", reps=(3, 1, 1)),
            describe(wire, "perm_rotation_shift", perm=np.random.default_rng(7).permutation(len(wire)), Q=turn,
                     shift=[2.0, 0.3, 0.1])]),
        "ternary": (["Nb", "Mo", "W"], tern, [
            describe(tern, "skew_751", U=SKEW_U["skew_751"]),
            describe(tern, "supercell_121_rotation", reps=(1, 2, 1), Q=turn)]),
        "quinary": (["Cr", "Nb", "Mo", "Ta", "W"], quin, [
            describe(quin, "skew_351", U=SKEW_U["skew_351"]),
            describe(quin, "perm_rotation", perm=perm16, Q=turn)]),
    }

# ------------------------------------------------------------------------------------------------
# the evaluator's launch report (tests/test_gpu_virial.py, tests/test_gpu_invariance.py)
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def dbg(monkeypatch, capfd):
    """A fresh context that reports its k_eval and Gram launches; ``dbg.launches()`` returns (and clears) the flags of every
    k_eval launch since the last look, ``dbg.grams()`` those of every Gram launch (``kernel`` is mfma, small, tiled or
    tiled_sub; the other fields are integers).  Device tables of the bases a test makes belong to that context and are dropped
    with it."""
    monkeypatch.setenv("UF3_DEBUG_LDS", "1")
    monkeypatch.setattr(_lib, "_contexts", {})
    bases, seen = [], set()
    pending = {"k_eval": [], "gram": []}

    def read():
        cap = capfd.readouterr()
        sys.stdout.write(cap.out)                  # (what the test printed stays in its report)
        for line in cap.err.splitlines():
            m = re.match(r"uf3: (k_eval|gram) (.*)", line)
            if m:
                pending[m.group(1)].append({k: int(v) if v.lstrip("-").isdigit() else v
                                            for k, v in (kv.split("=") for kv in m.group(2).split())})

    class Dbg:
        @staticmethod
        def basis(b):
            bases.append(b)
            return b

        @staticmethod
        def launches():
            read()
            out, pending["k_eval"] = pending["k_eval"], []
            seen.update(" ".join(f"{k}={v}" for k, v in d.items() if k not in ("atoms", "cap")) for d in out)
            return out

        @staticmethod
        def grams():
            read()
            out, pending["gram"] = pending["gram"], []
            seen.update(f"gram kernel={d['kernel']}" for d in out)
            return out

    yield Dbg
    Dbg.launches()
    Dbg.grams()
    print("k_eval instances and Gram kernels reached:\n  " + "\n  ".join(sorted(seen)))
    for b in bases:
        _lib.drop_device_basis(b)
    gc.collect()
