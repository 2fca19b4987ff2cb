"""
Four to eight species (the C ABI takes bases of 1 to 8, UF3_MAX_SPECIES): every kernel route against the oracle where the launch
decisions move with the species count S.  At the notebook settings T = S S(S+1)/2 trios and F columns give

    S      4     5     6      8
    T     40    75   126    288
    F   2992  5675  9618  22256

and with them: the evaluator's window table no longer fits its 40 KB (S >= 4: no CW / WIN instances), T > 64 leaves the TAB
instances (S >= 5), the featurizer's energy row stays in LDS up to 48 KB (S = 5 is the largest that does) and goes straight to HBM
beyond, the per-species Gram's segments are 3 n / S rows.  Every test runs on a fresh context made with UF3_DEBUG_LDS set and
asserts, from the launch lines on stderr, the route it means to reach; the routes each test saw are printed when it ends.

Tolerances are those of tests/test_gpu_parity.py and tests/test_gpu_virial.py.
"""
import gc
import re

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic, _lib
from uf3_amd.data import composition
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator
from uf3_amd.regression import least_squares as ls
from uf3_amd.representation import bspline, process
from _bases import ELEMENTS, mixed_trio_basis as _mixed_trio_basis
from _util import SPECIES_CASES, basis_from_meta, load_case, rel_err, worst_elementwise
from test_gpu_virial import _check_batch, _check_frame, _model

pytestmark = pytest.mark.gpu
TOL = 1e-9
F3, GENERIC, MFMA = 1 << 12, 0x3e, 0x3c0          # featurizer mode bits: k_featurize3 | output-stationary | matrix cores


def _z(els):
    return [composition.atomic_numbers[e] for e in els]


@pytest.fixture
def dbg(monkeypatch, capfd):
    """A fresh context whose launches report themselves on stderr.  ``dbg.lines()`` returns (and clears) what was launched since
    the last look: {"eval": [flags of every k_eval launch], "feat": [featurizer mode of every k_featurize launch],
    "feat3": number of k_featurize3 launches}.  ``dbg.note`` records a route for the summary printed at the end."""
    monkeypatch.setenv("UF3_DEBUG_LDS", "1")
    monkeypatch.setattr(_lib, "_contexts", {})
    bases, notes = [], []

    class Dbg:
        @staticmethod
        def basis(b):
            bases.append(b)
            return b

        @staticmethod
        def lines():
            out = {"eval": [], "feat": [], "feat3": 0}
            for line in capfd.readouterr().err.splitlines():
                m = re.match(r"uf3: k_eval (.*)", line)
                if m:
                    out["eval"].append({k: int(v) for k, v in (kv.split("=") for kv in m.group(1).split())})
                m = re.match(r"uf3 featurize mode (\d+):", line)
                if m:
                    out["feat"].append(int(m.group(1)))
                if line.startswith("uf3 featurize3:"):
                    out["feat3"] += 1
            return out

        @staticmethod
        def note(text):
            notes.append(text)

    yield Dbg
    Dbg.lines()
    print("routes:\n  " + "\n  ".join(notes))
    for b in bases:
        _lib.drop_device_basis(b)
    gc.collect()


def _all_species_frame(numbers, reps, a, seed, rattle=0.08, pbc=True):
    """A rattled bcc cell whose sites carry the species in equal shares (every species present), shuffled."""
    base = synthetic.lattice_frame("bcc", reps, a, [numbers[0]], seed, rattle=rattle)
    z = np.random.default_rng(seed).permutation(np.resize(np.asarray(numbers), len(base)))
    return Atoms(numbers=z, positions=base.get_positions(), cell=base.get_cell(), pbc=pbc)


def _ragged_batch(numbers, seed):
    """128 atoms with every species; a one-species frame; a frame without the lowest atomic number; an open cluster."""
    return [_all_species_frame(numbers, (4, 4, 4), 3.165, seed),
            synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [numbers[-1]], seed + 1),
            _all_species_frame(numbers[1:], (3, 3, 4), 3.165, seed + 2),
            _all_species_frame(numbers, (3, 3, 3), 3.165, seed + 3, pbc=False)]


def _check_rows(basis, frames, x_e, x_f, label, refs=None):
    ob = O.OracleBasis(basis)
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    for k, atoms in enumerate(frames):
        ref = refs[k] if refs is not None else O.featurize(ob, atoms)
        if x_e is not None:
            assert rel_err(x_e[k], ref["xe"]) < TOL and worst_elementwise(x_e[k], ref["xe"]) <= 1.0, (label, k)
        if x_f is not None:
            rows = x_f[off[k]:off[k + 1]]
            assert rel_err(rows, ref["xf"]) < TOL and worst_elementwise(rows, ref["xf"]) <= 1.0, (label, k)


def _family(dbg, monkeypatch, basis, frames, env):
    """Device tables built under ``env``: modes, the launches of the first call (capacities still estimates) and of a second
    call on the tuned context; rows of both calls, of an energy-only and of a forces-only call."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        _lib.drop_device_basis(basis)
        fz = process.BasisFeaturizer(basis)
        modes = fz._dev()[1].featurizer_modes
        dbg.lines()
        first = fz.featurize_frames(frames)
        said = dbg.lines()
        second = fz.featurize_frames(frames)
        said2 = dbg.lines()
        e_only = fz.featurize_frames(frames, forces=False)[0]
        f_only = fz.featurize_frames(frames, energy=False)[1]
        said_ef = dbg.lines()
    finally:
        for k in env:
            monkeypatch.delenv(k)
        _lib.drop_device_basis(basis)
    return modes, first, second, e_only, f_only, (said, said2, said_ef)


def _check_family(dbg, monkeypatch, basis, frames, env, label, refs=None):
    modes, (x_e, x_f, _), (x_e2, x_f2, _), e_only, f_only, said = _family(dbg, monkeypatch, basis, frames, env)
    _check_rows(basis, frames, x_e, x_f, label, refs)
    assert rel_err(x_e2, x_e) < 1e-12 and rel_err(x_f2, x_f) < 1e-12, f"{label}: second call on the tuned context"
    assert worst_elementwise(x_f2, x_f, rtol=1e-9, floor=1e-12) <= 1.0, label
    assert rel_err(e_only, x_e) < 1e-12 and rel_err(f_only, x_f) < 1e-12, label
    assert worst_elementwise(f_only, x_f, rtol=1e-12, floor=1e-14) <= 1.0, label
    dbg.note(f"{label}: modes {modes:#x}; force calls: k_featurize modes {sorted(set(said[1]['feat']))}, "
             f"k_featurize3 launches {said[1]['feat3']}; energy-only / forces-only: modes {sorted(set(said[2]['feat']))}, "
             f"k_featurize3 {said[2]['feat3']}")
    return modes, said


# ------------------------------------------------------------------------------------------------ reference captures
@pytest.mark.parametrize("name", list(SPECIES_CASES))
def test_feature_rows_against_the_captures_beyond_three_species(name, dbg, monkeypatch):
    """The reference's own rows at four species (notebook basis) and at eight (H ... U, Z = 1 ... 92) against every launch
    family: default, matrix cores, output-stationary."""
    d, meta, atoms = load_case(name)
    basis = dbg.basis(basis_from_meta(meta))
    refs = [{"xe": d["xe"], "xf": d["xf"]}]
    for env, label in (({}, "default"), ({"UF3_NO_FEAT3": "1"}, "matrix cores"),
                       ({"UF3_NO_FEAT3": "1", "UF3_NO_MFMA_FEAT": "1"}, "generic")):
        modes, _ = _check_family(dbg, monkeypatch, basis, [atoms], env, f"{name} {label}", refs)
        if label == "default":
            assert modes & F3, hex(modes)
        elif label == "generic":
            assert not (modes & (MFMA | F3)) and modes & GENERIC, hex(modes)


# ------------------------------------------------------------------------------------------------ feature rows
@pytest.mark.parametrize("S", [4, 5, 6, 8])
def test_feature_rows_of_every_launch_family(S, dbg, monkeypatch):
    """Notebook bases of S species on a ragged batch (every species in 128 atoms, one species alone, the lowest atomic number
    missing, an open cluster): k_featurize3 (bit 12) by default, the matrix-core kernels (bits 6-9) without it, the generic ones
    (bits 1-5) without either; the pair launch (mode 0) in each.  Energy row in LDS up to S = 5, in HBM beyond."""
    els = ELEMENTS[S]
    basis = dbg.basis(synthetic.notebook_basis(els))
    assert basis.n_feats == {4: 2992, 5: 5675, 6: 9618, 8: 22256}[S]
    frames = _ragged_batch(_z(els), 60 + S)
    assert sorted(set(frames[0].get_atomic_numbers().tolist())) == _z(els)
    refs = [O.featurize(O.OracleBasis(basis), a) for a in frames]
    modes, said = _check_family(dbg, monkeypatch, basis, frames, {}, f"S={S} default", refs)
    assert modes & F3 and said[1]["feat3"] >= 1 and said[1]["feat"] == [0], (hex(modes), said[1])
    modes, said = _check_family(dbg, monkeypatch, basis, frames, {"UF3_NO_FEAT3": "1"}, f"S={S} matrix cores", refs)
    assert modes & MFMA and not modes & F3 and said[1]["feat3"] == 0, (hex(modes), said[1])
    assert 0 in said[1]["feat"] and any(m in (6, 7, 8, 9, 10, 11) for m in said[1]["feat"]), said[1]
    modes, said = _check_family(dbg, monkeypatch, basis, frames, {"UF3_NO_FEAT3": "1", "UF3_NO_MFMA_FEAT": "1"},
                                f"S={S} generic", refs)
    assert not (modes & (MFMA | F3)) and modes & GENERIC and said[1]["feat3"] == 0, (hex(modes), said[1])
    assert 0 in said[1]["feat"] and any(1 <= m <= 5 for m in said[1]["feat"]) and max(said[1]["feat"]) <= 5, said[1]


def test_five_species_whose_trios_all_differ(dbg, monkeypatch):
    """S = 5, 75 trio blocks each with cut-offs and resolution of its own (several window layouts and featurizer modes in one
    basis, no k_featurize3): default and generic launches against the oracle."""
    els = ELEMENTS[5]
    basis = dbg.basis(_mixed_trio_basis(els, 5))
    assert len({(tuple(basis.r_max_map[t]), tuple(basis.resolution_map[t])) for t in basis.interactions_map[3]}) == 75
    frames = _ragged_batch(_z(els), 71)
    refs = [O.featurize(O.OracleBasis(basis), a) for a in frames]
    modes, said = _check_family(dbg, monkeypatch, basis, frames, {}, "S=5 mixed trios default", refs)
    assert not modes & F3 and said[1]["feat3"] == 0 and modes & (MFMA | GENERIC), hex(modes)
    assert set(said[1]["feat"]) - {0}, said[1]
    modes, said = _check_family(dbg, monkeypatch, basis, frames, {"UF3_NO_FEAT3": "1", "UF3_NO_MFMA_FEAT": "1"},
                                "S=5 mixed trios generic", refs)
    assert not (modes & (MFMA | F3)) and modes & GENERIC, hex(modes)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_bases_of_four_to_eight_species(seed, dbg):
    """Random species sets of 4 to 8 elements given in no particular order (the first draw spans H to Og, Z = 1 ... 118),
    random resolutions, trims, cut-offs, strained cells and periodicity: feature rows and the evaluator against the oracle."""
    rng = np.random.default_rng(700 + seed)
    symbols = composition.chemical_symbols[1:119]
    for draw in range(3):
        S = int(rng.integers(4, 9))
        if seed == 1 and draw == 0:
            els = ['Og', 'W'] + [str(s) for s in rng.choice(symbols[1:73], S - 3, replace=False)] + ['H']
        else:
            els = [str(s) for s in rng.choice(symbols, S, replace=False)]
        if els == sorted(els, key=composition.atomic_numbers.get):
            els = els[::-1]
        cs = composition.ChemicalSystem(els, 3)
        assert len(cs.element_list) == S
        pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
        r3 = float(rng.uniform(3.0, 4.0))
        res_l, res_n = int(rng.integers(4, 8)), int(rng.integers(8, 15))
        basis = dbg.basis(bspline.BSplineBasis(
            cs, r_min_map={**{p: float(rng.uniform(0.2, 1.0)) for p in pairs}, **{t: [float(rng.uniform(0.8, 1.6))] * 3 for t in trios}},
            r_max_map={**{p: float(rng.uniform(4.0, 6.0)) for p in pairs}, **{t: [r3, r3, 2 * r3] for t in trios}},
            resolution_map={**{p: int(rng.integers(6, 18)) for p in pairs}, **{t: [res_l, res_l, res_n] for t in trios}},
            leading_trim={2: 0, 3: 3 if S > 5 else int(rng.choice([0, 3]))}, trailing_trim={2: 3, 3: int(rng.choice([3, 2]))}))
        reps = tuple(int(x) for x in rng.integers(3, 5, 3))
        a = float(rng.uniform(2.9, 3.4))
        atoms = _all_species_frame(_z(cs.element_list), reps, a, int(rng.integers(1 << 30)), rattle=0.1)
        cell = np.asarray(atoms.get_cell()) @ (np.eye(3) + rng.normal(0, 0.02, (3, 3)))
        pbc = [True, True, True] if rng.random() < 0.6 else [bool(b) for b in rng.integers(0, 2, 3)]
        atoms = Atoms(numbers=atoms.get_atomic_numbers(), positions=atoms.get_positions(), cell=cell, pbc=pbc)
        fz = process.BasisFeaturizer(basis)
        modes = fz._dev()[1].featurizer_modes
        x_e, x_f, _ = fz.featurize_frames([atoms])
        said = dbg.lines()
        _check_rows(basis, [atoms], x_e, x_f, f"seed {seed} draw {draw} {cs.element_list}")
        dbg.note(f"seed {seed} draw {draw}: S={S} {cs.element_list} F={basis.n_feats} modes {modes:#x}, "
                 f"k_featurize modes {sorted(set(said['feat']))}, k_featurize3 {said['feat3']}")
        model, coeff = _model(basis, seed * 10 + draw)
        e, f, _ = calculator.UFCalculator(model, md_skin=0.0).evaluate_frames([atoms])
        e_ref, f_ref = O.evaluate(O.OracleBasis(basis), atoms, coeff)
        assert abs(e[0] - e_ref) <= TOL * max(1.0, abs(e_ref)) and worst_elementwise(f, f_ref, TOL) <= 1.0


# ------------------------------------------------------------------------------------------------ evaluator
def _eval_frames(numbers, seed):
    """bcc with every species, a compressed cell whose 3-body lists hold more than 16 entries, an open cluster."""
    return [_all_species_frame(numbers, (4, 4, 4), 3.165, seed),
            _all_species_frame(numbers, (4, 4, 4), 2.4, seed + 1, rattle=0.03),
            _all_species_frame(numbers, (3, 3, 3), 3.165, seed + 2, pbc=False)]


def _assert_instance(said, S, label):
    """S = 4: T = 40 <= 64 and one set of legs -- the TAB instances, but the window table (40 x 3 x 3 x 9 doubles) is past
    40 KB: no CW, no WIN.  S >= 5: T > 64, the plain one-wave instances."""
    for s in said:
        assert s["cw"] == 0 and s["win"] == 0 and s["tab"] == int(S == 4), (label, said)


@pytest.mark.parametrize("S", [4, 5, 8])
def test_evaluator_plain_and_gather_routes(S, dbg, monkeypatch):
    """md_skin = 0 on a ragged batch with lists longer than 16 entries: the centre pass + collection pass (with and without
    forces), the gather route (UF3_EVAL_GATHER): energies, forces and strain derivatives against the oracle."""
    els = ELEMENTS[S]
    basis = dbg.basis(synthetic.notebook_basis(els))
    model, coeff = _model(basis, 80 + S)
    ob = O.OracleBasis(basis)
    frames = _eval_frames(_z(els), 90 + S)
    refs = [O.evaluate(ob, a, coeff, virial=True) for a in frames]
    calc = calculator.UFCalculator(model, md_skin=0.0)
    for _ in range(2):
        calc.evaluate_frames(frames, virial=True)                 # (list capacity tuned)
    dbg.lines()
    for label, env, forces in (("plain", {}, True), ("gather", {"UF3_EVAL_GATHER": "1"}, True), ("forces=False", {}, False)):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e, f, off, v = calc.evaluate_frames(frames, forces=forces, virial=True)
        for k in env:
            monkeypatch.delenv(k)
        said = dbg.lines()["eval"]
        gather = int(label != "plain")
        assert said and all(s["vir"] == 1 and s["md"] == 0 and s["gather"] == gather for s in said), said
        if not gather:
            assert all(s["cap"] > 16 for s in said), said
            _assert_instance(said, S, label)
        dbg.note(f"S={S} {label}: " + "; ".join(sorted({" ".join(f"{k}={x}" for k, x in s.items() if k not in ("atoms",))
                                                         for s in said})))
        assert (f is None) == (not forces)
        for k, atoms in enumerate(frames):
            _check_frame(e[k], None if f is None else f[off[k]:off[k + 1]], v[k], ob, atoms, coeff, f"S={S} {label} {k}", refs[k])


@pytest.mark.parametrize("density", ["short_lists", "long_lists"])
@pytest.mark.parametrize("S", [4, 5, 8])
def test_evaluator_md_route_on_a_walk(S, density, dbg):
    """The MD route (skin 0.5) over six displaced steps, lists of at most 16 entries and of more: energy, forces and strain
    derivative of every step against the oracle; the instance of every step asserted."""
    els = ELEMENTS[S]
    basis = dbg.basis(synthetic.notebook_basis(els))
    model, coeff = _model(basis, 40 + S)
    ob = O.OracleBasis(basis)
    if density == "short_lists":
        start = _all_species_frame(_z(els), (4, 4, 4), 3.165, 51 + S)
    else:
        start = _all_species_frame(_z(els), (4, 4, 4), 2.4, 52 + S, rattle=0.03)
    plain = calculator.UFCalculator(model, md_skin=0.0)
    for _ in range(2):
        plain.evaluate_frames([start], virial=True)
    calc = calculator.UFCalculator(model, md_skin=0.5)
    rng = np.random.default_rng(6)
    pos = start.get_positions()
    dbg.lines()
    for step in range(6):
        pos = pos + rng.uniform(-0.03, 0.03, pos.shape)
        atoms = Atoms(numbers=start.get_atomic_numbers(), positions=pos, cell=start.get_cell(), pbc=True)
        out = calc.evaluate_frames([atoms], virial=True)
        said = dbg.lines()["eval"]
        assert said and said[-1]["vir"] == 1 and said[-1]["md"] == 1 and said[-1]["gather"] == 0, said
        assert (said[-1]["cap"] > 16) == (density == "long_lists"), said
        _assert_instance(said, S, f"md {density} step {step}")
        if step == 5:
            dbg.note(f"S={S} md {density}: " + " ".join(f"{k}={x}" for k, x in said[-1].items()))
        _check_batch(out, ob, [atoms], coeff, f"S={S} md {density} step {step}")


@pytest.mark.parametrize("S", [4, 5, 8])
def test_evaluator_atom_and_centre_shares(S, dbg):
    """uf3_eval_atoms (gather on a block) and uf3_eval_centres (centre pass on a block + its halo) over three shares: the sums
    equal the oracle's frame."""
    from uf3_amd import parallel
    els = ELEMENTS[S]
    basis = dbg.basis(synthetic.notebook_basis(els))
    model, coeff = _model(basis, 5 + S)
    ob = O.OracleBasis(basis)
    atoms = _all_species_frame(_z(els), (4, 5, 6), 3.165, 77 + S)
    n = len(atoms)
    ref = O.evaluate(ob, atoms, coeff, virial=True)
    calc = calculator.UFCalculator(model, md_skin=0.0)
    for _ in range(2):
        calc.evaluate_frames([atoms], virial=True)
    dbg.lines()
    for which in ("atoms", "centres"):
        share = calc.evaluate_atom_range if which == "atoms" else calc.evaluate_centre_range
        parts = [share(atoms, *parallel.shard_range(n, r, 3), virial=True) for r in range(3)]
        said = dbg.lines()["eval"]
        assert len(said) >= 3 and all(s["vir"] == 1 and s["centres"] == int(which == "centres") for s in said), said
        assert all(s["gather"] == int(which == "atoms") for s in said), said
        if which == "centres":
            _assert_instance(said, S, which)
        dbg.note(f"S={S} {which}: " + " ".join(f"{k}={x}" for k, x in said[-1].items()))
        _check_frame(sum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts), ob, atoms, coeff,
                     f"S={S} {which}", ref)


# ------------------------------------------------------------------------------------------------ Gram
@pytest.mark.parametrize("S", [4, 8])
def test_force_row_gram_by_species(S, dbg):
    """uf3_gram_force_rows_dev where its segments (3 n / S rows) reach the per-species route: S = 4 on the notebook basis at 88 k
    atoms, S = 8 on a 2-body basis at 176 k atoms with an uneven composition.  Overwrite, then accumulate; against uf3_gram_dev
    and an fp64 product of the same rows by torch, X^T y included; the rows vanish outside their species' blocks."""
    import torch
    dev = torch.device("cuda", 0)
    els = ELEMENTS[S]
    if S == 4:
        basis = dbg.basis(synthetic.notebook_basis(els))
        reps, numbers = (28, 28, 56), _z(els)
    else:
        basis = dbg.basis(bspline.BSplineBasis(composition.ChemicalSystem(els, 2)))
        reps, numbers = (28, 28, 112), _z(els) + [74, 74, 74, 42]
    fz = process.BasisFeaturizer(basis)
    ctx, db = fz._dev()
    F = basis.n_feats
    atoms = synthetic.lattice_frame("bcc", reps, 3.165, numbers, seed=910 + S)
    batch = _lib.FrameBatch([atoms])
    n_atoms = batch.n_atoms
    counts = np.bincount(np.searchsorted(_z(els), batch.z), minlength=S)
    assert 3 * n_atoms // S >= 65536 and counts.min() > 0 and F > 128, (n_atoms, counts)
    # (the plain product is taken unless some species leaves out at least one 64-column range: assert the route's premise)
    sizes, offsets = basis.get_interaction_partitions()
    inside = {}
    for el in els:
        cols = np.zeros(F, dtype=bool)
        for inter in sizes:
            if not isinstance(inter, str) and el in inter:
                cols[offsets[inter]:offsets[inter] + sizes[inter]] = True
        inside[el] = cols
    assert (max(c.sum() for c in inside.values()) + 63) // 64 < (F + 63) // 64
    d_pos, d_z = torch.from_numpy(batch.pos).to(dev), torch.from_numpy(batch.z).to(dev)
    x_e = torch.empty((1, F), dtype=torch.float64, device=dev)
    x_f = torch.empty((3 * n_atoms, F), dtype=torch.float64, device=dev)
    y_f = torch.from_numpy(np.random.default_rng(3).normal(size=3 * n_atoms)).to(dev)
    prev = ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        fz.featurize_device(batch.struct, d_pos.data_ptr(), d_z.data_ptr(), x_e.data_ptr(), x_f.data_ptr())
        g_ref, o_ref = torch.empty((F, F), dtype=torch.float64, device=dev), torch.empty(F, dtype=torch.float64, device=dev)
        g, o = torch.full((F, F), 7.0, dtype=torch.float64, device=dev), torch.full((F,), 7.0, dtype=torch.float64, device=dev)
        ctx.check(ctx.lib.uf3_gram_dev(ctx.handle, x_f.data_ptr(), y_f.data_ptr(), 3 * n_atoms, F, F, 0, g_ref.data_ptr(),
                                       o_ref.data_ptr()))
        ctx.check(ctx.lib.uf3_gram_force_rows_dev(db.handle, x_f.data_ptr(), y_f.data_ptr(), d_z.data_ptr(), n_atoms, F, 0,
                                                  g.data_ptr(), o.data_ptr()))
        ctx.synchronize()
        g1, o1 = g.cpu().numpy(), o.cpu().numpy()
        ctx.check(ctx.lib.uf3_gram_force_rows_dev(db.handle, x_f.data_ptr(), y_f.data_ptr(), d_z.data_ptr(), n_atoms, F, 1,
                                                  g.data_ptr(), o.data_ptr()))
        ctx.synchronize()
    finally:
        ctx.restore_stream(prev)
    g_t, o_t = (x_f.T @ x_f).cpu().numpy(), (x_f.T @ y_f).cpu().numpy()
    g_ref, o_ref = g_ref.cpu().numpy(), o_ref.cpu().numpy()
    scale = np.abs(g_t).max()
    assert scale > 0 and np.abs(g_ref - g_t).max() < 1e-12 * scale
    assert np.abs(g1 - g_ref).max() < 1e-12 * scale and np.abs(g1 - g_t).max() < 1e-12 * scale and np.array_equal(g1, g1.T)
    assert np.abs(o1 - o_ref).max() < 1e-11 * np.abs(o_ref).max() and np.abs(o1 - o_t).max() < 1e-11 * np.abs(o_t).max()
    assert np.abs(g.cpu().numpy() - 2 * g_t).max() < 2e-12 * scale
    assert np.abs(o.cpu().numpy() - 2 * o_t).max() < 2e-11 * np.abs(o_t).max()
    rows = x_f.view(n_atoms, 3, F)
    for el in els:
        assert 0 < inside[el].sum() < F
        idx = torch.from_numpy(np.flatnonzero(batch.z == composition.atomic_numbers[el])[:4000]).to(dev)
        assert len(idx) > 100
        outside = torch.from_numpy(np.flatnonzero(~inside[el])).to(dev)
        assert float(rows[idx][:, :, outside].abs().max()) == 0.0
    dbg.note(f"S={S}: F={F}, {n_atoms} atoms, species rows {counts.tolist()}, segments of {3 * n_atoms // S} rows")


# ------------------------------------------------------------------------------------------------ fit and histograms
def test_four_species_fit_through_both_accumulators(dbg):
    """WeightedLinearModel on S = 4: the library's fit accumulator and the torch-backed one (several chunks) against the oracle's
    fit on the rows, tolerances of test_native_fit_accumulator_matches_the_torch_backed_one_and_the_oracle."""
    from uf3_amd import pipeline
    els = ELEMENTS[4]
    basis = dbg.basis(synthetic.notebook_basis(els))
    frames = [_all_species_frame(_z(els), (3 + k % 2, 3, 3 + k % 3), 3.165, 500 + k) for k in range(8)]
    fz = process.BasisFeaturizer(basis)
    reg = basis.get_regularization_matrix(ridge_1b=1e-8, ridge_2b=0.0, ridge_3b=1e-8, curvature_2b=1e-8, curvature_3b=0.0)
    x_e, x_f, off = fz.featurize_frames(frames)
    x_f = x_f.reshape(-1, basis.n_feats)
    rng = np.random.default_rng(28)
    c_true = rng.normal(0, 1, basis.n_feats)
    c_true[basis.col_idx] = 0
    energies = x_e @ c_true + rng.normal(0, 1e-3, len(frames))
    forces_flat = x_f @ c_true + rng.normal(0, 1e-3, len(x_f))
    forces = [forces_flat[3 * off[k]:3 * off[k + 1]].reshape(-1, 3) for k in range(len(frames))]
    model = ls.WeightedLinearModel(basis, regularizer=reg)
    native = pipeline.NativeFitAccumulator(model, fz, max_atoms_per_chunk=150)
    native.add_frames(frames, energies, forces)
    assert native.n_chunks >= 3
    pieces = native.pieces()
    n = x_e[:, :4].sum(axis=1)
    assert np.array_equal(n, [len(f) for f in frames])
    ref = O.fit(basis, reg, x_e / n[:, None], energies / n, x_f, forces_flat, weight=0.3)
    for key in ("gram_e", "gram_f", "ord_e", "ord_f"):
        assert rel_err(pieces[key], ref[key]) < 1e-9, key
    torch_backed = pipeline.DeviceFitAccumulator(model, fz, max_atoms_per_chunk=150)
    torch_backed.add_frames(frames, energies, forces)
    other = torch_backed.pieces()
    for key in pieces:
        assert rel_err(pieces[key], other[key]) < 1e-11, key
    model.fit_from_pieces(pieces, weight=0.3)
    assert rel_err(model.predict(x_f), x_f @ ref["coefficients"]) < 1e-6


@pytest.mark.parametrize("n_bins,r_max", [(400, 10.0), (1200, 12.0)])
def test_eight_species_pair_histogram(n_bins, r_max, dbg):
    """36 species pairs: [36][400] int32 counters fit the kernel's 64 KB of LDS, [36][1200] take the global-atomics route;
    integer-equal to the NumPy restatement, with and without rattle."""
    from uf3_amd.data import analyze
    from test_gpu_analyze import restated
    species = _z(ELEMENTS[8])
    atoms = _all_species_frame(species, (4, 4, 5), 3.165, 11)
    edges = np.linspace(0, r_max, n_bins + 1)
    assert (36 * n_bins * 4 <= 65536) == (n_bins == 400)
    for rattle in (0.0, 0.03):
        got, pairs = analyze.pair_histograms([atoms], species, edges, 0.0, r_max, rattle=rattle)
        assert len(pairs) == 36 and got.shape == (36, n_bins)
        want = restated(atoms, species, edges, r_max, True, rattle=rattle)
        assert (want.sum(axis=1) > 0).all()
        np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------ limits
def test_nine_species_are_refused_and_the_context_carries_on(dbg):
    """A 9-species basis (the host ChemicalSystem takes it) is refused by uf3_basis_create with UF3_EINVAL and a message naming
    the range; the context then featurizes an 8-species frame as before.  A frame with an element outside an 8-species basis
    raises SpeciesError."""
    nine = ELEMENTS[8] + ['Og']
    basis9 = bspline.BSplineBasis(composition.ChemicalSystem(nine, 2))
    with pytest.raises(_lib.UF3Error) as err:
        _lib.device_basis(basis9, _lib.get_context(None))
    assert err.value.code == 1 and "1..8 species" in str(err.value), str(err.value)
    d, meta, atoms = load_case("case_bcc16_s8")
    basis = dbg.basis(basis_from_meta(meta))
    fz = process.BasisFeaturizer(basis)
    x_e, x_f, _ = fz.featurize_frames([atoms])
    _check_rows(basis, [atoms], x_e, x_f, "after the refusal", [{"xe": d["xe"], "xf": d["xf"]}])
    foreign = Atoms(numbers=np.where(atoms.get_atomic_numbers() == 40, 41, atoms.get_atomic_numbers()),
                    positions=atoms.get_positions(), cell=atoms.get_cell(), pbc=True)
    with pytest.raises(_lib.SpeciesError):
        fz.featurize_frames([foreign])
    x_e2, x_f2, _ = fz.featurize_frames([atoms])
    assert rel_err(x_e2, x_e) < 1e-12 and rel_err(x_f2, x_f) < 1e-12
