"""
Every featurizer and evaluator route the library's own debug lines tell apart, held to the extended-precision oracle: each
entry of every result within ``GAMMA u M`` of the ``long double`` value (tests/_precision.py; GAMMA = 16 max(rho_o, 1) with rho_o
the fp64 oracle's own worst ratio, measured on the CPU and never from a device result).  No entry is left out.  Every test
asserts from the launch reports (UF3_DEBUG_LDS, read when the context is made) that the route it means ran, and prints
``[precision] route, case: worst ratio per kind``; ``tools/precision_ratios.py`` collects those lines into
``profiles/precision_ratios.json``.

The frames are the smallest that reach every instance (at most 72 atoms); the references are computed once per case and shared.
"""
import ctypes as C
import re

import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.forcefield import calculator
from uf3_amd.regression import least_squares as ls
from uf3_amd.representation import process
import _precision as P
from _util import dbg  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

# case -> (window rows x columns, rounds) of its k_featurize3 instance, and the list capacity its tuned call is laid out for
# (None: whatever the cell needs -- recorded, not asserted)
FEAT3 = {"mow_cap16": ((3, 9, 1), 16), "w_cap16": ((3, 9, 1), 16), "mow_cap24": ((3, 9, 1), 24), "mow_cap32": ((3, 9, 1), 32),
         "w_sparse_generic": ((3, 9, 1), 8), "mow_2x7": ((2, 7, 1), None), "mow_4x11": ((4, 11, 2), None),
         "w_5x13": ((5, 13, 3), None), "mow_lead0": ((6, 12, 3), None), "uneven_lead3": ((3, 9, 1), None),
         "uneven_lead0": ((6, 12, 3), None), "bcc24_s4": (None, None), "w16_sym3": (None, None), "triclinic_thin": ((6, 12, 3), None),
         "cluster": ((6, 12, 3), None)}
# case -> the matrix-core mode bit its basis takes under UF3_NO_FEAT3 (tests/test_gpu_parity.py)
MFMA_BIT = {"mow_2x7": 6, "mow_cap16": 7, "mow_4x11": 8, "w_5x13": 9, "mow_lead0": 9, "uneven_lead3": 7, "bcc24_s4": None,
            "w16_sym3": None}
# case -> an output-stationary mode its basis must launch under UF3_NO_MFMA_FEAT (1 / 2: one source bin a column, 3 / 4: two, 5: six)
GENERIC_MODE = {"w16_sym3": 5, "mow_2x7": 1, "mow_cap16": 2, "uneven_lead3": 3, "w_5x13": 4}


# The launches that evaluate the 3-body leg functions from window rows of local cubic pieces (uf3_feat3.h: f3_eval; the grouped
# windows of the matrix-core launch, modes 7 and 10): their rows are held to the magnitudes widened for that (uf3_oracle.c:
# piece_abs, tests/_precision.py: ratios).  Every other launch is held to the plain ones.
PIECE_MODES = {7, 10}


def _check(route, name, got, pieces=False):
    r = P.ratios(got, name, pieces=pieces)
    assert r, (route, name)
    print(f"[precision] {route}{' (piece magnitudes)' if pieces else ''}, {name}: {P.fmt(r)}")
    for k, v in r.items():
        assert v <= P.GAMMA[k], (route, name, k, v, P.GAMMA[k])
    return r


@pytest.fixture
def fresh(monkeypatch, capfd):
    """``fresh(name, **env)`` -> (featurizer, basis, atoms) on a context and device tables of their own, made under ``env`` with
    the launch reports on; ``fresh.said()`` returns the reports since the last look."""
    made = []

    def make(name, **env):
        basis, atoms, _ = P.cases()[name]
        P.reference(name)                                             # (asserts the frame clear of discontinuities)
        monkeypatch.setenv("UF3_DEBUG_LDS", "1")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        monkeypatch.setattr(_lib, "_contexts", {})
        _lib.drop_device_basis(basis)
        made.append(basis)
        capfd.readouterr()
        return process.BasisFeaturizer(basis), basis, atoms

    def said():
        cap = capfd.readouterr()
        print(cap.out, end="")
        return cap.err

    make.said = said
    yield make
    for b in made:
        _lib.drop_device_basis(b)


def _rows(fz, atoms, **kw):
    x_e, x_f, _ = fz.featurize_frames([atoms], **kw)
    return {"xe": None if x_e is None else x_e[0], "xf": None if x_f is None else x_f.reshape(len(atoms), 3, -1)}


def _modes_launched(err):
    return sorted({int(m) for m in re.findall(r"uf3 featurize mode (\d+):", err)})


# ================================================================================================ featurizer
@pytest.mark.parametrize("name", list(FEAT3))
def test_bond_factorised_launch_and_pair_launch(name, fresh):
    """The pair launch (mode 0) + k_featurize3 on every instance -- (window rows, rounds) = (3, 1) at list capacity 16, 24, 32 and
    the generic one, (4, 2), (5, 3), (6, 3) -- with and without the energy row, on a context's first call (estimated capacity) and
    on its tuned call; and the energy-only call (the dense loops of the generic / matrix-core launches)."""
    fz, basis, atoms = fresh(name)
    window, cap = FEAT3[name]
    modes = fz._dev()[1].featurizer_modes
    if window is not None:
        assert modes & 0x1000, hex(modes)
    for call in ("first", "tuned"):
        both = _rows(fz, atoms)
        alone = _rows(fz, atoms, energy=False)
        err = fresh.said()
        assert 0 in _modes_launched(err), err
        if modes & 0x1000:
            lines = re.findall(r"uf3 featurize3: .*?, cap (\d+) \(lists \d+ apart\), selection \d+, .*?window (\d+) x (\d+), (\d+) round", err)
            assert len(lines) >= 2 and _modes_launched(err) == [0], err              # (with and without the energy row)
            if window is not None:
                assert {tuple(int(x) for x in ln[1:]) for ln in lines} == {window}, err
            if cap is not None and call == "tuned":
                # (lists longer than 16: a launch laid out for 16 in front, which leaves at once where the lists are longer)
                assert {int(ln[0]) for ln in lines} == ({cap} if cap <= 16 else {16, cap}), err
                assert err.count(f", cap {cap} (lists") == 2, err
            route = f"k_featurize3 {'x'.join(lines[-1][1:3])} r{lines[-1][3]} cap{lines[-1][0]} {call} call"
        else:
            route = f"featurize modes {_modes_launched(err)} {call} call"
        pieces = bool(modes & 0x1000 or set(_modes_launched(err)) & PIECE_MODES)
        _check(route + ", energy + force rows", name, both, pieces)
        _check(route + ", force rows alone", name, alone, pieces)
    e_only = _rows(fz, atoms, forces=False)
    err = fresh.said()
    launched = _modes_launched(err)
    assert "uf3 featurize3" not in err and 0 in launched and max(launched) >= 1, err
    _check(f"featurize modes {launched}, energy row alone", name, e_only, bool(set(launched) & PIECE_MODES))


def test_image_route_for_atoms_outside_the_cell(fresh):
    """A slab with atoms outside its cell: the pair launch and the 3-body launches on their image-range instances (the basis
    qualifies for k_featurize3, which leaves such a batch to them), rows as the reference defines them for positions as given."""
    fz, basis, atoms = fresh("slab_outside")
    assert fz._dev()[1].featurizer_modes & 0x1000
    frac = np.asarray(atoms.get_positions()) @ np.linalg.inv(np.asarray(atoms.get_cell(), float).reshape(3, 3))
    assert ((frac[:, :2] < 0) | (frac[:, :2] >= 1)).any()
    for call in ("first", "tuned"):
        both = _rows(fz, atoms)
        alone = _rows(fz, atoms, energy=False)
        err = fresh.said()
        launched = _modes_launched(err)
        # (a context starts on the ordinary launches, k_featurize3 among them, which leave such a batch alone and say so: the
        # entry repeats the call on the image route and stays there)
        assert 0 in launched and max(launched) >= 1 and not set(launched) & PIECE_MODES, err
        assert call == "first" or "uf3 featurize3" not in err, err
        _check(f"image route, featurize modes {launched} {call} call, energy + force rows", "slab_outside", both)
        _check(f"image route, featurize modes {launched} {call} call, force rows alone", "slab_outside", alone)


@pytest.mark.parametrize("generic", [False, True], ids=["matrix_core", "generic"])
@pytest.mark.parametrize("name", list(MFMA_BIT))
def test_matrix_core_and_generic_trio_launches(name, generic, fresh):
    """UF3_NO_FEAT3: the fp64 matrix-core launches (mode bits 6, 7, 8, 9; 10 and 11 are the grouped / banded forms of 7 and 9 the
    launch report names); with UF3_NO_MFMA_FEAT as well, the output-stationary launches (modes 1 to 5).  Energy + force rows,
    force rows alone, energy row alone."""
    env = {"UF3_NO_FEAT3": "1", **({"UF3_NO_MFMA_FEAT": "1"} if generic else {})}
    fz, basis, atoms = fresh(name, **env)
    modes = fz._dev()[1].featurizer_modes
    assert not modes & 0x1000, hex(modes)
    if generic:
        assert not modes & 0x3c0 and modes & 0x3e, hex(modes)
    elif MFMA_BIT[name] is not None:
        assert modes & (1 << MFMA_BIT[name]), hex(modes)
    else:
        assert modes & 0x3c0, hex(modes)
    for call in ("first", "tuned"):
        both = _rows(fz, atoms)
        alone = _rows(fz, atoms, energy=False)
        e_only = _rows(fz, atoms, forces=False)
        err = fresh.said()
        launched = _modes_launched(err)
        assert "uf3 featurize3" not in err and 0 in launched and max(launched) >= 1, err
        if generic:
            assert set(launched) <= {0, 1, 2, 3, 4, 5}, launched
            assert GENERIC_MODE.get(name, launched[-1]) in launched, launched
        else:
            assert set(launched) & {6, 7, 8, 9, 10, 11}, launched
        route = f"{'generic' if generic else 'matrix-core'} featurize modes {launched} {call} call"
        pieces = bool(set(launched) & PIECE_MODES)
        assert pieces == (not generic and (MFMA_BIT[name] == 7 or name == "bcc24_s4")), launched
        _check(route + ", energy + force rows", name, both, pieces)
        _check(route + ", force rows alone", name, alone, pieces)
        _check(route + ", energy row alone", name, e_only, pieces)


@pytest.mark.parametrize("name,want", [("mow_cap16", "lds"), ("w_cap16", "lds"), ("mow_lead0", "hbm"), ("uneven_lead3", "lds"),
                                       ("bcc24_s4", None), ("triclinic_thin", "hbm"), ("cluster", "hbm")])
def test_virial_rows_on_both_routes(name, want, fresh):
    """uf3_featurize_virial: the six strain rows kept in LDS, and added straight to HBM where they do not fit (F = 1798), with
    the energy and force rows of the same call, and the strain rows alone."""
    fz, basis, atoms = fresh(name)
    ctx, db = fz._dev()
    batch = _lib.FrameBatch([atoms])
    F = db.n_feat
    for call in ("first", "tuned"):
        x_e, x_f, x_v = np.empty((1, F)), np.empty((batch.n_atoms, 3, F)), np.empty((1, 6, F))
        ctx.check(ctx.lib.uf3_featurize_virial(db.handle, C.byref(batch.struct), _lib._p(batch.pos), _lib._p(batch.z),
                                               _lib._p(x_e), _lib._p(x_f), _lib._p(x_v)))
        alone = fz.featurize_virials([atoms])
        err = fresh.said()
        routes = {int(m.group(1)): m.group(2) for m in re.finditer(r"uf3 virial rows mode (\d+): lds \d+ B, rows in (lds|hbm)", err)}
        trio = {r for m, r in routes.items() if m >= 1}
        assert routes.get(0) == "lds" and trio, err
        if want is not None:
            assert trio == {want}, routes
        route = f"virial rows in {'/'.join(sorted(trio))} {call} call"
        # (the energy and force rows of the call come from the pair launch + k_featurize3 or the grouped launch; the strain rows
        # from k_virial_rows, which evaluates the recursion: plain magnitudes)
        assert "uf3 featurize3" in err or set(_modes_launched(err)) & PIECE_MODES, err
        _check(route + ", its energy and force rows", name, {"xe": x_e[0], "xf": x_f}, True)
        _check(route + ", with energy and force rows", name, {"xv": x_v[0]})
        _check(route + ", alone", name, {"xv": alone[0]})


# ================================================================================================ evaluator
EVAL_CASES = ["mow_cap16", "mow_cap32", "w_cap16", "mow_lead0", "uneven_lead3", "bcc24_s4", "w16_sym3", "triclinic_thin", "cluster"]


def _calc(basis, name, skin):
    model = ls.WeightedLinearModel(basis)
    model.coefficients = P.reference(name)[1].copy()              # (seeded as _on_knots.coefficients: frozen entries zero)
    return calculator.UFCalculator(model, md_skin=skin)


def _results(out, virial):
    return {"e": out[0][0], "f": out[1], "v": out[3][0] if virial else None}


def _flags(s):
    return " ".join(f"{k}={s[k]}" for k in ("cw", "win", "tab", "gather", "md", "cap16", "vir", "centres"))


_SWITCHES = {"default": {}, "no_cw": {"UF3_EVAL_NO_CW": "1"}, "no_tab": {"UF3_EVAL_NO_TAB": "1"},
             "no_cap16": {"UF3_EVAL_NO_CAP16": "1"}, "gather": {"UF3_EVAL_GATHER": "1"}}


@pytest.mark.parametrize("name", EVAL_CASES)
def test_plain_route_and_its_switches(name, dbg, monkeypatch):
    """md_skin = 0 on a tuned context: the centre pass + collection pass as it comes (tab / win as the basis and the lists
    allow), without the window table, without the per-bond table, without the capacity-16 instances, through the gather
    instance (UF3_EVAL_GATHER, and a call without forces) -- each with and without the strain derivative."""
    basis, atoms, _ = P.cases()[name]
    dbg.basis(basis)
    calc = _calc(basis, name, 0.0)
    for _ in range(2):
        calc.evaluate_frames([atoms], virial=True)                     # (list capacity tuned)
    dbg.launches()
    seen = set()
    for switch, env in _SWITCHES.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for virial in (True, False):
            out = calc.evaluate_frames([atoms], virial=virial)
            said = dbg.launches()
            assert said and all(s["vir"] == int(virial) and s["md"] == 0 for s in said), said
            if switch == "gather":
                assert all(s["gather"] == 1 for s in said), said
            if switch == "no_tab":
                assert all(s["tab"] == 0 and s["win"] == 0 and s["cw"] == 0 for s in said), said
            if switch == "no_cw":
                assert all(s["cw"] == 0 and s["win"] == 0 for s in said), said
            if switch == "no_cap16":
                assert all(s["cap16"] == 0 for s in said), said
            seen.update(_flags(s) for s in said)
            _check(f"k_eval plain {switch} [{_flags(said[-1])}]", name, _results(out, virial))
        for k in env:
            monkeypatch.delenv(k)
    for virial in (True, False):
        e, f, _, *v = calc.evaluate_frames([atoms], forces=False, virial=virial)
        said = dbg.launches()
        assert f is None and said and all(s["gather"] == 1 and s["vir"] == int(virial) for s in said), said
        _check(f"k_eval no forces [{_flags(said[-1])}]", name, {"e": e[0], "v": v[0][0] if virial else None})
    print(f"k_eval instances of {name}:\n  " + "\n  ".join(sorted(seen)))


@pytest.mark.parametrize("name", ["mow_cap16", "mow_cap32", "bcc24_s4"])
def test_blocks_of_atoms_and_of_centres(name, dbg):
    """uf3_eval_atoms (the gather instance on an atom range) and uf3_eval_centres (the centre pass on a block + its halo): three
    shares, summed (two additions an entry, within the bound's margin), with and without the strain derivative."""
    from uf3_amd import parallel
    basis, atoms, _ = P.cases()[name]
    dbg.basis(basis)
    calc = _calc(basis, name, 0.0)
    for _ in range(2):
        calc.evaluate_frames([atoms], virial=True)
    dbg.launches()
    n = len(atoms)
    for which in ("atoms", "centres"):
        share = calc.evaluate_atom_range if which == "atoms" else calc.evaluate_centre_range
        for virial in (True, False):
            parts = [share(atoms, *parallel.shard_range(n, r, 3), virial=virial) for r in range(3)]
            said = dbg.launches()
            assert len(said) >= 3 and all(s["vir"] == int(virial) and s["centres"] == int(which == "centres") for s in said), said
            assert all(s["gather"] == int(which == "atoms") for s in said), said
            _check(f"k_eval block of {which} x 3 [{_flags(said[-1])}]", name,
                   {"e": sum(p[0] for p in parts), "f": sum(p[1] for p in parts), "v": sum(p[2] for p in parts) if virial else None})


_MD = {"default": ({}, {"md": 1, "gather": 0}), "no_cw": ({"UF3_EVAL_NO_CW": "1"}, {"md": 1, "cw": 0}),
       "no_cap16": ({"UF3_EVAL_NO_CAP16": "1"}, {"md": 1, "cap16": 0})}


@pytest.mark.parametrize("name", ["mow_cap16", "mow_cap32", "w_cap16", "triclinic_thin", "cluster", "bcc24_s4"])
def test_md_list_route(name, dbg, monkeypatch):
    """The MD-list route (md_skin 0.5, persistent lists) on a tuned context, with and without the CW instances and the
    capacity-16 instances, with and without the strain derivative, on the frame the lists were built for and on its second call
    (lists reused)."""
    basis, atoms, _ = P.cases()[name]
    dbg.basis(basis)
    plain = _calc(basis, name, 0.0)
    for _ in range(2):
        plain.evaluate_frames([atoms], virial=True)
    cw_seen = set()
    for switch, (env, want) in _MD.items():
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        calc = _calc(basis, name, 0.5)
        dbg.launches()
        for step, virial in enumerate((True, False, True)):
            out = calc.evaluate_frames([atoms], virial=virial)
            said = dbg.launches()
            assert said and said[-1]["vir"] == int(virial), said
            for key, val in want.items():
                assert said[-1][key] == val, (switch, step, said)
            cw_seen.add(said[-1]["cw"])
            _check(f"k_eval md {switch} step {step} [{_flags(said[-1])}]", name, _results(out, virial))
        for k in env:
            monkeypatch.delenv(k)
    if name in ("mow_cap16", "w_cap16"):
        assert cw_seen == {0, 1}, cw_seen                              # (lists of at most 16 entries: the CW instances ran)
