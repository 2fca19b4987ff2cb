"""The plan ``uf3_basis_create`` makes of a basis, on the host alone (``uf3_basis_plan_debug``: the pure function ``basis_plan`` that
``uf3_basis_create`` itself calls and then uploads, no device).

1. Every table of every basis in ``_basis_plans.CASES`` hashes to tests/golden/basis_plan.json, recorded from the parent of the
   commit that introduced ``basis_plan`` (see tests/_basis_plans.py), and the readable summary is equal; the cases together reach
   every layout decision the function takes.
2. The content, independently of the library: window rows against ``bspline.basis_values``, knot records shared by identical
   sequences, column sources inside the window and in agreement with the LUT.
3. Every refusal, with its message."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.representation import bspline
import _basis_plans as BP

F3 = 1 << 12
HOST_PAIRS, PAIR_BYTES = 1608, 80                    # BasisDev::pairs, sizeof(PairDev): a LegDev, four ints, four doubles


@functools.lru_cache(maxsize=None)
def golden():
    with open(BP.golden_path()) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def plan(name, switches):
    return BP.tables(BP.spec(name)[0], switches)


def _kinds(entry):
    return [t for _, t in entry["trios"]]


# ------------------------------------------------------------------------------------------------ 1. the parent's bytes
@pytest.mark.parametrize("name,switches", BP.CASES, ids=[BP.key(*c) for c in BP.CASES])
def test_every_table_is_the_parents(name, switches):
    want, got = golden()[BP.key(name, switches)], BP.entry(plan(name, switches))
    assert got["summary"] == want["summary"]
    assert got["trios"] == want["trios"]
    assert got["bytes"] == want["bytes"]
    assert got["sha256"] == want["sha256"], [t for t in BP.TABLES if got["sha256"][t] != want["sha256"][t]]


def test_the_cases_reach_every_decision():
    """Over the golden summaries: what the list of bases is there for."""
    g = golden()
    assert list(g) == [BP.key(*c) for c in BP.CASES]
    sm = {k: v["summary"] for k, v in g.items()}
    kinds = {k: _kinds(v) for k, v in g.items()}
    every = [t for ts in kinds.values() for t in ts]
    modes = functools.reduce(int.__or__, (s["modes"] for s in sm.values()))
    vmodes = functools.reduce(int.__or__, (s["vmodes"] for s in sm.values()))
    assert all(modes >> b & 1 for b in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12)) and all(vmodes >> b & 1 for b in (1, 2, 3, 4, 5))
    assert any(t["dense"] == 7 and t["grouped"] for t in every)
    # two trios on one layout; two layouts in one basis
    assert sum(n for n, t in g["notebook_mow_lead3/0"]["trios"] if t["grouped"] and t["layout"] == 0) >= 2
    assert any(len({t["layout"] for t in ts if t["grouped"]}) > 1 for ts in kinds.values())
    assert any(t["dense"] == 9 and t["banded"] and min(t["thr"][2:]) < 1e299 for t in every)          # a finite band threshold
    assert any(t["dense"] == 7 and abs(t["thr"][0]) < 1e299 and abs(t["thr"][1]) < 1e299 for t in every)   # thr0 and thr2
    assert {s["f3_nr"] for s in sm.values() if s["feat3_ok"]} == {1, 2, 3}
    assert not sm["grid_binary/0"]["feat3_ok"] and not sm["grid_binary/0"]["trio_legs_uniform"]               # non-uniform legs
    assert not sm["grid_wide/0"]["feat3_ok"] and sm["grid_wide/0"]["trio_legs_uniform"]                # the window's shape
    assert sm["notebook_mow_lead3/0"]["feat3_ok"] and not sm[f"notebook_mow_lead3/{BP.NO_FEAT3}"]["feat3_ok"]
    assert sm["notebook_mow_lead3/0"]["modes"] & 0x3c0 and not sm[f"notebook_mow_lead3/{BP.NO_MFMA_FEAT}"]["modes"] & 0x3c0
    assert {s["eval_cw_ok"] for s in sm.values()} == {0, 1} and {s["eval_tab_ok"] for s in sm.values()} == {0, 1}
    assert {s["pairs_uniform"] for s in sm.values()} == {0, 1}
    n_species = {sum(1 for n in s["sp_ncols"] if n) for s in sm.values()}
    assert {1, 8} <= n_species
    assert g["two_body_mow/0"]["bytes"]["trios"] == 0 and g["two_body_mow/0"]["summary"]["c3_len"] == 0
    assert [t["nsrc"] for t in _kinds(g["raw_bins/0"])] == [1]


def test_the_switches_decide_nothing_else():
    """UF3_NO_FEAT3 takes bit 12 and the k_featurize3 tables and leaves every other table alone"""
    a, b = plan("notebook_mow_lead3", 0), plan("notebook_mow_lead3", BP.NO_FEAT3)
    for t in BP.TABLES:
        if t in ("f3rows", "f3src", "f3off"):
            assert len(a[t]) and not len(b[t])
        elif t != "summary":
            assert a[t] == b[t], t
    assert BP.summary(a)["modes"] == BP.summary(b)["modes"] | F3


# ------------------------------------------------------------------------------------------------ 2. the content
def _leg_knots(keep):
    """[trio][leg] -> knots"""
    cuts = np.concatenate([[0], np.cumsum(keep["trio_nk"].ravel())])
    return [[keep["trio_knots"][cuts[3 * t + d]:cuts[3 * t + d + 1]] for d in range(3)] for t in range(len(keep["trio_nk"]))]


def _check_rows(rows, knots, window, label):
    """rows [nk - 7][18] of one leg against basis_values: ``window(i) -> (w_lo, w_ext, sb)`` restates the slot rule"""
    nk = len(knots)
    assert len(rows) == nk - 7
    n_checked = 0
    for i in range(3, nk - 4):
        row = rows[i - 3]
        assert row[0] == knots[i] and row[1] == knots[i + 1], label
        w_lo, w_ext, sb = window(i)
        coef = row[2:].reshape(4, 4)
        x = knots[i] + np.array([0.25, 0.5, 0.75]) * (knots[i + 1] - knots[i])
        first, values, _ = bspline.basis_values(knots, x)
        u = x - knots[i]
        for fq in range(4):
            if sb + fq >= w_ext:
                assert not coef[fq].any(), (label, i, fq)           # past the window: exactly zero
                continue
            j = w_lo + sb + fq
            got = coef[fq, 0] + u * (coef[fq, 1] + u * (coef[fq, 2] + u * coef[fq, 3]))
            want = np.array([values[k, j - first[k]] if 0 <= j - first[k] <= 3 and 0 <= j <= nk - 5 else 0.0 for k in range(3)])
            if knots[i + 1] > knots[i]:
                assert np.allclose(got, want, rtol=1e-12, atol=1e-13), (label, i, fq, got, want)
                n_checked += want.any()
    return n_checked


@pytest.mark.parametrize("name", ["notebook_mow_lead3", "uneven_lead3", "mixed_trios_5_species", "asymmetric_window"])
def test_window_rows_of_the_grouped_layouts(name):
    tab, keep = plan(name, 0), BP.spec(name)[1]
    sm, trios, knots = BP.summary(tab), BP.trios(tab), _leg_knots(keep)
    assert sm["n_wrows"] > 0
    doubles = np.frombuffer(tab["recs"], dtype=np.float64)[12 * sm["wrow_lo"]:]
    assert len(doubles) == -(-18 * sm["n_wrows"] // 12) * 12 and not doubles[18 * sm["n_wrows"]:].any()
    rows = doubles[:18 * sm["n_wrows"]].reshape(-1, 18)
    n_checked, layouts = 0, set()
    for t, td in enumerate(trios):
        if not td["grouped"]:
            continue
        layouts.add(int(td["layout"]))
        lo, ext = td["lo"], td["ext"]

        def window(a, i):
            if a < 2:
                return int(lo[a]), int(ext[0]) if a == 0 else 3, 0
            f = i - 3 - int(lo[2])
            grp = 0 if f <= 1 else (2 if f >= 4 else 1)
            return int(lo[2]) + 2 * grp, min(5, int(ext[2]) - 2 * grp), max(0, min(1, f - 2 * grp))
        for a in range(3):
            nk = len(knots[t][a])
            n_checked += _check_rows(rows[td["wrow"][a]:td["wrow"][a] + nk - 7], knots[t][a], functools.partial(window, a), (name, t, a))
    assert n_checked > 0 and layouts == set(range(len(layouts)))


@pytest.mark.parametrize("name", ["notebook_w_lead3", "notebook_mow_lead0", "resolution_5_5_10", "resolution_7_7_14",
                                  "resolution_8_8_16_w", "grid_nonuniform_lead3", "notebook_8_species"])
def test_window_rows_of_k_featurize3(name):
    tab, keep = plan(name, 0), BP.spec(name)[1]
    sm, knots = BP.summary(tab), _leg_knots(keep)
    assert sm["feat3_ok"]
    rows = np.frombuffer(tab["f3rows"], dtype=np.float64).reshape(-1, 18)
    assert len(rows) == sm["n_f3rows"]
    n_checked = 0
    for kind, a, w_lo, w_ext in ((0, 0, sm["f3_lo_p"], sm["f3_ext_p"]), (1, 2, sm["f3_lo_n"], sm["f3_ext_n"])):
        nk, row0 = int(sm["f3_leg_nk"][kind]), int(sm["f3_leg_row0"][kind])
        assert nk == len(knots[0][a])
        n_checked += _check_rows(rows[row0:row0 + nk - 7], knots[0][a],
                                 lambda i: (int(w_lo), int(w_ext), max(0, min(max(0, int(w_ext) - 4), i - 3 - int(w_lo)))), (name, kind))
    assert n_checked > 0


@pytest.mark.parametrize("name", ["notebook_mow_lead3", "uneven_lead0", "grid_binary", "notebook_8_species", "raw_bins"])
def test_identical_knot_sequences_share_their_records(name):
    tab, keep = plan(name, 0), BP.spec(name)[1]
    host, sm = tab["host"], BP.summary(tab)
    cuts = np.concatenate([[0], np.cumsum(keep["pair_nk"])])
    legs = [(keep["pair_knots"][cuts[p]:cuts[p + 1]],
             np.frombuffer(host, dtype=BP.LEG, count=1, offset=HOST_PAIRS + PAIR_BYTES * p)[0]) for p in range(len(keep["pair_nk"]))]
    for t, td in enumerate(BP.trios(tab)):
        legs += [(_leg_knots(keep)[t][d], td["leg"][d]) for d in range(3)]
    seen = {}
    for k, leg in legs:
        assert leg["nk"] == len(k) and leg["t0"] == k[0] and leg["tlast"] == k[-1]
        assert 0 <= leg["rec_off"] and leg["rec_off"] + len(k) - 1 <= sm["wrow_lo"]
        assert seen.setdefault(k.tobytes(), int(leg["rec_off"])) == leg["rec_off"]
    assert len(seen) < len(legs)                              # (something was shared)
    # and the records are the sequence's: the six knots around interval i
    recs = np.frombuffer(tab["recs"], dtype=np.float64).reshape(-1, 12)
    for k, leg in legs:
        for i in range(3, len(k) - 4):
            assert np.array_equal(recs[leg["rec_off"] + i, :6], k[i - 2:i + 4])


@pytest.mark.parametrize("name", ["notebook_mow_lead3", "notebook_w_lead0", "uneven_lead3", "sym3_unary", "raw_bins"])
def test_column_sources_lie_in_the_window_and_agree_with_the_lut(name):
    tab = plan(name, 0)
    colsrc, lut = np.frombuffer(tab["colsrc"], dtype=np.int32), np.frombuffer(tab["lut"], dtype=np.int32)
    n_src = 0
    for td in BP.trios(tab):
        src = colsrc[td["src_off"]:td["src_off"] + td["ncol"] * td["nsrc"]].reshape(td["ncol"], td["nsrc"])
        for col, row in enumerate(src):
            live = row[row >= 0]
            assert np.all(row[len(live):] == -1) and len(set(live.tolist())) == len(live)
            lmn = np.stack([live & 255, (live >> 8) & 255, (live >> 16) & 255], axis=1)
            assert np.all(lmn >= td["lo"]) and np.all(lmn < td["lo"] + td["ext"])
            at = td["lut_off"] + (lmn[:, 0] * td["dim_m"] + lmn[:, 1]) * td["dim_n"] + lmn[:, 2]
            assert np.all(lut[at] == td["col"] + col)
            n_src += len(live)
        grid = lut[td["lut_off"]:td["lut_off"] + td["dim_l"] * td["dim_m"] * td["dim_n"]]
        assert np.count_nonzero(grid >= 0) == np.count_nonzero(src >= 0)          # every kept raw bin is some column's source
    assert n_src > 0


# ------------------------------------------------------------------------------------------------ 3. refusals
def _respec(keep, s0, **scalars):
    s = _lib.BasisSpec()
    for f, _ in _lib.BasisSpec._fields_:
        setattr(s, f, getattr(s0, f))
    for name in ("species_z", "pair_z", "pair_nk", "pair_knots", "pair_rmin", "pair_rmax", "pair_col",
                 "trio_z", "trio_nk", "trio_knots", "trio_col", "trio_ncol", "trio_lut"):
        setattr(s, name, _lib._p(keep[name]))
    for f, v in scalars.items():
        setattr(s, f, v)
    return s


def _mutated(what):
    """(spec, keep-alive) of the Mo / W notebook basis with one thing wrong"""
    s0, keep0 = BP.spec("notebook_mow_lead3")
    keep = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in keep0.items()}
    scalars = {}
    if what == "species count":
        scalars["n_species"] = 9
    elif what == "n_pairs":
        scalars["n_pairs"] = 2
    elif what == "species order":
        keep["species_z"][:] = [74, 42]
    elif what == "pair species":
        keep["pair_z"][1, 1] = 13
    elif what == "pair atomic number":
        keep["pair_z"][0, 0] = 120
    elif what == "pair knots":
        keep["pair_nk"][0] = 7
    elif what == "pair column":
        keep["pair_col"][0] = -1
    elif what == "trio species":
        keep["trio_z"][0, 0] = 13
    elif what == "trio neighbour order":
        keep["trio_z"][1] = [42, 74, 42]
    elif what == "trio atomic number above":
        keep["trio_z"][2, 1] = 500
    elif what == "trio atomic number below":
        keep["trio_z"][2, 2] = -3
    elif what == "trio column":
        keep["trio_col"][1] = -5
    elif what == "trio width":
        keep["trio_ncol"][1] = -1
    elif what == "trio knots":
        keep["trio_nk"][0, 2] = 7
    elif what == "lut entry":
        keep["trio_lut"][np.flatnonzero(keep["trio_lut"] >= 0)[0]] = keep["trio_ncol"][0]
    elif what == "n_feat":
        scalars["n_feat"] = s0.n_feat + 1
    else:
        # hand-made W descriptions: a leg of 256 functions | every raw bin on one column
        k8 = np.repeat([1.5, 3.5], 4)
        if what == "grid dimension":
            k260 = np.concatenate([[1.5] * 3, np.linspace(1.5, 7.0, 254), [7.0] * 3])
            s, keep = _lib.flatten_raw([74], trios=[((74, 74, 74), [k8, k8, k260], np.full(4 * 4 * 256, -1, np.int32))])
        elif what == "bins per column":
            s, keep = _lib.flatten_raw([74], trios=[((74, 74, 74), [k8, k8, k8], np.r_[np.zeros(7, np.int32), np.full(57, -1, np.int32)])])
        return s, keep
    return _respec(keep, s0, **scalars), keep


REFUSALS = [("species count", "uf3_basis_create: 1..8 species supported"), ("n_pairs", "uf3_basis_create: n_pairs must be S(S+1)/2"),
            ("species order", "species_z must be ascending atomic numbers"),
            ("pair species", "bad pair block"), ("pair atomic number", "bad pair block"), ("pair knots", "bad pair block"),
            ("pair column", "bad pair block"),
            ("trio species", "bad trio block"), ("trio neighbour order", "bad trio block"), ("trio atomic number above", "bad trio block"),
            ("trio atomic number below", "bad trio block"), ("trio column", "bad trio block"), ("trio width", "bad trio block"),
            ("trio knots", "trio knot vector too short"), ("lut entry", "trio_lut entry out of range"),
            ("grid dimension", "3-body grid dimension > 255"), ("bins per column", "a 3-body column is fed by more than 6 raw bins"),
            ("n_feat", "column blocks do not add up to n_feat")]


@pytest.mark.parametrize("what,message", REFUSALS, ids=[w.replace(" ", "_") for w, _ in REFUSALS])
def test_a_bad_spec_is_refused(what, message):
    s, keep = _mutated(what)
    lib, n = _lib.load(), C.c_int64(-1)
    for table in (0, 2):
        assert lib.uf3_basis_plan_debug(C.byref(s), 0, table, None, 0, C.byref(n)) == 1          # UF3_EINVAL
        assert lib.uf3_last_error(None).decode() == message
    del keep


def test_the_valid_spec_the_refusals_start_from_and_the_entry_itself():
    s0, keep0 = BP.spec("notebook_mow_lead3")
    s = _respec(keep0, s0)
    assert BP.tables(s, 0) == plan("notebook_mow_lead3", 0)
    lib, n = _lib.load(), C.c_int64(-1)
    assert lib.uf3_basis_plan_debug(C.byref(s), 0, len(BP.TABLES), None, 0, C.byref(n)) == 1      # no such table
    buf = np.zeros(8, dtype=np.uint8)
    assert lib.uf3_basis_plan_debug(C.byref(s), 0, 2, buf.ctypes.data_as(C.c_void_p), 8, C.byref(n)) == 1 and not buf.any()
    assert lib.uf3_basis_plan_debug(None, 0, 0, None, 0, C.byref(n)) == 1
