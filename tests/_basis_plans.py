"""The bases tests/test_basis_plan_host.py pins, how a plan is read through ``uf3_basis_plan_debug``, and how a plan becomes an
entry of tests/golden/basis_plan.json.

The golden was recorded from the PARENT of the commit that split ``basis_plan`` from ``uf3_basis_create``: that commit's library
with profiles/basis_plan_parent_dump.patch applied (a dump of the host vectors in front of the uploads, ``uf3_basis_dump_debug``),
through ``python tests/_basis_plans.py <patched library> tests/golden/basis_plan.json``.  A later intended change of the plan is
recorded from the tree's own ``uf3_basis_plan_debug`` (``python tests/_basis_plans.py - tests/golden/basis_plan.json``) and shows up
as a diff of the readable summaries."""
import ctypes as C
import functools
import hashlib
import json
import os
import sys

import numpy as np

from uf3_amd import _lib, synthetic
import _bases
import _on_knots
import _precision
import _uneven
import test_oracle_virial as OV
from _util import basis_from_meta, load_case

NO_MFMA_FEAT, NO_FEAT3 = 1, 2                          # bits of `switches` (UF3_NO_MFMA_FEAT, UF3_NO_FEAT3)
ENV = {NO_MFMA_FEAT: "UF3_NO_MFMA_FEAT", NO_FEAT3: "UF3_NO_FEAT3"}
TABLES = ["summary", "host", "recs", "lut", "colsrc", "dsrc", "gsrc", "trios", "f3rows", "f3src", "f3off", "sp_cols", "bounds",
          "cw_lut_off", "cw_dim_l"]                    # selector of uf3_basis_plan_debug = position here
MAX_SPECIES = 8

i32, i64, f64 = np.int32, np.int64, np.float64
SUMMARY = np.dtype([("c2_len", i64), ("c3_len", i64), ("n_recs", i64), ("n_pair_recs", i64), ("trio_rec_lo", i64), ("wrow_lo", i64),
                    ("n_dsrc", i64), ("n_gsrc", i64), ("r_cut", f64), ("f3_leg", f64, (2, 3)), ("f3_leg_nk", i32, 2),
                    ("f3_leg_row0", i32, 2), ("n_wrows", i32), ("modes", i32), ("vmodes", i32), ("all_grouped7", i32),
                    ("all_banded9", i32), ("feat3_ok", i32), ("eval_tab_ok", i32), ("eval_cw_ok", i32), ("cw_lo", i32),
                    ("cw_ext", i32), ("cw_dim_m", i32), ("cw_dim_n", i32), ("cw_zero", i32), ("cw_bytes", i32), ("f3_lo_p", i32),
                    ("f3_ext_p", i32), ("f3_lo_n", i32), ("f3_ext_n", i32), ("f3_nr", i32), ("n_f3rows", i32), ("n_f3src", i32),
                    ("pairs_uniform", i32), ("trio_legs_uniform", i32), ("sp_ncols", i32, MAX_SPECIES), ("dense_stride", i32, 16),
                    ("dense_stride_f", i32, 16), ("dense_grouped", i32, 16), ("dense_dump", i32, 16)], align=True)
LEG = np.dtype([("rec_off", i32), ("nk", i32), ("t0", f64), ("tlast", f64), ("inv_h", f64)], align=True)
TRIO = np.dtype([("head", i32, 8), ("leg", LEG, 3), ("col", i32), ("ncol", i32), ("lut_off", i32), ("dim_m", i32), ("dim_n", i32),
                 ("dim_l", i32), ("sc", i32), ("sa", i32), ("sb", i32), ("nsrc", i32), ("src_off", i32), ("dense", i32),
                 ("lo", i32, 3), ("ext", i32, 3), ("thr0", f64), ("thr2", f64), ("gthr0", f64), ("gthr2", f64), ("grouped", i32),
                 ("banded", i32), ("band_tile", i32, 3), ("layout", i32), ("gsrc_off", i32), ("wrow", i32, 3)], align=True)
KNOT_REC = 96                                          # bytes of a knot record: 12 doubles
assert LEG.itemsize == 32 and TRIO.itemsize == 272 and SUMMARY.itemsize == 520


# ------------------------------------------------------------------------------------------------ the bases
def _raw_spec():
    """A ``RawDeviceBasis``-style description (uf3_amd/representation/angles.py::_raw_tables): the raw bins kept by a leading trim
    of 1 and a trailing trim of 2 are the columns, no symmetry fold"""
    ks = [np.concatenate([[1.5] * 3, np.linspace(1.5, 3.5, 5), [3.5] * 3]), np.concatenate([[1.5] * 3, np.linspace(1.5, 3.5, 6), [3.5] * 3]),
          np.concatenate([[1.5] * 3, np.linspace(1.5, 7.0, 8), [7.0] * 3])]
    on = [np.zeros(len(k) - 4, dtype=bool) for k in ks]
    for flags in on:
        flags[1:len(flags) - 2] = True
    keep = on[0][:, None, None] & on[1][None, :, None] & on[2][None, None, :]
    lut = np.full(keep.shape, -1, dtype=np.int32)
    lut[keep] = np.arange(int(keep.sum()), dtype=np.int32)
    return _lib.flatten_raw([42, 74], pairs={(42, 74): (0.5, 5.0)}, trios=[((74, 42, 74), ks, lut.ravel())], r_cut=7.0)


BUILDERS = {
    "notebook_w_lead3": lambda: synthetic.notebook_basis(["W"], lead3=3),
    "notebook_w_lead0": lambda: synthetic.notebook_basis(["W"], lead3=0),
    "notebook_mow_lead3": lambda: synthetic.notebook_basis(["Mo", "W"], lead3=3),
    "notebook_mow_lead0": lambda: synthetic.notebook_basis(["Mo", "W"], lead3=0),
    **{name: functools.partial(_on_knots.basis, name) for name in _on_knots.BASES},
    **{name: functools.partial(_uneven.basis, name) for name in _uneven.BASES},
    "resolution_5_5_10": lambda: _precision._resolution_basis([5, 5, 10]),
    "resolution_7_7_14": lambda: _precision._resolution_basis([7, 7, 14]),
    "resolution_8_8_16_w": lambda: _precision._resolution_basis([8, 8, 16], ("W",)),
    "asymmetric_window": OV._asymmetric_window_basis,
    **{f"notebook_{S}_species": functools.partial(synthetic.notebook_basis, _bases.ELEMENTS[S]) for S in (4, 5, 6, 8)},
    "mixed_trios_5_species": lambda: _bases.mixed_trio_basis(_bases.ELEMENTS[5], 5),
    "wide": _bases.wide_basis,
    "two_body_mow": lambda: OV._two_body_basis(["Mo", "W"]),
    "raw_bins": _raw_spec,
    "sym3_unary": lambda: basis_from_meta(load_case("case_w16_sym3")[1]),          # (three equal legs: six raw bins a column)
}
# (basis, switches): every basis as the library runs it, and the switched-off families where they decide something else
CASES = [(name, 0) for name in BUILDERS] + [
    ("notebook_mow_lead3", NO_FEAT3), ("notebook_mow_lead3", NO_MFMA_FEAT), ("notebook_mow_lead3", NO_MFMA_FEAT | NO_FEAT3),
    ("notebook_w_lead0", NO_MFMA_FEAT | NO_FEAT3), ("uneven_lead0", NO_MFMA_FEAT), ("sym1_binary", NO_MFMA_FEAT),
    ("mixed_trios_5_species", NO_MFMA_FEAT | NO_FEAT3), ("raw_bins", NO_MFMA_FEAT),
    ("sym3_unary", NO_MFMA_FEAT | NO_FEAT3)]


def key(name, switches):
    return f"{name}/{switches}"


@functools.lru_cache(maxsize=None)
def spec(name):
    """(BasisSpec, keep-alive arrays) of a named basis"""
    made = BUILDERS[name]()
    return made if isinstance(made, tuple) else _lib.flatten_basis(made)


# ------------------------------------------------------------------------------------------------ reading a plan
def _fetch(call, selector_or_name):
    n = C.c_int64()
    call(selector_or_name, None, 0, C.byref(n))
    buf = np.zeros(max(n.value, 1), dtype=np.uint8)
    call(selector_or_name, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
    return buf[:n.value].tobytes()


def tables(s, switches, dump_lib=None):
    """name -> bytes of every table of the plan: from the tree's ``uf3_basis_plan_debug``, or from ``uf3_basis_dump_debug`` of a
    library patched to dump (the switches through the environment, as that library reads them)"""
    if dump_lib is None:
        lib = _lib.load()

        def call(sel, out, cap, n):
            rc = lib.uf3_basis_plan_debug(C.byref(s), switches, sel, out, cap, n)
            if rc:
                raise _lib.UF3Error(rc, lib.uf3_last_error(None).decode())
        return {name: _fetch(call, k) for k, name in enumerate(TABLES)}
    for bit, var in ENV.items():
        os.environ.pop(var, None)
        if switches & bit:
            os.environ[var] = "1"
    try:
        def call(name, out, cap, n):
            rc = dump_lib.uf3_basis_dump_debug(C.byref(s), name.encode(), out, cap, n)
            assert rc == 0, (rc, name)
        return {name: _fetch(call, name) for name in TABLES}
    finally:
        for var in ENV.values():
            os.environ.pop(var, None)


def summary(tab):
    assert len(tab["summary"]) == SUMMARY.itemsize
    return np.frombuffer(tab["summary"], dtype=SUMMARY)[0]


def trios(tab):
    return np.frombuffer(tab["trios"], dtype=TRIO)


def entry(tab):
    """What the golden keeps of a plan: the sha256 of every table, their lengths, and the decisions in readable form"""
    sm, tr = summary(tab), trios(tab)
    facts = {}
    for f in SUMMARY.names:
        v = sm[f]
        facts[f] = v.tolist() if isinstance(v, np.ndarray) else (float(v) if SUMMARY[f] == f64 else int(v))
    for f in ("dense_stride", "dense_stride_f", "dense_grouped", "dense_dump"):       # (modes 6 .. 9 are the ones that have any)
        assert not any(facts[f][:6]) and not any(facts[f][10:])
        facts[f] = facts[f][6:10]
    return {"sha256": {name: hashlib.sha256(tab[name]).hexdigest() for name in TABLES},
            "bytes": {name: len(tab[name]) for name in TABLES},
            "summary": facts,
            "trios": _runs([{"dense": int(t["dense"]), "nsrc": int(t["nsrc"]), "grouped": int(t["grouped"]), "banded": int(t["banded"]),
                             "layout": int(t["layout"]), "band_tile": t["band_tile"].tolist(), "lo": t["lo"].tolist(),
                             "ext": t["ext"].tolist(), "thr": [float(t[f]) for f in ("thr0", "thr2", "gthr0", "gthr2")]} for t in tr])}


def _runs(items):
    """[[count, item], ...] of a list: equal neighbours once"""
    out = []
    for it in items:
        if out and out[-1][1] == it:
            out[-1][0] += 1
        else:
            out.append([1, it])
    return out


def golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basis_plan.json")


if __name__ == "__main__":
    dump = None
    if sys.argv[1] != "-":
        dump = C.CDLL(sys.argv[1])
        dump.uf3_basis_dump_debug.argtypes = [C.POINTER(_lib.BasisSpec), C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    out = {key(name, sw): entry(tables(spec(name)[0], sw, dump)) for name, sw in CASES}
    with open(sys.argv[2], "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"{len(out)} plans -> {sys.argv[2]}")
