"""Host side of uf3_amd.data.analyze: the post-processing of DataAnalyzer.analyze() fed the reference's own raw histograms
(tests/golden/analyze_*.npz, make_analyze_golden.py), Atoms.rattle, get_pair_hashes, and the loud failure without a device."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.data import analyze, composition
from uf3_amd.data.atoms import Atoms
from uf3_amd.representation import distances

from _util import GOLDEN, load_case

CASES = ["case_steel", "case_w16", "case_nexe32", "case_ternary24_slab", "case_h2o", "case_ch4"]


def _golden(case):
    g = np.load(os.path.join(GOLDEN, f"analyze_{case}.npz"))
    _, meta, _ = load_case(case)
    return g, composition.ChemicalSystem(meta["element_list"], 2), json.loads(str(g["settings"]))


def _fed(g, cs, name, kw):
    """A DataAnalyzer whose accumulators hold the reference's raw capture."""
    an = analyze.DataAnalyzer(cs, progress=None, **kw)
    keys = [int(k) for k in g[f"{name}_keys"]]
    an.histogram_values = {k: np.array(v, dtype=float) for k, v in zip(keys, g[f"{name}_hist"])}
    an.pairs_acc = {k: v for k, v in zip(keys, g[f"{name}_pairs_acc"])}
    an.totals_acc = g[f"{name}_totals"][()]
    an.sizes = list(g[f"{name}_sizes"])
    an.volumes = list(g[f"{name}_volumes"])
    an.compositions = [list(c) for c in g[f"{name}_compositions"]]
    return an


@pytest.mark.parametrize("case", CASES)
def test_analyze_on_captured_histograms_matches_reference(case):
    g, cs, settings = _golden(case)
    for name, kw in settings.items():
        an = _fed(g, cs, name, kw)
        if f"{name}_a_error" in g:
            with pytest.raises(KeyError), contextlib.redirect_stdout(io.StringIO()):
                an.analyze()
            continue
        with contextlib.redirect_stdout(io.StringIO()):
            res = an.analyze()
        np.testing.assert_array_equal(res["bin_edges"], g[f"{name}_a_bin_edges"])
        np.testing.assert_allclose([res["atomic_volumes"][el] for el in cs.element_list], g[f"{name}_a_atomic_volumes"],
                                   rtol=1e-6)
        for p, pair in enumerate(cs.interactions_map[2]):
            np.testing.assert_array_equal(res["histograms"][pair], g[f"{name}_a_hist{p}"])
            if f"{name}_a_rdf{p}" not in g:
                assert pair not in res["rdfs"]
                continue
            np.testing.assert_allclose(res["rdfs"][pair], g[f"{name}_a_rdf{p}"], rtol=1e-12)
            np.testing.assert_allclose(res["reference"][pair], g[f"{name}_a_reference{p}"], rtol=1e-12)
            np.testing.assert_allclose(res["coverage"][pair], g[f"{name}_a_coverage{p}"], rtol=1e-9)
            assert res["lower_bounds"][pair] == g[f"{name}_a_lower{p}"][()]
            np.testing.assert_allclose(res["peaks"][pair], g[f"{name}_a_peaks{p}"], rtol=1e-12)
            np.testing.assert_allclose(res["valleys"][pair], g[f"{name}_a_valleys{p}"], rtol=1e-12)


def test_bin_layout_matches_reference_rules():
    cs = composition.ChemicalSystem(["W"], 2)
    an = analyze.DataAnalyzer(cs, r_cut=12.0, bins=0.01)
    assert an.n_bins == 1200 and len(an.bin_edges) == 1201 and an.bin_edges[-1] == 12.0
    an = analyze.DataAnalyzer(cs, r_cut=8.0, bins=150)
    assert an.n_bins == 150
    np.testing.assert_array_equal(an.bin_edges, np.linspace(0, 8.0, 151))


def test_module_functions():
    bins = np.linspace(0, 5, 11)
    norm = analyze.get_uniform_normalization(bins, 10, 100.0)
    np.testing.assert_allclose(norm, 4 / 3 * np.pi * (bins[1:] ** 3 - bins[:-1] ** 3) / 10.0 * 10, rtol=1e-12)
    binned = analyze.apply_binning({5: np.array([0.1, 0.5, 4.99, 5.0])}, bins)
    np.testing.assert_array_equal(binned[5], np.histogram([0.1, 0.5, 4.99, 5.0], bins)[0])
    hist = np.array([0, 0, 3, 5, 8, 4, 2, 6, 9, 3.0])
    ref = np.linspace(0.5, 5, 10)
    assert np.isclose(analyze.compute_coverage(1.0, hist.copy(), ref), np.sum(np.minimum(hist, ref)), rtol=1e-12)
    assert np.isfinite(analyze.score_coverage(1.0, hist, ref))
    idx, val = analyze.find_closest_value(np.array([1.0, 2.5, 4.0]), 2.7)
    assert idx == 1 and val == 2.5
    x = np.linspace(0, 10, 101)
    pk, pos = analyze.find_peaks(x, np.sin(x))
    np.testing.assert_allclose(pos, [1.6, 7.9])


def test_atoms_rattle_is_ase_rattle():
    d, _, atoms = load_case("case_w16")
    a = atoms.copy()
    a.rattle(0.05)
    np.testing.assert_array_equal(a.get_positions(), d["positions"] + np.random.RandomState(42).normal(scale=0.05,
                                                                                                       size=(16, 3)))
    b = atoms.copy()
    b.rattle(0.05)
    np.testing.assert_array_equal(a.get_positions(), b.get_positions())          # same seed on every call
    c = atoms.copy()
    c.rattle(0.01, seed=7)
    np.testing.assert_array_equal(c.get_positions(), d["positions"] + np.random.RandomState(7).normal(scale=0.01,
                                                                                                      size=(16, 3)))
    with pytest.raises(ValueError):
        c.rattle(0.01, seed=1, rng=np.random.RandomState(1))


def test_pair_hashes_sort_by_reference_order():
    zi, zj = np.array([26, 6]), np.array([26, 6, 6, 26])
    si, sj = ["Fe", "C"], ["Fe", "C", "C", "Fe"]
    h = composition.get_pair_hashes((zi, zj), (si, sj), (np.array([0, 0, 1, 1]), np.array([0, 1, 2, 3])))
    fe_fe, c_fe, c_c = 26 * 26 + 26 + 26, 26 * 26 + 6 + 26, 6 * 6 + 6 + 6
    np.testing.assert_array_equal(h, [fe_fe, c_fe, c_c, c_fe])
    assert composition.hash_to_symbols(c_fe) == ("C", "Fe")


def test_no_gpu_means_loud_failure_for_histograms():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _, meta, atoms = load_case("case_w16")
    cs = composition.ChemicalSystem(meta["element_list"], 2)
    an = analyze.DataAnalyzer(cs, r_cut=6.0)
    with pytest.raises(_lib.HipUnavailable):
        an.load_entries([atoms])
    with pytest.raises(_lib.HipUnavailable):
        an.process_geometry(atoms)
    with pytest.raises(_lib.HipUnavailable):
        distances.summarize_distances([atoms], cs, r_cut=6.0, print_stats=False)
    assert isinstance(atoms, Atoms)
