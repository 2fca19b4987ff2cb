"""Pair-distance histograms on the device (uf3_pair_histogram[_dev], uf3_amd.data.analyze, distances.summarize_distances):
integer-exact against the reference's captures (tests/golden/analyze_*.npz) and against a NumPy restatement of the reference
(explicit supercell from the oracle, scipy cdist in chunks, np.histogram) on large frames, at cut-off probes, and on the
global-atomics route for histograms that do not fit in LDS."""
import contextlib
import ctypes as C
import io
import json
import os
import warnings

import numpy as np
import pytest
from scipy.spatial import distance

from uf3_amd import _lib, synthetic
from uf3_amd.data import analyze, composition
from uf3_amd.data.atoms import Atoms
from uf3_amd.representation import distances

from _util import GOLDEN, load_case

pytestmark = pytest.mark.gpu

CASES = ["case_steel", "case_w16", "case_nexe32", "case_ternary24_slab", "case_h2o", "case_ch4"]


def _golden(case):
    g = np.load(os.path.join(GOLDEN, f"analyze_{case}.npz"))
    _, meta, atoms = load_case(case)
    return g, composition.ChemicalSystem(meta["element_list"], 2), json.loads(str(g["settings"])), atoms


def restated(atoms, species, edges, r_max, upper_inclusive, rattle=0.0, chunk=64):
    """The reference's counting in NumPy: cdist of the frame against its explicit supercell (oracle.supercell, the
    reference's image order), ASE's rattle noise on the supercell, the range mask, np.histogram per species pair."""
    from oracle import oracle
    pos = np.asarray(atoms.get_positions(), dtype=float)
    z = np.asarray(atoms.get_atomic_numbers())
    if np.any(atoms.get_pbc()):
        sup, sz, _ = oracle.supercell(atoms, r_max)
    else:
        sup, sz = pos.copy(), z.copy()
    if rattle > 0:
        sup = sup + np.random.RandomState(42).normal(scale=rattle, size=sup.shape)
    pairs = [(species[i], species[j]) for i in range(len(species)) for j in range(i, len(species))]
    out = np.zeros((len(pairs), len(edges) - 1), dtype=np.int64)
    col = {p: k for k, p in enumerate(pairs)}
    for lo in range(0, len(pos), chunk):
        d = distance.cdist(pos[lo:lo + chunk], sup)
        mask = (d > 0) & ((d <= r_max) if upper_inclusive else (d < r_max))
        i, j = np.nonzero(mask)
        zi, zj = z[lo:lo + chunk][i], sz[j]
        a, b = np.minimum(zi, zj), np.maximum(zi, zj)
        dd = d[mask]
        for p, (za, zb) in enumerate(pairs):
            sel = (a == za) & (b == zb)
            out[col[(za, zb)]] += np.histogram(dd[sel], edges)[0]
    return out


@pytest.mark.parametrize("case", CASES)
def test_analyzer_counts_equal_reference_captures(case):
    g, cs, settings, atoms0 = _golden(case)
    for name, kw in settings.items():
        an = analyze.DataAnalyzer(cs, progress=None, **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            an.load_entries([atoms0.copy()])
        keys = [int(k) for k in g[f"{name}_keys"]]
        assert sorted(an.histogram_values) == keys, name
        for k, h, n in zip(keys, g[f"{name}_hist"], g[f"{name}_pairs_acc"]):
            np.testing.assert_array_equal(an.histogram_values[k], h, err_msg=f"{case} {name} {k}")
            assert an.pairs_acc[k] == n
        assert an.totals_acc == g[f"{name}_totals"][()]
        np.testing.assert_array_equal(an.sizes, g[f"{name}_sizes"])
        np.testing.assert_array_equal(an.volumes, g[f"{name}_volumes"])
        np.testing.assert_array_equal(an.compositions, g[f"{name}_compositions"])
        # process_geometry: the same counts one frame at a time
        an2 = analyze.DataAnalyzer(cs, progress=None, **kw)
        an2.process_geometry(atoms0.copy())
        for k in keys:
            np.testing.assert_array_equal(an2.histogram_values[k], an.histogram_values[k])
        if f"{name}_a_error" in g:
            with pytest.raises(KeyError), contextlib.redirect_stdout(io.StringIO()):
                an.analyze()
        else:
            with contextlib.redirect_stdout(io.StringIO()):
                res = an.analyze()
            for p, pair in enumerate(cs.interactions_map[2]):
                np.testing.assert_array_equal(res["histograms"][pair], g[f"{name}_a_hist{p}"])
                if f"{name}_a_peaks{p}" in g:
                    np.testing.assert_allclose(res["peaks"][pair], g[f"{name}_a_peaks{p}"], rtol=1e-12)


@pytest.mark.parametrize("case", CASES)
def test_summarize_distances_matches_reference(case):
    g, cs, _, atoms0 = _golden(case)
    if "sd_error" in g:
        with pytest.raises(IndexError), contextlib.redirect_stdout(io.StringIO()):
            distances.summarize_distances([atoms0], cs, r_cut=10.0, n_bins=100)
        return
    with contextlib.redirect_stdout(io.StringIO()):
        hist, edges, lower = distances.summarize_distances([atoms0], cs, r_cut=10.0, n_bins=100)
    np.testing.assert_array_equal(edges, g["sd_edges"])
    for p, pair in enumerate(cs.interactions_map[2]):
        np.testing.assert_allclose(hist[pair], g["sd_hist"][p], rtol=1e-12, atol=0)
        assert lower[pair] == g["sd_lower"][p]


@pytest.mark.parametrize("upper_inclusive", [True, False])
def test_large_frame_counts_equal_restatement(upper_inclusive):
    atoms, _ = synthetic.config_c4(0)
    assert len(atoms) >= 10_000
    species = [42, 74]
    edges = np.linspace(0, 12.0, 1201)
    got, pairs = analyze.pair_histograms([atoms], species, edges, 0.0, 12.0, upper_inclusive=upper_inclusive)
    want = restated(atoms, species, edges, 12.0, upper_inclusive)
    assert pairs == [(42, 42), (42, 74), (74, 74)]
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("upper_inclusive", [True, False])
def test_cutoff_probe_counts_equal_restatement(upper_inclusive):
    atoms = synthetic.cutoff_probe_frame([4.0, 6.0], elements=(42, 74))
    species = [42, 74]
    edges = np.linspace(0, 6.0, 601)          # 4.0 and 6.0 are edges: both the range and the bin rule are probed
    got, _ = analyze.pair_histograms([atoms], species, edges, 0.0, 6.0, upper_inclusive=upper_inclusive)
    want = restated(atoms, species, edges, 6.0, upper_inclusive)
    np.testing.assert_array_equal(got, want)
    assert got.sum() > 0


def test_lds_overflow_route_equals_restatement():
    # five elements at 0.01 A bins to 12 A: 15 x 1200 int32 counters are more than the kernel keeps in LDS
    species = [23, 24, 41, 42, 74]
    atoms = synthetic.lattice_frame("bcc", (4, 4, 5), 3.165, species, seed=11)
    edges = np.linspace(0, 12.0, 1201)
    assert 15 * 1200 * 4 > 65536
    for rattle in (0.0, 0.03):
        got, _ = analyze.pair_histograms([atoms], species, edges, 0.0, 12.0, rattle=rattle)
        np.testing.assert_array_equal(got, restated(atoms, species, edges, 12.0, True, rattle=rattle))


def test_rattled_large_frame_counts_equal_restatement():
    atoms = synthetic.lattice_frame("bcc", (8, 8, 8), 3.165, [42, 74], seed=5)
    species = [42, 74]
    edges = np.linspace(0, 9.0, 901)
    got, _ = analyze.pair_histograms([atoms], species, edges, 0.0, 9.0, rattle=0.2)
    np.testing.assert_array_equal(got, restated(atoms, species, edges, 9.0, True, rattle=0.2))


def _mixed_frames():
    frames = [load_case(c)[2] for c in ("case_steel", "case_w16", "case_ch4", "case_h2o")]
    frames.append(synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74, 26], seed=3))
    return frames, sorted({int(z) for f in frames for z in f.get_atomic_numbers()})


def test_batch_sum_and_per_frame_equal_single_frame_calls():
    frames, species = _mixed_frames()
    edges = np.linspace(0, 8.0, 401)
    for rattle in (0.0, 0.05):
        singles = np.array([analyze.pair_histograms([f], species, edges, 0.0, 8.0, rattle=rattle)[0] for f in frames])
        total, _ = analyze.pair_histograms(frames, species, edges, 0.0, 8.0, rattle=rattle)
        per, _ = analyze.pair_histograms(frames, species, edges, 0.0, 8.0, rattle=rattle, per_frame=True)
        np.testing.assert_array_equal(total, singles.sum(axis=0))
        np.testing.assert_array_equal(per, singles)
        # several device calls (tiny batches) add up to the same
        small, _ = analyze.pair_histograms(frames, species, edges, 0.0, 8.0, rattle=rattle, max_atoms=20)
        np.testing.assert_array_equal(small, total)


def test_dev_entry_equals_host_entry():
    import torch
    frames, species = _mixed_frames()
    frames = [f for f in frames if np.any(f.get_pbc())]
    edges = np.linspace(0, 8.0, 801)
    noise = np.random.RandomState(42).normal(scale=0.05, size=(200_000, 3))
    db = analyze._hist_basis(species, 0.0, 8.0)
    fb = _lib.FrameBatch(frames)
    for per_frame in (False, True):
        want = _lib.pair_histogram(db, fb, edges, noise=noise, per_frame=per_frame)
        pos = torch.from_numpy(fb.pos).cuda()
        z = torch.from_numpy(fb.z).cuda()
        out = torch.full(want.shape, -1, dtype=torch.int64, device="cuda")
        prev = db.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            _lib.pair_histogram_dev(db, fb.struct, pos.data_ptr(), z.data_ptr(), out.data_ptr(), edges, noise=noise,
                                    per_frame=per_frame)
            torch.cuda.synchronize()
        finally:
            db.ctx.restore_stream(prev)
        np.testing.assert_array_equal(out.cpu().numpy(), want)


def test_foreign_element_warns_and_is_histogrammed():
    g, _, settings, atoms0 = _golden("case_steel")
    cs = composition.ChemicalSystem(["Fe"], 2)             # the frame also holds C
    an = analyze.DataAnalyzer(cs, progress=None, **settings["plain"])
    with pytest.warns(UserWarning, match="Invalid element"):
        an.load_entries([atoms0])
    keys = [int(k) for k in g["plain_keys"]]
    assert sorted(an.histogram_values) == keys
    for k, h in zip(keys, g["plain_hist"]):
        np.testing.assert_array_equal(an.histogram_values[k], h)
    assert an.compositions == [[int(np.count_nonzero(atoms0.get_atomic_numbers() == 26))]]


def test_abi_rejects_bad_arguments():
    _, _, atoms = load_case("case_w16")
    db = analyze._hist_basis([74], 0.0, 6.0)
    fb = _lib.FrameBatch([atoms])
    good = np.linspace(0, 6.0, 61)
    with pytest.raises(_lib.UF3Error) as e:
        _lib.pair_histogram(db, fb, good[:1])                               # n_bins = 0
    assert e.value.code == 1
    for edges in (good[::-1].copy(), np.linspace(-1.0, 6.0, 61), np.array([0.0, 1.0, 1.0, 2.0])):
        with pytest.raises(_lib.UF3Error) as e:
            _lib.pair_histogram(db, fb, edges)
        assert e.value.code == 1
    with pytest.raises(_lib.UF3Error) as e:                                 # 16 atoms x 27 images needed
        _lib.pair_histogram(db, fb, good, noise=np.zeros((100, 3)))
    assert e.value.code == 1
    lib, ctx = db.ctx.lib, db.ctx
    args = (db.handle, C.byref(fb.struct), _lib._p(fb.pos), _lib._p(fb.z), 60, _lib._p(good), 1, None, 0, 0)
    assert lib.uf3_pair_histogram(*args, None) == 1                         # null out
    out = np.zeros((1, 60), dtype=np.int64)
    assert lib.uf3_pair_histogram(db.handle, C.byref(fb.struct), _lib._p(fb.pos), _lib._p(fb.z), 60, None, 1, None, 0, 0,
                                  _lib._p(out)) == 1                        # null edges
    assert lib.uf3_pair_histogram(db.handle, C.byref(fb.struct), _lib._p(fb.pos), _lib._p(fb.z), 60, _lib._p(good), 1,
                                  None, 10, 0, _lib._p(out)) == 1           # n_noise > 0 without noise
    assert lib.uf3_pair_histogram_dev(db.handle, C.byref(fb.struct), None, None, 60, _lib._p(good), 1, None, 0, 0,
                                      None) == 1
    assert lib.uf3_pair_histogram(None, C.byref(fb.struct), _lib._p(fb.pos), _lib._p(fb.z), 60, _lib._p(good), 1, None, 0,
                                  0, _lib._p(out)) == 1
    # a frame whose element is not in the basis
    other = Atoms(numbers=[26] * 16, positions=atoms.get_positions(), cell=atoms.get_cell(), pbc=True)
    with pytest.raises(_lib.SpeciesError):
        _lib.pair_histogram(db, _lib.FrameBatch([other]), good)
    # the context still works
    assert _lib.pair_histogram(db, fb, good).sum() > 0
    del ctx
