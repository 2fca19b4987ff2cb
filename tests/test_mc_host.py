"""Host side of the species-swap Monte Carlo (uf3_amd/forcefield/mc.py, tests/_mc_ref.py), no GPU: the proposal arithmetic of the
restatement against hand-computed words, the Warren-Cowley parameters against a brute-force loop, every argument check of
``MonteCarlo`` (made before the library is touched), ``HipUnavailable`` without the library, and the record reshaping."""
import itertools

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import mc
import _md_ref
import _mc_ref as R


class _Calc:
    """What ``MonteCarlo`` reads of a calculator before it touches the device."""
    device = None

    def __init__(self, elements=("Mo", "W")):
        self.bspline_config = synthetic.notebook_basis(list(elements))
        self._c1 = np.zeros(len(elements))
        self._c2 = np.zeros(1)
        self._c3 = np.zeros(1)


def _frame(n=(2, 2, 2), numbers=(42, 74)):
    return synthetic.lattice_frame("bcc", n, 3.2, list(numbers), seed=3, rattle=0.02)


# ---- the proposal arithmetic ----------------------------------------------------------------------------------------------
def test_philox_words_and_index_arithmetic():
    # Random123's known-answer vectors of Philox4x32-10: counter and key all zero, and all ones
    assert R.words(0, 0, 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = _md_ref.philox(np.full((1, 4), 0xFFFFFFFF, dtype=np.uint32), np.full((1, 2), 0xFFFFFFFF, dtype=np.uint32))[0]
    assert [int(x) for x in ones] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # the counter layout: (frame, trial lo, trial hi, 0), key (seed lo, seed hi)
    t, seed = (5 << 32) | 7, (9 << 32) | 11
    want = _md_ref.philox(np.array([[3, 7, 5, 0]], dtype=np.uint32), np.array([[11, 9]], dtype=np.uint32))[0]
    assert R.words(3, t, seed) == [int(x) for x in want]
    # (word * n) >> 32 by hand
    assert R.pick(0, 54) == 0 and R.pick(0xFFFFFFFF, 54) == 53 and R.pick(0x80000000, 54) == 27
    assert R.pick(0x6627E8D5, 16) == 6 and R.pick(0xE169C58D, 16) == 14          # 0x6... / 2^28, 0xE... / 2^28
    assert R.pick(0x7FFFFFFF, 1) == 0 and R.pick(0xFFFFFFFF, 2) == 1
    # two words -> a double in (0, 1): ((hi << 32 | lo) >> 11) + 0.5) 2^-53
    assert R.uniform(0, 0) == 0.5 * 2.0 ** -53
    assert R.uniform(0x80000000, 0) == 0.5 + 0.5 * 2.0 ** -53
    assert R.uniform(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 0.5 * 2.0 ** -53
    assert R.uniform(0, 1 << 11) == 1.5 * 2.0 ** -53


def test_proposals():
    species = np.array([0, 1, 1, 0])
    w = lambda i, j, n=4: [(i << 32) // n + 1, (j << 32) // n + 1, 0, 0]         # words that pick i and j of n
    assert R.pick(w(2, 3)[0], 4) == 2 and R.pick(w(2, 3)[1], 4) == 3
    mv = R.propose(R.SWAP, w(0, 1), species)
    assert (mv["null"], mv["i"], mv["j"], mv["new_i"], mv["new_j"]) == (False, 0, 1, 1, 0)
    assert R.propose(R.SWAP, w(1, 2), species)["null"]                            # like species
    assert R.propose(R.SWAP, w(2, 2), species)["null"]                            # the same atom twice
    assert R.propose(R.SWAP, w(0, 1), species, swappable=[1, 0, 1, 1])["null"]    # j may not change
    assert not R.propose(R.SWAP, w(0, 2), species, swappable=[1, 0, 1, 1])["null"]
    mu = np.array([0.0, -np.inf, 0.3, 0.1])                                       # species 1 is not allowed
    sp = np.array([0, 1, 2, 3])
    pick_k = lambda k, m: (k << 32) // m + 1
    mv = R.propose(R.TRANSMUTE, [w(0, 0)[0], pick_k(0, 2), 0, 0], sp, mu=mu)      # 0 -> first of (2, 3)
    assert (mv["null"], mv["new_i"], mv["j"]) == (False, 2, -1) and mv["dmu"] == 0.3
    mv = R.propose(R.TRANSMUTE, [w(0, 0)[0], pick_k(1, 2), 0, 0], sp, mu=mu)      # 0 -> second of (2, 3)
    assert mv["new_i"] == 3 and mv["dmu"] == 0.1
    mv = R.propose(R.TRANSMUTE, [w(3, 0)[0], pick_k(1, 2), 0, 0], sp, mu=mu)      # 3 -> second of (0, 2)
    assert mv["new_i"] == 2 and abs(mv["dmu"] - 0.2) < 1e-15
    assert R.propose(R.TRANSMUTE, [w(1, 0)[0], 0, 0, 0], sp, mu=mu)["null"]       # its own species is not allowed
    assert R.propose(R.TRANSMUTE, [w(0, 0)[0], 0, 0, 0], sp, swappable=[0, 1, 1, 1], mu=mu)["null"]


def test_chains_of_the_restatement():
    # energy = number of unlike nearest neighbours on a ring: the running energy telescopes, T = 0 never goes up, records add up
    def energies_of(spec):
        return np.array([float(np.sum(s != np.roll(s, 1))) for s in spec])
    rng = np.random.default_rng(0)
    start = [rng.integers(0, 2, 12), rng.integers(0, 2, 20)]
    ch = R.Chains(energies_of, start, [0.0, 5000.0], R.SWAP, 4, 2)
    rec = ch.run(200, record_every=10)
    assert rec.shape == (20, 2, 5)
    assert np.all(np.diff(rec[:, 0, 0]) <= 0) and np.array_equal(ch.energy, energies_of(ch.species))
    assert np.array_equal(rec[-1, :, 1], ch.accepted) and np.array_equal(rec[-1, :, 2], [200, 200])
    assert np.array_equal(rec[:, 0, 3:].sum(1), np.full(20, 12)) and np.array_equal(rec[0, 1, 3:], rec[-1, 1, 3:])
    again = R.Chains(energies_of, start, [0.0, 5000.0], R.SWAP, 4, 2)
    again.run(80)
    again.run(120)
    assert all(np.array_equal(a, b) for a, b in zip(again.species, ch.species)) and np.array_equal(again.energy, ch.energy)
    assert abs(R.site_occupancy(0.1, 0.04, 1200.0) - 1.0 / (1.0 + np.exp(0.06 / (8.617333262e-5 * 1200.0)))) < 1e-15
    assert R.site_occupancy(0.0, 0.0, 300.0) == 0.5


# ---- short-range order ----------------------------------------------------------------------------------------------------
def _brute_alpha(atoms, r_shell):
    z, pos, cell = atoms.get_atomic_numbers(), atoms.get_positions(), np.asarray(atoms.get_cell())
    species = sorted(set(int(q) for q in z))
    counts = np.zeros((len(species), len(species)))
    for i in range(len(z)):
        for j in range(len(z)):
            for s in itertools.product(range(-2, 3), repeat=3):
                if i == j and s == (0, 0, 0):
                    continue
                d = np.linalg.norm(pos[j] + np.array(s) @ cell - pos[i])
                if d <= r_shell:
                    counts[species.index(z[i]), species.index(z[j])] += 1
    conc = np.array([np.mean(z == q) for q in species])
    return 1.0 - counts / counts.sum(1, keepdims=True) / conc[None, :], counts


def test_short_range_order_on_b2_and_a_random_alloy():
    a = 3.2
    grid = np.stack(np.meshgrid(*[np.arange(2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pos = np.concatenate([grid * a, (grid + 0.5) * a])
    b2 = Atoms(numbers=[42] * 8 + [74] * 8, positions=pos, cell=np.eye(3) * 2 * a, pbc=True)
    first, second = 0.5 * np.sqrt(3) * a + 0.05, a + 0.05
    out = mc.short_range_order(b2, first)
    assert out["species"] == [42, 74] and np.array_equal(out["neighbours"], [[0, 64], [64, 0]])
    assert np.allclose(out["alpha"], [[1.0, -1.0], [-1.0, 1.0]], atol=1e-14)          # -1 between unlike atoms on the first shell
    want, counts = _brute_alpha(b2, first)
    assert np.allclose(out["alpha"], want, atol=1e-14) and np.array_equal(out["neighbours"], counts)
    shell2 = mc.short_range_order(b2, second, r_inner=first)                          # the second shell holds like atoms only
    assert np.allclose(shell2["alpha"], [[-1.0, 1.0], [1.0, -1.0]], atol=1e-14)
    rnd = synthetic.lattice_frame("bcc", (2, 2, 2), 3.2, [42, 74], seed=12, rattle=0.03, strain=0.01)
    assert 0 < np.sum(rnd.get_atomic_numbers() == 42) < 16
    out = mc.short_range_order(rnd, 3.0)
    want, counts = _brute_alpha(rnd, 3.0)
    assert np.array_equal(out["neighbours"], counts) and np.allclose(out["alpha"], want, atol=1e-13)
    assert counts.sum() == 16 * 8                                                      # the rattled first shell, images included
    cluster = Atoms(numbers=rnd.get_atomic_numbers(), positions=rnd.get_positions(), cell=np.zeros((3, 3)), pbc=False)
    assert mc.short_range_order(cluster, 3.0)["neighbours"].sum() < counts.sum()
    with pytest.raises(ValueError):
        mc.short_range_order(rnd, -1.0)
    with pytest.raises(ValueError):
        mc.short_range_order(rnd, 2.0, r_inner=2.5)


# ---- argument checks ------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """Any touch of the library fails the test: the checks come first."""
    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "get_context", boom)
    monkeypatch.setattr(_lib, "device_basis", boom)


@pytest.mark.parametrize("kw, match", [
    (dict(temperature_K=-1.0), "temperature_K"),
    (dict(temperature_K=np.nan), "temperature_K"),
    (dict(temperature_K=[300.0, 400.0]), "2 temperatures for 1 frames"),
    (dict(temperature_K="hot"), "temperature_K"),
    (dict(mode="displace"), "mode must be"),
    (dict(mode="swap", chemical_potentials={"Mo": 0.0, "W": 0.1}), "belong to mode='transmute'"),
    (dict(mode="transmute"), "needs chemical_potentials"),
    (dict(mode="transmute", chemical_potentials={"Mo": 0.0, "Xx": 0.1}), "unknown element"),
    (dict(mode="transmute", chemical_potentials={"Mo": 0.0, "Ta": 0.1}), "not a species of the model"),
    (dict(mode="transmute", chemical_potentials={"Mo": 0.0, "W": np.nan}), "finite or -inf"),
    (dict(mode="transmute", chemical_potentials={"Mo": 0.0, "W": np.inf}), "finite or -inf"),
    (dict(mode="transmute", chemical_potentials={"Mo": 0.0, "W": "x"}), "must be a number"),
    (dict(mode="transmute", chemical_potentials={"Mo": 0.0}), "at least two species"),
    (dict(mode="transmute", chemical_potentials={"Mo": 0.0, "W": -np.inf}), "at least two species"),
    (dict(swappable=np.ones(15, dtype=bool)), "15 entries for 16 atoms"),
    (dict(swappable=np.ones(16)), "boolean mask"),
    (dict(seed=-1), "seed"),
    (dict(seed=1.5), "seed"),
    (dict(seed=1 << 64), "seed"),
])
def test_arguments_are_checked_before_the_library_is_touched(no_library, kw, match):
    kw = dict(temperature_K=300.0, **kw) if "temperature_K" not in kw else kw
    with pytest.raises(ValueError, match=match):
        mc.MonteCarlo(_Calc(), _frame(), **kw)


def test_frames_are_checked_before_the_library_is_touched(no_library):
    with pytest.raises(ValueError, match="no frames"):
        mc.MonteCarlo(_Calc(), [], 300.0)
    with pytest.raises(ValueError, match="outside the model: V"):
        mc.MonteCarlo(_Calc(), _frame(numbers=(23, 74)), 300.0)
    a = _frame()
    a.positions[2, 1] = np.inf
    with pytest.raises(ValueError, match="positions must be finite"):
        mc.MonteCarlo(_Calc(), a, 300.0)
    with pytest.raises(AssertionError, match="the library was touched"):          # (good arguments do reach the library)
        mc.MonteCarlo(_Calc(), _frame(), [300.0], mode="transmute", chemical_potentials={42: 0.0, "W": 0.05},
                      swappable=np.ones(16, dtype=bool), seed=(1 << 64) - 1)


def test_hip_unavailable_without_the_library(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_contexts", {})
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libuf3hip.so"))
    with pytest.raises(_lib.HipUnavailable):
        mc.MonteCarlo(_Calc(), _frame(), 300.0)


def test_closed_objects_and_run_arguments(monkeypatch):
    obj = mc.MonteCarlo.__new__(mc.MonteCarlo)
    obj.handle = None
    obj.mode, obj.seed, obj.chemical_potentials = "swap", 0, None
    obj.temperature_K = np.array([300.0])
    obj._batch = _lib.FrameBatch([_frame()])
    obj.element_list = ["Mo", "W"]
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="n_trials"):
            obj.run(bad)
    with pytest.raises(ValueError, match="record_every"):
        obj.run(10, record_every=-2)
    with pytest.raises(RuntimeError, match="closed"):
        obj.run(10)
    obj.close()                                                                    # (closing twice is fine)


# ---- records --------------------------------------------------------------------------------------------------------------
def test_record_reshaping():
    raw = np.zeros((3, 2, 5))
    raw[..., 0] = [[-1.5, -2.5], [-1.75, -2.5], [-2.0, -3.0]]
    raw[..., 1] = [[1, 0], [2, 0], [3, 1]]
    raw[..., 2] = [[10, 10], [20, 20], [30, 30]]
    raw[..., 3:] = [[[9, 7], [5, 11]], [[9, 7], [5, 11]], [[8, 8], [5, 11]]]
    rec = mc.run_records(raw, first_trial=100, every=10)
    assert np.array_equal(rec["trial"], [110, 120, 130]) and rec["trial"].dtype == np.int64
    assert np.array_equal(rec["energy"], raw[..., 0]) and rec["energy"] is not raw
    assert rec["accepted"].dtype == np.int64 and np.array_equal(rec["accepted"], [[1, 0], [2, 0], [3, 1]])
    assert np.array_equal(rec["trials"][:, 0], [10, 20, 30])
    assert rec["composition"].shape == (3, 2, 2) and np.array_equal(rec["composition"][2, 0], [8, 8])
    empty = mc.run_records(np.zeros((0, 2, 5)), 0, 1)
    assert empty["energy"].shape == (0, 2) and empty["composition"].shape == (0, 2, 2) and empty["trial"].shape == (0,)
    z = np.array([42, 74, 74, 42, 42, 42])
    assert np.array_equal(mc.composition(z, np.array([0, 2, 6]), ["Mo", "W"]), [[1, 1], [3, 1]])
