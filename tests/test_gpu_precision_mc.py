"""
mc_delta (uf3_mc.h, through k_mc_delta and k_mc_trials) held to the extended-precision oracle: the energy difference of every
chosen move within ``GAMMA["dE"] u M`` of ``oracle.mc_delta_x``, M the sum of the magnitudes of the terms the move touches over
both species assignments (tests/_precision.py; GAMMA = 16 max(rho_o, 1) with rho_o the fp64 oracle entry's own worst ratio,
measured on the CPU and never from a device result).  A swap touches terms whose magnitudes sum to some 1e3 eV at ordinary
densities, so the bound is about 2e-12 eV: three orders below the 1e-9 max(1, |E_frame|) of tests/test_gpu_mc.py and its
siblings, which stay as they are.  No move is left out; a move that changes nothing (i == j, like species) must give exactly 0.

mc_delta is the one evaluator with term bookkeeping of its own -- weights 2 and 1 on pair entries, the LDS list of affected
centres de-duplicated in rounds of 256 threads, the float-sqrt inversion of the pair index, leg order by (species, supercell
index), trio_of[(sm 8 + s1) 8 + s2] -- so the cases go to that bookkeeping's edges (``P.mc_cases``): lists past one round with
mostly distinct atoms, heavy de-duplication over several rounds, a frame past 256 atoms, eight species, a ragged batch, and the
limit itself: a 3-body list of exactly UF3_MC_MAX_N3 = 512 entries, whose swap fills the candidate list to its last slot
(n_c = 1026) and reaches the largest pair index 130815.  Every shape is asserted from host-side counts first.

Every test prints ``[precision] k_mc_delta <mode>, <case>: dE <ratio>``; ``tools/precision_ratios.py`` collects those lines into
``profiles/precision_ratios.json``.  The extended references are computed once per case and mode (about a minute in all).
"""
import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import _lib
from uf3_amd.data.composition import atomic_numbers
from uf3_amd.forcefield import calculator, mc
from uf3_amd.regression import least_squares as ls
import _mc_ref as R
import _precision as P
from _on_knots import with_numbers

pytestmark = pytest.mark.gpu

BATCH = ("cluster", "slab_outside", "triclinic_thin")         # one basis object, three boundary conditions, 9 + 12 + 3 atoms
MAX_N3 = 512                                                  # UF3_MC_MAX_N3
ROUND = 256                                                   # UF3_MC_THREADS: candidates looked at per round


def _calc(basis, coeff):
    model = ls.WeightedLinearModel(basis)
    model.coefficients = np.array(coeff, dtype=float)
    return calculator.UFCalculator(model, md_skin=0.0)


def _chain(calc, frames, mode, temperature_K=300.0, **kw):
    extra = dict(chemical_potentials={e: 0.0 for e in calc.bspline_config.element_list}) if mode == "transmute" else {}
    return mc.MonteCarlo(calc, frames, temperature_K, mode=mode, **extra, **kw)


def _device(name, mode):
    basis, atoms, _, _ = P.mc_cases()[name]
    ref = P.mc_reference(name, mode)
    with _chain(_calc(basis, ref["coeff"]), [atoms], mode) as chain:
        return chain.delta_energy(np.zeros(len(ref["i"]), dtype=int), ref["i"], list(ref["second"]))


def _hold(route, name, got, ref):
    r = P.ratio(got, ref["dE"], ref["M"])                     # (asserts exact zeros where M == 0: the null moves)
    print(f"[precision] {route}, {name}: dE {r:.3g}")
    assert r <= P.GAMMA["dE"], (route, name, r, P.GAMMA["dE"])
    return r


def _assert_classes(name, mode):
    """every class of moves the frame's geometry can have is among the chosen ones"""
    basis, atoms, _, _ = P.mc_cases()[name]
    ref = P.mc_reference(name, mode)
    z = np.asarray(atoms.get_atomic_numbers())
    labels = ref["label"]
    assert "null" in labels
    if mode == "swap":
        chosen = {(int(i), int(j)) for i, j, lab in zip(ref["i"], ref["second"], labels) if lab != "null"}
        for k, pool in P.mc_move_classes(basis, atoms).items():
            assert not pool or chosen & set(pool), (name, k)
        nulls = [(int(i), int(j)) for i, j, lab in zip(ref["i"], ref["second"], labels) if lab == "null"]
        assert any(i == j for i, j in nulls) and all(z[i] == z[j] for i, j in nulls)
        assert len(set(z.tolist())) == len(z) or any(i != j for i, j in nulls)       # (like species, where the frame has any)
    else:
        els = list(basis.chemical_system.element_list)
        for a in {int(i) for i, lab in zip(ref["i"], labels) if lab != "null"}:
            to = {s for i, s, lab in zip(ref["i"], ref["second"], labels) if int(i) == a and lab != "null"}
            assert to == {e for e in els if atomic_numbers[e] != z[a]}, (name, a)


# ================================================================================================ the evaluator's cases
ORDINARY = ["mow_cap16", "mow_cap32", "mow_lead0", "uneven_lead3", "uneven_lead0", "w16_sym3_binary", "triclinic_thin", "cluster",
            "slab_outside", "mow_2body", "bcc24_s4", "bcc24_s8"]


@pytest.mark.parametrize("mode", P.MC_MODES)
@pytest.mark.parametrize("name", ORDINARY)
def test_every_move_within_the_bound(name, mode):
    """k_mc_delta on one frame: moves of every class the geometry has (j in i's 3-body range, in pair range only, in neither,
    met through several images), the moves that change nothing, every transmutation of the chosen atoms."""
    _assert_classes(name, mode)
    assert len(P.mc_reference(name, mode)["i"]) <= 200
    _hold(f"k_mc_delta {mode}", name, _device(name, mode), P.mc_reference(name, mode))


# ================================================================================================ new shapes
@pytest.mark.parametrize("mode", P.MC_MODES)
def test_ragged_batch_equals_its_frames_alone_bit_for_bit(mode):
    """A cluster, a slab with atoms outside its cell and a 3-atom cell thinner than the reach in ONE object, the proposals
    addressed to the frames in mixed order: the results are those of one-frame objects bit for bit, and within the bound."""
    frames = [P.mc_cases()[k][1] for k in BATCH]
    assert len({id(P.mc_cases()[k][0]) for k in BATCH}) == 1 and [len(a) for a in frames] == [9, 12, 3]
    assert [tuple(bool(x) for x in a.get_pbc()) for a in frames] == [(False,) * 3, (True, True, False), (True,) * 3]
    refs = [P.mc_reference(k, mode) for k in BATCH]
    f = np.concatenate([np.full(len(r["i"]), k) for k, r in enumerate(refs)])
    i = np.concatenate([r["i"] for r in refs])
    second = [s for r in refs for s in r["second"]]
    order = np.random.default_rng(7).permutation(len(f))
    assert np.any(np.diff(f[order]) < 0)                      # (mixed order indeed)
    with _chain(_calc(P.mc_cases()[BATCH[0]][0], refs[0]["coeff"]), frames, mode) as chain:
        got = np.empty(len(f))
        got[order] = chain.delta_energy(f[order], i[order], [second[q] for q in order])
    for k, name in enumerate(BATCH):
        assert np.array_equal(got[f == k], _device(name, mode)), name
        _hold(f"k_mc_delta {mode}, batch of three", name, got[f == k], refs[k])


@pytest.mark.parametrize("mode", P.MC_MODES)
def test_frame_of_more_than_256_atoms(mode):
    """288 atoms: the species reach LDS by a strided load, and at least a third of the moves touch an atom past 255."""
    name = "mow288"
    ref = P.mc_reference(name, mode)
    n = len(P.mc_cases()[name][1])
    high = np.array([(i >= 256) or (mode == "swap" and int(j) >= 256) for i, j in zip(ref["i"], ref["second"])])
    assert 288 <= n <= 432 and 3 * high.sum() >= len(high) and len(high) <= 200
    _assert_classes(name, mode)
    _hold(f"k_mc_delta {mode}", name, _device(name, mode), ref)


def _list_shape(name, mode):
    """(n_c, distinct affected centres outside T, most entries one real atom has in the list) of the case's live moves"""
    basis, atoms, _, _ = P.mc_cases()[name]
    ref = P.mc_reference(name, mode)
    c = P.mc_counts(basis, atoms)
    out = []
    for i, j, lab in zip(ref["i"], ref["second"], ref["label"]):
        if lab == "null":
            continue
        T = [int(i)] + ([int(j)] if mode == "swap" else [])
        entries = sum(c["in3"][t] for t in T)
        out.append((2 + int(sum(c["n3"][t] for t in T)), int(np.count_nonzero(np.delete(entries, T))), int(entries.max())))
    return out


@pytest.mark.parametrize("mode", P.MC_MODES)
def test_candidate_list_past_one_round_with_mostly_distinct_atoms(mode):
    """Compressed bcc 6 x 6 x 6: a swap's candidate list holds more than 256 entries and more than 200 DISTINCT centres -- the
    later rounds look back over real work, not over repeats.  (A transmutation's list is half as long: one round, 120 centres.)"""
    name = "dense432"
    shape = _list_shape(name, mode)
    print(f"dense432 {mode} (n_c, distinct centres, most repeats):", shape)
    assert 1 <= len(shape) <= 8
    if mode == "swap":
        assert all(n_c > ROUND and distinct > 200 for n_c, distinct, _ in shape)
    _assert_classes(name, mode)
    _hold(f"k_mc_delta {mode}", name, _device(name, mode), P.mc_reference(name, mode))


@pytest.mark.parametrize("mode", P.MC_MODES)
@pytest.mark.parametrize("name, past", [("thin16_r3", 2 * ROUND), ("thin16_r4", 3 * ROUND)])
def test_heavy_de_duplication_over_several_rounds(name, past, mode):
    """A 16-atom cell of 2 A against a reach of 7: a swap's n_c past 512 (three rounds) and past 768 (four), at most 14 distinct
    centres outside T, every real atom dozens of times in the list; a transmutation's list is half as long (two rounds)."""
    shape = _list_shape(name, mode)
    print(f"{name} {mode} (n_c, distinct centres, most repeats):", shape)
    assert shape and all(n_c > (past if mode == "swap" else ROUND) and distinct <= 15 and repeats >= 24 for n_c, distinct, repeats in shape)
    assert mode != "swap" or past + ROUND >= max(s[0] for s in shape)
    _assert_classes(name, mode)
    _hold(f"k_mc_delta {mode}", name, _device(name, mode), P.mc_reference(name, mode))


def test_the_limit_of_512_entries_is_reached_and_513_is_refused():
    """The longest 3-body list holds exactly UF3_MC_MAX_N3 entries and the swap of that atom with its translate of the other
    species fills the candidate list to n_c = 1026, the last slot of the fifth round; the atom's pair index runs to
    512 * 511 / 2 - 1 = 130815.  The neighbouring cell whose longest list holds 513 is refused by uf3_mc_create with the
    message of the limit, and the context then evaluates an ordinary frame as before."""
    name = "limit512"
    basis, atoms, _, _ = P.mc_cases()[name]
    over = P.limit_frames()[1]
    n3 = P.mc_counts(basis, atoms)["n3"]
    ref = P.mc_reference(name, "swap")
    k = ref["label"].index("last_slot")
    i, j = int(ref["i"][k]), int(ref["second"][k])
    assert n3.max() == MAX_N3 == n3[i] == n3[j] and 2 + n3[i] + n3[j] == 2 + 2 * MAX_N3 == 1026 and 1026 > 4 * ROUND
    assert MAX_N3 * (MAX_N3 - 1) // 2 - 1 == 130815
    assert P.mc_counts(basis, over)["n3"].max() == MAX_N3 + 1
    P.clear_of_discontinuities(basis, over)
    calc = _calc(basis, ref["coeff"])
    ordinary = P.cases()["mow_lead0"][1]
    e_before = calc.evaluate_frames([ordinary], forces=False)[0]
    _assert_classes(name, "swap")                              # (a transmutation's list, n_c = 514, is the thin cells' ground)
    _hold("k_mc_delta swap", name, _device(name, "swap"), ref)
    with pytest.raises(_lib.UF3Error, match=r"has 513 neighbours in the 3-body range, more than the 512 the trial kernel's LDS list holds"):
        _chain(calc, [over], "swap")
    e_after = calc.evaluate_frames([ordinary], forces=False)[0]
    _, _, val, mag = P.reference("mow_lead0")
    assert np.array_equal(e_before, e_after) and P.ratio(e_after[0], val["e"], mag["e"]) <= P.GAMMA["e"]
    with _chain(calc, [ordinary], "swap") as chain:            # (and Monte Carlo itself carries on)
        r0 = P.mc_reference("mow_lead0", "swap")
        _hold("k_mc_delta swap, after the refusal", "mow_lead0", chain.delta_energy(np.zeros(len(r0["i"]), dtype=int), r0["i"], list(r0["second"])), r0)


# ================================================================================================ the running energy
RUN_CASE, RUN_TRIALS, RUN_T = "bcc24_s4", 200, 4000.0
RUN_SEEDS = {"swap": 41, "transmute": 42}


@pytest.mark.parametrize("mode", P.MC_MODES)
def test_running_energy_of_a_chain(mode):
    """k_mc_trials: 200 trials on 24 atoms of four species, replayed by tests/_mc_ref.py on extended-oracle energies rounded to
    double.  No decision of the replay hangs on less than 1e-6, so decisions, species and counters are identical, and the
    running energy E_0 + sum of the accepted dE lies within
        u (GAMMA_e M_e(initial) + GAMMA_dE sum_k M_dE,k + sum_k |E_k|)
    of the extended energy of the final species: the evaluator's bound on E_0, mc_delta's on every accepted difference, and
    one rounding of ``E += dE`` per accepted move k (E_k the running energy after it)."""
    basis, atoms, _, _ = P.mc_cases()[RUN_CASE]
    assert len(atoms) <= 24
    ref = P.mc_reference(RUN_CASE, mode)
    ob, coeff = ref["ob"], ref["coeff"]
    els = list(basis.chemical_system.element_list)
    zs = np.array([atomic_numbers[e] for e in els])
    seed = RUN_SEEDS[mode]

    def energies_of(spec):
        return [float(O.evaluate_x(ob, with_numbers(atoms, zs[s]), coeff, virial=False, forces=False)[0]["e"]) for s in spec]
    species0 = np.searchsorted(zs, atoms.get_atomic_numbers())
    mu = None if mode == "swap" else [0.0] * len(els)
    replay = R.Chains(energies_of, [species0], [RUN_T], R.SWAP if mode == "swap" else R.TRANSMUTE, seed, len(els), mu=mu)
    replay.run(RUN_TRIALS)
    worst = min(replay.margins)
    print(f"{mode}: {sum(1 for d in replay.decisions if not d[2])} live trials, {int(replay.accepted[0])} accepted, smallest margin {worst:.3e}")
    assert worst >= 1e-6 and replay.accepted[0] >= 10
    # the accepted moves once more, for their magnitudes and the running energies after each
    spec, run_e = species0.copy(), float(energies_of([species0])[0])
    sum_m, sum_e = np.longdouble(0), np.longdouble(0)
    for (_, t, null, accepted, dE) in replay.decisions:
        if null or not accepted:
            continue
        mv = R.propose(R.SWAP if mode == "swap" else R.TRANSMUTE, R.words(0, t, seed), spec, None, None if mu is None else np.array(mu))
        now = with_numbers(atoms, zs[spec])
        second = mv["j"] if mode == "swap" else els[mv["new_i"]]
        sum_m += O.mc_delta_x(ob, now, coeff, [mv["i"]], [second], mode)[1][0]
        spec[mv["i"]] = mv["new_i"]
        if mv["j"] >= 0:
            spec[mv["j"]] = mv["new_j"]
        run_e += dE
        sum_e += abs(run_e)
    assert np.array_equal(spec, replay.species[0])
    with _chain(_calc(basis, coeff), [atoms], mode, temperature_K=RUN_T, seed=seed) as chain:
        out = chain.run(RUN_TRIALS)
        got_z = chain.numbers
    assert np.array_equal(got_z, zs[replay.species[0]])
    assert np.array_equal(out["accepted"], replay.accepted) and np.array_equal(out["trials"], replay.trials)
    final, _ = O.evaluate_x(ob, with_numbers(atoms, zs[replay.species[0]]), coeff, virial=False, forces=False)
    m_e0 = O.evaluate_x(ob, atoms, coeff, virial=False, forces=False)[1]["e"]
    bound = P.U * (P.GAMMA["e"] * np.longdouble(m_e0) + P.GAMMA["dE"] * sum_m + sum_e)
    err = abs(np.longdouble(out["energy"][0]) - final["e"])
    print(f"|E_run - E_x(final)| = {float(err):.3e}, bound {float(bound):.3e}; in units of u (M_e + sum M_dE + sum |E_k|):")
    print(f"[precision] k_mc_trials {mode} running energy, {RUN_CASE}: dE {float(err / (P.U * (np.longdouble(m_e0) + sum_m + sum_e))):.3g}")
    assert err <= bound
