"""NumPy restatement of the device Monte Carlo (uf3_amd/csrc/uf3_mc.h) for tests/test_mc_host.py and tests/test_gpu_mc.py:
the proposals from ``_md_ref.philox``, the energy difference as the difference of two FULL energies from a callable, the
Metropolis rule, the records, and the analytic site occupancy of a model with one-body terms only."""
import numpy as np

from uf3_amd.forcefield.mc import KB
import _md_ref

SWAP, TRANSMUTE = 0, 1


def words(frame, trial, seed):
    """r0 .. r3 (Python ints) of frame ``frame`` at absolute trial ``trial``: counter (f, t lo, t hi, 0), key (seed lo, seed hi)."""
    ctr = np.array([[frame & 0xFFFFFFFF, trial & 0xFFFFFFFF, (trial >> 32) & 0xFFFFFFFF, 0]], dtype=np.uint64).astype(np.uint32)
    key = np.array([[seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]], dtype=np.uint64).astype(np.uint32)
    return [int(x) for x in _md_ref.philox(ctr, key)[0]]


def pick(word, n):
    """(word * n) >> 32 in integer arithmetic: an index in [0, n)."""
    return (int(word) * int(n)) >> 32


def uniform(hi, lo):
    return float(_md_ref._uniform(np.array([hi], dtype=np.uint32), np.array([lo], dtype=np.uint32))[0])


def propose(mode, r, species, swappable=None, mu=None):
    """The move of words ``r`` on a frame whose atoms have the species indices ``species``: dict(null, i, j, new_i, new_j, dmu)
    (j = -1 and new_j = None in transmute mode; a null trial changes nothing)."""
    n = len(species)
    i = pick(r[0], n)
    ok = (lambda a: True) if swappable is None else (lambda a: bool(swappable[a]))
    if mode == SWAP:
        j = pick(r[1], n)
        null = i == j or species[i] == species[j] or not (ok(i) and ok(j))
        return dict(null=null, i=i, j=j, new_i=int(species[j]), new_j=int(species[i]), dmu=0.0)
    allowed = [s for s in range(len(mu)) if np.isfinite(mu[s])]
    zo = int(species[i])
    others = [s for s in allowed if s != zo]
    null = not ok(i) or zo not in allowed or not others
    if null:
        return dict(null=True, i=i, j=-1, new_i=zo, new_j=None, dmu=0.0)
    new = others[pick(r[1], len(allowed) - 1)]
    return dict(null=False, i=i, j=-1, new_i=new, new_j=None, dmu=float(mu[new] - mu[zo]))


def site_occupancy(de1, dmu, temperature_K):
    """Probability of species B on a site of a model with one-body terms only: 1 / (1 + exp((de1 - dmu) / kT)), de1 = e1(B) -
    e1(A), dmu = mu(B) - mu(A) (detailed balance of the transmutation move between two allowed species)."""
    return 1.0 / (1.0 + np.exp((de1 - dmu) / (KB * temperature_K)))


class Chains:
    """A batch of chains.  ``energies_of(list of species-index arrays) -> [n_frames]`` full energies.  ``species``: list of int
    arrays (indices into the element list), changed in place by ``run``."""

    def __init__(self, energies_of, species, temperatures_K, mode, seed, n_species, mu=None, swappable=None):
        self.energies_of = energies_of
        self.species = [np.array(s, dtype=np.int64) for s in species]
        self.kT = KB * np.asarray(temperatures_K, dtype=float)
        self.mode, self.seed, self.S = mode, int(seed), int(n_species)
        self.mu = None if mu is None else np.asarray(mu, dtype=float)
        off = np.cumsum([0] + [len(s) for s in self.species])
        self.swappable = [None if swappable is None else np.asarray(swappable)[off[k]:off[k + 1]] for k in range(len(self.species))]
        self.trial = 0
        nf = len(self.species)
        self.e_full = np.array(self.energies_of(self.species), dtype=float)      # full energy of the current species
        self.energy = self.e_full.copy()                                          # running: start + accepted differences
        self.accepted = np.zeros(nf, dtype=np.int64)
        self.trials = np.zeros(nf, dtype=np.int64)
        self.margins = []             # |exp(-dE' / kT) - u| of every non-null trial (kT > 0)
        self.decisions = []           # (frame, trial, null, accepted, dE)

    def run(self, n_trials, record_every=0):
        nf = len(self.species)
        records = []
        for k in range(n_trials):
            t = self.trial
            moves, proposed = [], []
            for f in range(nf):
                r = words(f, t, self.seed)
                mv = propose(self.mode, r, self.species[f], self.swappable[f], self.mu)
                mv["u"] = uniform(r[2], r[3])
                z = self.species[f].copy()
                if not mv["null"]:
                    z[mv["i"]] = mv["new_i"]
                    if mv["j"] >= 0:
                        z[mv["j"]] = mv["new_j"]
                moves.append(mv)
                proposed.append(z)
            e_new = np.asarray(self.energies_of(proposed), dtype=float) if any(not m["null"] for m in moves) else self.e_full
            for f, mv in enumerate(moves):
                self.trials[f] += 1
                if mv["null"]:
                    self.decisions.append((f, t, True, False, 0.0))
                    continue
                dE = e_new[f] - self.e_full[f]
                dEp = dE - mv["dmu"]
                if self.kT[f] > 0:
                    p = np.exp(-dEp / self.kT[f])
                    self.margins.append(abs(p - mv["u"]))
                    accept = dEp <= 0 or mv["u"] < p
                else:
                    accept = dEp <= 0
                if accept:
                    self.species[f] = proposed[f]
                    self.e_full[f] = e_new[f]
                    self.energy[f] += dE
                    self.accepted[f] += 1
                self.decisions.append((f, t, False, bool(accept), float(dE)))
            self.trial += 1
            if record_every and (k + 1) % record_every == 0:
                records.append([[self.energy[f], self.accepted[f], self.trials[f]] +
                                [int(np.sum(self.species[f] == s)) for s in range(self.S)] for f in range(nf)])
        return np.array(records, dtype=float).reshape(-1, nf, 3 + self.S)
