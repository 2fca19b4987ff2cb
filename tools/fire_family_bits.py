#!/usr/bin/env python3
"""Bit identity of the FIRE family (relaxation, NEB, cell NEB, IDPP bands) between two builds of libuf3hip.so.

    UF3_LIB_PATH=/path/to/libuf3hip.so python tools/fire_family_bits.py OUT.json [ARRAYS.npz]

runs one fixed set of cases on the library UF3_LIB_PATH names (uf3_amd/_lib.py's switch; default: the tree's) and writes the
sha256 of every array the drivers return.  Run it once per library, each in a process of its own, and compare the files: every
digest must be equal, only "build_id" may differ (python tools/fire_family_bits.py --compare A.json B.json does that).

The cases are the smallest that reach every line of uf3_relax.h and uf3_neb.h: frames and images of 300 atoms (two chunks,
256 + 44, so the strided sum over chunk partials has more than one term) next to ones of 3 and 4 atoms, fixed masks, skewed
and changing cells, climbing off and on, a default and a given cell factor, and neb_forces asked of bands that have stopped
(the all = 1 path).  The models and builders are the tests' own (tests/test_gpu_relax.py, test_gpu_neb.py, test_gpu_ssneb.py).

A condition on the inputs: the NumPy restatements (tests/_relax_ref.py, _neb_ref.py, _ssneb_ref.py) run on the same inputs, and
in each of the three families they must take every FIRE branch at least once -- the first move, g.v > 0 past NMIN (the time
step grows), the uphill reset, and the trust-radius cut.  The counts go into the file; no digest is written if one is zero."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

BRANCHES = ("first_move", "downhill_past_nmin", "uphill_reset", "trust_radius_cut")
STEPS = 25
# two runs per handle: a long first time step so that a move overshoots within 25 steps, then a trust radius that always cuts
WIDE = dict(dt=0.3, dt_max=1.0, maxstep=0.2)
TIGHT = dict(dt=0.3, dt_max=1.0, maxstep=0.005)
NEVER = 1e-9            # fmax no case reaches: every run makes all its steps
ALWAYS = 1e9            # fmax every band meets: run(0, fmax=ALWAYS) stops them all without a move


def compare(a, b):
    A, B = (json.load(open(p)) for p in (a, b))
    A.pop("build_id"), B.pop("build_id")
    flat = lambda d, pre="": {k2: v2 for k, v in d.items()
                              for k2, v2 in (flat(v, pre + k + "/") if isinstance(v, dict) else {pre + k: v}).items()}
    A, B = flat(A), flat(B)
    bad = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
    print(f"{len(A)} entries, {len(bad)} differ" + "".join(f"\n  {k}" for k in bad))
    return 1 if bad else 0


def main(out_path, arrays_path=None):
    import numpy as np
    from uf3_amd import _lib
    from uf3_amd.data.atoms import Atoms
    from uf3_amd.forcefield import neb
    from uf3_amd.forcefield.neb import CellNudgedElasticBand, IDPP, NudgedElasticBand
    from uf3_amd.forcefield.relax import Relaxation
    from _relax_ref import N_MIN
    import test_gpu_neb as TN
    import test_gpu_relax as TR
    import test_gpu_ssneb as TS

    calc = TN._unary()
    digests, counts, raw = {}, {}, {}

    def put(case, **arrays):
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            raw[f"{case}/{name}"] = a
            digests.setdefault(case, {})[name] = f"{a.dtype}{list(a.shape)}:" + hashlib.sha256(a.tobytes()).hexdigest()

    def put_run(case, out):
        rec = out.pop("records")
        flat = {k: (np.concatenate(v) if k == "energies" else v) for k, v in out.items() if k != "status"}
        put(case, status=np.array([str(s) for s in out["status"]]), **flat, **{"rec_" + k: v for k, v in rec.items()})

    def watch(ref, unit, family):
        """Count the FIRE branches ``ref`` takes: ``unit`` is its per-frame / per-band step, seen from its state around it."""
        tally = counts.setdefault(family, dict.fromkeys(BRANCHES, 0))
        inner, now = getattr(ref, unit), {}

        def step(u, *a):
            first, n_pos, steps = bool(ref.first[u]), int(ref.n_pos[u]), int(ref.steps[u])
            seen, ref.max_dr = ref.max_dr, 0.0
            inner(u, *a)
            if ref.steps[u] > steps:
                tally["first_move"] += int(first)
                tally["uphill_reset"] += int(not first and ref.n_pos[u] == 0)
                tally["downhill_past_nmin"] += int(not first and ref.n_pos[u] > 0 and n_pos > N_MIN)
                tally["trust_radius_cut"] += int(ref.max_dr > now["maxstep"] * (1 - 1e-9))  # (a cut step is maxstep long to rounding)
            ref.max_dr = max(seen, ref.max_dr)
        setattr(ref, unit, step)

        def run(steps, **kw):
            now["maxstep"] = kw["maxstep"]
            ref.run(steps, **kw)
        return run

    def sheared(a, eps):
        d = np.eye(3) + np.asarray(eps, float)
        return Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions() @ d, cell=np.asarray(a.get_cell(), float) @ d,
                     pbc=a.get_pbc())

    # ---- relaxation: a 300-atom frame and a 3-atom frame in one batch ---------------------------------------------------
    a = TR.A0_W
    three = Atoms(numbers=[74] * 3, positions=np.array([[0.05, 0.0, 0.02], [0.5 * a, 0.52 * a, 0.49 * a], [0.02, -0.03, 0.98 * a]]),
                  cell=np.diag([a, a, 1.5 * a]), pbc=True)
    skew = [[0.0, 0.02, -0.01], [0.015, 0.0, 0.03], [0.0, -0.02, 0.0]]
    for case, frames, relax_cell, fixed in (
            ("relax_fixed", [TR._w300(), three], False, np.arange(303) % 7 == 3),
            ("relax_cell", [sheared(TR._w300(), skew), sheared(three, skew)], True, None)):
        ref_run = watch(TR._reference(calc, frames, relax_cell, fixed), "_frame", "relax")
        with Relaxation(calc, frames, relax_cell=relax_cell, fixed=fixed) as rel:
            for k, kw in enumerate((WIDE, TIGHT)):
                put_run(f"{case}/run{k}", rel.run(STEPS, fmax=NEVER, record_every=1, **kw))
                ref_run(STEPS, fmax=NEVER, **kw)
                put(f"{case}/run{k}", positions=rel.get_positions(), cells=rel.get_cells(), forces=rel.get_forces())

    # ---- bands: 3 images of 300 atoms and 5 images of 4 atoms in one batch ----------------------------------------------
    def pushed(m, reps, seed, strain):
        """tests/test_gpu_ssneb.py's band between two rattled ends, atom 3 of the last pushed aside; with ``strain`` None
        every image in the first end's cell."""
        if strain is not None:
            return TS._strained_band(m, reps, seed, strain=strain, push=[0.25, 0.1, -0.15])
        frac, cell, z = TS._bcc(reps, seed=seed)
        ini, fin = TS._end(frac, cell, z, seed, 0.002), TS._end(frac, cell, z, seed + 1000, 0.005)
        fin.positions[3] += [0.25, 0.1, -0.15]
        return neb.interpolate(ini, fin, m)

    shapes = ((3, (5, 5, 6), 5), (5, (2, 1, 1), 3))
    spring = np.array([0.1, 0.3])

    def band_runs(case, band, ref_run, extra):
        for k, (climb, kw) in enumerate(((False, WIDE), (True, TIGHT))):
            put_run(f"{case}/run{k}", band.run(STEPS, fmax=NEVER, climb=climb, record_every=1, **kw))
            ref_run(STEPS, fmax=NEVER, climb=climb, **kw)
            put(f"{case}/run{k}", positions=band.get_positions())
        put_run(f"{case}/stopped", band.run(0, fmax=ALWAYS, climb=True, record_every=1, **TIGHT))
        put(f"{case}/stopped", positions=band.get_positions(), forces=band.get_forces(), neb_forces=band.get_neb_forces(),
            **{k: f() for k, f in extra.items()})

    bands = [pushed(m, reps, seed, None) for m, reps, seed in shapes]
    assert [(len(b), len(b[0])) for b in bands] == [(3, 300), (5, 4)]
    fixed = np.concatenate([np.tile(np.arange(len(b[0])) % 11 == 1, len(b)) for b in bands])
    with NudgedElasticBand(calc, bands, spring=spring, fixed=fixed) as band:
        band_runs("neb", band, watch(TN._reference(calc, bands, spring=spring, fixed=fixed), "_band", "neb"), {})

    bands = [pushed(m, reps, seed, (0.01, 0.04)) for m, reps, seed in shapes]
    for case, cf in (("ssneb_default_factor", None), ("ssneb_given_factor", np.array([450.0, 6.0]))):
        ref_run = watch(TS._reference(calc, bands, spring=spring, cell_factor=cf), "_band", "ssneb")
        with CellNudgedElasticBand(calc, bands, spring=spring, cell_factor=cf) as band:
            band_runs(case, band, ref_run, dict(cells=band.get_cells, virials=band.get_virials, cell_forces=band.get_cell_forces,
                                                neb_cell_forces=band.get_neb_cell_forces))

    # ---- IDPP: 5 images of 20 atoms in a skewed periodic cell ----------------------------------------------------------
    frac, cell, z = TS._bcc((5, 2, 1))
    ini, fin = sheared(TS._end(frac, cell, z, 21, 0.002), skew), sheared(TS._end(frac, cell, z, 1021, 0.005), skew)
    fin.positions[3] += [0.25, 0.1, -0.15]
    with IDPP(neb.interpolate(ini, fin, 5), spring=0.1, fixed=np.tile(np.arange(20) == 7, 5)) as band:
        put_run("idpp/run0", band.run(STEPS, fmax=NEVER, record_every=1, **WIDE))
        put("idpp/run0", positions=band.get_positions(), forces=band.get_forces(), neb_forces=band.get_neb_forces())

    print(json.dumps(counts))
    missing = [f"{fam}: {b}" for fam, t in counts.items() for b in BRANCHES if not t[b]]
    if missing:
        sys.exit("the restatements never took: " + ", ".join(missing) + " -- no digests written")
    with open(out_path, "w") as f:
        json.dump(dict(build_id=_lib.build_id(), branches={fam: {b: int(n) for b, n in t.items()} for fam, t in counts.items()},
                       digests=digests), f, indent=1, sort_keys=True)
        f.write("\n")
    if arrays_path:                     # where a digest differs: the arrays themselves, to see which entries do
        np.savez(arrays_path, **raw)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) == 3 else None)
