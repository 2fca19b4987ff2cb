#!/usr/bin/env python3
"""Bit identity of the MD family (NVE / Langevin runs, heat-current and grade samples, NPH / NPT) between two builds of
libuf3hip.so.

    UF3_LIB_PATH=/path/to/libuf3hip.so python tools/md_family_bits.py OUT.json [ARRAYS.npz]

runs one fixed set of cases on the library UF3_LIB_PATH names (uf3_amd/_lib.py's switch; default: the tree's) and writes the
sha256 of every array the driver returns.  Run it once per library, each in a process of its own, and compare the files: every
digest must be equal, only "build_id" may differ (python tools/md_family_bits.py --compare A.json B.json; the comparison is
tools/fire_family_bits.py's).

The cases are the smallest that reach every line of the run loop, its samplers, uf3_md.h and uf3_npt.h: one batch of a
300-atom frame (two NPT chunks, 256 + 44; a thread of the 256-wide thermo sum with two terms) and a 3-atom frame (idle threads),
at most 30 steps a run; every <LANGEVIN, THERMO> instance, records with and without stress, on the final close and not; flux
and grade samples on steps with and without a thermo record and on the last step; a grade run that stops inside, and the run
that goes on from there; NPH and NPT as one run and as two (the second opens with the first's G), in a skewed cell, under a
compression that rebuilds the lists; positions and velocities set between runs.  The models are the tests' own
(tests/test_gpu_md.py's and test_gpu_flux.py's unary model, test_gpu_site_grade.py's with a posterior), the 300-atom frame is
test_gpu_npt.py's.

After every run: positions, velocities, forces, energies, the raw thermo records, the flux or grade records and steps_done,
cells, scales, strain rates and the step counter.  No digest is written unless the stopped grade run made fewer steps than asked
and more than zero, the compression saw more than one list build, and every two-run case advanced the step counter by the sum;
what was observed goes into the file."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def main(out_path, arrays_path=None):
    import numpy as np
    from uf3_amd import _lib, synthetic
    from uf3_amd.data.atoms import Atoms
    from uf3_amd.forcefield import calculator, md
    import test_gpu_md as TM
    import test_gpu_site_grade as TG

    digests, observed, raw, thermo_raw = {}, {}, {}, []

    def keep_raw(inner):                    # the raw records of a run, on their way into the dict it returns
        def records(raw_records, *a, **kw):
            out = inner(raw_records, *a, **kw)      # (npt_records calls thermo_records on a slice: the whole record comes last)
            thermo_raw.append(np.array(raw_records))
            return out
        return records
    md.thermo_records, md.npt_records = keep_raw(md.thermo_records), keep_raw(md.npt_records)

    def put(case, dyn, rec):
        arrays = dict(positions=dyn.get_positions(), velocities=dyn.get_velocities(), forces=dyn.get_forces(),
                      energies=dyn.get_potential_energies(), cells=dyn.cells, scales=dyn.cell_scales, strain_rates=dyn.strain_rates,
                      step=np.array(dyn.step), thermo_raw=thermo_raw[-1], **{"rec_" + k: np.asarray(v) for k, v in rec.items()})
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            raw[f"{case}/{name}"] = a
            digests.setdefault(case, {})[name] = f"{a.dtype}{list(a.shape)}:" + hashlib.sha256(a.tobytes()).hexdigest()

    def two_runs(case, dyn, first, between, second):
        """run(**first), ``between(dyn)``, run(**second) on one object; the step counter must advance by the sum"""
        t0 = dyn.step
        put(case + "/run0", dyn, dyn.run(**first))
        between(dyn)
        put(case + "/run1", dyn, dyn.run(**second))
        observed.setdefault("two_run_steps", {})[case] = [first["n_steps"], second["n_steps"], dyn.step - t0]

    a = 3.165
    w300 = synthetic.lattice_frame("bcc", (5, 5, 6), a, [74], seed=17)
    three = Atoms(numbers=[74] * 3, positions=np.array([[0.05, 0.0, 0.02], [0.5 * a, 0.52 * a, 0.49 * a], [0.02, -0.03, 0.98 * a]]),
                  cell=np.diag([a, a, 1.5 * a]), pbc=True)
    frames = [w300, three]
    assert [len(f) for f in frames] == [300, 3]

    def sheared(f):
        d = np.eye(3) + np.array([[0.0, 0.02, -0.01], [0.015, 0.0, 0.03], [0.0, -0.02, 0.0]])
        return Atoms(numbers=f.get_atomic_numbers(), positions=f.get_positions() @ d, cell=np.asarray(f.get_cell(), float) @ d, pbc=True)

    def start(calc, frames=frames, friction=0.0, **kw):
        dyn = md.MolecularDynamics(calc, frames, 1.0, masses=TM.MASSES, temperature_K=300.0, friction_per_fs=friction, seed=7, **kw)
        dyn.initialize_velocities(300.0, seed=3)
        return dyn

    calc = TM._unary()
    nothing = lambda dyn: None                                  # noqa: E731

    # ---- constant volume: every <LANGEVIN, THERMO> instance, a record on the final close and none ------------------------
    for name, friction in (("nve", 0.0), ("langevin", 0.02)):
        with start(calc, friction=friction) as dyn:
            for k, kw in enumerate((dict(n_steps=7), dict(n_steps=7, thermo_every=1), dict(n_steps=9, thermo_every=3, stress=True),
                                    dict(n_steps=10, thermo_every=3, stress=True))):
                put(f"{name}/run{k}", dyn, dyn.run(**kw))
        # samples on steps with a thermo record (6, 12) and without, and on the last step
        with start(calc, friction=friction) as dyn:
            put(f"{name}/flux", dyn, dyn.run(12, thermo_every=3, stress=True, flux_every=2))

    # ---- positions set between two runs: the forces are evaluated again --------------------------------------------------
    def shift(dyn):
        dyn.set_positions(dyn.get_positions() + 0.01 * np.sin(np.arange(3 * 303, dtype=float)).reshape(303, 3))
    with start(calc, friction=0.02) as dyn:
        two_runs("set_positions", dyn, dict(n_steps=5, thermo_every=2), shift, dict(n_steps=6, thermo_every=2))

    # ---- grade samples: a free run, one that a sample stops strictly inside, and the run that goes on from there ---------
    graded = calculator.UFCalculator(TG._graded_model(), md_skin=0.0)
    asked = 12
    for name, friction in (("nve", 0.0), ("langevin", 0.02)):
        with start(graded, friction=friction) as dyn:
            free = dyn.run(asked, thermo_every=3, grade_every=2)
            put(f"{name}/grade_free", dyn, free)
        maxima = free["grade"].max(axis=1)
        stop = 0.5 * (maxima[:-1].min() + maxima[:-1].max())        # a sample before the last exceeds it
        with start(graded, friction=friction) as dyn:
            rec = dyn.run(asked, thermo_every=3, grade_every=2, grade_stop=stop)
            put(f"{name}/grade_stopped", dyn, rec)
            done = int(rec["steps_done"])
            put(f"{name}/grade_goes_on", dyn, dyn.run(6, thermo_every=3, grade_every=2))
            observed.setdefault("grade_stop", {})[name] = dict(maxima=[float(x) for x in maxima], stop=float(stop), asked=asked,
                                                               steps_done=done, step_after_both=dyn.step)

    # ---- constant pressure: NPH and NPT (piston friction), one run and two; a skewed cell; velocities drawn between runs ----
    baro = dict(pressure_eV_A3=0.02, barostat_time_fs=1000.0)
    for name, kw, fr in (("nph", dict(friction=0.0, **baro), frames),
                         ("npt", dict(friction=0.05, barostat_friction_per_fs=0.02, **baro), frames),
                         ("npt_skewed", dict(friction=0.05, barostat_friction_per_fs=0.02, **baro), [sheared(f) for f in frames])):
        with start(calc, fr, **kw) as dyn:
            put(f"{name}/one_run", dyn, dyn.run(12, thermo_every=3))
        with start(calc, fr, **kw) as dyn:
            two_runs(name, dyn, dict(n_steps=7, thermo_every=3), nothing, dict(n_steps=5, thermo_every=1))
    with start(calc, friction=0.05, barostat_friction_per_fs=0.02, **baro) as dyn:
        two_runs("npt_new_velocities", dyn, dict(n_steps=5), lambda d: d.initialize_velocities(300.0, seed=5),
                 dict(n_steps=5, thermo_every=5))

    # ---- a compression that uses up the skin: the lists are built again on the way (tests/test_gpu_npt.py's, shorter) ------
    ctx = _lib.get_context(calc.device)
    builds = ctx.md_stats()["builds"]
    with start(calc, friction=0.0, skin=0.1, pressure_eV_A3=0.3, barostat_time_fs=1000.0) as dyn:
        put("nph_compression", dyn, dyn.run(30, thermo_every=10))
        observed["compression"] = dict(builds=int(ctx.md_stats()["builds"] - builds), scales=[float(s) for s in dyn.cell_scales])

    print(json.dumps(observed))
    wrong = [f"grade run of {name}: {g['steps_done']} of {g['asked']} steps" for name, g in observed["grade_stop"].items()
             if not 0 < g["steps_done"] < g["asked"] or g["step_after_both"] != g["steps_done"] + 6]
    wrong += [f"compression: {observed['compression']['builds']} list build"] * (observed["compression"]["builds"] < 2)
    wrong += [f"{case}: {n0} + {n1} steps advanced the counter by {d}" for case, (n0, n1, d) in observed["two_run_steps"].items()
              if d != n0 + n1]
    if wrong:
        sys.exit("the inputs miss their paths: " + "; ".join(wrong) + " -- no digests written")
    with open(out_path, "w") as f:
        json.dump(dict(build_id=_lib.build_id(), observed=observed, digests=digests), f, indent=1, sort_keys=True)
        f.write("\n")
    if arrays_path:                     # where a digest differs: the arrays themselves, to see which entries do
        np.savez(arrays_path, **raw)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        from fire_family_bits import compare
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) == 3 else None)
