#!/usr/bin/env python3
"""Bits and routes of the evaluator (every ``uf3_eval*`` entry, i.e. eval_impl and eval_host) between two builds of libuf3hip.so.

    UF3_LIB_PATH=/path/to/libuf3hip.so python tools/eval_bits.py OUT.json [ARRAYS.npz]
    python tools/eval_bits.py --compare A.json B.json                       (tools/fire_family_bits.py's comparison)
    python tools/eval_bits.py --verdict PARENT_A PARENT_B TREE OUT.json     (stems: STEM.json and STEM.npz of three runs)

runs one fixed list of cases on the library UF3_LIB_PATH names (uf3_amd/_lib.py's switch; default: the tree's), one process per
library, and writes per case: the sha256 of energies, forces and strain derivatives, the ``uf3: k_eval ...`` launch reports the
library wrote meanwhile (UF3_DEBUG_LDS; fd 2 goes to a file for the run and is read back), ``uf3_ctx_md_stats`` and the context's
3-body list capacity afterwards (``uf3_n3_lists_debug``).

The main cases run in a fixed order on ONE context, so "first call" and "tuned" are part of a case: unary W (notebook basis) bcc
frames of 128 (what bench.py's eval_128 runs), 2000 (zero-copy mirror, polled wait), 2662 (pinned result copy), 6750 and 8192
(part sums begin) and 24 334 atoms (unpinned results) through the host entries -- energies only (gather), forces, forces + strain
derivative, without and with a skin --, a seeded +-0.01 A walk with the skin and then one atom moved by 0.3 A (the step is
discarded and repeated), a cell change, blocks of atoms and of centres [0, 50) [50, 128) with and without the skin on host and
device entries, the device entries on 128 and 8192 atoms; then a Mo-W model: a species change on the MD route, a batch of three
frames (one of 3 atoms) dense enough for lists beyond 16 entries, and denser frames after sparse ones so that the list capacity
regrows in both retry loops.  Each switch of the evaluator then runs the 128-atom skin case (UF3_NO_PART_SUMS: 8192 atoms,
UF3_NO_HALO: centres) on a context of its own.

No digest is written unless the moved atom advanced ``redone``, the species change did, and the capacity was seen to grow.

--verdict: a case whose digests differ between the two parent runs (sums through LDS atomics need not reproduce) is held to
max |tree - parent A| <= 4 max |parent B - parent A| per array -- the same terms in another order, and the largest of a few
thousand rounding differences varies by a small factor between draws; every other case, and every report line, statistic and
capacity, must be equal.  Both figures and the names of those cases go into OUT.json, with the tree's record of every case in
which it differs from parent A's (none, where the builds agree): OUT.json beside PARENT_A.json is the whole comparison."""
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

SKIN = 0.5
SWITCHES = ("UF3_EVAL_GATHER", "UF3_SEPARATE_N3", "UF3_NO_MD", "UF3_EVAL_NO_TAB", "UF3_EVAL_NO_CW", "UF3_EVAL_NO_CAP16",
            "UF3_NO_HALO", "UF3_NO_PART_SUMS", "UF3_NO_TAIL_SPIN", "UF3_NO_ZERO_COPY", "UF3_NO_BAR_STAGE", "UF3_BAR_FORCE_FAIL")


def main(out_path, arrays_path=None):
    os.environ["UF3_DEBUG_LDS"] = "1"
    log = tempfile.TemporaryFile(mode="w+b")
    sys.stderr.flush()
    keep_err = os.dup(2)
    os.dup2(log.fileno(), 2)
    try:
        result, raw = run_cases(log)
    finally:
        sys.stderr.flush()
        os.dup2(keep_err, 2)
        os.close(keep_err)
        log.seek(0)
        rest = [ln for ln in log.read().decode(errors="replace").splitlines() if not ln.startswith("uf3: ")]
        if rest:
            sys.stderr.write("\n".join(rest[-40:]) + "\n")
    import numpy as np
    print(json.dumps(result["observed"]))
    ob = result["observed"]
    wrong = [f"{k}: redone did not advance" for k in ("moved_atom_host", "moved_atom_dev", "species_change") if ob[k]["redone"] < 1]
    wrong += [f"{k}: capacity {ob[k]['cap_before']} -> {ob[k]['cap_after']}" for k in ("regrow_host", "regrow_dev")
              if not ob[k]["cap_after"] > ob[k]["cap_before"]]
    if wrong:
        sys.exit("the inputs miss their paths: " + "; ".join(wrong) + " -- no digests written")
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    if arrays_path:
        np.savez(arrays_path, **raw)


def run_cases(log):
    import numpy as np
    import torch                                    # (before the library: one HIP runtime)
    from uf3_amd import _lib, synthetic
    from uf3_amd.data.atoms import Atoms
    from uf3_amd.forcefield import calculator
    from uf3_amd.regression import least_squares as ls

    dev = torch.device("cuda", 0)
    cases, raw, observed = {}, {}, {}
    seen = [0]

    def reports():
        """the k_eval report lines written since the last look"""
        sys.stderr.flush()
        log.seek(seen[0])
        data = log.read()
        seen[0] += len(data)
        return [ln for ln in data.decode(errors="replace").splitlines() if ln.startswith("uf3: k_eval")]

    def model_of(elements, seed):
        basis = synthetic.notebook_basis(elements)
        model = ls.WeightedLinearModel(basis)
        coeff = np.random.default_rng(seed).normal(0, 0.05, basis.n_feats)
        coeff[basis.col_idx] = 0.0
        model.coefficients = coeff
        return model

    def ctx():
        return _lib.get_context(None)

    def capacity(calc, natoms):
        cap = C.c_int64(0)
        db = _lib.device_basis(calc.bspline_config, ctx())
        rc = ctx().lib.uf3_n3_lists_debug(db.handle, int(natoms), C.byref(cap), None, None, 0)
        return int(cap.value) if rc == 0 else -1           # (-1: the last call built no 3-body lists of this batch)

    def put(case, natoms, calc, **arrays):
        rec = cases.setdefault(case, dict(digests={}))
        for name, a in arrays.items():
            if a is None:
                continue
            a = np.ascontiguousarray(a)
            raw[f"{case}/{name}"] = a
            rec["digests"][name] = f"{a.dtype}{list(a.shape)}:" + hashlib.sha256(a.tobytes()).hexdigest()
        rec["reports"] = rec.get("reports", []) + reports()
        rec["md_stats"] = ctx().md_stats()
        rec["n3_cap"] = capacity(calc, natoms)

    def host(case, calc, frames, skin, forces=True, virial=False):
        calc.md_skin, calc.md_auto = skin, False
        out = calc.evaluate_frames(frames, forces=forces, virial=virial)
        put(case, sum(len(a) for a in frames), calc, energies=out[0], forces=out[1], virials=out[3] if virial else None)

    class Dev:
        """positions, species and outputs of one batch in device memory, for the *_dev entries"""
        def __init__(self, calc, frames):
            self.calc, self.batch = calc, _lib.FrameBatch(frames)
            b = self.batch
            self.pos, self.z = torch.from_numpy(b.pos).to(dev), torch.from_numpy(b.z).to(dev)
            self.e = torch.zeros(b.n_frames, dtype=torch.float64, device=dev)
            self.f = torch.zeros((b.n_atoms, 3), dtype=torch.float64, device=dev)
            self.v = torch.zeros((b.n_frames, 6), dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)

        def call(self, case, skin, entry="uf3_eval_dev", block=None):
            c, b = ctx(), self.batch
            c.md_skin(skin)
            db = _lib.device_basis(self.calc.bspline_config, c)
            p = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
            head = (db.handle, C.byref(b.struct), p(self.pos), p(self.z), *self.calc._pc)
            if entry == "uf3_eval_dev":
                c.check(c.lib.uf3_eval_dev(*head, p(self.e), p(self.f)))
            elif entry == "uf3_eval_virial_dev":
                c.check(c.lib.uf3_eval_virial_dev(*head, p(self.e), p(self.f), p(self.v)))
            else:
                c.check(getattr(c.lib, entry)(*head, int(block[0]), int(block[1]), p(self.e), p(self.f), p(self.v)))
            c.synchronize()
            virial = entry != "uf3_eval_dev"
            put(case, b.n_atoms, self.calc, energies=self.e.cpu().numpy(), forces=self.f.cpu().numpy(),
                virials=self.v.cpu().numpy() if virial else None)

        def move(self, delta):
            self.pos.add_(torch.from_numpy(np.ascontiguousarray(delta)).to(dev))
            torch.cuda.synchronize(dev)

    def moved(a, delta):
        b = a.copy()
        b.positions = b.positions + delta
        return b

    def walk(n, step):
        return np.random.default_rng(1000 + step).uniform(-0.01, 0.01, (n, 3))

    def kick(n):
        d = np.zeros((n, 3))
        d[n // 3] = [0.3, 0.0, 0.0]                         # > skin / 2: the step on the old lists is void
        return d

    def fresh_context(*calcs):
        for calc in calcs:
            _lib.drop_device_basis(calc.bspline_config)
        _lib._contexts.clear()
        import gc
        gc.collect()

    w = calculator.UFCalculator(model_of(['W'], 9), md_skin=0.0)
    shapes = {128: (4, 4, 4), 2000: (10, 10, 10), 2662: (11, 11, 11), 6750: (15, 15, 15), 8192: (16, 16, 16), 24334: (23, 23, 23)}
    frames = {n: synthetic.lattice_frame("bcc", reps, 3.165, [74], seed=300 + k) for k, (n, reps) in enumerate(shapes.items())}
    assert [len(frames[n]) for n in shapes] == list(shapes)

    # ---- host entries, every size: rebuild route, then the lists ----------------------------------------------------------
    for n, a in frames.items():
        host(f"w{n}/skin0/energies", w, [a], 0.0, forces=False)
        host(f"w{n}/skin0/forces", w, [a], 0.0)
        host(f"w{n}/skin0/virial", w, [a], 0.0, virial=True)
        host(f"w{n}/skin/forces_first", w, [a], SKIN)
        host(f"w{n}/skin/forces", w, [a], SKIN)
        host(f"w{n}/skin/virial", w, [a], SKIN, virial=True)
        host(f"w{n}/skin/energies", w, [a], SKIN, forces=False)
    # ---- a walk on the lists, then an atom past skin / 2; a cell change -----------------------------------------------------
    for n in (128, 2000):
        a = frames[n]
        for step in range(12):
            a = moved(a, walk(n, step))
            host(f"w{n}/walk/step{step:02d}", w, [a], SKIN, virial=(step % 4 == 3))
        before = ctx().md_stats()["redone"]
        host(f"w{n}/walk/moved_atom", w, [moved(a, kick(n))], SKIN)
        if n == 128:
            observed["moved_atom_host"] = dict(redone=ctx().md_stats()["redone"] - before)
        b = moved(a, kick(n))
        b = Atoms(numbers=b.get_atomic_numbers(), positions=1.002 * b.get_positions(), cell=1.002 * np.asarray(b.get_cell()), pbc=True)
        host(f"w{n}/walk/cell_change", w, [b], SKIN)
    # ---- blocks of atoms and of centres, host and device entries ------------------------------------------------------------
    a = frames[128]
    d128 = Dev(w, [a])
    for skin, tag in ((0.0, "skin0"), (SKIN, "skin")):
        for lo, hi in ((0, 50), (50, 128)):
            ctx().md_skin(skin)
            e, f, v = w.evaluate_atom_range(a, lo, hi, virial=True)
            put(f"w128/{tag}/atoms_{lo}_{hi}", 128, w, energies=np.array([e]), forces=f, virials=v)
            w.md_skin, w.md_auto = skin, False
            e, f, v = w.evaluate_centre_range(a, lo, hi, virial=True)
            put(f"w128/{tag}/centres_{lo}_{hi}", 128, w, energies=np.array([e]), forces=f, virials=v)
            d128.call(f"w128/{tag}/atoms_dev_{lo}_{hi}", skin, "uf3_eval_atoms_dev", (lo, hi))
            d128.call(f"w128/{tag}/centres_dev_{lo}_{hi}", skin, "uf3_eval_centres_dev", (lo, hi))
    # ---- device entries: 128 and 8192 atoms ---------------------------------------------------------------------------------
    for n in (128, 8192):
        d = d128 if n == 128 else Dev(w, [frames[n]])
        d.call(f"w{n}/dev/skin0/forces", 0.0)
        d.call(f"w{n}/dev/skin0/virial", 0.0, "uf3_eval_virial_dev")
        d.call(f"w{n}/dev/skin/forces_first", SKIN)
        for step in range(12):
            d.move(walk(n, 100 + step))
            d.call(f"w{n}/dev/walk/step{step:02d}", SKIN, "uf3_eval_virial_dev" if step % 4 == 3 else "uf3_eval_dev")
        before = ctx().md_stats()["redone"]
        d.move(kick(n))
        d.call(f"w{n}/dev/walk/moved_atom", SKIN)
        if n == 128:
            observed["moved_atom_dev"] = dict(redone=ctx().md_stats()["redone"] - before)
    # ---- two species: a species change on the lists, a dense batch, the capacity regrown ------------------------------------
    mw = calculator.UFCalculator(model_of(['Mo', 'W'], 11), md_skin=0.0)
    a = synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, [42, 74], seed=77)
    for step in range(3):
        a = moved(a, walk(128, 200 + step))
        host(f"mow128/skin/step{step}", mw, [a], SKIN)
    z = a.get_atomic_numbers().copy()
    z[5] = 42 if z[5] == 74 else 74
    b = Atoms(numbers=z, positions=a.get_positions(), cell=a.get_cell(), pbc=True)
    before = ctx().md_stats()["redone"]
    host("mow128/skin/species_change", mw, [b], SKIN, virial=True)
    observed["species_change"] = dict(redone=ctx().md_stats()["redone"] - before)
    a0 = 3.165
    three = Atoms(numbers=[42, 74, 74], positions=np.array([[0.05, 0.0, 0.02], [0.5 * a0, 0.52 * a0, 0.49 * a0], [0.02, -0.03, 0.98 * a0]]),
                  cell=np.diag([a0, a0, 1.5 * a0]), pbc=True)
    # (on a context of its own: the capacity only grows, and the frames above have raised it.  bcc neighbours inside the 3-body
    # range of 3.5 A: 8 at a = 3.6, 26 at 2.45 -- the shell at a sqrt 2 --, 50 at 2.05)
    fresh_context(w, mw)
    sparse = synthetic.lattice_frame("bcc", (3, 3, 4), 3.6, [42, 74], seed=3600)
    host("regrow/sparse_first", mw, [sparse], 0.0, virial=True)            # (tunes the capacity to the lists it saw)
    host("regrow/sparse", mw, [sparse], 0.0, virial=True)
    cap0 = capacity(mw, len(sparse))
    dense = synthetic.lattice_frame("bcc", (4, 4, 5), 2.45, [42, 74], seed=2450)
    host("regrow/host_denser", mw, [dense], 0.0, virial=True)              # (eval_host's loop: the words travel with the results)
    cap1 = capacity(mw, len(dense))
    observed["regrow_host"] = dict(cap_before=cap0, cap_after=cap1)
    batch = [dense, synthetic.lattice_frame("bcc", (3, 3, 4), 2.45, [42, 74], seed=2451), three]
    host("batch3/skin0/virial", mw, batch, 0.0, virial=True)
    host("batch3/skin/virial_first", mw, batch, SKIN, virial=True)
    host("batch3/skin/virial", mw, batch, SKIN, virial=True)
    denser = synthetic.lattice_frame("bcc", (4, 4, 5), 2.05, [42, 74], seed=2050)
    Dev(mw, [denser]).call("regrow/dev_densest", 0.0, "uf3_eval_virial_dev")  # (eval_impl's loop: the pinned status block)
    cap2 = capacity(mw, len(denser))
    observed["regrow_dev"] = dict(cap_before=cap1, cap_after=cap2)
    host("regrow/host_densest_skin", mw, [denser], SKIN, virial=True)
    observed["longest_capacity"] = cap2
    observed["tab_layout_beyond_36_entries"] = ("reached" if cap1 > 36 else
                                                "not reached by these models: tests/test_eval_plan_host.py covers that layout's bytes")
    # ---- the switches, each on a context of its own -------------------------------------------------------------------------
    for sw in SWITCHES:
        fresh_context(w, mw)
        os.environ[sw] = "1"
        try:
            n = 8192 if sw == "UF3_NO_PART_SUMS" else 128
            a = frames[n]
            for step in range(4):
                a = moved(a, walk(n, 300 + step))
                if sw == "UF3_NO_HALO":
                    for skin, tag in ((0.0, "skin0"), (SKIN, "skin")):
                        w.md_skin, w.md_auto = skin, False
                        e, f, v = w.evaluate_centre_range(a, 50, 128, virial=True)
                        put(f"switch/{sw}/{tag}/centres_step{step}", n, w, energies=np.array([e]), forces=f, virials=v)
                else:
                    host(f"switch/{sw}/step{step}", w, [a], SKIN, virial=(step == 3))
            if n == 8192:
                d = Dev(w, [a])
                d.call(f"switch/{sw}/dev", SKIN)
                d.call(f"switch/{sw}/dev_virial", SKIN, "uf3_eval_virial_dev")
        finally:
            del os.environ[sw]
    fresh_context(w, mw)
    return dict(build_id=_lib.build_id(), observed=observed, cases=cases), raw


def verdict(parent_a, parent_b, tree, out_path):
    import numpy as np
    J = {k: json.load(open(k + ".json")) for k in (parent_a, parent_b, tree)}
    Z = {k: np.load(k + ".npz") for k in (parent_a, parent_b, tree)}
    A, B, T = J[parent_a]["cases"], J[parent_b]["cases"], J[tree]["cases"]
    bad, loose = [], {}
    if set(A) != set(T) or set(A) != set(B):
        bad.append("the runs hold different cases")
    if J[parent_a]["observed"] != J[tree]["observed"]:
        bad.append("observed: " + json.dumps([J[parent_a]["observed"], J[tree]["observed"]]))
    for case in sorted(set(A) & set(B) & set(T)):
        for key in ("reports", "md_stats", "n3_cap"):
            if not A[case][key] == B[case][key] == T[case][key]:
                bad.append(f"{case}: {key} differ")
        if A[case]["digests"] == B[case]["digests"]:
            if T[case]["digests"] != A[case]["digests"]:
                bad.append(f"{case}: digests differ from the parent's, which reproduce")
            continue
        loose[case] = {}
        for name in A[case]["digests"]:
            k = f"{case}/{name}"
            pp = float(np.abs(Z[parent_b][k] - Z[parent_a][k]).max())
            tp = float(np.abs(Z[tree][k] - Z[parent_a][k]).max())
            loose[case][name] = dict(parent_against_parent=pp, tree_against_parent=tp)
            if tp > 4 * pp:
                bad.append(f"{case}/{name}: tree against parent {tp:.3e} > 4 x parent against parent {pp:.3e}")
    # (the tree's record, against the parent's file: only what differs from it is written out)
    differing = {case: T[case] for case in sorted(T) if T[case] != A.get(case)}
    out = dict(parent_build_id=J[parent_a]["build_id"], tree_build_id=J[tree]["build_id"], cases=len(A),
               parent_runs_equal=A == B,
               cases_not_reproduced_by_the_parent=loose, tree_observed=J[tree]["observed"],
               tree_cases_differing_from_the_parent=differing, failures=bad)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(A)} cases, {len(loose)} not reproduced by the parent itself, {len(bad)} failures" + "".join(f"\n  {b}" for b in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        from fire_family_bits import compare
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 6 and sys.argv[1] == "--verdict":
        sys.exit(verdict(*sys.argv[2:6]))
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) == 3 else None)
