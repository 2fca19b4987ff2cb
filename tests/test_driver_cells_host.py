"""What the references of tests/_driver_cells.py prove on their own (no GPU): the NumPy restatements of the MD, NPT, relaxation
and NEB drivers, driven by the oracle alone, on skewed, turned, reflected, permuted and shifted descriptions of one crystal.

(a) the references are covariant: original against description, mapped back, over the GPU tests' step counts.  The spread is
    the dynamics' amplification of rounding; ten times it (and not less than the parity bound) is the covariance tolerance of
    tests/test_gpu_driver_cells.py.  Measured: positions 1.0e-13 A, velocities 5e-16 A/fs, forces 4.1e-13 eV/A, energies 7.5e-13 eV,
    strain derivatives 1.1e-12 eV, D 9e-16, NEB forces 7.0e-11 eV/A (climbing, fixed atoms).  Asserted: 1e-10 (SPREAD): ten times it
    is the parity bound.
(b) discrete decisions are made with room: FIRE's normalised power stays 0.068 away from 0 (asserted: 1e-3), the NEB tangent's energy comparisons
    1e-6 eV apart, the NPT crossing frames cross (and the reference ends on the far side).
(c) every atom stays inside the window of fractional width fac + 1 - r_cut / h around its current cell
    throughout every reference run.
(d) the frames have teeth: restatements that are wrong on purpose (x = q D^T, G = -D^-1 W / n, cell = D cell0, g = F D, Voigt yz
    and xy exchanged) leave the right one by at least 1e-6 A on the sheared start (4.5e-6 A for g = F D, 8e-5 for G, 1e-2 for
    x, A for the other two; on skew_751_reflection under the seeded model D moves by 1.9e-3 only and G and g would move the
    run by 7e-9 and 1.5e-8 A: that frame is not used here), and the D / D^T family stays within 1e-9 on test_gpu_relax.py's cubic start.
    The sixth, an NPT list rule that takes edge lengths for heights, shows in the rebuild decision and not in the trajectory
    (while every atom is inside the window of (c), no pair needs the image a kept range lacks: forces from the build's
    images alone moved no position on the U_110 frame): a restatement of the list rule, replayed on the reference
    trajectories, goes void once on the crossing step with heights and never with edge lengths, on all three frames.
    tests/test_gpu_driver_cells.py holds the device's build and redo counts to it.

Seeds and step counts: the frames of tests/_util.py: equivalence_cases (seeds 81 to 86), velocities from Philox seed 4 at
300 K, Langevin seed 9, 30 steps of MD, NPT, FIRE and NEB, 40 on the crossing frames."""
import numpy as np
import pytest

from uf3_amd.data.atoms import Atoms
import _driver_cells as DC
import _relax_ref as R
from test_relax_host import pair_energy

O = DC.ORIGINAL
SPREAD = 1e-10
SEPARATES = 1e-6
NEB_MARGIN = 1e-6               # eV: tests/test_gpu_neb.py's MARGIN
POWER_MARGIN = 1e-3           # of |g| |v|: ten orders above the rounding of the sums

BULK = [("bcc_mow", l) for l in ("skew_821", "skew_351", "perm_rotation_shift", "skew_751_reflection")]
_ids = lambda pairs: [f"{c}-{l}" for c, l in pairs]                       # noqa: E731


def _origin(label):
    return "sheared" if label == "sheared_turned" else O


def _report(what, figures):
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()))


# ================================================================================================ (a) covariance, (c) the window
def _admissible(pairs, plain, noisy):
    """(case, label, langevin) of every run that is covariant: the Langevin ones only where the description keeps atom order
    and axes (Pair.admissible)."""
    return [(c, l, lang) for c, l in pairs for lang in (False, True) if DC.get_pair(c, l).admissible(noisy if lang else plain)]


def _ids3(params, names):
    return [f"{c}-{l}-{names[lang]}" for c, l, lang in params]


MD_RUNS = _admissible(DC.MD_DESCRIPTIONS, "nve", "langevin")


@pytest.mark.parametrize("case,label,langevin", MD_RUNS, ids=_ids3(MD_RUNS, ["nve", "langevin"]))
def test_md_reference_is_covariant(case, label, langevin):
    P = DC.get_pair(case, label)
    a, b = DC.md_reference(((case, O),), langevin), DC.md_reference(((case, label),), langevin)
    assert np.abs(P.residual(b["x0"], a["x0"])).max() <= 1e-12               # (the mapping, the shift included, at step 0)
    fig = dict(x=np.abs(P.residual(b["x"], a["x"])).max(), v=np.abs(b["v"] - P.vectors(a["v"])).max(),
               f=np.abs(b["f"] - P.vectors(a["f"])).max(), e=abs(b["e"][0] - P.energy(a["e"][0])),
               w=np.abs(b["w"][0] - P.strain(a["w"][0])).max(), room=min(a["room"], b["room"]),
               moved=np.abs(a["x"] - a["x0"]).max())
    _report(f"md {case} {label} langevin={langevin}", fig)
    assert max(fig[k] for k in "xvfew") <= SPREAD, fig
    assert fig["room"] > 0 and fig["moved"] > 1e-3, fig


NPT_DESCRIPTIONS = BULK + [("ternary", "skew_751")]
NPT_RUNS = _admissible(NPT_DESCRIPTIONS, "nph", "npt")


def test_which_runs_are_compared():
    """Langevin runs only on pure U descriptions; every description under NVE and NPH."""
    assert [(c, l) for c, l, lang in MD_RUNS if lang] == [("bcc_mow", "skew_821"), ("bcc_mow", "skew_351"), ("ternary", "skew_751"),
                                                          ("slab_mow", "skew_in_plane_531")]
    assert [(c, l) for c, l, lang in NPT_RUNS if lang] == [("bcc_mow", "skew_821"), ("bcc_mow", "skew_351"), ("ternary", "skew_751")]
    assert [(c, l) for c, l, lang in MD_RUNS if not lang] == DC.MD_DESCRIPTIONS
    assert [(c, l) for c, l, lang in NPT_RUNS if not lang] == NPT_DESCRIPTIONS


@pytest.mark.parametrize("case,label,langevin", NPT_RUNS, ids=_ids3(NPT_RUNS, ["nph", "npt"]))
def test_npt_reference_is_covariant(case, label, langevin):
    P = DC.get_pair(case, label)
    a, b = DC.npt_reference(((case, O),), langevin), DC.npt_reference(((case, label),), langevin)
    fig = dict(x=np.abs(P.residual(b["x"], a["x"], P.cell0 * a["s"][0])).max(), v=np.abs(b["v"] - P.vectors(a["v"])).max(),
               f=np.abs(b["f"] - P.vectors(a["f"])).max(), e=abs(b["e"][0] - a["e"][0]), s=abs(b["s"][0] - a["s"][0]),
               veps=abs(b["veps"][0] - a["veps"][0]), room=min(a["room"], b["room"]), scale=np.abs(a["s_hist"] - 1.0).max())
    _report(f"npt {case} {label} langevin={langevin}", fig)
    assert max(fig[k] for k in ("x", "v", "f", "e", "s", "veps")) <= SPREAD, fig
    assert fig["room"] > 0 and fig["scale"] > 1e-4, fig


FIRE_DESCRIPTIONS = BULK + [(DC.W_UNARY, "sheared_turned"), ("ternary", "skew_751"), ("slab_mow", "skew_in_plane_531"),
                            ("wire_mow", "perm_rotation_shift")]


@pytest.mark.parametrize("relax_cell", [False, True], ids=["positions", "cell"])
@pytest.mark.parametrize("case,label", FIRE_DESCRIPTIONS, ids=_ids(FIRE_DESCRIPTIONS))
def test_fire_reference_is_covariant_and_decides_with_room(case, label, relax_cell):
    P = DC.get_pair(case, label)
    assert P.admissible("fire")
    a, b = DC.fire_reference(((case, _origin(label)),), relax_cell), DC.fire_reference(((case, label),), relax_cell)
    assert a["status"].tolist() == [R.RUNNING] and b["status"].tolist() == [R.RUNNING] and a["steps"].tolist() == [DC.N_STEPS]
    fig = dict(x=np.abs(P.residual(b["x"], a["x"], a["cells"][0])).max(), D=np.abs(b["D"][0] - P.deformation(a["D"][0])).max(),
               cell=np.abs(b["cells"][0] - np.asarray(P.d.atoms.get_cell(), float) @ b["D"][0]).max(),
               f=np.abs(b["f"] - P.vectors(a["f"])).max(), e=abs(b["e"][0] - a["e"][0]),
               power=min(np.abs(a["power"]).min(), np.abs(b["power"]).min()), room=min(a["room"], b["room"]),
               D_off_identity=np.abs(a["D"][0] - np.eye(3)).max(), D_asymmetry=np.abs(b["D"][0] - b["D"][0].T).max())
    _report(f"fire {case} {label} relax_cell={relax_cell}", fig)
    assert max(fig[k] for k in ("x", "D", "cell", "f", "e")) <= SPREAD, fig
    assert fig["power"] >= POWER_MARGIN and len(a["power"]) == DC.N_STEPS - 1, fig
    assert fig["room"] > 0, fig
    periodic = bool(np.all(P.pbc))
    assert (fig["D_off_identity"] > 1e-3) == (relax_cell and periodic), fig          # (slab and wire keep their cells)


@pytest.mark.parametrize("fixed", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("climb", [False, True], ids=["plain", "climb"])
def test_neb_reference_is_covariant_and_decides_with_room(climb, fixed):
    P, band = DC.neb_band("skew_351_turned")
    a, b = DC.neb_reference(O, climb, fixed), DC.neb_reference("skew_351_turned", climb, fixed)
    n = len(P.base)
    img = lambda x, k: x[k * n:(k + 1) * n]                                             # noqa: E731
    fig = dict(x=max(np.abs(P.residual(img(b["x"], k), img(a["x"], k))).max() for k in range(len(band))),
               g=max(np.abs(img(b["g"], k) - P.vectors(img(a["g"], k))).max() for k in range(len(band))),
               e=np.abs(a["e"] - b["e"]).max(), crit=abs(a["crit"][0] - b["crit"][0]),
               margin=min(a["margins"].min(), b["margins"].min()), power=min(np.abs(a["power"]).min(), np.abs(b["power"]).min()),
               room=min(a["room"], b["room"]))
    _report(f"neb climb={climb} fixed={fixed} (climbing image {a['climbing'].tolist()})", fig)
    assert a["climbing"].tolist() == b["climbing"].tolist() == ([4] if climb else [-1])
    assert a["status"].tolist() == b["status"].tolist() == [R.RUNNING]
    assert max(fig[k] for k in ("x", "g", "e", "crit")) <= SPREAD, fig
    assert fig["margin"] >= NEB_MARGIN and fig["power"] >= POWER_MARGIN and fig["room"] > 0, fig
    if fixed:
        mask = DC.neb_fixed("skew_351_turned")
        x0 = np.concatenate([im.get_positions() for im in band])
        assert np.array_equal(b["x"][mask], x0[mask]) and mask.sum() == 3 * len(band)


@pytest.mark.parametrize("cases", [tuple(DC.MIXED), tuple(DC.MIXED_FIRE)], ids=["md_batch", "fire_batch"])
def test_mixed_batches_stay_in_their_windows(cases):
    """The batches that hold a skewed bulk, a slab and a wire frame: the runs the GPU tests compare alone against in a batch."""
    if cases == tuple(DC.MIXED):
        rooms = [DC.md_reference(cases, lang)["room"] for lang in (False, True)]
    else:
        rooms = [DC.fire_reference(cases, rc)["room"] for rc in (False, True)]
    print("room", rooms)
    assert min(rooms) > 0


# ======================================================================================================== (b) the crossings
@pytest.mark.parametrize("name", list(DC.CROSSINGS))
def test_crossing_frames_cross(name):
    """r_cut / (s(t) h_0) passes an integer inside the run at the crossing pressure and the reference ends beyond it with room;
    at the other pressure it stays on its side for the whole run."""
    cross, stay = DC.crossing_reference(name, True), DC.crossing_reference(name, False)
    r0 = cross["ratio0"]
    hist = r0[None, :] / cross["s_hist"]                       # [evaluations, 3]
    hist_stay = r0[None, :] / stay["s_hist"]
    fac0 = np.ceil(r0)
    print(f"{name}: r_cut / h at the start {r0}, at the end {hist[-1]} (crossing pressure), {hist_stay[-1]} (the other); "
          f"s {cross['s'][0]:.6f} / {stay['s'][0]:.6f}; room {cross['room']:.3f} / {stay['room']:.3f} A")
    assert np.array_equal(np.ceil(hist_stay), np.broadcast_to(fac0, hist_stay.shape))
    changed = np.ceil(hist) != fac0
    assert changed[-1, 0] and not changed[:, 1:].any()
    first = int(np.argmax(changed[:, 0]))
    assert 5 <= first <= DC.CROSS_STEPS - 5 and changed[first:, 0].all()              # inside the run, and it stays across
    assert abs(hist[-1, 0] - np.rint(hist[-1, 0])) > 0.02                             # far side, with room
    assert min(cross["room"], stay["room"]) > 0


def test_where_the_oracle_forces_are_no_gradient_the_reference_takes_the_cubic_cell():
    """In the thin cells of two crossing frames the oracle's forces lose ghost-centred terms (its energy does not): they
    differ from those of the cubic description of the same crystal, which are minus the energy's gradient.  The reference
    runs therefore show the oracle the cubic cell (OracleFrames: recell); on every 16-atom frame the oracle's forces are
    covariant as they are (the tests above)."""
    from oracle import oracle as OR
    ob, c = DC._oracle_model("bcc_mow")
    lost = {}
    for name in DC.CROSSINGS:
        P = DC.crossing(name)
        e0, f0 = OR.evaluate(ob, P.base, c)
        e1, f1 = OR.evaluate(ob, P.atoms, c)
        ora = DC.OracleFrames("bcc_mow", [P.atoms], [DC.crossing_recell(name)])
        e2, f2, _ = ora(P.atoms.get_positions())
        lost[name] = np.abs(f1 - f0).max()
        print(f"{name}: oracle forces in the skewed cell against the cubic one {lost[name]:.2e} eV/A, energies {abs(e1 - e0):.1e} eV; "
              f"through recell {np.abs(f2 - f0).max():.1e}")
        assert abs(e1 - e0) <= 1e-11 and abs(e2[0] - e0) <= 1e-11 and np.abs(f2 - f0).max() <= 1e-11
        i = int(np.argmax(np.abs(f1 - f0).max(1)))
        x, h, fd = P.base.get_positions(), 1e-5, np.zeros(3)
        for a in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, a] += h
            xm[i, a] -= h
            ep, em = (OR.evaluate(ob, Atoms(numbers=P.base.get_atomic_numbers(), positions=y, cell=P.base.get_cell(), pbc=True), c,
                                  forces=False)[0] for y in (xp, xm))
            fd[a] = -(ep - em) / (2 * h)
        assert np.abs(fd - f0[i]).max() <= 1e-7, (name, fd, f0[i])          # the cubic cell's forces are the gradient
    assert lost["skew_821_5to6"] > 1e-3 and lost["skew_751_5to4"] > 1e-3 and lost["u110_1to2"] <= 1e-11, lost


@pytest.mark.parametrize("name", list(DC.CROSSINGS))
def test_the_list_rule_rebuilds_at_the_crossing_and_edge_lengths_do_not(name):
    """The restatement of k_npt_frame's list rule (_driver_cells.list_rule), replayed on the reference trajectories at the
    GPU test's skin.  With perpendicular heights the lists go void exactly once, on the step on which ceil(r_cut / (s h_0))
    changes, and not because an atom outran the skin (no early warning was pending: the rebuild is the image rule's own); at
    the other pressure they never do.  The sixth mutation -- edge lengths for heights -- never goes void, and neither does
    the rule with its image test taken out: both differ from the right rule in the (builds, redone) the GPU test asserts."""
    for cross in (True, False):
        ref = DC.crossing_reference(name, cross)
        right, edges, none = ref["lists"], ref["lists_edge_lengths"], ref["lists_no_image_rule"]
        print(f"{name} cross={cross}: heights {right}; edge lengths builds {edges['builds']} redone {edges['redone']}; "
              f"no image rule builds {none['builds']} redone {none['redone']}")
        assert edges["redone"] == 0 and none["redone"] == 0
        if not cross:
            assert right["redone"] == 0 and right == edges == none
            continue
        ratio = ref["ratio0"][0] / ref["s_hist"][:, 0]
        first = int(np.argmax(np.ceil(ratio) != np.ceil(ratio[0])))
        assert right["void_steps"] == [first] and right["redone"] == 1, (right, first)
        assert (right["builds"], right["redone"]) != (edges["builds"], edges["redone"])
        assert (right["builds"], right["redone"]) != (none["builds"], none["redone"])
        P = DC.crossing(name)
        assert np.abs(DC.edge_lengths(P.atoms.get_cell()) / DC.heights(P.atoms.get_cell()) - 1.0)[0] > 0.5     # (a skewed cell)


def test_the_exchange_band_is_the_sibling_tests_construction():
    """_driver_cells._exchange at turn = 1 is tests/test_gpu_neb.py's _exchange, bit for bit."""
    import test_gpu_neb as TN
    base = DC.RH.CASES["bcc_mow"][0]
    ours, theirs = DC._exchange(base, DC.NEB_IMAGES, DC.NEB_SEED, turn=1.0), TN._exchange(base, DC.NEB_IMAGES, DC.NEB_SEED)
    assert all(np.array_equal(a.get_positions(), b.get_positions()) for a, b in zip(ours, theirs)) and len(ours) == len(theirs)


# ======================================================================================================== (d) the mutations
class WrongFire(R.Fire):
    """_relax_ref.Fire with one formula swapped (``wrong``): never part of the product."""
    wrong = ""

    def _frame(self, f, e, F, W, fmax, dt0, dt_max, maxstep, can_move):
        lo, hi = self.off[f], self.off[f + 1]
        n = hi - lo
        Ff = F[lo:hi]
        G = np.zeros((3, 3))
        D = self.D[f]
        if self.cellf[f]:
            w = W[f]
            Wm = R.voigt_to_matrix(w[[0, 1, 2, 5, 4, 3]] if self.wrong == "voigt" else w)
            G = -(np.linalg.inv(D) @ Wm) / n if self.wrong == "G" else R.cell_force(D, Wm, n)
        self.e_last[f] = e
        if not can_move:
            return
        g = (Ff @ D if self.wrong == "g" else Ff @ D.T) if self.cellf[f] else Ff.copy()
        v, vc = self.v[lo:hi], self.vc[f]
        dt = dt0 if self.first[f] else self.dt[f]
        if not self.first[f]:
            if np.vdot(g, v) + np.vdot(G, vc) > 0:
                vn = np.sqrt(np.vdot(v, v) + np.vdot(vc, vc))
                gn = np.sqrt(np.vdot(g, g) + np.vdot(G, G))
                c = self.alpha[f] * vn / gn
                v, vc = (1 - self.alpha[f]) * v + c * g, (1 - self.alpha[f]) * vc + c * G
                if self.n_pos[f] > R.N_MIN:
                    dt = min(dt * R.F_INC, dt_max)
                    self.alpha[f] *= R.F_A
                self.n_pos[f] += 1
            else:
                v, vc = 0.0 * v, 0.0 * vc
                self.alpha[f], dt, self.n_pos[f] = R.A_START, dt * R.F_DEC, 0
        v, vc = v + dt * g, vc + dt * G
        dr, drc = dt * v, dt * vc
        norm = np.sqrt(np.vdot(dr, dr) + np.vdot(drc, drc))
        if norm > maxstep:
            dr, drc = dr * (maxstep / norm), drc * (maxstep / norm)
        self.v[lo:hi], self.vc[f] = v, vc
        if self.cellf[f]:
            self.q[lo:hi] += dr
            self.D[f] = D = D + drc / n
            self.cells[f] = D @ self.cell0[f] if self.wrong == "cell" else self.cell0[f] @ D
            self.x[lo:hi] = self.q[lo:hi] @ (D.T if self.wrong == "x" else D)
        else:
            self.x[lo:hi] += dr
        self.dt[f], self.first[f] = dt, False
        self.steps[f] += 1


def _wrong(kind):
    return type("Wrong_" + (kind or "none"), (WrongFire,), dict(wrong=kind))


MUTATIONS = {"x": "x = q D^T", "G": "G = -D^-1 W / n", "cell": "cell = D cell0", "g": "g = F D", "voigt": "Voigt yz and xy exchanged"}
CELL_STARTS = [(DC.W_UNARY, "sheared_turned")]


@pytest.mark.parametrize("case,label", CELL_STARTS, ids=_ids(CELL_STARTS))
def test_wrong_cell_algebra_separates_on_the_new_frames(case, label):
    right = DC.fire_reference(((case, label),), True)
    # the copy above with nothing swapped is the restatement
    same, _, _ = DC.fire(((case, label),), True, fire_class=_wrong(""))
    same.run(DC.N_STEPS, fmax=DC.NEVER, **DC.fire_kw(case))
    assert np.array_equal(same.x, right["x"]) and np.array_equal(same.cells, right["cells"])
    for kind in MUTATIONS:
        ref, _, _ = DC.fire(((case, label),), True, fire_class=_wrong(kind))
        ref.run(DC.N_STEPS, fmax=DC.NEVER, **DC.fire_kw(case))
        dx, dc = np.abs(ref.x - right["x"]).max(), np.abs(ref.cells - right["cells"]).max()
        print(f"{label}: {MUTATIONS[kind]}: positions {dx:.2e} A, cell {dc:.2e} A off the restatement after {DC.N_STEPS} steps")
        assert max(dx, dc) >= SEPARATES, (kind, dx, dc)


def test_the_cubic_start_cannot_see_the_transposes():
    """tests/test_gpu_relax.py's w_vacancy_cluster start (a cubic cell, D = 1 at the start) under the pair potential of
    tests/test_relax_host.py: the D / D^T family stays within 1e-9 A of the restatement over the first steps."""
    from test_gpu_relax import _vacancy
    a = _vacancy(3, reps=(3, 3, 3))                                  # (the 53-atom sibling of the batch's 127-atom frame: the
    cell0 = np.asarray(a.get_cell(), float)                          #  same cubic cell and start, a quarter of the pair sums)
    assert np.array_equal(cell0, np.diag(np.diag(cell0)))

    def evaluate(x, cells):
        e, F, W = pair_energy(x, cells[0], True)
        return np.array([e]), F, np.array([W])

    def run(kind, steps):
        ref = _wrong(kind)(evaluate, a.get_positions(), [cell0], [[True] * 3], np.array([0, len(a)]), relax_cell=True)
        ref.run(steps, fmax=DC.NEVER, dt=0.1, dt_max=1.0, maxstep=0.2)             # (test_gpu_relax.py's settings)
        return ref
    steps = 8
    right = run("", steps)
    assert np.abs(right.D[0] - np.eye(3)).max() > 1e-4
    for kind in ("x", "G", "cell", "g"):
        ref = run(kind, steps)
        dx, dc = np.abs(ref.x - right.x).max(), np.abs(ref.cells - right.cells).max()
        print(f"cubic start: {MUTATIONS[kind]}: positions {dx:.2e} A, cell {dc:.2e} A off the restatement after {steps} steps")
        assert max(dx, dc) <= 1e-9, (kind, dx, dc)
