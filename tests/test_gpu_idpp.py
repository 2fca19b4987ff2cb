"""IDPP band initialisation on the device (``uf3_idpp_create``, ``k_idpp``; ``neb.IDPP``, ``neb.idpp_interpolate``) against the
NumPy restatement in tests/_idpp_ref.py: one evaluation against the ``longdouble`` yardstick, step-by-step parity, what a user
gets on a band whose linear interpolation drives two atoms through each other, the band as a start for NEB, determinism and
batch independence, fixed atoms, a non-finite band, nearest images on the device and the library's refusals."""
import ctypes as C
import functools
import os
import warnings

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator, neb
from uf3_amd.forcefield.neb import IDPP
from uf3_amd.regression import least_squares as ls
import _idpp_ref as I
from _relax_ref import RUNNING, CONVERGED, NONFINITE
from _util import GOLDEN, rotation

pytestmark = pytest.mark.gpu
TOL = 1e-9              # tests/test_gpu_neb.py's
MARGIN = 1e-6           # 1 / A^2: every ordering of S the restatement branched on must be at least this clear
NEVER = 1e-12
STATUS = {RUNNING: "running", CONVERGED: "converged", NONFINITE: "nonfinite"}
KW = dict(dt=0.1, dt_max=1.0, maxstep=0.2)
TURN = rotation([1, 2, 3], 0.7)


def _frame_rel(a, ref, off=None):
    """The largest deviation of ``a`` from ``ref``, per frame relative to the frame's largest |ref| (a frame whose reference is
    zero throughout must be met exactly)."""
    a, ref = np.asarray(a, np.longdouble), np.asarray(ref, np.longdouble)
    worst = 0.0
    for f in range(len(ref) if off is None else len(off) - 1):
        x, r = (a[f:f + 1], ref[f:f + 1]) if off is None else (a[off[f]:off[f + 1]], ref[off[f]:off[f + 1]])
        top = np.abs(r).max()
        if top == 0:
            assert np.all(x == 0), f
            continue
        worst = max(worst, float(np.abs(x - r).max() / top))
    return worst


@functools.lru_cache(None)
def _yardstick():
    """The batch, its float64 and longdouble restatements and e_ref (S, F): the float64 restatement's largest deviation from
    the longdouble one, per frame relative to the quantity's largest magnitude there."""
    bands = I.batch()
    _, off, first, _, _ = I.layout(bands)
    S, F = I.evaluate_bands(bands)
    SL, FL = I.evaluate_bands(bands, dtype=np.longdouble)
    return bands, off, first, SL, FL, (_frame_rel(S, SL), _frame_rel(F, FL, off))


def _device(bands, **kw):
    with IDPP(bands, **kw) as band:
        band.run(0)
        return np.concatenate(band.get_potential_energies()), band.get_forces()


def test_one_evaluation_against_the_restatement():
    """The device lies within 16 e_ref of the longdouble restatement, e_ref the float64 restatement's own deviation from it: two
    float64 evaluations of one formula differ by summation order and fused multiply-adds, not more.  Measured on an MI355X:
    e_ref 1.12e-15 (S) and 9.28e-15 (F), the device 7.2e-16 and 7.78e-15."""
    bands, off, first, SL, FL, e_ref = _yardstick()
    assert [(len(b), len(b[0])) for b in bands] == [(3, 2), (3, 1), (4, 257), (5, 53), (4, 54), (6, 16)]
    assert not any(bands[0][0].get_pbc()) and list(bands[4][0].get_pbc()) == [True, True, False]
    S, F = _device(bands)
    dev = (_frame_rel(S, SL), _frame_rel(F, FL, off))
    print(f"idpp one evaluation: e_ref S {e_ref[0]:.3g} F {e_ref[1]:.3g}; device S {dev[0]:.3g} F {dev[1]:.3g}")
    assert 0 < 16 * e_ref[0] <= 1e-10 and 0 < 16 * e_ref[1] <= 1e-10          # else the inputs are ill-conditioned
    assert dev[0] <= 16 * e_ref[0] and dev[1] <= 16 * e_ref[1]
    for k in range(len(bands)):
        assert S[first[k]] == 0.0 and S[first[k + 1] - 1] == 0.0
    assert np.all(S[first[1]:first[2]] == 0.0) and np.all(F[off[first[1]]:off[first[2]]] == 0.0)    # one atom: no pair
    assert np.all(np.asarray(SL, float)[[first[k] + 1 for k in (0, 2, 3, 4, 5)]] > 0)


@pytest.mark.parametrize("name", list(I.PARITY))
def test_parity_with_the_restatement(name):
    ref = I.parity_run(name)
    make, spring = I.PARITY[name]
    fmax = 1e-2
    worst = [0.0, 0.0, 0.0]
    with IDPP(make(), spring=spring) as band:
        for k, (x_ref, e_ref, crit_ref, status_ref) in enumerate(ref["first"]):
            out = band.run(1, fmax=fmax, **KW)
            x, e = band.get_positions(), np.concatenate(out["energies"])
            worst = [max(worst[0], np.abs(x - x_ref).max()), max(worst[1], np.abs(e - e_ref).max()),
                     max(worst[2], np.abs(out["criterion"] - crit_ref).max())]
            assert np.abs(x - x_ref).max() <= TOL, (k, np.abs(x - x_ref).max())
            assert np.abs(e - e_ref).max() <= TOL, (k, e, e_ref)
            assert np.abs(out["criterion"] - crit_ref).max() <= 1e-8
            assert out["status"] == [STATUS[s] for s in status_ref]
        out = band.run(400, fmax=fmax, **KW)
        tail = np.abs(band.get_positions() - ref["x"]).max()
        print(f"idpp parity {name}: 30 steps dx {worst[0]:.3g} dS {worst[1]:.3g} dcrit {worst[2]:.3g}; tail dx {tail:.3g}; "
              f"smallest margin {ref['margins'].min():.3g}; steps {ref['steps'].tolist()} status {ref['status'].tolist()}")
        assert ref["margins"].min() >= MARGIN
        assert out["status"] == [STATUS[s] for s in ref["status"]]
        assert out["steps"].tolist() == ref["steps"].tolist()
        assert tail <= 1e-7
        assert out["climbing_image"].tolist() == [-1]


def test_a_band_through_a_collision_comes_out_apart():
    ini, fin = I.straight_exchange_ends()
    linear = neb.interpolate(ini, fin, 7)
    d_lin = I.min_distances(linear)
    assert len(ini) == 54 and d_lin[3] < 0.05 and d_lin[0] > 2.5, d_lin      # the linear band: two atoms on top of each other
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        images, info = neb.idpp_interpolate(ini, fin, 7)
    assert info["status"] == ["converged"] and info["criterion"][0] < 0.1
    d = I.min_distances(images)
    S_lin = np.asarray(I.evaluate_bands([linear])[0], float)
    S = info["energies"][0]
    print(f"idpp straight exchange: smallest distances linear {np.round(d_lin, 3).tolist()} idpp {np.round(d, 3).tolist()}; "
          f"S linear {S_lin.tolist()} idpp {S.tolist()}; steps {info['steps'].tolist()}")
    assert d.min() >= 0.5 * min(d[0], d[-1]), d
    assert np.all(S <= S_lin)
    for a, b in ((images[0], linear[0]), (images[-1], linear[-1])):       # (interpolate's end points, unwrapped, as they were)
        assert np.array_equal(a.get_positions(), b.get_positions())


def test_the_band_feeds_neb():
    import test_gpu_neb as T
    calc, bands, info = T._converged()                                   # from interpolate's band (six images, climbing)
    ends, rinfo = calc.relax_frames(list(T._hop_ends()), fmax=1e-5, max_steps=2000)
    assert np.all(rinfo["converged"]) and len(ends[0]) == 127
    start, iinfo = neb.idpp_interpolate(ends[0], ends[1], 6)
    assert iinfo["status"] == ["converged"]
    _, out = calc.neb_bands([start], fmax=1e-3, climb=True, max_steps=3000)
    print(f"W vacancy hop: barrier from idpp_interpolate {out['barrier'][0]:.6f} eV ({out['steps'].tolist()} steps), from "
          f"interpolate {info['barrier'][0]:.6f} eV ({info['steps'].tolist()} steps); IDPP steps {iinfo['steps'].tolist()}")
    assert out["status"] == ["converged"]
    assert abs(out["barrier"][0] - info["barrier"][0]) <= 1e-4


def _run(bands, steps, spring=0.1, fixed=None, fmax=NEVER):
    with IDPP(bands, spring=spring, fixed=fixed) as band:
        band.run(0)
        e0, f0 = np.concatenate(band.get_potential_energies()), band.get_forces()
        outs = [band.run(n, fmax=fmax, **KW) for n in steps]
        return dict(e0=e0, f0=f0, x=band.get_positions(), g=band.get_neb_forces(), f=band.get_forces(),
                    e=np.concatenate(band.get_potential_energies()), out=outs[-1])


def test_runs_are_deterministic_and_bands_independent():
    a, b = I.hop53(), I.exchange16()
    both = _run([a, b], [60], spring=[0.1, 0.2])
    again = _run([a, b], [60], spring=[0.1, 0.2])
    for k in ("e0", "f0", "x", "g", "f", "e"):
        assert np.array_equal(both[k], again[k]), k
    na = 53 * 5
    alone = [_run([a], [60], spring=0.1), _run([b], [60], spring=0.2)]
    for k, (r, atoms, frames) in enumerate(zip(alone, (slice(0, na), slice(na, None)), (slice(0, 5), slice(5, None)))):
        assert np.array_equal(r["e0"], both["e0"][frames]) and np.array_equal(r["f0"], both["f0"][atoms]), k
        assert np.abs(r["x"] - both["x"][atoms]).max() <= 1e-8
    split = _run([a, b], [25, 35], spring=[0.1, 0.2])
    assert np.abs(split["x"] - both["x"]).max() <= 1e-10
    assert split["out"]["steps"].tolist() == both["out"]["steps"].tolist() == [60, 60]


def test_fixed_atoms_and_end_points_are_never_written():
    bands = [I.exchange16()]
    x0, off, first, _, _ = I.layout(bands)
    one = np.zeros(16, bool)
    one[[2, 7, 12]] = True
    fixed = np.tile(one, 6)
    ref = I.band_of(bands, spring=0.2, fixed=fixed)
    ref.run(30, fmax=NEVER, **KW)
    r = _run(bands, [30], spring=0.2, fixed=fixed)
    ends = np.zeros(len(x0), bool)
    ends[:16] = ends[-16:] = True
    still = fixed | ends
    assert np.array_equal(r["x"][still], x0[still])
    assert np.all(r["g"][still] == 0.0)
    assert np.abs(r["x"] - ref.x).max() <= TOL and np.abs(r["x"] - x0).max() > 1e-3
    # fixed atoms enter the others' sums and have forces of their own; only g drops them
    F_ref = np.asarray(I.evaluate_bands(bands, positions=r["x"])[1], float)
    assert np.abs(r["f"] - F_ref).max() <= 1e-9 * np.abs(F_ref).max()
    assert np.abs(r["f"][fixed & ~ends]).max() > 1e-3
    free = _run(bands, [0], spring=0.2)
    assert np.array_equal(free["f0"], r["f0"]) and np.array_equal(free["e0"], r["e0"])


def test_coincident_atoms_freeze_only_their_band():
    bad, good = I.exchange16(), I.hop53()
    x = bad[2].get_positions()
    x[5] = x[9]
    bad[2] = Atoms(numbers=bad[2].get_atomic_numbers(), positions=x, cell=bad[2].get_cell(), pbc=bad[2].get_pbc())
    both = _run([bad, good], [60], spring=[0.2, 0.1], fmax=1e-2)
    alone = _run([good], [60], spring=0.1, fmax=1e-2)
    assert both["out"]["status"][0] == "nonfinite" and both["out"]["steps"][0] == 0
    assert both["out"]["status"][1] == alone["out"]["status"][0] and both["out"]["steps"][1] == alone["out"]["steps"][0]
    assert not np.isfinite(both["e"][2]) and np.all(np.isfinite(both["e"][6:]))
    assert np.array_equal(both["x"][:96], np.concatenate([a.get_positions() for a in bad]))
    assert np.abs(both["x"][96:] - alone["x"]).max() <= 1e-8


def test_nearest_images_on_the_device():
    """An atom moved by a lattice vector in every image, and the band in a skewed and in a turned cell: the same S and F (turned
    back) within the bound of the one-evaluation test."""
    e_ref = _yardstick()[5]
    base = I.exchange16()
    cell = np.array(base[0].get_cell(), float).reshape(3, 3)

    def moved(band, atom, n):
        out = []
        for a in band:
            x = a.get_positions()
            x[atom] += np.asarray(n) @ np.array(a.get_cell(), float).reshape(3, 3)
            out.append(Atoms(numbers=a.get_atomic_numbers(), positions=x, cell=a.get_cell(), pbc=a.get_pbc()))
        return out
    skew = I.recelled(base, U=I.SKEW)
    variants = {"moved": (moved(base, 4, [1, -2, 1]), None), "skewed": (skew, None), "skewed_moved": (moved(skew, 11, [-1, 1, 2]), None),
                "turned": (I.recelled(base, Q=TURN), TURN), "skewed_turned": (I.recelled(base, U=I.SKEW, Q=TURN), TURN)}
    assert I.orthogonal(cell, [True] * 3) and not I.orthogonal(I.SKEW @ cell, [True] * 3)
    S, F = _device([base] + [v[0] for v in variants.values()])
    S, F = S.reshape(-1, 6), F.reshape(-1, 96, 3)
    off = 16 * np.arange(7)
    for k, (name, (_, Q)) in enumerate(variants.items(), 1):
        Fk = F[k] if Q is None else F[k] @ Q                             # (row vectors: x' = x Q^T, so F = F' Q)
        dS, dF = _frame_rel(S[k], S[0]), _frame_rel(Fk, F[0], off)
        print(f"idpp nearest images, {name}: dS {dS:.3g} dF {dF:.3g} (bound {16 * e_ref[0]:.3g} / {16 * e_ref[1]:.3g})")
        assert dS <= 16 * e_ref[0] and dF <= 16 * e_ref[1], name


def _create(bands, fixed=None, spring=None, edit=None, out=True):
    ctx = _lib.get_context()
    frames = [a for b in bands for a in b]
    batch = _lib.FrameBatch(frames)
    if edit:
        edit(batch)
    first = np.ascontiguousarray(np.cumsum([0] + [len(b) for b in bands]), dtype=np.int32)
    sp = np.ascontiguousarray(np.full(len(bands), 0.1) if spring is None else spring, dtype=float)
    h = C.c_void_p()
    rc = ctx.lib.uf3_idpp_create(ctx.handle, C.byref(batch.struct), _lib._p(batch.pos), _lib._p(batch.z), _lib._p(fixed), len(bands),
                                 _lib._p(first), _lib._p(sp), C.byref(h) if out else None)
    msg = ctx.lib.uf3_last_error(ctx.handle).decode()
    if rc == 0:
        ctx.lib.uf3_neb_destroy(h)
    return rc, msg


def test_library_refusals_and_the_context_left_alone():
    small = lambda m=4: I.exchange16(m)
    assert _create([small()])[0] == 0
    rc, msg = _create([small(), small()[:2]])
    assert rc == 1 and "uf3_idpp_create: band 1 has 2 images" in msg

    def species(batch):
        batch.z[16 + 4] = 29
    rc, msg = _create([small()], edit=species)
    assert rc == 1 and "species" in msg

    def same(batch):
        batch.pos[32:48] = batch.pos[16:32]
    rc, msg = _create([small()], edit=same)
    assert rc == 1 and "identical to image 1" in msg
    rc, msg = _create([small()], out=False)
    assert rc == 1 and "out is NULL" in msg
    # a run on such a handle: no climbing image, and the context's MD skin and lists stay as they were
    calc = calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json")), md_skin=0.3)
    ctx = _lib.get_context(calc.device)
    other = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=61)
    e0, f0, _ = calc.evaluate_frames([other])
    calc.evaluate_frames([other])
    builds = ctx.md_stats()["builds"]
    calc.evaluate_frames([other])
    assert ctx.md_stats()["builds"] == builds                            # (nothing moved: the lists are reused)
    with IDPP(small()) as band:
        lib, h = band.ctx.lib, band.handle
        assert band.ctx is ctx
        assert lib.uf3_neb_run(h, 10, 1e-3, 0.1, 1.0, 0.2, 0.7, 1, 1, 0, None) == 1
        assert "climbing" in lib.uf3_last_error(ctx.handle).decode()
        assert lib.uf3_neb_run(h, 10, 1e-3, 0.1, 1.0, 0.2, 0.7, 0, 1, 0, None) == 0
        assert band.run(0)["steps"].tolist() == [10]
    e1, f1, _ = calc.evaluate_frames([other])
    assert ctx.md_stats()["builds"] == builds and getattr(ctx, "_md_skin", 0.0) == 0.3
    assert np.array_equal(e0, e1) and np.array_equal(f0, f1)
