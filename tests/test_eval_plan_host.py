"""The evaluator's launch plan, on the host alone (``uf3_eval_plan_debug``: the pure function eval_impl itself calls, no device).

The three LDS layouts of ``k_eval`` are restated here from the sizes the kernel's carve uses -- not from the library's
expressions -- and the rules of the instance choice (CW, WIN, TAB, cap16) and of the overflow verdict are asserted over a grid of
inputs."""
import ctypes as C
import itertools

import pytest

from uf3_amd import _lib

CW, WIN, TAB, CAP16 = 1, 2, 4, 8                     # bits of `instance`
NO_TAB, NO_CW, NO_CAP16 = 1, 2, 4                    # bits of `switches`
WAVE, EVAL_Q, EVAL_TAB_KN, EVAL_TAB_CAP, EVAL_CW_WAVES = 64, 5, 24, 36, 8
KNOT_REC = 96                                        # bytes of a knot record
LDS_LIMIT = 160 * 1024 - 512                         # UF3_LDS_LIMIT
LDS_MAX = 160 * 1024                                 # what an MI355X grants a workgroup


def plan(cap, two_pass=True, md_step=False, n2=23, n_recs=60, cw_bytes=8192, tab_ok=True, has_window=True, lds_max=LDS_MAX,
         switches=0):
    lib = _lib.load()
    inst, lds, per_wave, fits = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32()
    rc = lib.uf3_eval_plan_debug(cap, int(two_pass), int(md_step), n2, n_recs, cw_bytes, int(tab_ok), int(has_window), lds_max,
                                 switches, C.byref(inst), C.byref(lds), C.byref(per_wave), C.byref(fits))
    if rc:
        raise _lib.UF3Error(rc, lib.uf3_last_error(None).decode())
    return inst.value, lds.value, per_wave.value, bool(fits.value)


def up16(n):
    return (n + 15) // 16 * 16


def plain_bytes(cap, walk_order=True):
    """Own list: 32 + 20 B per entry and two counters; a 16-byte head; the queue of bonds, 2 x 64 x EVAL_Q doubles; the force on the
    entries, 24 B each; the walk-order entries + keys of the fused list build, 48 B each."""
    return (32 + 20) * cap + 8 + 16 + 2 * WAVE * EVAL_Q * 8 + 24 * cap + (48 * cap if walk_order else 0)


def tab_bytes(cap):
    """+ a 16-byte head and leg n's knot records; + the per-bond leg tables (136 B per entry, a 16-byte head) where they do not
    fit over the queue."""
    return plain_bytes(cap) + 16 + EVAL_TAB_KN * KNOT_REC + (136 * cap + 16 if cap > EVAL_TAB_CAP else 0)


def cw_per_wave(cap, md_step):
    return up16(plain_bytes(cap, walk_order=not md_step))


def cw_bytes_total(cap, md_step, n2, n_recs, cw_bytes):
    return cw_bytes + KNOT_REC * n_recs + up16(8 * n2) + EVAL_CW_WAVES * cw_per_wave(cap, md_step)


def test_the_pinned_byte_counts():
    assert plain_bytes(16) == 7128 and tab_bytes(16) == 7128 + 16 + 24 * 96 == 9448
    assert plain_bytes(40) == 10104 and tab_bytes(40) == 17880
    assert plan(16, tab_ok=False) == (CAP16, 7128, 0, True)
    assert plan(16, has_window=False) == (TAB | CAP16, 9448, 0, True)
    assert plan(40, tab_ok=False) == (0, 10104, 0, True)
    assert plan(40, has_window=False) == (TAB, 17880, 0, True)
    # MD route, capacity 16: the CW layout, its waves without the walk-order arrays
    assert cw_per_wave(16, True) == up16(7128 - 768) == 6368
    n2, n_recs, cwb = 23, 60, 8192
    inst, lds, per_wave, fits = plan(16, md_step=True, n2=n2, n_recs=n_recs, cw_bytes=cwb)
    assert inst == CW | TAB | CAP16 and per_wave == 6368 and fits
    assert lds == cwb + 96 * n_recs + up16(8 * n2) + 8 * 6368


GRID = list(itertools.product((1, 8, 15, 16, 17, 24, 36, 37, 40, 64, 248), (False, True), (False, True), (False, True),
                              (False, True), range(8)))


def test_the_instance_rules_over_a_grid_of_inputs():
    """CW only with md_step, TAB, the window table, capacity <= 16 and a total <= UF3_LDS_LIMIT / 2; WIN exactly when TAB holds, CW
    does not and the table is present; each switch removes exactly its instance; the bytes are those of the layout chosen."""
    assert LDS_LIMIT // 2 == 81664
    n_cw = n_win = n_tab = n_plain = 0
    for (cap, two_pass, md_step, tab_ok, has_window, switches), (n2, n_recs, cwb) in itertools.product(
            GRID, ((23, 60, 8192), (0, 3, 1024), (23, 60, 40960))):
        if md_step and not two_pass:
            continue                                 # (the MD route is a two-pass route)
        inst, lds, per_wave, fits = plan(cap, two_pass, md_step, n2, n_recs, cwb, tab_ok, has_window, LDS_MAX, switches)
        key = (cap, two_pass, md_step, tab_ok, has_window, switches, cwb)
        tab = two_pass and tab_ok and tab_bytes(cap) <= LDS_MAX and not switches & NO_TAB
        total = cw_bytes_total(cap, md_step, n2, n_recs, cwb)
        cw = tab and md_step and has_window and cap <= 16 and total <= LDS_LIMIT // 2 and not switches & NO_CW
        win = tab and not cw and has_window and not switches & NO_CW
        cap16 = two_pass and cap == 16 and not switches & NO_CAP16
        assert inst == (CW * cw | WIN * win | TAB * tab | CAP16 * cap16), key
        assert lds == (total if cw else tab_bytes(cap) if tab else plain_bytes(cap)), key
        assert per_wave == (cw_per_wave(cap, md_step) if cw else 0), key
        assert fits == (cw or lds <= LDS_MAX), key
        n_cw += cw; n_win += win; n_tab += tab and not cw and not win; n_plain += not tab
    assert min(n_cw, n_win, n_tab, n_plain) >= 16, (n_cw, n_win, n_tab, n_plain)         # (every arm is met)


@pytest.mark.parametrize("md_step", [False, True])
def test_each_switch_removes_exactly_its_instance(md_step):
    base = plan(16, md_step=md_step)[0]
    assert base == ((CW if md_step else WIN) | TAB | CAP16)
    assert plan(16, md_step=md_step, switches=NO_CAP16)[0] == base & ~CAP16
    assert plan(16, md_step=md_step, switches=NO_CW)[0] == TAB | CAP16
    assert plan(16, md_step=md_step, switches=NO_TAB)[0] == CAP16
    # a CW layout past half of the LDS limit: the WIN instance instead
    big = plan(16, md_step=True, cw_bytes=40960)
    assert cw_bytes_total(16, True, 23, 60, 40960) > LDS_LIMIT // 2 and big[0] == WIN | TAB | CAP16 and big[1] == 9448


def test_a_layout_above_the_grant_is_the_overflow_verdict_and_a_cw_layout_is_not():
    # plain: the gather instances at the default 64 KB grant
    cap = next(k for k in range(8, 2000, 8) if plain_bytes(k) > 65536)
    assert plan(cap - 8, two_pass=False, lds_max=65536)[3] and plan(cap - 8, two_pass=False, lds_max=65536)[1] == plain_bytes(cap - 8)
    assert plan(cap, two_pass=False, lds_max=65536) == (0, plain_bytes(cap), 0, False)
    # TAB: the longer layout is dropped when it alone does not fit; the plain layout above the grant overflows
    cap = next(k for k in range(40, 2000, 8) if tab_bytes(k) > 65536)
    assert plain_bytes(cap) <= 65536
    assert plan(cap, lds_max=65536) == (0, plain_bytes(cap), 0, True)
    assert plan(cap - 8, lds_max=65536) == (WIN | TAB, tab_bytes(cap - 8), 0, True)
    # CW: larger than the default grant, and not an overflow (its launch asks for the larger grant itself)
    inst, lds, _, fits = plan(16, md_step=True, cw_bytes=16384, lds_max=65536)
    assert inst & CW and 65536 < lds <= LDS_LIMIT // 2 and fits


def test_bad_arguments_are_refused():
    with pytest.raises(_lib.UF3Error):
        plan(0)
    with pytest.raises(_lib.UF3Error):
        plan(16, n2=-1)
