"""uf3_fit_add's chunk plan, on the host alone (``uf3_fit_plan_debug``: the planner uf3_fit_add itself calls, no device).

The header promises chunks of at most ``max_atoms_per_chunk`` atoms unless a chunk is a single frame; the staging and row
buffers are sized from the plan, so a chunk past the limit grows them past the caller's cap."""
import ctypes as C

import numpy as np
import pytest

from uf3_amd import _lib


def plan(counts, max_atoms, first_fraction):
    lib = _lib.load()
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    ends = np.zeros(max(1, len(counts)), dtype=np.int32)
    n = C.c_int32()
    rc = lib.uf3_fit_plan_debug(len(counts), _lib._p(counts), int(max_atoms), float(first_fraction), _lib._p(ends), C.byref(n))
    if rc:
        raise _lib.UF3Error(rc, lib.uf3_last_error(None).decode())
    return [int(e) for e in ends[:n.value]]


def ramp_limits(max_atoms, first_fraction):
    """The ramp chunks' own limits, in order (uf3_fit_add: first_fraction of the limit, doubling while below 1)."""
    out, fr = [], first_fraction
    while fr < 1.0:
        out.append(max(1, int(max_atoms * fr)))
        fr = min(1.0, 2.0 * fr)
    return out


def even_spread_plan(counts, max_atoms, first_fraction):
    """The planner's even spread behind the ramp, restated: the plan it makes wherever that spread keeps the bound, or None
    where no spread up to one chunk per frame does."""
    n, ends, s0 = len(counts), [], 0
    for limit in ramp_limits(max_atoms, first_fraction):
        if s0 >= n:
            break
        s1, atoms = s0, 0
        while s1 < n and (s1 == s0 or atoms + counts[s1] <= limit):
            atoms += counts[s1]
            s1 += 1
        ends.append(s1)
        s0 = s1
    if s0 >= n:
        return ends
    rest = sum(counts[s0:])
    n_chunks = (rest + max_atoms - 1) // max_atoms
    while True:
        tail, q0, run, fits, k = [], s0, 0, True, 0
        while k < n_chunks and q0 < n:
            target = (rest * (k + 1) + n_chunks - 1) // n_chunks
            q1, atoms = q0, 0
            while q1 < n and (q1 == q0 or run + atoms < target):
                atoms += counts[q1]
                q1 += 1
            if k == n_chunks - 1:
                while q1 < n:
                    atoms += counts[q1]
                    q1 += 1
            fits = fits and (atoms <= max_atoms or q1 == q0 + 1)
            run += atoms
            tail.append(q1)
            q0 = q1
            k += 1
        if fits:
            return ends + tail
        if n_chunks >= n - s0:
            return None
        n_chunks += 1


def check_plan(counts, max_atoms, first_fraction):
    ends = plan(counts, max_atoms, first_fraction)
    n = len(counts)
    assert ends and ends[-1] == n, (counts, ends)
    starts = [0] + ends[:-1]
    assert all(e > s for s, e in zip(starts, ends)), (counts, ends)                 # contiguous, non-empty, every frame
    sizes = [sum(counts[s:e]) for s, e in zip(starts, ends)]
    for k, (s, e) in enumerate(zip(starts, ends)):
        assert e - s == 1 or sizes[k] <= max_atoms, (counts, max_atoms, first_fraction, ends)
    for k, limit in enumerate(ramp_limits(max_atoms, first_fraction)[:len(ends)]):
        assert ends[k] - starts[k] == 1 or sizes[k] <= limit, (counts, max_atoms, first_fraction, ends)
    return ends


@pytest.mark.parametrize("counts,max_atoms,first_fraction", [([40, 70, 40, 70], 100, 1.0)] +
                         [([73, 109, 103], m, f) for m in range(120, 201, 10) for f in (1.0, 0.5, 0.125)])
def test_counterexamples_of_the_even_spread_keep_the_limit(counts, max_atoms, first_fraction):
    """Where no even spread fits, the tail used to be accepted anyway at one chunk per remaining frame -- a first chunk of 110
    atoms at a limit of 100, a chunk of 182 atoms at every limit from 120 to 200."""
    ends = check_plan(counts, max_atoms, first_fraction)
    assert even_spread_plan(counts, max_atoms, first_fraction) is None or ends == even_spread_plan(counts, max_atoms, first_fraction)


def test_random_frame_sequences_keep_the_limit_and_the_even_spread_where_it_fits():
    rng = np.random.default_rng(20261015)
    n_even = n_greedy = 0
    for _ in range(3000):
        n = int(rng.integers(1, 41))
        hi = int(rng.choice([8, 60, 200, 1000]))
        counts = [int(v) for v in rng.integers(1, hi + 1, size=n)]
        max_atoms = int(rng.choice([hi // 2 + 1, hi, 2 * hi, 5 * hi, 37 * hi]))
        for first_fraction in (1.0, 0.5, 0.125):
            ends = check_plan(counts, max_atoms, first_fraction)
            even = even_spread_plan(counts, max_atoms, first_fraction)
            if even is not None:
                assert ends == even, (counts, max_atoms, first_fraction)           # unchanged wherever the even spread fits
                n_even += 1
            else:
                n_greedy += 1
    assert n_even > 1000 and n_greedy > 100, (n_even, n_greedy)


def test_the_planned_chunk_counts_of_the_fit_tests_and_the_benchmark():
    """test_fit_chunk_plan_ramps_then_spreads_the_rest_evenly (16-atom frames at 512: 4 + 8 + 16 frames then 4 x 25; 37 frames:
    4 + 8 + 16 + 9), test_config4_fit_in_chunks_10k_atom_tungsten_frames (3 + 6 + 12 + 23 + 22) and
    test_two_element_fit_in_chunks_through_the_tiled_gram_kernel (two chunks: 4 + 4)."""
    assert plan([16] * 128, 512, 0.125) == [4, 12, 28, 53, 78, 103, 128]
    assert plan([16] * 37, 512, 0.125) == [4, 12, 28, 37]
    assert plan([16] * 128, 1 << 20, 1.0) == [128]
    assert plan([10000] * 66, 250000, 0.125) == [3, 9, 21, 44, 66]
    assert plan([10000] * 8, 50000, 1.0) == [4, 8]


def test_bad_arguments_are_refused():
    with pytest.raises(_lib.UF3Error):
        plan([16, 0, 16], 100, 1.0)
    with pytest.raises(_lib.UF3Error):
        plan([16], 100, 0.0)
    with pytest.raises(_lib.UF3Error):
        plan([16], 100, 1.5)
    assert plan([], 100, 1.0) == []
    assert plan([500], 100, 0.125) == [1]                 # a single frame past the limit is a chunk of its own
