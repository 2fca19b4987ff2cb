"""
The normal equations every fit is solved from: uf3_gram_dev / uf3_gram (k_gram_mfma, k_gram_small, k_gram_tiled) and
uf3_gram_force_rows_dev (k_gram_tiled on per-species row lists), held to exact sums.

Exact data: entries m 2^e with integer |m| <= 15 and e in [-3, 3].  Every product is a multiple of 2^-6 below 2^14, so with
at most 2^18 rows every partial sum, in any order (FMA, MFMA, atomics), is a multiple of 2^-6 below 2^32: 38 bits, exact in
fp64.  NumPy's X^T X is then exact too, and every route must equal it bit for bit, whatever its chunking or atomic order.
Sentinels sit where the kernels must not look: NaN in the columns F .. ld of a row, NaN rows past n_rows, NaN in the outputs
before an overwriting call.  Every test asserts the kernel it means to reach (UF3_DEBUG_LDS lines, the ``dbg`` fixture).

Exact data is exact in fp32 as well, so real feature rows are compared too, entry by entry, against the error bound of an fp64
sum of n products: |G - G_ref| <= gamma_n (|X|^T |X|)_ij, gamma_n = n u / (1 - n u), u = 2^-53.
"""
import ctypes as C

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data import composition
from uf3_amd.representation import process
from _util import dbg  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
NAN = float("nan")


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def exact_values(rng, shape):
    """m 2^e, |m| <= 15 (about 40 % zeros), e in [-3, 3]; drawn in blocks of rows (the widest cases hold 2 GB)."""
    out = np.empty(shape)
    flat = out.reshape(-1)
    for b in range(0, flat.size, 1 << 22):
        k = min(flat.size - b, 1 << 22)
        m = rng.integers(-15, 16, size=k).astype(np.float64)
        m[rng.random(k) < 0.4 * 31 / 30 - 1 / 30] = 0.0
        flat[b:b + k] = np.ldexp(m, rng.integers(-3, 4, size=k))
    return out


def assert_exactly_summable(x, y=None):
    """The premise, from the data drawn: multiples of 2^-3, and n max|x|^2 below 2^32 (and so every partial sum)."""
    for a in (x, y):
        if a is None or not a.size:
            continue
        assert np.array_equal(a * 8.0, np.round(a * 8.0))
        amax = float(np.abs(a).max())
        assert amax <= 120.0
    n = x.shape[0]
    assert n <= 1 << 18
    assert n * 120.0 * 120.0 < 2.0 ** 32


def ref_pieces(x, y):
    g = x.T @ x
    return g, (x.T @ y if y is not None else None)


class Gram:
    """The _dev entries on torch buffers, on torch's current stream, with sentinels around the operands."""

    def __init__(self, ctx):
        import torch
        self.torch, self.ctx = torch, ctx
        self.dev = torch.device("cuda", ctx.device)

    def x(self, x, ld, extra_rows=3):
        """[n + extra_rows][ld] on the device: x in the first F columns, NaN in the padding columns and the rows past n."""
        n, F = x.shape
        h = np.full((n + extra_rows, ld), NAN)
        h[:n, :F] = x
        return self.torch.from_numpy(h).to(self.dev)

    def y(self, y, extra_rows=3):
        return self.torch.from_numpy(np.concatenate([y, np.full(extra_rows, NAN)])).to(self.dev)

    def out(self, F, fill=NAN):
        t = self.torch
        return t.full((F, F), fill, dtype=t.float64, device=self.dev), t.full((F,), fill, dtype=t.float64, device=self.dev)

    def put(self, g0, o0):
        t = self.torch
        return t.from_numpy(np.array(g0)).to(self.dev), t.from_numpy(np.array(o0)).to(self.dev)

    @staticmethod
    def _ptr(a):
        return None if a is None else C.c_void_p(a.data_ptr())

    def run(self, dx, dy, n_rows, F, ld, acc, g, o):
        ctx = self.ctx
        prev = ctx.set_stream(self.torch.cuda.current_stream(self.dev).cuda_stream)
        try:
            ctx.check(ctx.lib.uf3_gram_dev(ctx.handle, self._ptr(dx), self._ptr(dy), n_rows, F, ld, acc, self._ptr(g), self._ptr(o)))
        finally:
            ctx.restore_stream(prev)

    def force_rows(self, db, dx, dy, dz, n_atoms, ld, acc, g, o):
        ctx = self.ctx
        prev = ctx.set_stream(self.torch.cuda.current_stream(self.dev).cuda_stream)
        try:
            ctx.check(ctx.lib.uf3_gram_force_rows_dev(db.handle, self._ptr(dx), self._ptr(dy), C.c_void_p(dz.data_ptr()), n_atoms,
                                                      ld, acc, self._ptr(g), self._ptr(o)))
        finally:
            ctx.restore_stream(prev)


def odd_ld(F):
    return F + 2 if F % 2 else F + 3


def one_launch(dbg, kernel, **fields):
    said = dbg.grams()
    assert len(said) == 1 and said[0]["kernel"] == kernel, said
    for k, v in fields.items():
        assert said[0][k] == v, (k, said)
    return said[0]


def check_route(dbg, gram, rng, n, F, kernel, ld=None):
    """Overwrite over NaN outputs, then accumulate on top of an exact non-zero G0 / o0: both bit-exact."""
    ld = ld or odd_ld(F)
    x, y = exact_values(rng, (n, F)), exact_values(rng, n)
    assert_exactly_summable(x, y)
    g_ref, o_ref = ref_pieces(x, y)
    dx, dy = gram.x(x, ld), gram.y(y)
    g, o = gram.out(F)
    gram.run(dx, dy, n, F, ld, 0, g, o)
    one_launch(dbg, kernel, rows=n, feat=F, ld=ld, acc=0, ord=1)
    assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(o.cpu().numpy(), o_ref)
    g0 = exact_values(rng, (F, F))
    g0 = g0 + g0.T
    o0 = exact_values(rng, F)
    g, o = gram.put(g0, o0)
    gram.run(dx, dy, n, F, ld, 1, g, o)
    one_launch(dbg, kernel, rows=n, feat=F, ld=ld, acc=1, ord=1)
    assert np.array_equal(g.cpu().numpy(), g0 + g_ref) and np.array_equal(o.cpu().numpy(), o0 + o_ref)


@pytest.fixture
def gram(dbg):
    return Gram(_lib.get_context())


# ------------------------------------------------------------------------------------------------
# exact sums on every route
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,F,kernel", [(16383, 80, "mfma"), (16384, 80, "small"), (16384, 81, "mfma"),
                                        (65536, 128, "mfma"), (65535, 129, "mfma"), (65536, 129, "tiled")])
def test_both_sides_of_every_route_edge_are_exact(n, F, kernel, dbg, gram):
    """The route changes at F = 80 / 81 (k_gram_small's width), 128 / 129 and 16 384 / 65 536 rows: each side, exact, with
    NaN padding columns (odd ld), NaN rows past n_rows, NaN outputs before an overwrite, then accumulate."""
    check_route(dbg, gram, np.random.default_rng(n + F), n, F, kernel)


@pytest.mark.parametrize("F", [1, 16, 17, 32, 33, 64, 80])
def test_slab_kernel_exact_at_every_tile_count(F, dbg, gram):
    """k_gram_small: one to five 16-column tiles, columns that end inside a tile, row counts no multiple of the 32-row slab."""
    n = 16384 + 32 * F + 7 + 2 * F
    assert n % 32
    check_route(dbg, gram, np.random.default_rng(F), n, F, "small")


@pytest.mark.parametrize("F", [192, 193, 257, 1798])
def test_tiled_kernel_exact_at_odd_range_counts(F, dbg, gram):
    """k_gram_tiled: 3, 4 (ending one column into a range), 5 and 29 column ranges (an odd count: the plan packer's
    shuffles run), row counts no multiple of the 16-row slab."""
    n = 65536 + 9 if F < 1000 else 65536 + 13
    assert n % 16
    check_route(dbg, gram, np.random.default_rng(F), n, F, "tiled")


def species_masks(basis, fz):
    """Per species, the columns its atoms' force rows can be non-zero on: the non-zero pattern of featurised rows of that
    species (a subset of the columns the device multiplies for it)."""
    elements = basis.element_list
    nums = [composition.atomic_numbers[el] for el in elements]
    frame = synthetic.lattice_frame("bcc", (6, 6, 6), 3.165, nums, seed=71)
    _, x_f, _ = fz.featurize_frames([frame], energy=False, forces=True)
    z = frame.get_atomic_numbers()
    masks = {}
    for num in nums:
        rows = x_f[z == num]
        assert len(rows) > 20
        masks[num] = (rows != 0).any(axis=(0, 1))
        assert 0 < masks[num].sum() < basis.n_feats
    return masks


def species_rows(rng, masks, z):
    """Exact force rows, [3 n][F]: an atom's rows are exact data on its species' columns and zero elsewhere."""
    F = len(next(iter(masks.values())))
    x = exact_values(rng, (3 * len(z), F))
    keep = np.stack([masks[int(v)] for v in z])
    x *= np.repeat(keep, 3, axis=0)
    return x


def test_one_buffer_accumulated_through_three_routes(dbg, gram):
    """F = 434: k_gram_mfma on 1 000 rows, then k_gram_tiled on 70 001 rows, then the per-species route, all into one buffer."""
    basis = dbg.basis(synthetic.notebook_basis(['Mo', 'W']))
    fz = process.BasisFeaturizer(basis)
    ctx, db = fz._dev()
    assert ctx is gram.ctx
    F = basis.n_feats
    assert F == 434
    rng = np.random.default_rng(434)
    masks = species_masks(basis, fz)
    dbg.grams()
    ld = odd_ld(F)
    x1, y1 = exact_values(rng, (1000, F)), exact_values(rng, 1000)
    x2, y2 = exact_values(rng, (70001, F)), exact_values(rng, 70001)
    n_atoms = 43691
    z = rng.choice([42, 74], size=n_atoms).astype(np.int32)
    x3, y3 = species_rows(rng, masks, z), exact_values(rng, 3 * n_atoms)
    total = 1000 + 70001 + 3 * n_atoms
    assert_exactly_summable(np.concatenate([x1, x2, x3]), np.concatenate([y1, y2, y3]))
    assert total <= 1 << 18
    g, o = gram.out(F)
    gram.run(gram.x(x1, ld), gram.y(y1), 1000, F, ld, 0, g, o)
    one_launch(dbg, "mfma", acc=0)
    gram.run(gram.x(x2, ld), gram.y(y2), 70001, F, ld, 1, g, o)
    one_launch(dbg, "tiled", acc=1)
    d_z = gram.torch.from_numpy(z).to(gram.dev)
    gram.force_rows(db, gram.x(x3, ld), gram.y(y3), d_z, n_atoms, ld, 1, g, o)
    said = dbg.grams()
    assert [d["kernel"] for d in said] == ["tiled_sub", "tiled_sub"] and all(d["acc"] == 1 for d in said), said
    g_ref = x1.T @ x1 + x2.T @ x2 + x3.T @ x3
    o_ref = x1.T @ y1 + x2.T @ y2 + x3.T @ y3
    assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(o.cpu().numpy(), o_ref)


@pytest.mark.parametrize("n,F,kernel", [(3001, 100, "mfma"), (16411, 40, "small"), (65537, 200, "tiled")])
def test_without_ordinate_and_without_rows(n, F, kernel, dbg, gram):
    """y = NULL or ord = NULL: the Gram is still exact; with y = NULL an ord buffer is zeroed by an overwrite and left alone
    by an accumulate.  n_rows = 0: zeros, or the buffers unchanged."""
    rng = np.random.default_rng(n)
    ld = odd_ld(F)
    x = exact_values(rng, (n, F))
    assert_exactly_summable(x)
    g_ref = x.T @ x
    dx = gram.x(x, ld)
    g, o = gram.out(F)
    gram.run(dx, None, n, F, ld, 0, g, o)
    one_launch(dbg, kernel, ord=0, acc=0)
    assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(o.cpu().numpy(), np.zeros(F))
    o0 = exact_values(rng, F)
    g, o = gram.put(np.zeros((F, F)), o0)
    gram.run(dx, None, n, F, ld, 1, g, o)
    one_launch(dbg, kernel, ord=0, acc=1)
    assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(o.cpu().numpy(), o0)
    g, _ = gram.out(F)
    gram.run(dx, gram.y(exact_values(rng, n)), n, F, ld, 0, g, None)
    one_launch(dbg, kernel, ord=0, acc=0)
    assert np.array_equal(g.cpu().numpy(), g_ref)
    # no rows
    g, o = gram.out(F)
    gram.run(dx, gram.y(exact_values(rng, n)), 0, F, ld, 0, g, o)
    assert np.array_equal(g.cpu().numpy(), np.zeros((F, F))) and np.array_equal(o.cpu().numpy(), np.zeros(F))
    g0 = exact_values(rng, (F, F))
    g, o = gram.put(g0, o0)
    gram.run(dx, gram.y(exact_values(rng, n)), 0, F, ld, 1, g, o)
    assert np.array_equal(g.cpu().numpy(), g0) and np.array_equal(o.cpu().numpy(), o0)
    assert dbg.grams() == []


def test_tiled_plan_cache_evicts_and_rebuilds(dbg, gram):
    """One context, tiled calls at 3 .. 13 column ranges (F = 64 k + 1): eleven widths for nine plan slots, then the first
    widths again (evicted: planned anew) and the last (still held) -- every result exact."""
    rng = np.random.default_rng(13)
    n, F_max = 65537, 64 * 12 + 1
    ld = F_max + 2
    x, y = exact_values(rng, (n, F_max)), exact_values(rng, n)
    assert_exactly_summable(x, y)
    g_all, o_all = ref_pieces(x, y)
    dx, dy = gram.x(x, ld), gram.y(y)
    seen = {}
    for k in list(range(2, 13)) + [2, 3, 12]:
        F = 64 * k + 1
        g, o = gram.out(F)
        gram.run(dx, dy, n, F, ld, 0, g, o)
        said = one_launch(dbg, "tiled", cols=F, feat=F)
        seen.setdefault(k, []).append(said["plan_new"])
        assert np.array_equal(g.cpu().numpy(), g_all[:F, :F]), F
        assert np.array_equal(o.cpu().numpy(), o_all[:F]), F
    assert all(v[0] == 1 for v in seen.values())
    assert seen[2] == [1, 1] and seen[3] == [1, 1] and seen[12] == [1, 0], seen


def test_direct_kernel_table_follows_the_width(dbg, gram):
    """k_gram_mfma's tile-pair table is keyed by n_feat: alternating widths on one context rebuild it, a repeat does not."""
    rng = np.random.default_rng(300)
    n, ld = 1000, 303
    x, y = exact_values(rng, (n, 300)), exact_values(rng, n)
    g_all, o_all = ref_pieces(x, y)
    dx, dy = gram.x(x, ld), gram.y(y)
    flags = []
    for F in (300, 200, 300, 300, 97, 200):
        g, o = gram.out(F)
        gram.run(dx, dy, n, F, ld, 0, g, o)
        flags.append(one_launch(dbg, "mfma", feat=F)["table_new"])
        assert np.array_equal(g.cpu().numpy(), g_all[:F, :F]) and np.array_equal(o.cpu().numpy(), o_all[:F]), F
    assert flags == [1, 1, 1, 0, 1, 1]


@pytest.mark.parametrize("n,F,kernel", [(1000, 100, "mfma"), (16411, 40, "small"), (65537, 200, "tiled")])
def test_host_entry_on_every_route(n, F, kernel, dbg):
    """uf3_gram: host arrays with a leading dimension (NaN padding), overwrite, then accumulate on a host G0 / o0."""
    ctx = _lib.get_context()
    rng = np.random.default_rng(F)
    ld = odd_ld(F)
    x, y = exact_values(rng, (n, F)), exact_values(rng, n)
    assert_exactly_summable(x, y)
    g_ref, o_ref = ref_pieces(x, y)
    xh = np.full((n, ld), NAN)
    xh[:, :F] = x
    g, o = np.full((F, F), NAN), np.full(F, NAN)
    ctx.check(ctx.lib.uf3_gram(ctx.handle, _lib._p(xh), _lib._p(y), n, F, ld, 0, _lib._p(g), _lib._p(o)))
    one_launch(dbg, kernel, acc=0, ld=ld)
    assert np.array_equal(g, g_ref) and np.array_equal(o, o_ref)
    g0 = exact_values(rng, (F, F))
    g0 = g0 + g0.T
    o0 = exact_values(rng, F)
    g, o = g0.copy(), o0.copy()
    ctx.check(ctx.lib.uf3_gram(ctx.handle, _lib._p(xh), _lib._p(y), n, F, ld, 1, _lib._p(g), _lib._p(o)))
    one_launch(dbg, kernel, acc=1, ld=ld)
    assert np.array_equal(g, g0 + g_ref) and np.array_equal(o, o0 + o_ref)


@pytest.mark.parametrize("elements,probs,n_atoms", [(['Mo', 'W'], [0.5, 0.5], 43691), (['Mo', 'Nb', 'W'], [0.6, 0.3, 0.1], 65536)])
def test_force_rows_by_species_are_exact(elements, probs, n_atoms, dbg, gram):
    """uf3_gram_force_rows_dev on its per-species route: exact rows on each species' own columns, an even and an uneven
    composition; overwrite over NaN outputs, then accumulate."""
    basis = dbg.basis(synthetic.notebook_basis(elements))
    fz = process.BasisFeaturizer(basis)
    ctx, db = fz._dev()
    assert ctx is gram.ctx
    F = basis.n_feats
    rng = np.random.default_rng(n_atoms)
    masks = species_masks(basis, fz)
    dbg.grams()
    nums = [composition.atomic_numbers[el] for el in elements]
    z = rng.choice(nums, size=n_atoms, p=probs).astype(np.int32)
    x, y = species_rows(rng, masks, z), exact_values(rng, 3 * n_atoms)
    assert_exactly_summable(x, y)
    g_ref, o_ref = ref_pieces(x, y)
    ld = odd_ld(F)
    dx, dy = gram.x(x, ld), gram.y(y)
    del x
    d_z = gram.torch.from_numpy(z).to(gram.dev)
    g, o = gram.out(F)
    gram.force_rows(db, dx, dy, d_z, n_atoms, ld, 0, g, o)
    said = dbg.grams()
    assert [d["kernel"] for d in said] == ["tiled_sub"] * len(elements), said
    assert all(d["rows"] == 3 * n_atoms and d["acc"] == 0 and d["ord"] == 1 and d["cols"] < F for d in said), said
    assert np.array_equal(g.cpu().numpy(), g_ref) and np.array_equal(o.cpu().numpy(), o_ref)
    gram.force_rows(db, dx, dy, d_z, n_atoms, ld, 1, g, o)
    assert all(d["kernel"] == "tiled_sub" and d["acc"] == 1 for d in dbg.grams())
    assert np.array_equal(g.cpu().numpy(), 2 * g_ref) and np.array_equal(o.cpu().numpy(), 2 * o_ref)


# ------------------------------------------------------------------------------------------------
# cached launch tables across streams
# ------------------------------------------------------------------------------------------------
def test_cached_tables_are_not_rewritten_under_a_running_launch(dbg, gram):
    """A long direct Gram (F = 300) on stream A; the context moves to stream B and, with no host wait, runs F = 200 -- whose
    tile-pair table fits the old buffer and is rewritten in place.  Then two force-row Grams on two streams (their species row
    lists are refilled in place).  Every result exact."""
    torch = gram.torch
    ctx = gram.ctx
    rng = np.random.default_rng(5)
    sa, sb = torch.cuda.Stream(gram.dev), torch.cuda.Stream(gram.dev)
    n1, x1, y1 = 60000, exact_values(rng, (60000, 300)), exact_values(rng, 60000)
    n2, x2, y2 = 1000, exact_values(rng, (1000, 200)), exact_values(rng, 1000)
    assert_exactly_summable(x1, y1)
    dx1, dy1, dx2, dy2 = gram.x(x1, 301), gram.y(y1), gram.x(x2, 203), gram.y(y2)
    g1, o1 = gram.out(300)
    g2, o2 = gram.out(200)
    torch.cuda.synchronize(gram.dev)
    prev = ctx.set_stream(sa.cuda_stream)
    try:
        ctx.check(ctx.lib.uf3_gram_dev(ctx.handle, C.c_void_p(dx1.data_ptr()), C.c_void_p(dy1.data_ptr()), n1, 300, 301, 0,
                                       C.c_void_p(g1.data_ptr()), C.c_void_p(o1.data_ptr())))
        ctx.set_stream(sb.cuda_stream)
        ctx.check(ctx.lib.uf3_gram_dev(ctx.handle, C.c_void_p(dx2.data_ptr()), C.c_void_p(dy2.data_ptr()), n2, 200, 203, 0,
                                       C.c_void_p(g2.data_ptr()), C.c_void_p(o2.data_ptr())))
    finally:
        ctx.restore_stream(prev)
    sa.synchronize()
    sb.synchronize()
    assert [(d["kernel"], d["feat"], d["table_new"]) for d in dbg.grams()] == [("mfma", 300, 1), ("mfma", 200, 1)]
    r1, r2 = ref_pieces(x1, y1), ref_pieces(x2, y2)
    assert np.array_equal(g1.cpu().numpy(), r1[0]) and np.array_equal(o1.cpu().numpy(), r1[1])
    assert np.array_equal(g2.cpu().numpy(), r2[0]) and np.array_equal(o2.cpu().numpy(), r2[1])
    del dx1, dx2
    # the species row lists
    basis = dbg.basis(synthetic.notebook_basis(['Mo', 'W']))
    fz = process.BasisFeaturizer(basis)
    _, db = fz._dev()
    F = basis.n_feats
    masks = species_masks(basis, fz)
    dbg.grams()
    runs = []
    for k, (n_atoms, p_mo) in enumerate([(60000, 0.5), (45000, 0.2)]):
        z = rng.choice([42, 74], size=n_atoms, p=[p_mo, 1 - p_mo]).astype(np.int32)
        x, y = species_rows(rng, masks, z), exact_values(rng, 3 * n_atoms)
        assert_exactly_summable(x, y)
        runs.append(dict(n=n_atoms, ref=ref_pieces(x, y), dx=gram.x(x, F, extra_rows=16), dy=gram.y(y),
                         dz=torch.from_numpy(z).to(gram.dev), out=gram.out(F)))
    torch.cuda.synchronize(gram.dev)
    prev = ctx.set_stream(sa.cuda_stream)
    try:
        for r, s in zip(runs, (sa, sb)):
            ctx.set_stream(s.cuda_stream)
            ctx.check(ctx.lib.uf3_gram_force_rows_dev(db.handle, C.c_void_p(r["dx"].data_ptr()), C.c_void_p(r["dy"].data_ptr()),
                                                      C.c_void_p(r["dz"].data_ptr()), r["n"], F, 0, C.c_void_p(r["out"][0].data_ptr()),
                                                      C.c_void_p(r["out"][1].data_ptr())))
    finally:
        ctx.restore_stream(prev)
    sa.synchronize()
    sb.synchronize()
    assert [d["kernel"] for d in dbg.grams()] == ["tiled_sub"] * 4
    for r in runs:
        assert np.array_equal(r["out"][0].cpu().numpy(), r["ref"][0]) and np.array_equal(r["out"][1].cpu().numpy(), r["ref"][1])


# ------------------------------------------------------------------------------------------------
# real rows against the error bound of an fp64 sum
# ------------------------------------------------------------------------------------------------
def check_against_bounds(label, x, y, g, o):
    """Every entry: |G - G_np| <= 2 gamma_n (|X|^T |X|)_ij.  The diagonal, all of X^T y and 2 000 sampled off-diagonal
    entries: |G - G_ld| <= gamma_n (|X|^T |X|)_ij, G_ld the column dot product in long double.  Returns the largest ratio."""
    n = x.shape[0]
    u = 2.0 ** -53
    gamma = n * u / (1 - n * u)
    ax = np.abs(x)
    bound = gamma * (ax.T @ ax)
    bound_o = gamma * (ax.T @ np.abs(y))
    g_np, o_np = x.T @ x, x.T @ y
    assert np.all(np.abs(g - g_np) <= 2 * bound), label
    assert np.all(np.abs(o - o_np) <= 2 * bound_o), label
    F = x.shape[1]
    rng = np.random.default_rng(F)
    ii, jj = rng.integers(0, F, 2000), rng.integers(0, F, 2000)
    pick = ii != jj
    ii, jj = np.concatenate([np.arange(F), ii[pick]]), np.concatenate([np.arange(F), jj[pick]])
    xt, yl = np.ascontiguousarray(x.T), y.astype(np.longdouble)
    cols = {c: xt[c].astype(np.longdouble) for c in np.unique(np.concatenate([ii, jj]))}
    g_ld = np.array([np.dot(cols[i], cols[j]) for i, j in zip(ii, jj)])
    o_ld = np.array([np.dot(cols[c], yl) if c in cols else np.dot(xt[c].astype(np.longdouble), yl) for c in range(F)])
    err = np.abs(g[ii, jj].astype(np.longdouble) - g_ld)
    err_o = np.abs(o.astype(np.longdouble) - o_ld)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = max(np.nanmax(np.where(bound[ii, jj] > 0, err / bound[ii, jj], 0.0)),
                    np.nanmax(np.where(bound_o > 0, err_o / bound_o, 0.0)))
    assert np.all(err <= bound[ii, jj]), label
    assert np.all(err_o <= bound_o), label
    print(f"{label}: n = {n}, F = {F}, largest |G - G_ld| / (gamma_n |X|^T|X|) = {float(ratio):.3g}")
    return float(ratio)


def test_c4_binary_force_rows_within_the_fp64_bound(dbg, gram):
    """Featurised W/Mo frames (F = 434): five frames, 150 000 force rows through the per-species route, and one frame through
    the direct kernel."""
    basis = dbg.basis(synthetic.notebook_basis(['Mo', 'W']))
    fz = process.BasisFeaturizer(basis)
    ctx, db = fz._dev()
    F = basis.n_feats
    frames = [synthetic.config_c4(frame=k)[0] for k in range(5)]
    _, x_f, _ = fz.featurize_frames(frames, energy=False, forces=True)
    dbg.grams()
    x = x_f.reshape(-1, F)
    del x_f
    n_atoms = x.shape[0] // 3
    y = np.random.default_rng(1).normal(size=3 * n_atoms)
    z = np.concatenate([f.get_atomic_numbers() for f in frames]).astype(np.int32)
    ld = odd_ld(F)
    g, o = gram.out(F)
    gram.force_rows(db, gram.x(x, ld), gram.y(y), gram.torch.from_numpy(z).to(gram.dev), n_atoms, ld, 0, g, o)
    assert [d["kernel"] for d in dbg.grams()] == ["tiled_sub"] * 2
    check_against_bounds("c4 x 5, per-species tiled", x, y, g.cpu().numpy(), o.cpu().numpy())
    n1 = 30000
    g, o = gram.out(F)
    gram.run(gram.x(x[:n1], ld), gram.y(y[:n1]), n1, F, ld, 0, g, o)
    one_launch(dbg, "mfma")
    check_against_bounds("c4 x 1, mfma", x[:n1], y[:n1], g.cpu().numpy(), o.cpu().numpy())


def test_lead0_force_rows_within_the_fp64_bound(dbg, gram):
    """The lead-0 basis (F = 1798, 29 column ranges) through the tiled kernel."""
    basis = dbg.basis(synthetic.notebook_basis(['Mo', 'W'], lead3=0))
    fz = process.BasisFeaturizer(basis)
    F = basis.n_feats
    assert F == 1798
    frames = [synthetic.lattice_frame("bcc", (10, 15, 15), 3.165, [42, 74], seed=3100 + k) for k in range(5)]
    _, x_f, _ = fz.featurize_frames(frames, energy=False, forces=True)
    dbg.grams()
    x = x_f.reshape(-1, F)
    del x_f
    n = x.shape[0]
    assert n >= 65536
    y = np.random.default_rng(2).normal(size=n)
    ld = odd_ld(F)
    g, o = gram.out(F)
    gram.run(gram.x(x, ld), gram.y(y), n, F, ld, 0, g, o)
    one_launch(dbg, "tiled")
    check_against_bounds("lead0, tiled", x, y, g.cpu().numpy(), o.cpu().numpy())


def test_energy_rows_within_the_fp64_bound(dbg, gram):
    """Energy rows of the one-species W basis (F = 73) over 16 400 small frames: the slab kernel."""
    basis = dbg.basis(synthetic.notebook_basis(['W']))
    fz = process.BasisFeaturizer(basis)
    F = basis.n_feats
    frames = [synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=7000 + k) for k in range(16400)]
    x, _, _ = fz.featurize_frames(frames, energy=True, forces=False)
    dbg.grams()
    n = x.shape[0]
    y = np.random.default_rng(3).normal(size=n)
    ld = odd_ld(F)
    g, o = gram.out(F)
    gram.run(gram.x(x, ld), gram.y(y), n, F, ld, 0, g, o)
    one_launch(dbg, "small")
    check_against_bounds("W energy rows, small", x, y, g.cpu().numpy(), o.cpu().numpy())


# ------------------------------------------------------------------------------------------------
# the fit's chunk plan on the device
# ------------------------------------------------------------------------------------------------
def test_native_fit_follows_the_host_plan_on_uneven_frames(dbg):
    """Frames of 40 / 70 atoms at a limit of 100 (no even spread fits): NativeFitAccumulator makes the chunks
    uf3_fit_plan_debug reports, and its pieces equal DeviceFitAccumulator's."""
    from uf3_amd import pipeline
    from uf3_amd.regression import least_squares as ls
    basis = dbg.basis(synthetic.notebook_basis(['W']))
    frames = []
    for k in range(8):
        reps = (2, 2, 5) if k % 2 == 0 else (1, 5, 7)
        frames.append(synthetic.lattice_frame("bcc", reps, 3.165, [74], seed=800 + k))
    counts = np.array([len(f) for f in frames], dtype=np.int64)
    assert list(counts[:4]) == [40, 70, 40, 70]
    rng = np.random.default_rng(8)
    energies = rng.normal(size=len(frames))
    forces = [rng.normal(size=(len(f), 3)) for f in frames]
    lib = _lib.load()
    ends, n = np.zeros(len(frames), dtype=np.int32), C.c_int32()
    assert lib.uf3_fit_plan_debug(len(frames), _lib._p(counts), 100, 1.0, _lib._p(ends), C.byref(n)) == 0
    starts = np.concatenate([[0], ends[:n.value - 1]])
    assert all(counts[s:e].sum() <= 100 or e - s == 1 for s, e in zip(starts, ends[:n.value]))
    model = ls.WeightedLinearModel(basis)
    fz = process.BasisFeaturizer(basis)
    native = pipeline.NativeFitAccumulator(model, fz, max_atoms_per_chunk=100)
    native.ctx.check(native.ctx.lib.uf3_fit_first_chunk(native.handle, 1.0))
    native.add_frames(frames, energies, forces)
    assert native.n_chunks == n.value
    device = pipeline.DeviceFitAccumulator(model, fz, max_atoms_per_chunk=100, first_chunk_fraction=1.0)
    device.add_frames(frames, energies, forces)
    assert device.n_chunks == n.value
    a, b = native.pieces(), device.pieces()
    for key in a:
        assert np.allclose(a[key], b[key], rtol=1e-12, atol=1e-12 * max(1.0, np.abs(b[key]).max())), key
