/*
 * uf3_oracle.c -- CPU restatement of the UF3 hot path.  TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * this library; it is the checker, never the product.  The product path is the
 * HIP library under uf3_amd/csrc and fails loudly when that library is missing.
 *
 * What is restated (plain C, fp64, single thread), with the reference lines
 * (/root/reference, uf3 v0.4.0) each function follows:
 *
 *   supercell tiling and ghost indexing      uf3/data/geometry.py:14-149
 *   2-body distances / energy features       uf3/representation/distances.py:19-75
 *                                            uf3/representation/bspline.py:810-849
 *   2-body force features                    distances.py:78-143,331-364; bspline.py:852-895
 *   3-body neighbour pairs                   uf3/representation/angles.py:289-346
 *   triplet enumeration, species sort, masks angles.py:424-514
 *   per-leg basis values / derivatives       angles.py:517-632; bspline.py:950-974
 *   4x4x4 scatter (energy, forces)           angles.py:104-139, 235-286, 142-232
 *   symmetry fold + template mask            bspline.py:664-690
 *   energy / force evaluation of a model     uf3/forcefield/calculator.py:183-343
 *
 * The reference evaluates basis functions through scipy.interpolate.BSpline
 * (basis_element, extrapolate=False, NaN -> 0) and, in the calculator, through
 * ndsplines.NDSpline; neither is vendored in the reference tree.  Here every
 * basis element is evaluated from the Cox-de Boor recursion on its own five
 * knots (0/0 := 0, half-open knot intervals [t_i, t_{i+1}); like scipy's basis_element the
 * value at the element's own last knot is 0, also at the 4-fold end knot).
 *
 * Deliberately kept close to the reference's formulation (explicit supercell,
 * ghost-centre loop for 3-body forces) so that it is independent of the product,
 * which uses periodic neighbour lists with image shifts and a per-atom gather.
 * The one liberty: candidate pairs come from a uniform grid over the supercell
 * instead of a dense cdist matrix; the accepted pairs and their order (row-major
 * over (i, j) supercell indices) are identical.
 *
 * Pinned against: tests/golden/rattled_steel_features.json (reference's own
 * golden), the literal H2O / CH4 vectors and calculator energies/forces of the
 * reference's tests, and captures made by importing the reference in the build
 * container (tests/golden/make_golden.py).  See tests/test_oracle_golden.py.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/*
 * One source, two builds (oracle/Makefile).  `real` is the type of every VALUE: differences of positions and knots, norms,
 * Cox-de Boor, direction cosines, products, accumulators.  libuf3oracle.so is built with real = double and is the oracle of
 * the parity tests; libuf3oracle_x.so is built with -DUF3O_REAL='long double' (64-bit mantissa) and is what
 * tests/_precision.py measures both the fp64 build and the kernels against.  Every DECISION -- cut-offs, the 3-body list range,
 * leg masks, strict support masks, the half-open knot intervals of the recursion, searchsorted -- is taken on the fp64 distance
 * by the expressions of the fp64 build, in both builds, so that both sum the same terms.  The inputs of both are the same
 * doubles: the tiled supercell positions as build_supercell rounds them, the knots, the coefficients.
 *
 * The *_x entries return, beside every output entry, a magnitude M (double): a first-order running error bound,
 *
 *     M = sum over the entry's terms t of ( |t|_abs + sum over the term's distances r of rho_r |dt/dr|_abs ),
 *
 * where |.|_abs replaces every subtraction inside a term by the sum of the absolute values of its operands (the two summands
 * of a derivative element, the three products of a 3-body force term, |cos|, |coefficient|), and the second part is the term's
 * sensitivity to a relative rounding of its distances: rho_r = r for a pair distance and for the two centre legs of a triplet,
 * rho_r = r_ij + r_ik for the third leg (any fp64 formulation of r_jk -- a difference of tiled positions rounded at
 * |p + offset|, or of centre-relative vectors -- inherits roundings of the order of the lengths it is formed from).  A result
 * computed in fp64 is expected within a modest multiple of 2^-53 M of the exact value: tests/_precision.py.
 */
#ifndef UF3O_REAL
#define UF3O_REAL double
#endif
typedef UF3O_REAL real;
_Static_assert(sizeof(real) == sizeof(double) || LDBL_MANT_DIG >= 64, "the extended build needs a 64-bit mantissa");
#define rsqrt_(x) _Generic((real)0, long double: sqrtl, default: sqrt)(x)
#define rabs(x) _Generic((real)0, long double: fabsl, default: fabs)(x)

/* mantissa bits of `real` in this build (53 in libuf3oracle.so; LDBL_MANT_DIG in libuf3oracle_x.so) */
int uf3o_real_mant_dig(void) { return sizeof(real) == sizeof(double) ? DBL_MANT_DIG : LDBL_MANT_DIG; }

typedef struct {
    int n_species;            /* S, ascending Z */
    const int *species_z;     /* [S] */
    int n_pairs;              /* pair blocks in column order */
    const int *pair_z;        /* [P][2] atomic numbers, pair_z[p][0] <= pair_z[p][1] */
    const int *pair_nk;       /* [P] knots per pair */
    const double *pair_knots; /* concatenated */
    const double *pair_rmin;  /* [P] r_min_map (raw) */
    const double *pair_rmax;  /* [P] */
    const int *pair_col;      /* [P] column offset of block */
    int lead2, trail2, lead3, trail3;
    int n_trios;
    const int *trio_z;        /* [T][3] centre, n1 <= n2 */
    const int *trio_nk;       /* [T][3] */
    const double *trio_knots; /* concatenated l, m, n per trio */
    const int *trio_sym;      /* [T] 1, 2, 3 */
    const int *trio_col;      /* [T] column offset */
    const int *trio_ncol;     /* [T] compressed size */
    const int64_t *trio_mask; /* concatenated template_mask */
    const double *trio_w;     /* concatenated flat_weights */
    int n_feat;               /* F (1-body columns included) */
    double r_cut;             /* supercell radius (BSplineBasis.r_cut) */
} uf3o_spec;

typedef struct {
    int n_atoms;
    const double *pos;  /* [N][3] */
    const int *z;       /* [N] */
    const double *cell; /* [3][3] rows = lattice vectors */
    const int *pbc;     /* [3] */
} uf3o_frame;

/* ---------------------------------------------------------------- supercell */
typedef struct {
    int n_img, n_atoms, m;     /* m = n_img * n_atoms */
    int fac[3], cnt[3];
    int *shift;                /* [n_img][3] */
    double *pos;               /* [m][3] */
    int *z;                    /* [m] */
} supercell_t;

static void cross3(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
static double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* geometry.py:54-83: ceil(r_cut / |projection of a_i on the normal of the other two|) */
static void supercell_factors(const double *cell, double r_cut, int *fac) {
    int all_zero = 1, any_zero_vec = 0;
    for (int i = 0; i < 9; i++) if (cell[i] != 0.0) all_zero = 0;
    for (int i = 0; i < 3; i++) if (sqrt(dot3(cell + 3 * i, cell + 3 * i)) == 0.0) any_zero_vec = 1;
    if (all_zero || any_zero_vec) { fac[0] = fac[1] = fac[2] = 1; return; }
    const double *a = cell, *b = cell + 3, *c = cell + 6;
    double n[3][3];
    cross3(b, c, n[0]); cross3(a, c, n[1]); cross3(a, b, n[2]);
    for (int i = 0; i < 3; i++) {
        const double *v = cell + 3 * i;
        double s = dot3(v, n[i]) / dot3(n[i], n[i]);
        double p[3] = {n[i][0] * s, n[i][1] * s, n[i][2] * s};
        fac[i] = (int)ceil(r_cut / sqrt(dot3(p, p)));
    }
}

/* k-th entry of the per-axis image list 0, +1, -1, +2, -2, ... (geometry.py:131-138) */
static int axis_image(int k) { return (k == 0) ? 0 : ((k & 1) ? (k + 1) / 2 : -(k / 2)); }

static void build_supercell(const uf3o_frame *f, double r_cut, supercell_t *sc) {
    int any_pbc = f->pbc[0] || f->pbc[1] || f->pbc[2];
    sc->n_atoms = f->n_atoms;
    if (!any_pbc) { sc->fac[0] = sc->fac[1] = sc->fac[2] = 0; }
    else supercell_factors(f->cell, r_cut, sc->fac);
    for (int d = 0; d < 3; d++) sc->cnt[d] = (any_pbc && f->pbc[d]) ? 2 * sc->fac[d] + 1 : 1;
    sc->n_img = sc->cnt[0] * sc->cnt[1] * sc->cnt[2];
    sc->m = sc->n_img * f->n_atoms;
    sc->shift = (int *)malloc(sizeof(int) * 3 * (size_t)sc->n_img);
    sc->pos = (double *)malloc(sizeof(double) * 3 * (size_t)sc->m);
    sc->z = (int *)malloc(sizeof(int) * (size_t)sc->m);
    int img = 0;
    /* meshgrid(xy) flatten: b slowest, a middle, c fastest (geometry.py:108-114) */
    for (int ib = 0; ib < sc->cnt[1]; ib++)
        for (int ia = 0; ia < sc->cnt[0]; ia++)
            for (int ic = 0; ic < sc->cnt[2]; ic++, img++) {
                int s[3] = {axis_image(ia), axis_image(ib), axis_image(ic)};
                memcpy(sc->shift + 3 * img, s, sizeof(s));
                double off[3];
                for (int k = 0; k < 3; k++)
                    off[k] = s[0] * f->cell[k] + s[1] * f->cell[3 + k] + s[2] * f->cell[6 + k];
                for (int a = 0; a < f->n_atoms; a++) {
                    size_t j = (size_t)img * f->n_atoms + a;
                    for (int k = 0; k < 3; k++) sc->pos[3 * j + k] = f->pos[3 * a + k] + off[k];
                    sc->z[j] = f->z[a];
                }
            }
}
static void free_supercell(supercell_t *sc) { free(sc->shift); free(sc->pos); free(sc->z); }

/* ------------------------------------------------- uniform grid over supercell */
typedef struct {
    double lo[3], inv;
    int n[3];
    int *start;   /* [nbins+1] */
    int *items;   /* supercell indices, ascending within a bin */
} grid_t;

static void build_grid(const supercell_t *sc, double h, grid_t *g) {
    double hi[3] = {-1e300, -1e300, -1e300};
    g->lo[0] = g->lo[1] = g->lo[2] = 1e300;
    for (int j = 0; j < sc->m; j++)
        for (int k = 0; k < 3; k++) {
            double v = sc->pos[3 * (size_t)j + k];
            if (v < g->lo[k]) g->lo[k] = v;
            if (v > hi[k]) hi[k] = v;
        }
    if (h <= 0) h = 1.0;
    g->inv = 1.0 / h;
    size_t nb = 1;
    for (int k = 0; k < 3; k++) {
        g->n[k] = (int)floor((hi[k] - g->lo[k]) * g->inv) + 1;
        if (g->n[k] < 1) g->n[k] = 1;
        nb *= (size_t)g->n[k];
    }
    g->start = (int *)calloc(nb + 1, sizeof(int));
    g->items = (int *)malloc(sizeof(int) * (size_t)(sc->m > 0 ? sc->m : 1));
    int *bin = (int *)malloc(sizeof(int) * (size_t)(sc->m > 0 ? sc->m : 1));
    for (int j = 0; j < sc->m; j++) {
        int c[3];
        for (int k = 0; k < 3; k++) {
            c[k] = (int)floor((sc->pos[3 * (size_t)j + k] - g->lo[k]) * g->inv);
            if (c[k] < 0) c[k] = 0;
            if (c[k] >= g->n[k]) c[k] = g->n[k] - 1;
        }
        bin[j] = (c[0] * g->n[1] + c[1]) * g->n[2] + c[2];
        g->start[bin[j] + 1]++;
    }
    for (size_t b = 0; b < nb; b++) g->start[b + 1] += g->start[b];
    int *fill = (int *)malloc(sizeof(int) * nb);
    for (size_t b = 0; b < nb; b++) fill[b] = g->start[b];
    for (int j = 0; j < sc->m; j++) g->items[fill[bin[j]]++] = j;
    free(fill); free(bin);
}
static void free_grid(grid_t *g) { free(g->start); free(g->items); }

static int cmp_int(const void *a, const void *b) { return (*(const int *)a > *(const int *)b) - (*(const int *)a < *(const int *)b); }

/* all supercell atoms within the 27 bins around x, ascending index (np.where order) */
static int gather_candidates(const supercell_t *sc, const grid_t *g, const double *x, int **buf, int *cap) {
    int c[3], n = 0;
    for (int k = 0; k < 3; k++) {
        c[k] = (int)floor((x[k] - g->lo[k]) * g->inv);
        if (c[k] < 0) c[k] = 0;
        if (c[k] >= g->n[k]) c[k] = g->n[k] - 1;
    }
    for (int a = c[0] - 1; a <= c[0] + 1; a++) {
        if (a < 0 || a >= g->n[0]) continue;
        for (int b = c[1] - 1; b <= c[1] + 1; b++) {
            if (b < 0 || b >= g->n[1]) continue;
            for (int d = c[2] - 1; d <= c[2] + 1; d++) {
                if (d < 0 || d >= g->n[2]) continue;
                int bi = (a * g->n[1] + b) * g->n[2] + d;
                for (int t = g->start[bi]; t < g->start[bi + 1]; t++) {
                    if (n == *cap) { *cap = *cap ? *cap * 2 : 256; *buf = (int *)realloc(*buf, sizeof(int) * (size_t)*cap); }
                    (*buf)[n++] = g->items[t];
                }
            }
        }
    }
    (void)sc;
    qsort(*buf, (size_t)n, sizeof(int), cmp_int);
    return n;
}

static double dist3(const double *a, const double *b) {
    double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}
/* the same distance as a VALUE: from the same doubles, in `real` (dist3 itself where real is double) */
static real rdist3(const double *a, const double *b) {
    real d0 = (real)a[0] - b[0], d1 = (real)a[1] - b[1], d2 = (real)a[2] - b[2];
    return rsqrt_(d0 * d0 + d1 * d1 + d2 * d2);
}

/* ------------------------------------------------------------ basis elements */
/* Cox-de Boor on the element's own knots t[0..4]; degree k basis starting at knot s */
/* (xd: the fp64 distance, which picks the knot interval; x: the distance as a value) */
static real bspl(const double *t, int s, int k, double xd, real x) {
    if (k == 0) return (t[s] <= xd && xd < t[s + 1]) ? 1.0 : 0.0;
    real a = 0.0, b = 0.0, d1 = (real)t[s + k] - t[s], d2 = (real)t[s + k + 1] - t[s + 1];
    if (d1 > 0) a = (x - t[s]) / d1 * bspl(t, s, k - 1, xd, x);
    if (d2 > 0) b = (t[s + k + 1] - x) / d2 * bspl(t, s + 1, k - 1, xd, x);
    return a + b;
}
/* value (nu=0) or first derivative (nu=1) of the cubic element on knots t[0..4]; 0 outside [t0,t4] */
static real basis_element(const double *t, double xd, real x, int nu) {
    if (!(xd >= t[0] && xd <= t[4])) return 0.0;   /* extrapolate=False -> NaN -> 0 */
    if (nu == 0) return bspl(t, 0, 3, xd, x);
    real a = 0.0, b = 0.0, d1 = (real)t[3] - t[0], d2 = (real)t[4] - t[1];
    if (nu == 2) {      /* the recursion once more: the quadratic elements' derivatives from the linear elements */
        real qd[2];
        for (int s = 0; s < 2; s++) {
            real e1 = (real)t[s + 2] - t[s], e2 = (real)t[s + 3] - t[s + 1];
            qd[s] = (e1 > 0 ? 2.0 / e1 * bspl(t, s, 1, xd, x) : 0.0) - (e2 > 0 ? 2.0 / e2 * bspl(t, s + 1, 1, xd, x) : 0.0);
        }
        if (d1 > 0) a = 3.0 / d1 * qd[0];
        if (d2 > 0) b = 3.0 / d2 * qd[1];
        return a - b;
    }
    if (d1 > 0) a = 3.0 / d1 * bspl(t, 0, 2, xd, x);
    if (d2 > 0) b = 3.0 / d2 * bspl(t, 1, 2, xd, x);
    return a - b;
}
/* |B'''|_abs of the cubic element: the third derivative is constant on a knot interval (a step function), so this is the
   interval's own -- every subtraction of the recursion down to the degree-0 elements replaced by an addition */
static real basis_element_abs3(const double *t, double xd, real x) {
    if (!(xd >= t[0] && xd <= t[4])) return 0.0;
    real la[3], d3 = 0.0;
    for (int s = 0; s < 3; s++) {
        real g1 = (real)t[s + 1] - t[s], g2 = (real)t[s + 2] - t[s + 1];
        la[s] = (g1 > 0 ? bspl(t, s, 0, xd, x) / g1 : 0.0) + (g2 > 0 ? bspl(t, s + 1, 0, xd, x) / g2 : 0.0);
    }
    for (int s = 0; s < 2; s++) {
        real e1 = (real)t[s + 2] - t[s], e2 = (real)t[s + 3] - t[s + 1], c = (real)t[s + 3] - t[s];
        real qdd = (e1 > 0 ? 2.0 / e1 * la[s] : 0.0) + (e2 > 0 ? 2.0 / e2 * la[s + 1] : 0.0);
        if (c > 0) d3 += 3.0 / c * qdd;
    }
    return d3;
}
/* for the magnitudes: |B'|_abs (the derivative's two summands added, not subtracted) and |B''|_abs (likewise, down to the four
   linear elements) of the cubic element.  The value itself is a sum of non-negative products: |B|_abs = B. */
static void basis_element_abs(const double *t, double xd, real x, real *d1abs, real *d2abs) {
    *d1abs = *d2abs = 0.0;
    if (!(xd >= t[0] && xd <= t[4])) return;
    real lin[3], q[2], qd[2];
    for (int s = 0; s < 3; s++) lin[s] = bspl(t, s, 1, xd, x);
    for (int s = 0; s < 2; s++) {
        real e1 = (real)t[s + 2] - t[s], e2 = (real)t[s + 3] - t[s + 1];
        q[s] = bspl(t, s, 2, xd, x);
        qd[s] = (e1 > 0 ? 2.0 / e1 * lin[s] : 0.0) + (e2 > 0 ? 2.0 / e2 * lin[s + 1] : 0.0);
    }
    real c1 = (real)t[3] - t[0], c2 = (real)t[4] - t[1];
    if (c1 > 0) { *d1abs += 3.0 / c1 * q[0]; *d2abs += 3.0 / c1 * qd[0]; }
    if (c2 > 0) { *d1abs += 3.0 / c2 * q[1]; *d2abs += 3.0 / c2 * qd[1]; }
}
/* np.searchsorted(knots, x, side='left') */
static int searchsorted_left(const double *t, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) { int mid = (lo + hi) / 2; if (t[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

/*
 * The same three magnitudes for a leg function that is evaluated from its local cubic PIECE: the kernels that keep window rows
 * (k_featurize3 and the grouped matrix-core launch; uf3_hip.hip "window rows", uf3_feat3.h f3_eval) store, per knot interval
 * (t_i, t_i+1], the four coefficients of every function alive there in powers of u = x - t_i and run Horner's rule with fused
 * multiply-adds.  Horner's error is bounded by a small multiple of u_fp64 times  p~(u) = sum_k |c_k| u^k  (Higham, Accuracy and
 * Stability of Numerical Algorithms, section 5.1), NOT times |p(u)|: for the functions that decay on the interval the
 * coefficients alternate, p~ stays O(1) while p itself goes to 0 like (t_i+1 - x)^3, and the value carries an absolute error of
 * order u_fp64 however small it is.  (Cox-de Boor, a sum of non-negative products, has no such term: its |B|_abs is B.)  That
 * is inherent in the choice of pieces about the interval's lower knot, a documented design choice, so
 * for those routes the magnitudes are widened by the quantity the choice is sensitive to, which follows from the inputs alone
 * (knots and distance): m0 = p~(u), m1 = sum_k k |c_k| u^(k-1), m2 = sum_k k (k-1) |c_k| u^(k-2), each taken where it exceeds
 * the Cox-de Boor magnitude.  The coefficients come from the recursion itself, carried out on polynomials in u on the interval
 * that holds x.
 */
static void piece_abs(const double *t, double xd, real x, real *m0, real *m1, real *m2) {
    int m = -1;
    for (int s = 0; s < 4; s++) if (t[s] <= xd && xd < t[s + 1]) m = s;
    *m0 = *m1 = *m2 = 0.0;
    if (m < 0) return;
    real P[4][4] = {{0}};
    P[m][0] = 1.0;
    for (int k = 1; k <= 3; k++)
        for (int s = 0; s + k <= 3; s++) {
            real np[4] = {0}, d1 = (real)t[s + k] - t[s], d2 = (real)t[s + k + 1] - t[s + 1];
            for (int j = 0; j < 4; j++) {
                if (d1 > 0) { np[j] += ((real)t[m] - t[s]) / d1 * P[s][j]; if (j < 3) np[j + 1] += P[s][j] / d1; }
                if (d2 > 0) { np[j] += ((real)t[s + k + 1] - t[m]) / d2 * P[s + 1][j]; if (j < 3) np[j + 1] -= P[s + 1][j] / d2; }
            }
            for (int j = 0; j < 4; j++) P[s][j] = np[j];
        }
    real u = rabs(x - t[m]), c0 = rabs(P[0][0]), c1 = rabs(P[0][1]), c2 = rabs(P[0][2]), c3 = rabs(P[0][3]);
    *m0 = c0 + u * (c1 + u * (c2 + u * c3));
    *m1 = c1 + u * (2.0 * c2 + u * 3.0 * c3);
    *m2 = 2.0 * c2 + u * 6.0 * c3;
}

static int species_index(const uf3o_spec *s, int z) {
    for (int i = 0; i < s->n_species; i++) if (s->species_z[i] == z) return i;
    return -1;
}
static int pair_index(const uf3o_spec *s, int za, int zb) {
    if (za > zb) { int t = za; za = zb; zb = t; }
    for (int p = 0; p < s->n_pairs; p++) if (s->pair_z[2 * p] == za && s->pair_z[2 * p + 1] == zb) return p;
    return -1;
}
static int trio_index(const uf3o_spec *s, int zc, int za, int zb) {
    for (int t = 0; t < s->n_trios; t++)
        if (s->trio_z[3 * t] == zc && s->trio_z[3 * t + 1] == za && s->trio_z[3 * t + 2] == zb) return t;
    return -1;
}

/* Voigt order (xx, yy, zz, yz, xz, xy) */
static const int VOIGT[6][2] = {{0, 0}, {1, 1}, {2, 2}, {1, 2}, {0, 2}, {0, 1}};

/* feature rows of one frame: values and, beside a value, its magnitudes (any may be NULL) */
typedef struct {
    real *xe, *xf, *xv;       /* [F], [N][3][F], [6][F] */
    double *me, *mf, *mv;
    int pieces;               /* the 3-body magnitudes of a route that evaluates leg functions from local pieces: piece_abs */
    real *xb;                 /* [N][F] site rows: the energy row's terms credited to their centre (with xe and me) */
    double *mb;
    double sc_r;              /* supercell radius in place of the basis' r_cut (0: r_cut) */
} rows_t;

/* ------------------------------------------------------------------ 2-body */
/*
 * Energy row: sum over real i, supercell j of B_b(d) for the pair block of (Z_i, Z_j),
 * max(r_min,0) < d < r_max strict (distances.py:60-69), bases [lead, nb-trail).
 * Force rows: x[m,c,b] = -sum_p B'_b(r_p) (delta_mj - delta_mi)(R_j-R_i)_c / r_p over directed
 * supercell pairs with a real end (distances.py:116-141, bspline.py:877-895).  A (ghost x, real y)
 * pair is the periodic image of the (real y', ghost x') pair seen from y, so both delta terms of
 * atom m are collected while visiting m's own neighbours.
 * Strain rows (no counterpart in the reference; the convention of eval_worker's virial6): the derivative of the energy row,
 * sum over the same directed pairs of B'_b(d) r_a r_b / d.
 * Magnitudes: a term B'(d) w with a weight w of degree 0 or 1 in the bond vector (a cosine, r_a r_b / d) has
 * |t|_abs = |B'|_abs |w| and d |dt/dd|_abs = d |B''|_abs |w| + |B'|_abs |w|.
 * Optional dump: per pair block, (i, j) supercell indices in np.where order.
 */
static void two_body(const uf3o_spec *s, const supercell_t *sc, const grid_t *g, const rows_t *o,
                     int64_t *pair_cnt, int64_t *pair_ij, int64_t pair_cap) {
    int *cand = NULL, cap = 0, N = sc->n_atoms, F = s->n_feat;
    real *xe = o->xe, *xf = o->xf, *xv = o->xv;
    int want_m = o->me || o->mf || o->mv;
    const double **knots = (const double **)malloc(sizeof(double *) * (size_t)(s->n_pairs + 1));
    const double *kp = s->pair_knots;
    for (int p = 0; p < s->n_pairs; p++) { knots[p] = kp; kp += s->pair_nk[p]; }
    if (pair_cnt) memset(pair_cnt, 0, sizeof(int64_t) * (size_t)s->n_pairs);
    for (int i = 0; i < N; i++) {
        const double *ri = sc->pos + 3 * (size_t)i;
        int nc = gather_candidates(sc, g, ri, &cand, &cap);
        for (int c = 0; c < nc; c++) {
            int j = cand[c];
            int p = pair_index(s, sc->z[i], sc->z[j]);
            if (p < 0) continue;
            const double *rj = sc->pos + 3 * (size_t)j;
            double d = dist3(ri, rj);
            double rmin = s->pair_rmin[p] > 0 ? s->pair_rmin[p] : 0.0;
            if (!(d > rmin && d < s->pair_rmax[p])) continue;
            if (pair_cnt) {
                if (pair_ij && pair_cnt[p] < pair_cap) {
                    pair_ij[2 * ((size_t)p * pair_cap + pair_cnt[p])] = i;
                    pair_ij[2 * ((size_t)p * pair_cap + pair_cnt[p]) + 1] = j;
                }
                pair_cnt[p]++;
            }
            real dr = rdist3(ri, rj);
            int nb = s->pair_nk[p] - 4;
            for (int b = o->xb ? 0 : s->lead2; b < (o->xb ? nb : nb - s->trail2); b++) {
                const double *t = knots[p] + b;
                real a1 = 0.0, a2 = 0.0;
                if (want_m) basis_element_abs(t, d, dr, &a1, &a2);
                if (b < s->lead2 || b >= nb - s->trail2) {
                    /* a trimmed pair function: no entry of the energy row, but a column of the site row, which holds
                       b_i . c = U_i for EVERY coefficient vector and the evaluator takes all pair coefficients (uf3_site_rows.h) */
                    real val = basis_element(t, d, dr, 0);
                    o->xb[(size_t)i * F + s->pair_col[p] + b] += val;
                    o->mb[(size_t)i * F + s->pair_col[p] + b] += (double)(val + dr * a1);
                    continue;
                }
                if (xe) {
                    real val = basis_element(t, d, dr, 0);
                    xe[s->pair_col[p] + b] += val;
                    if (o->me) o->me[s->pair_col[p] + b] += (double)(val + dr * a1);
                    if (o->xb) {
                        o->xb[(size_t)i * F + s->pair_col[p] + b] += val;
                        o->mb[(size_t)i * F + s->pair_col[p] + b] += (double)(val + dr * a1);
                    }
                }
                if ((xf || xv) && d > t[0] && d < t[4]) {           /* strict support mask, bspline.py:884 */
                    real dv = basis_element(t, d, dr, 1);
                    real gm = 2.0 * a1 + dr * a2;
                    if (xf) for (int k = 0; k < 3; k++) {
                        real cosk = ((real)rj[k] - ri[k]) / dr;
                        /* pair (i,j): m=i term  -B'*(-1)*cos ; mirrored pair (j',i): m=i term -B'*(+1)*(-cos) */
                        real *dst = xf + ((size_t)i * 3 + k) * F + s->pair_col[p] + b;
                        *dst += dv * cosk;
                        *dst += dv * cosk;
                        if (o->mf) o->mf[((size_t)i * 3 + k) * F + s->pair_col[p] + b] += (double)(2.0 * gm * rabs(cosk));
                    }
                    if (xv) for (int v = 0; v < 6; v++) {
                        real da = (real)rj[VOIGT[v][0]] - ri[VOIGT[v][0]], db = (real)rj[VOIGT[v][1]] - ri[VOIGT[v][1]];
                        xv[(size_t)v * F + s->pair_col[p] + b] += dv * da * db / dr;
                        if (o->mv) o->mv[(size_t)v * F + s->pair_col[p] + b] += (double)(gm * rabs(da * db) / dr);
                    }
                }
            }
        }
    }
    free(cand); free((void *)knots);
}

/* ------------------------------------------------------------------ 3-body */
typedef struct {
    const double *k[3];
    int nk[3], dim[3];
    const int64_t *mask;
    const double *w;
    int *inv_start;   /* [L*M*N+1] raw bin -> range in inv_col */
    int *inv_col;     /* compressed columns fed by the raw bin (with multiplicity) */
} trio_view;

/* images of (l,m,n) summed by compress_3B (bspline.py:674-687) */
static int sym_images(int sym, int l, int m, int n, int M, int N, int64_t *out) {
#define U(a, b, c) (((int64_t)(a) * M + (b)) * N + (c))
    if (sym == 1) { out[0] = U(l, m, n); return 1; }
    if (sym == 2) { out[0] = U(l, m, n); out[1] = U(m, l, n); return 2; }
    out[0] = U(l, m, n); out[1] = U(l, n, m); out[2] = U(m, l, n);
    out[3] = U(n, l, m); out[4] = U(m, n, l); out[5] = U(n, m, l);
    return 6;
#undef U
}

static void free_trio_views(const uf3o_spec *s, trio_view *v) {
    for (int t = 0; t < s->n_trios; t++) { free(v[t].inv_start); free(v[t].inv_col); }
    free(v);
}

static void trio_views(const uf3o_spec *s, trio_view *v, double *rmin3, double *rmax3) {
    const double *kp = s->trio_knots;
    const int64_t *mp = s->trio_mask;
    const double *wp = s->trio_w;
    double lo = 1e300, hi = -1e300;
    for (int t = 0; t < s->n_trios; t++) {
        for (int d = 0; d < 3; d++) {
            v[t].k[d] = kp; v[t].nk[d] = s->trio_nk[3 * t + d]; v[t].dim[d] = v[t].nk[d] - 4;
            for (int q = 0; q < v[t].nk[d]; q++) {
                if (kp[q] < lo) lo = kp[q];
                if (d < 2 && kp[q] > hi) hi = kp[q];   /* first two legs only, angles.py:322-325 */
            }
            kp += v[t].nk[d];
        }
        v[t].mask = mp; v[t].w = wp;
        /* invert "column c = sum of grid over the symmetry images of its bin" */
        int M = v[t].dim[1], N = v[t].dim[2];
        size_t sz = (size_t)v[t].dim[0] * M * N;
        v[t].inv_start = (int *)calloc(sz + 1, sizeof(int));
        v[t].inv_col = (int *)malloc(sizeof(int) * 6 * (size_t)(s->trio_ncol[t] + 1));
        for (int rep = 0; rep < 2; rep++) {
            int *fill = rep ? (int *)malloc(sizeof(int) * (sz + 1)) : NULL;
            if (rep) { for (size_t u = sz; u > 0; u--) v[t].inv_start[u] = v[t].inv_start[u - 1]; v[t].inv_start[0] = 0;
                       for (size_t u = 0; u < sz; u++) v[t].inv_start[u + 1] += v[t].inv_start[u];
                       memcpy(fill, v[t].inv_start, sizeof(int) * (sz + 1)); }
            for (int c = 0; c < s->trio_ncol[t]; c++) {
                int64_t u = mp[c], img[6];
                int l = (int)(u / ((int64_t)M * N)), m = (int)((u / N) % M), n = (int)(u % N);
                int ni = sym_images(s->trio_sym[t], l, m, n, M, N, img);
                for (int q = 0; q < ni; q++) {
                    if (!rep) v[t].inv_start[img[q]]++;
                    else v[t].inv_col[fill[img[q]]++] = c;
                }
            }
            free(fill);
        }
        mp += s->trio_ncol[t]; wp += s->trio_ncol[t];
    }
    *rmin3 = lo > 0 ? lo : 0.0;
    *rmax3 = hi;
}

/* the four candidate bases of one leg at r: values, derivatives and, for the magnitudes, |B'|_abs and |B''|_abs */
typedef struct { real v[4], d[4], a1[4], a2[4], m0[4], m1[4], m2[4];              /* m: v, a1, a2, or widened (piece_abs) */
                 real dd[4], a3[4]; } leg_t;                                     /* der = 2: B'' and (with mag) |B'''|_abs */

/* values (and derivatives) of the four candidate bases of leg `d` at r (angles.py:545-566, 607-630); rd: the fp64 distance;
   mag: 0 no magnitudes, 1 Cox-de Boor's (m0 = the value), 2 widened to those of the local piece */
static int leg_values(const trio_view *v, int d, double rd, real r, int lead, int trail, leg_t *g, int der, int mag) {
    int first = searchsorted_left(v->k[d], v->nk[d], rd) - 4;
    for (int a = 0; a < 4; a++) {
        int b = first + a;
        g->v[a] = 0.0; g->d[a] = 0.0; g->a1[a] = 0.0; g->a2[a] = 0.0; g->m0[a] = 0.0; g->m1[a] = 0.0; g->m2[a] = 0.0;
        g->dd[a] = 0.0; g->a3[a] = 0.0;
        if (b < lead || b >= v->dim[d] - trail) continue;   /* trimmed, or wrapped negative index */
        g->v[a] = basis_element(v->k[d] + b, rd, r, 0);
        if (der) g->d[a] = basis_element(v->k[d] + b, rd, r, 1);
        if (der == 2) { g->dd[a] = basis_element(v->k[d] + b, rd, r, 2); if (mag) g->a3[a] = basis_element_abs3(v->k[d] + b, rd, r); }
        if (mag) {
            basis_element_abs(v->k[d] + b, rd, r, &g->a1[a], &g->a2[a]);
            g->m0[a] = g->v[a]; g->m1[a] = g->a1[a]; g->m2[a] = g->a2[a];
        }
        if (mag == 2) {
            real p0, p1, p2;
            piece_abs(v->k[d] + b, rd, r, &p0, &p1, &p2);
            if (p0 > g->m0[a]) g->m0[a] = p0;
            if (p1 > g->m1[a]) g->m1[a] = p1;
            if (p2 > g->m2[a]) g->m2[a] = p2;
        }
    }
    return first;
}

/*
 * Magnitudes of one product of three leg functions, times |c|: q[0] the value, q[1..3] the three first partials, q[4..9] the
 * second partials 00, 01, 02, 11, 12, 22 -- each with |B'|_abs, |B''|_abs in place of B', B''.
 */
/* magnitude of a product of three factors of magnitudes a, b, c whose error magnitudes are ma >= a, mb >= b, mc >= c: to first
   order one factor's excess at a time (a b c itself where nothing is widened) */
static real wprod(real a, real ma, real b, real mb, real c, real mc) {
    return a * b * c + (ma - a) * b * c + a * (mb - b) * c + a * b * (mc - c);
}
static void q_add_n(real *q, real c, const leg_t *l, const leg_t *m, const leg_t *n, int x, int y, int w, int nq) {
#define F0(g, i) g->v[i], g->m0[i]
#define F1(g, i) g->a1[i], g->m1[i]
#define F2(g, i) g->a2[i], g->m2[i]
    q[0] += c * wprod(F0(l, x), F0(m, y), F0(n, w));
    q[1] += c * wprod(F1(l, x), F0(m, y), F0(n, w));
    q[2] += c * wprod(F0(l, x), F1(m, y), F0(n, w));
    q[3] += c * wprod(F0(l, x), F0(m, y), F1(n, w));
    if (nq <= 4) return;                  /* (a caller that takes mag_value alone: the value and the three first partials) */
    q[4] += c * wprod(F2(l, x), F0(m, y), F0(n, w));
    q[5] += c * wprod(F1(l, x), F1(m, y), F0(n, w));
    q[6] += c * wprod(F1(l, x), F0(m, y), F1(n, w));
    q[7] += c * wprod(F0(l, x), F2(m, y), F0(n, w));
    q[8] += c * wprod(F0(l, x), F1(m, y), F1(n, w));
    q[9] += c * wprod(F0(l, x), F0(m, y), F2(n, w));
#undef F0
#undef F1
#undef F2
}
static void q_add(real *q, real c, const leg_t *l, const leg_t *m, const leg_t *n, int x, int y, int w) {
    q_add_n(q, c, l, m, n, x, y, w, 10);
}
/* M of an energy term V(r_ij, r_ik, r_jk): |V|_abs + sum_legs rho_leg |dV/dr_leg|_abs, rho = (r_ij, r_ik, r_ij + r_ik) */
static real mag_value(const real *q, const real *r) {
    return q[0] + r[0] * q[1] + r[1] * q[2] + (r[0] + r[1]) * q[3];
}
/*
 * M of a gradient term g_0 w_0 + g_1 w_1 + g_2 w_2 (g_l = dV/dr_l; w_l a direction cosine of leg l, or r_a r_b / r of leg l:
 * of degree 0 or 1 in the leg's vector, so that r_l |dw_l/dr_l| = |w_l|): the three products with absolute values, and per leg
 * rho_l times ( sum_l' |d2V/dr_l dr_l'|_abs |w_l'| + |g_l|_abs |w_l| / r_l ).  wa: |w|.
 */
static real mag_grad(const real *q, const real *wa, const real *r) {
    real rho[3] = {r[0], r[1], r[0] + r[1]};
    return q[1] * wa[0] + q[2] * wa[1] + q[3] * wa[2]
         + rho[0] * (wa[0] * (q[4] + q[1] / r[0]) + wa[1] * q[5] + wa[2] * q[6])
         + rho[1] * (wa[0] * q[5] + wa[1] * (q[7] + q[2] / r[1]) + wa[2] * q[8])
         + rho[2] * (wa[0] * q[6] + wa[1] * q[8] + wa[2] * (q[9] + q[3] / r[2]));
}

/* fold the symmetry images, keep template bins, weight (bspline.py:664-690), accumulate into out */
static void compress_add(const uf3o_spec *s, const trio_view *v, int t, const real *grid, real *out, real sign) {
    int M = v->dim[1], N = v->dim[2], sym = s->trio_sym[t];
    for (int c = 0; c < s->trio_ncol[t]; c++) {
        int64_t u = v->mask[c];
        int l = (int)(u / ((int64_t)M * N)), m = (int)((u / N) % M), n = (int)(u % N);
        int64_t img[6];
        int ni = sym_images(sym, l, m, n, M, N, img);
        real val = 0.0;
        for (int q = 0; q < ni; q++) val += grid[img[q]];
        out[s->trio_col[t] + c] += sign * val * v->w[c];
    }
}
/* the same fold of a grid of magnitudes, with |weight| */
static void compress_add_abs(const uf3o_spec *s, const trio_view *v, int t, const double *grid, double *out) {
    int M = v->dim[1], N = v->dim[2], sym = s->trio_sym[t];
    for (int c = 0; c < s->trio_ncol[t]; c++) {
        int64_t u = v->mask[c];
        int l = (int)(u / ((int64_t)M * N)), m = (int)((u / N) % M), n = (int)(u % N);
        int64_t img[6];
        int ni = sym_images(sym, l, m, n, M, N, img);
        double val = 0.0;
        for (int q = 0; q < ni; q++) val += grid[img[q]];
        out[s->trio_col[t] + c] += val * fabs(v->w[c]);
    }
}

static int wrap_idx(int i, int n) { return i < 0 ? i + n : i; }  /* numpy negative indexing */

/*
 * 3-body energy grid and (optionally) per-atom force grids.
 * Energy: real centres only (angles.py:339).  Forces: every supercell atom may be a centre; a ghost
 * centre keeps only triplets whose first-listed neighbour is real (angles.py:451-460).
 * Neighbour pairs: r_min3 < d <= r_max3.  j<k by supercell index, then the two neighbours are put in
 * ascending-Z order (stable), interaction = (Z_i; Z_j, Z_k); legs masked t[0] <= r <= t[-1].
 * Strain rows: real centres, the three legs of the centre's own triplet (as eval_worker's virial6).
 */
static void three_body(const uf3o_spec *s, const supercell_t *sc, const grid_t *g, const rows_t *o,
                       int64_t *n3_cnt, int64_t *n3_ij, int64_t n3_cap) {
    int T = s->n_trios, N = sc->n_atoms, F = s->n_feat;
    real *xe = o->xe, *xf = o->xf, *xv = o->xv;
    trio_view *v = (trio_view *)malloc(sizeof(trio_view) * (size_t)T);
    double rmin3, rmax3;
    trio_views(s, v, &rmin3, &rmax3);
    real **egrid = (real **)malloc(sizeof(real *) * (size_t)T), **vgrid = (real **)calloc((size_t)T, sizeof(real *));
    double **megrid = (double **)calloc((size_t)T, sizeof(double *)), **mvgrid = (double **)calloc((size_t)T, sizeof(double *));
    for (int t = 0; t < T; t++) {
        size_t sz = (size_t)v[t].dim[0] * v[t].dim[1] * v[t].dim[2];
        egrid[t] = (real *)calloc(sz, sizeof(real));
        if (xv) vgrid[t] = (real *)calloc(6 * sz, sizeof(real));
        if (xe && o->me) megrid[t] = (double *)calloc(sz, sizeof(double));
        if (xv && o->mv) mvgrid[t] = (double *)calloc(6 * sz, sizeof(double));
    }
    /* site rows: the energy grids of one centre at a time, folded into its row when the centre is done */
    real **bgrid = o->xb ? (real **)malloc(sizeof(real *) * (size_t)T) : NULL;
    double **mbgrid = o->xb ? (double **)malloc(sizeof(double *) * (size_t)T) : NULL;
    for (int t = 0; bgrid && t < T; t++) {
        size_t sz = (size_t)v[t].dim[0] * v[t].dim[1] * v[t].dim[2];
        bgrid[t] = (real *)calloc(sz, sizeof(real)); mbgrid[t] = (double *)calloc(sz, sizeof(double));
    }
    int *cand = NULL, cap = 0, *nbr = NULL, nbr_cap = 0;
    double *nbr_d = NULL;
    int64_t cnt = 0;
    int want_m = ((xe && o->me) || (xf && o->mf) || (xv && o->mv)) ? (o->pieces ? 2 : 1) : 0;

    int n_centres = xf ? sc->m : N;
    for (int pass = 0; pass < (xf ? 2 : 1); pass++) {
        /* pass 0: energy (and strain rows) over real centres; pass 1: forces over all centres */
        int nc_max = pass == 0 ? N : n_centres;
        if (pass == 0 && !xe && !xv && !n3_cnt) continue;
        for (int i = 0; i < nc_max; i++) {
            const double *ri = sc->pos + 3 * (size_t)i;
            int nc = gather_candidates(sc, g, ri, &cand, &cap), nn = 0;
            for (int c = 0; c < nc; c++) {
                double d = dist3(ri, sc->pos + 3 * (size_t)cand[c]);
                if (d > rmin3 && d <= rmax3) {
                    if (nn == nbr_cap) {
                        nbr_cap = nbr_cap ? 2 * nbr_cap : 64;
                        nbr = (int *)realloc(nbr, sizeof(int) * (size_t)nbr_cap);
                        nbr_d = (double *)realloc(nbr_d, sizeof(double) * (size_t)nbr_cap);
                    }
                    nbr[nn] = cand[c]; nbr_d[nn] = d; nn++;
                    if (pass == 0 && n3_cnt) {
                        if (n3_ij && cnt < n3_cap) { n3_ij[2 * cnt] = i; n3_ij[2 * cnt + 1] = cand[c]; }
                        cnt++;
                    }
                }
            }
            if (pass == 0 && !xe && !xv) continue;
            int ghost = i >= N;
            for (int a = 0; a < nn; a++) {
                for (int b = 0; b < nn; b++) {
                    /* meshgrid(i_group_filtered, i_group): j from the (real-only, for ghost centres)
                       list, k from the full list, keep j < k */
                    int j = nbr[a], k = nbr[b];
                    if (!(j < k)) continue;
                    if (ghost && j >= N) continue;
                    double rij = nbr_d[a], rik = nbr_d[b];
                    int zj = sc->z[j], zk = sc->z[k];
                    if (zj > zk) { int ti = j; j = k; k = ti; ti = zj; zj = zk; zk = ti; double td = rij; rij = rik; rik = td; }
                    int t = trio_index(s, sc->z[i], zj, zk);
                    if (t < 0) continue;
                    const double *rj = sc->pos + 3 * (size_t)j, *rk = sc->pos + 3 * (size_t)k;
                    double rjk = dist3(rj, rk);
                    const trio_view *tv = v + t;
                    if (!(rij >= tv->k[0][0] && rij <= tv->k[0][tv->nk[0] - 1])) continue;
                    if (!(rik >= tv->k[1][0] && rik <= tv->k[1][tv->nk[1] - 1])) continue;
                    if (!(rjk >= tv->k[2][0] && rjk <= tv->k[2][tv->nk[2] - 1])) continue;
                    real r[3] = {rdist3(ri, rj), rdist3(ri, rk), rdist3(rj, rk)};
                    leg_t gl, gm, gn;
                    int L = tv->dim[0], M = tv->dim[1], Nn = tv->dim[2];
                    int der = pass || xv;
                    int il = leg_values(tv, 0, rij, r[0], s->lead3, s->trail3, &gl, der, want_m);
                    int im = leg_values(tv, 1, rik, r[1], s->lead3, s->trail3, &gm, der, want_m);
                    int in = leg_values(tv, 2, rjk, r[2], s->lead3, s->trail3, &gn, der, want_m);
                    const real *vl = gl.v, *vm = gm.v, *vn = gn.v, *dl = gl.d, *dm = gm.d, *dn = gn.d;
                    size_t sz = (size_t)L * M * Nn;
                    if (pass == 0) {
                        for (int x = 0; x < 4; x++) for (int y = 0; y < 4; y++) for (int w = 0; w < 4; w++) {
                            size_t u = ((size_t)wrap_idx(il + x, L) * M + wrap_idx(im + y, M)) * Nn + wrap_idx(in + w, Nn);
                            real q[10] = {0};
                            if (want_m) q_add(q, 1.0, &gl, &gm, &gn, x, y, w);
                            if (xe) {
                                real val = vl[x] * vm[y] * vn[w];
                                if (val != 0.0) {
                                    egrid[t][u] += val;
                                    if (megrid[t]) megrid[t][u] += (double)mag_value(q, r);
                                    if (bgrid) { bgrid[t][u] += val; mbgrid[t][u] += (double)mag_value(q, r); }
                                }
                            }
                            if (xv) for (int e = 0; e < 6; e++) {
                                int ca = VOIGT[e][0], cb = VOIGT[e][1];
                                real wij = ((real)rj[ca] - ri[ca]) * ((real)rj[cb] - ri[cb]) / r[0];
                                real wik = ((real)rk[ca] - ri[ca]) * ((real)rk[cb] - ri[cb]) / r[1];
                                real wjk = ((real)rk[ca] - rj[ca]) * ((real)rk[cb] - rj[cb]) / r[2];
                                vgrid[t][e * sz + u] += dl[x] * vm[y] * vn[w] * wij + vl[x] * dm[y] * vn[w] * wik + vl[x] * vm[y] * dn[w] * wjk;
                                if (mvgrid[t]) {
                                    real wa[3] = {rabs(wij), rabs(wik), rabs(wjk)};
                                    mvgrid[t][e * sz + u] += (double)mag_grad(q, wa, r);
                                }
                            }
                        }
                    } else {
                        /* direction cosines restricted to real atoms (distances.py:354-363) */
                        int idx[3] = {i, j, k};
                        for (int who = 0; who < 3; who++) {
                            int m = idx[who];
                            if (m >= N) continue;
                            /* an atom may appear once only in a triplet, but two of i,j,k can be images
                               of one real atom only as distinct supercell indices, so m matches one slot */
                            for (int c3 = 0; c3 < 3; c3++) {
                                real dij = ((m == j) - (m == i)) * ((real)rj[c3] - ri[c3]) / r[0];
                                real dik = ((m == k) - (m == i)) * ((real)rk[c3] - ri[c3]) / r[1];
                                real djk = ((m == k) - (m == j)) * ((real)rk[c3] - rj[c3]) / r[2];
                                if (dij == 0 && dik == 0 && djk == 0) continue;
                                real wa[3] = {rabs(dij), rabs(dik), rabs(djk)};
                                /* force_grid[m][c] -= val, then compress_3B: a raw bin u reaches every
                                   column whose symmetry images contain u, times that column's weight */
                                real *row = xf + ((size_t)m * 3 + c3) * F + s->trio_col[t];
                                double *mrow = o->mf ? o->mf + ((size_t)m * 3 + c3) * F + s->trio_col[t] : NULL;
                                for (int x = 0; x < 4; x++) for (int y = 0; y < 4; y++) for (int w = 0; w < 4; w++) {
                                    real val = dl[x] * vm[y] * vn[w] * dij + vl[x] * dm[y] * vn[w] * dik + vl[x] * vm[y] * dn[w] * djk;
                                    if (val == 0.0) continue;
                                    size_t u = ((size_t)wrap_idx(il + x, L) * M + wrap_idx(im + y, M)) * Nn + wrap_idx(in + w, Nn);
                                    double mag = 0.0;
                                    if (mrow) { real q[10] = {0}; q_add(q, 1.0, &gl, &gm, &gn, x, y, w); mag = (double)mag_grad(q, wa, r); }
                                    for (int e = tv->inv_start[u]; e < tv->inv_start[u + 1]; e++) {
                                        row[tv->inv_col[e]] -= val * tv->w[tv->inv_col[e]];
                                        if (mrow) mrow[tv->inv_col[e]] += mag * fabs(tv->w[tv->inv_col[e]]);
                                    }
                                }
                            }
                        }
                    }
                }
            }
            if (pass == 0 && bgrid) for (int t = 0; t < T; t++) {
                size_t sz = (size_t)v[t].dim[0] * v[t].dim[1] * v[t].dim[2];
                compress_add(s, v + t, t, bgrid[t], o->xb + (size_t)i * F, 1.0);
                compress_add_abs(s, v + t, t, mbgrid[t], o->mb + (size_t)i * F);
                for (size_t u = 0; u < sz; u++) { bgrid[t][u] = 0.0; mbgrid[t][u] = 0.0; }
            }
        }
    }
    for (int t = 0; bgrid && t < T; t++) { free(bgrid[t]); free(mbgrid[t]); }
    free(bgrid); free(mbgrid);
    for (int t = 0; t < T; t++) {
        size_t sz = (size_t)v[t].dim[0] * v[t].dim[1] * v[t].dim[2];
        if (xe) compress_add(s, v + t, t, egrid[t], xe, 1.0);
        if (megrid[t]) compress_add_abs(s, v + t, t, megrid[t], o->me);
        for (int e = 0; e < 6; e++) {
            if (xv) compress_add(s, v + t, t, vgrid[t] + e * sz, xv + (size_t)e * F, 1.0);
            if (mvgrid[t]) compress_add_abs(s, v + t, t, mvgrid[t] + e * sz, o->mv + (size_t)e * F);
        }
    }
    if (n3_cnt) *n3_cnt = cnt;
    for (int t = 0; t < T; t++) { free(egrid[t]); free(vgrid[t]); free(megrid[t]); free(mvgrid[t]); }
    free(egrid); free(vgrid); free(megrid); free(mvgrid); free(cand); free(nbr); free(nbr_d); free_trio_views(s, v);
}

/* ------------------------------------------------------------------- entry */
static int featurize_worker(const uf3o_spec *s, const uf3o_frame *f, const rows_t *o,
                            int64_t *pair_cnt, int64_t *pair_ij, int64_t pair_cap,
                            int64_t *n3_cnt, int64_t *n3_ij, int64_t n3_cap, int64_t *sc_info) {
    supercell_t sc;
    grid_t g;
    for (int a = 0; a < f->n_atoms; a++) if (species_index(s, f->z[a]) < 0) return 2;
    build_supercell(f, o->sc_r > 0 ? o->sc_r : s->r_cut, &sc);
    double rmin3 = 0, rmax3 = 0, h = 0;
    for (int p = 0; p < s->n_pairs; p++) if (s->pair_rmax[p] > h) h = s->pair_rmax[p];
    if (s->n_trios > 0) {
        trio_view *v = (trio_view *)malloc(sizeof(trio_view) * (size_t)s->n_trios);
        trio_views(s, v, &rmin3, &rmax3);
        free_trio_views(s, v);
        if (rmax3 > h) h = rmax3;
    }
    build_grid(&sc, h * (1.0 + 1e-9) + 1e-9, &g);
    size_t F = (size_t)s->n_feat, NF = F * 3 * (size_t)f->n_atoms;
    if (o->xe) {
        for (size_t q = 0; q < F; q++) o->xe[q] = 0.0;
        if (o->me) memset(o->me, 0, sizeof(double) * F);
        for (int a = 0; a < f->n_atoms; a++) {
            o->xe[species_index(s, f->z[a])] += 1.0;
            if (o->me) o->me[species_index(s, f->z[a])] += 1.0;
        }
    }
    if (o->xb) {
        for (size_t q = 0; q < F * (size_t)f->n_atoms; q++) { o->xb[q] = 0.0; o->mb[q] = 0.0; }
        for (int a = 0; a < f->n_atoms; a++) {
            o->xb[(size_t)a * F + species_index(s, f->z[a])] += 1.0;
            o->mb[(size_t)a * F + species_index(s, f->z[a])] += 1.0;
        }
    }
    if (o->xf) for (size_t q = 0; q < NF; q++) o->xf[q] = 0.0;
    if (o->xf && o->mf) memset(o->mf, 0, sizeof(double) * NF);
    if (o->xv) for (size_t q = 0; q < 6 * F; q++) o->xv[q] = 0.0;
    if (o->xv && o->mv) memset(o->mv, 0, sizeof(double) * 6 * F);
    two_body(s, &sc, &g, o, pair_cnt, pair_ij, pair_cap);
    if (s->n_trios > 0) three_body(s, &sc, &g, o, n3_cnt, n3_ij, n3_cap);
    else if (n3_cnt) *n3_cnt = 0;
    if (sc_info) {
        sc_info[0] = sc.n_img; sc_info[1] = sc.m;
        for (int d = 0; d < 3; d++) { sc_info[2 + d] = sc.fac[d]; sc_info[5 + d] = sc.cnt[d]; }
    }
    free_grid(&g); free_supercell(&sc);
    return 0;
}

/*
 * Feature rows of one frame (process.py:293-367 without the y column):
 *   xe [F]        1-body counts | 2-body | 3-body         (NULL to skip)
 *   xf [N][3][F]  1-body zeros  | 2-body | 3-body         (NULL to skip)
 * Index dumps (any may be NULL):
 *   pair_cnt [P], pair_ij [P][pair_cap][2]   2-body (i, j) per pair block
 *   n3_cnt [1],  n3_ij [n3_cap][2]           identify_ij(square=False) pairs
 *   sc_info [8]: n_img, m, fac[3], cnt[3]
 * (Rows are arrays of `real`: double in libuf3oracle.so.)
 */
int uf3o_featurize(const uf3o_spec *s, const uf3o_frame *f, real *xe, real *xf,
                   int64_t *pair_cnt, int64_t *pair_ij, int64_t pair_cap,
                   int64_t *n3_cnt, int64_t *n3_ij, int64_t n3_cap, int64_t *sc_info) {
    rows_t o = {xe, xf, NULL, NULL, NULL, NULL, 0, NULL, NULL, 0.0};
    return featurize_worker(s, f, &o, pair_cnt, pair_ij, pair_cap, n3_cnt, n3_ij, n3_cap, sc_info);
}

/*
 * The rows with the strain rows xv [6][F] (Voigt; d(energy row)/d(strain), the convention of uf3o_eval_virial) and the
 * magnitudes me [F], mf [N][3][F], mv [6][F] (doubles; NULL to skip, each only beside its row); pair_cnt [P] and n3_cnt [1] as
 * above, to show that both builds sum the same terms.  pieces != 0: the magnitudes of the 3-body columns for a route that
 * evaluates leg functions from local cubic pieces (piece_abs); the values do not depend on it.
 */
int uf3o_featurize_x(const uf3o_spec *s, const uf3o_frame *f, real *xe, real *xf, real *xv,
                     double *me, double *mf, double *mv, int pieces, int64_t *pair_cnt, int64_t *n3_cnt) {
    rows_t o = {xe, xf, xv, me, mf, mv, pieces, NULL, NULL, 0.0};
    return featurize_worker(s, f, &o, pair_cnt, NULL, 0, n3_cnt, NULL, 0, NULL);
}

/*
 * Site rows b [N][F] with magnitudes mb: the energy row's terms credited to their centre -- the one-body 1 of atom i, its
 * directed pair entries, the triplets it is the centre of (uf3_site_rows.h's partition: b_i . c = U_i of uf3o_site_terms_x) --
 * each folded into columns exactly as the energy row is; beside them the energy row xe [F] and me of the same walk
 * (sum_i b_i = xe up to the order of the additions).  One difference, uf3_site_rows.h's: a pair function that the basis trims
 * has no entry in the energy row but keeps its column in the site row, because b_i . c = U_i holds for EVERY flat coefficient
 * vector and the evaluator takes all pair coefficients; sum_i b_i = xe on the columns the energy row keeps, and xe is exactly
 * zero on the others.  A column no term of atom i reaches has b = 0 and M = 0.  sc_r: the
 * radius the supercell is built for (>= the basis' r_cut; wider where atoms lie outside their cell, so that every image a
 * real atom's terms reach is there: these rows are those of the frame with every atom counted as its image inside the cell).
 */
int uf3o_site_rows_x(const uf3o_spec *s, const uf3o_frame *f, double sc_r, real *xb, double *mb, real *xe, double *me) {
    rows_t o = {xe, NULL, NULL, me, NULL, NULL, 0, xb, mb, sc_r};
    return featurize_worker(s, f, &o, NULL, NULL, 0, NULL, NULL, 0, NULL);
}

/* supercell positions / species in reference order; returns m (call with out=NULL to size) */
int64_t uf3o_supercell(const uf3o_frame *f, double r_cut, double *pos_out, int *z_out, int *shift_out) {
    supercell_t sc;
    build_supercell(f, r_cut, &sc);
    int64_t m = sc.m;
    if (pos_out) memcpy(pos_out, sc.pos, sizeof(double) * 3 * (size_t)sc.m);
    if (z_out) memcpy(z_out, sc.z, sizeof(int) * (size_t)sc.m);
    if (shift_out) memcpy(shift_out, sc.shift, sizeof(int) * 3 * (size_t)sc.n_img);
    free_supercell(&sc);
    return m;
}

/* ------------------------------------------------------------- evaluator */
/* tensor-product cubic spline value / first partials from a full coefficient grid; q (may be NULL): the magnitudes of q_add,
   summed over the 64 products with |coefficient| */
static void spline3_n(const trio_view *tv, const double *c, const double *rd, const real *r, real *val, real *grad, real *q, int nq) {
    leg_t gl, gm, gn;
    int L = tv->dim[0], M = tv->dim[1], N = tv->dim[2];
    int il = leg_values(tv, 0, rd[0], r[0], 0, 0, &gl, 1, q != NULL), im = leg_values(tv, 1, rd[1], r[1], 0, 0, &gm, 1, q != NULL),
        in = leg_values(tv, 2, rd[2], r[2], 0, 0, &gn, 1, q != NULL);
    const real *vl = gl.v, *vm = gm.v, *vn = gn.v, *dl = gl.d, *dm = gm.d, *dn = gn.d;
    real v = 0, g0 = 0, g1 = 0, g2 = 0;
    if (q) for (int x = 0; x < 10; x++) q[x] = 0.0;
    for (int x = 0; x < 4; x++) for (int y = 0; y < 4; y++) for (int w = 0; w < 4; w++) {
        int a = il + x, b = im + y, d = in + w;
        if (a < 0 || b < 0 || d < 0 || a >= L || b >= M || d >= N) continue;
        real cc = c[((size_t)a * M + b) * N + d];
        v += cc * vl[x] * vm[y] * vn[w];
        g0 += cc * dl[x] * vm[y] * vn[w];
        g1 += cc * vl[x] * dm[y] * vn[w];
        g2 += cc * vl[x] * vm[y] * dn[w];
        if (q) q_add_n(q, rabs(cc), &gl, &gm, &gn, x, y, w, nq);
    }
    *val = v; grad[0] = g0; grad[1] = g1; grad[2] = g2;
}
static void spline3(const trio_view *tv, const double *c, const double *rd, const real *r, real *val, real *grad, real *q) {
    spline3_n(tv, c, rd, r, val, grad, q, 10);
}

/* virial6 += g * r (x) r / |r| for one energy term g(|r|) of the bond vector r (Voigt); m6 (may be NULL) += gm |r_a r_b| / |r| */
static void strain_add(real *virial6, double *m6, real g, real gm, const double *ra, const double *rb, real r) {
    for (int v = 0; v < 6; v++) {
        int a = VOIGT[v][0], b = VOIGT[v][1];
        virial6[v] += g * ((real)rb[a] - ra[a]) * ((real)rb[b] - ra[b]) / r;
        if (m6) m6[v] += (double)(gm * rabs(((real)rb[a] - ra[a]) * ((real)rb[b] - ra[b])) / r);
    }
}

/*
 * ---- per-centre and second-derivative outputs of the evaluator's term loop (uf3o_site_terms_x, uf3o_hessian_x) -------------
 *
 * A term of the energy is a function V of nl leg lengths (a pair term: one leg; a triplet: ij, ik, jk) between ns slots (slot 0
 * the centre, then its neighbour images); leg q runs from slot legs[q][0] to slot legs[q][1], sg[q][s] = +1 / -1 / 0 is
 * d r_q / d(slot s) in units of the leg's unit vector u_q.  In leg space the term has the value, the gradient g_q and the
 * symmetric leg Hessian K_qq', from B-spline values, first and second derivatives by the recursion (basis_element, nu = 0, 1, 2).
 *
 * Every output entry below is linear in g or bilinear in (K, g) with geometric weights that the entry fixes:
 *     first order   e = sum_q g_q w_q                                       (site virials, the heat current's potential part)
 *     second order  e = sum_qq' K_qq' X_q Y_q' + sum_q g_q Z_q              (H, mixed, born)
 * Magnitudes, by the definition at the top of this file (absolute values wherever a term takes signs, plus the sensitivity to a
 * relative rounding of each leg length, rho = r for a pair leg and a centre leg, r_ij + r_ik for the third leg):
 *     M1 = sum_q |g_q|_abs |w_q|_abs + sum_l rho_l ( sum_q |K_lq|_abs |w_q|_abs + |g_l|_abs |w_l|_abs / r_l )
 * which is mag_grad's expression (a pair: (2 |phi'|_abs + r |phi''|_abs) |w|, two_body's gm), and
 *     M2 = sum_qq' |K_qq'|_abs |X_q| |Y_q'| + sum_q |g_q|_abs |Z_q|_abs
 *        + sum_l rho_l ( sum_qq' |T_qq'l|_abs |X_q| |Y_q'| + sum_q |K_ql|_abs |Z_q|_abs
 *                        + ( sum_q' (|K_lq'|_abs |X_l| |Y_q'| + |K_q'l|_abs |X_q'| |Y_l|) + 2 |g_l|_abs |Z_l|_abs ) / r_l )
 * T = d3V / dr_q dr_q' dr_l: the derivative of K with respect to a leg length.  For a cubic spline the third derivative of a leg
 * function is a step function; its |.|_abs is the interval's own (basis_element_abs3).  The last line is the weights' own
 * sensitivity: a weight X_l or Y_l is of degree 0 or 1 in the vector of leg l (a cosine, d_a d_b / r) and counts once, as in
 * mag_grad; Z_l is a quotient of products of the leg's components by its length ((I - uu^T) / r and its strain analogues) and
 * counts twice.  |w|_abs, |Z|_abs: the weight with every subtraction inside it replaced by an addition (I - uu^T -> I + |u||u|^T,
 * d_ik[a] - d_ij[a] -> |d_ik[a]| + |d_ij[a]|).  An entry that no term reaches keeps M = 0.
 */
typedef struct {
    int nl, ns;
    int legs[3][2];
    real d[3][3], r[3], rho[3];        /* leg vectors (from -> to), lengths, rounding weights */
    real g[3], K[3][3];                /* leg gradient, leg Hessian (K only for the second-order outputs) */
    real ga[3], Ka[3][3], Ta[3][3][3]; /* |.|_abs of g, K and T */
} term_t;

typedef struct {
    double sc_r;                       /* supercell radius in place of the basis' r_cut (0: r_cut) */
    int n;                             /* real atoms */
    const double *vel;                 /* [N][3] or NULL */
    real *U, *W, *J;                   /* [N], [N][9], [N][3] (J only with vel); NULL: not wanted */
    double *mU, *mW, *mJ;
    real *H, *L, *B;                   /* [3N][3N], [3N][6], [6][6]; NULL: not wanted */
    double *mH, *mL, *mB;
    struct touch_s *mc;                /* the terms that contain an atom of a Monte Carlo move (uf3o_mc_delta_x); NULL: not wanted */
} sink_t;

/*
 * ---- the terms a Monte Carlo move touches (uf3o_mc_delta_x; uf3_mc.h) ---------------------------------------------------------
 * touch [N]: 1 for the real atoms of T.  The term loop hands over every term whose parent atoms (centre included) contain an atom
 * of T, and no other: E and M are the sums of their values and of their magnitudes mval, in the loop's own order.  Terms without
 * an atom of T are skipped before they are evaluated, and so are the centres that cannot reach T (the lists are symmetric under
 * lattice translations: a centre has an image of t within the list range exactly when t has an image of the centre within it).
 * rec (may be NULL): one record of UF3O_MC_TERM_W doubles per term, for the planted defects of tests/test_mc_precision_host.py:
 *   pass (0 old species, 1 new) | kind (1 one-body, 2 pair, 3 triplet) | centre | parent of slot 1 | parent of slot 2 (-1) |
 *   value | magnitude | distance (pair: d; triplet: r_jk) | the triplet with its l and m leg lengths exchanged | the triplet with
 *   its l leg length rounded through fp32 | r_ij | r_ik (triplets; 0 otherwise)
 */
#define UF3O_MC_TERM_W 12
typedef struct touch_s {
    const unsigned char *touch;
    unsigned char *reach;              /* [N] scratch: centres with an image of an atom of T within the list range */
    real E;
    double M;
    int pass;
    double *rec;
    int64_t n_rec, cap;
    double x_d, x_swap, x_f32, x_ra, x_rb; /* the extra fields of the term about to be handed over */
} touch_t;

static void touch_term(touch_t *m, int kind, int i, int p1, int p2, real val, real mval) {
    m->E += val; m->M += (double)mval;
    if (m->rec) {
        if (m->n_rec < m->cap) {
            double *o = m->rec + UF3O_MC_TERM_W * (size_t)m->n_rec;
            o[0] = m->pass; o[1] = kind; o[2] = i; o[3] = p1; o[4] = p2; o[5] = (double)val; o[6] = (double)mval;
            o[7] = m->x_d; o[8] = m->x_swap; o[9] = m->x_f32; o[10] = m->x_ra; o[11] = m->x_rb;
        }
        m->n_rec++;
    }
}

static real m1_of(const term_t *t, const real *wa) {
    real m = 0.0;
    for (int q = 0; q < t->nl; q++) m += t->ga[q] * wa[q];
    for (int l = 0; l < t->nl; l++) {
        real s = t->ga[l] * wa[l] / t->r[l];
        for (int q = 0; q < t->nl; q++) s += t->Ka[l][q] * wa[q];
        m += t->rho[l] * s;
    }
    return m;
}
static real e2_of(const term_t *t, const real *X, const real *Y, const real *Z) {
    real e = 0.0;
    for (int q = 0; q < t->nl; q++) for (int p = 0; p < t->nl; p++) e += t->K[q][p] * X[q] * Y[p];
    for (int q = 0; q < t->nl; q++) e += t->g[q] * Z[q];
    return e;
}
static real m2_of(const term_t *t, const real *X, const real *Y, const real *Za) {
    real m = 0.0, xa[3], ya[3];
    int nl = t->nl;
    for (int q = 0; q < nl; q++) { xa[q] = rabs(X[q]); ya[q] = rabs(Y[q]); }
    for (int q = 0; q < nl; q++) for (int p = 0; p < nl; p++) m += t->Ka[q][p] * xa[q] * ya[p];
    for (int q = 0; q < nl; q++) m += t->ga[q] * Za[q];
    for (int l = 0; l < nl; l++) {
        real s = 0.0, geo = 2.0 * t->ga[l] * Za[l];
        for (int q = 0; q < nl; q++) for (int p = 0; p < nl; p++) s += t->Ta[q][p][l] * xa[q] * ya[p];
        for (int q = 0; q < nl; q++) s += t->Ka[q][l] * Za[q];
        for (int p = 0; p < nl; p++) geo += t->Ka[l][p] * xa[l] * ya[p] + t->Ka[p][l] * xa[p] * ya[l];
        m += t->rho[l] * (s + geo / t->r[l]);
    }
    return m;
}
/* the strain direction of Voigt component v applied to d: d(d)/dt_v = E_v d, eps_ab = eps_ba = t / 2 off the diagonal */
static void strain_dir(int v, const real *d, real *o) {
    int a = VOIGT[v][0], b = VOIGT[v][1];
    o[0] = o[1] = o[2] = 0.0;
    if (a == b) o[a] = d[a];
    else { o[a] = 0.5 * d[b]; o[b] = 0.5 * d[a]; }
}

/* one term of centre i into the sinks; par[s]: the parent atom of slot s; val, mval: the term's value and its magnitude */
static void sink_term(const sink_t *k, int i, const int *par, const term_t *t, real val, real mval) {
    int nl = t->nl, ns = t->ns, N = k->n;
    if (k->mc) { touch_term(k->mc, t->ns, i, par[1], t->ns > 2 ? par[2] : -1, val, mval); return; }
    real u[3][3], sg[3][3] = {{0}};
    for (int q = 0; q < nl; q++) {
        for (int c = 0; c < 3; c++) u[q][c] = t->d[q][c] / t->r[q];
        sg[q][t->legs[q][1]] += 1.0; sg[q][t->legs[q][0]] -= 1.0;
    }
    if (k->U) { k->U[i] += val; k->mU[i] += (double)mval; }
    /* slot s >= 1 lies at d_s from the centre: the vector of the centre leg that ends in it (leg s - 1 in both kinds of term);
       dU_i / dr_s = sum_q g_q sg[q][s] u_q */
    if (k->W) for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) {
        real w[3], wa[3], e = 0.0;
        for (int q = 0; q < nl; q++) {
            real c = 0.0, ca = 0.0;
            for (int s = 1; s < ns; s++) { c += sg[q][s] * t->d[s - 1][a]; ca += rabs(sg[q][s] * t->d[s - 1][a]); }
            w[q] = c * u[q][b]; wa[q] = ca * rabs(u[q][b]);
            e += t->g[q] * w[q];
        }
        k->W[(size_t)i * 9 + 3 * a + b] += e;
        k->mW[(size_t)i * 9 + 3 * a + b] += (double)m1_of(t, wa);
    }
    if (k->J) for (int a = 0; a < 3; a++) {
        real wa[3], e = 0.0;
        for (int q = 0; q < nl; q++) {
            real c = 0.0, ca = 0.0;
            for (int s = 1; s < ns; s++) {
                const double *vs = k->vel + 3 * (size_t)par[s];
                real uv = 0.0, uva = 0.0;
                for (int b = 0; b < 3; b++) { uv += u[q][b] * vs[b]; uva += rabs(u[q][b] * vs[b]); }
                c += sg[q][s] * t->d[s - 1][a] * uv; ca += rabs(sg[q][s] * t->d[s - 1][a]) * uva;
            }
            wa[q] = ca;
            e += t->g[q] * c;
        }
        k->J[(size_t)i * 3 + a] -= e;
        k->mJ[(size_t)i * 3 + a] += (double)m1_of(t, wa);
    }
    if (!k->H) return;
    size_t ld = 3 * (size_t)N;
    real w6[3][6], ed[3][6][3];
    for (int q = 0; q < nl; q++) for (int v = 0; v < 6; v++) {
        w6[q][v] = t->d[q][VOIGT[v][0]] * t->d[q][VOIGT[v][1]] / t->r[q];
        strain_dir(v, t->d[q], ed[q][v]);
    }
    real X[3], Y[3], Z[3], Za[3];
    for (int s = 0; s < ns; s++) for (int a = 0; a < 3; a++) {
        for (int q = 0; q < nl; q++) X[q] = sg[q][s] * u[q][a];
        /* H: X = sg_s u[a], Y = sg_s' u[b], Z = sg_s sg_s' (delta_ab - u_a u_b) / r */
        for (int s2 = 0; s2 < ns; s2++) for (int b = 0; b < 3; b++) {
            for (int q = 0; q < nl; q++) {
                Y[q] = sg[q][s2] * u[q][b];
                Z[q] = sg[q][s] * sg[q][s2] * ((a == b ? 1.0 : 0.0) - u[q][a] * u[q][b]) / t->r[q];
                Za[q] = rabs(sg[q][s] * sg[q][s2]) * ((a == b ? 1.0 : 0.0) + rabs(u[q][a] * u[q][b])) / t->r[q];
            }
            size_t at = (3 * (size_t)par[s] + a) * ld + 3 * (size_t)par[s2] + b;
            k->H[at] += e2_of(t, X, Y, Z);
            k->mH[at] += (double)m2_of(t, X, Y, Za);
        }
        /* mixed: Y = d_a d_b / r of the Voigt component, Z = sg_s (P E_v d)[a] / r, P = I - uu^T */
        if (k->L) for (int v = 0; v < 6; v++) {
            for (int q = 0; q < nl; q++) {
                real ue = 0.0, uea = 0.0;
                for (int c = 0; c < 3; c++) { ue += u[q][c] * ed[q][v][c]; uea += rabs(u[q][c] * ed[q][v][c]); }
                Y[q] = w6[q][v];
                Z[q] = sg[q][s] * (ed[q][v][a] - u[q][a] * ue) / t->r[q];
                Za[q] = rabs(sg[q][s]) * (rabs(ed[q][v][a]) + rabs(u[q][a]) * uea) / t->r[q];
            }
            size_t at = (3 * (size_t)par[s] + a) * 6 + v;
            k->L[at] += e2_of(t, X, Y, Z);
            k->mL[at] += (double)m2_of(t, X, Y, Za);
        }
    }
    /* born: X = w_v1, Y = w_v2, Z = d2 r / dt_v1 dt_v2 = ((E_v1 d) . (E_v2 d) - w_v1 w_v2) / r  (d is linear in t) */
    if (k->B) for (int v1 = 0; v1 < 6; v1++) for (int v2 = 0; v2 < 6; v2++) {
        for (int q = 0; q < nl; q++) {
            real ee = 0.0, eea = 0.0;
            for (int c = 0; c < 3; c++) { ee += ed[q][v1][c] * ed[q][v2][c]; eea += rabs(ed[q][v1][c] * ed[q][v2][c]); }
            X[q] = w6[q][v1]; Y[q] = w6[q][v2];
            Z[q] = (ee - w6[q][v1] * w6[q][v2]) / t->r[q];
            Za[q] = (eea + rabs(w6[q][v1] * w6[q][v2])) / t->r[q];
        }
        k->B[6 * v1 + v2] += e2_of(t, X, Y, Z);
        k->mB[6 * v1 + v2] += (double)m2_of(t, X, Y, Za);
    }
}

/* leg Hessian K and |T|_abs of a triplet: spline3's contraction with B'' (leg_values, der = 2) and |B'''|_abs */
static void spline3_d2(const trio_view *tv, const double *c, const double *rd, const real *r, term_t *t) {
    leg_t g[3];
    int L = tv->dim[0], M = tv->dim[1], N = tv->dim[2], first[3];
    for (int q = 0; q < 3; q++) first[q] = leg_values(tv, q, rd[q], r[q], 0, 0, &g[q], 2, 1);
    for (int q = 0; q < 3; q++) for (int p = 0; p < 3; p++) { t->K[q][p] = 0.0; for (int l = 0; l < 3; l++) t->Ta[q][p][l] = 0.0; }
    for (int x = 0; x < 4; x++) for (int y = 0; y < 4; y++) for (int w = 0; w < 4; w++) {
        int a = first[0] + x, b = first[1] + y, d = first[2] + w, at[3] = {x, y, w};
        if (a < 0 || b < 0 || d < 0 || a >= L || b >= M || d >= N) continue;
        real cc = c[((size_t)a * M + b) * N + d], ca = rabs(cc);
        real f[3][3], fa[3][4];     /* per leg: value / first / second derivative, and the |.|_abs of orders 0 .. 3 */
        for (int q = 0; q < 3; q++) {
            f[q][0] = g[q].v[at[q]]; f[q][1] = g[q].d[at[q]]; f[q][2] = g[q].dd[at[q]];
            fa[q][0] = g[q].v[at[q]]; fa[q][1] = g[q].a1[at[q]]; fa[q][2] = g[q].a2[at[q]]; fa[q][3] = g[q].a3[at[q]];
        }
        for (int q = 0; q < 3; q++) for (int p = q; p < 3; p++) {
            int o[3] = {0, 0, 0};
            o[q]++; o[p]++;
            t->K[q][p] += cc * f[0][o[0]] * f[1][o[1]] * f[2][o[2]];
            for (int l = p; l < 3; l++) {
                int o3[3] = {o[0], o[1], o[2]};
                o3[l]++;
                t->Ta[q][p][l] += ca * fa[0][o3[0]] * fa[1][o3[1]] * fa[2][o3[2]];
            }
        }
    }
    for (int q = 0; q < 3; q++) for (int p = 0; p < q; p++) t->K[q][p] = t->K[p][q];
    for (int q = 0; q < 3; q++) for (int p = 0; p < 3; p++) for (int l = 0; l < 3; l++) {
        int a = q, b = p, d = l, h;       /* sorted */
        if (a > b) { h = a; a = b; b = h; }
        if (b > d) { h = b; b = d; d = h; }
        if (a > b) { h = a; a = b; b = h; }
        t->Ta[q][p][l] = t->Ta[a][b][d];
    }
}

/*
 * Energy and forces of a fitted model (calculator.py:156-343).
 *   c1 [S] one-body, c2 concatenated pair coefficient vectors (nk-4 each, ALL bases),
 *   c3 concatenated full L*M*N grids (decompress_3B output) per trio.
 * virial6 (may be NULL): dE/dt for the symmetric strain eps_ab = eps_ba = t/2 (t on the diagonal), Voigt order -- the
 * construction of the reference's numerical stress (calculator.py:399-404) -- from the energy terms alone: every term
 * V(r_1 .. r_k) of the sum over real i and supercell j (pairs) or real centres (trios) contributes
 * sum_legs dV/dr_l r_l,a r_l,b / r_l, with r_l the leg's image vector.
 * me [1], mf [N][3], mv [6] (may be NULL, each only beside its value): the magnitudes.
 */
static int eval_worker(const uf3o_spec *s, const uf3o_frame *f, const double *c1, const double *c2, const double *c3,
                       real *energy, real *forces, real *virial6, double *me, double *mf, double *mv, const sink_t *sk) {
    supercell_t sc;
    grid_t g;
    for (int a = 0; a < f->n_atoms; a++) if (species_index(s, f->z[a]) < 0) return 2;
    build_supercell(f, sk && sk->sc_r > 0 ? sk->sc_r : s->r_cut, &sc);
    int T = s->n_trios, N = sc.n_atoms;
    trio_view *v = T ? (trio_view *)malloc(sizeof(trio_view) * (size_t)T) : NULL;
    double rmin3 = 0, rmax3 = 0, h = 0;
    for (int p = 0; p < s->n_pairs; p++) if (s->pair_rmax[p] > h) h = s->pair_rmax[p];
    if (T) { trio_views(s, v, &rmin3, &rmax3); if (rmax3 > h) h = rmax3; }
    build_grid(&sc, h * (1.0 + 1e-9) + 1e-9, &g);
    real e = 0.0;
    double em = 0.0;
    if (!forces) mf = NULL;
    if (!virial6) mv = NULL;
    int want_m = me || mf || mv || sk;
    if (forces) for (int q = 0; q < 3 * N; q++) forces[q] = 0.0;
    if (virial6) for (int q = 0; q < 6; q++) virial6[q] = 0.0;
    if (mf) memset(mf, 0, sizeof(double) * 3 * (size_t)N);
    if (mv) memset(mv, 0, sizeof(double) * 6);
    for (int a = 0; a < N; a++) { e += c1[species_index(s, f->z[a])]; em += fabs(c1[species_index(s, f->z[a])]); }
    if (sk && sk->U) for (int a = 0; a < N; a++) { sk->U[a] += c1[species_index(s, f->z[a])]; sk->mU[a] += fabs(c1[species_index(s, f->z[a])]); }
    touch_t *mc = sk ? sk->mc : NULL;
    if (mc) {
        int *cd = NULL, ccap = 0;
        for (int a = 0; a < N; a++) mc->reach[a] = mc->touch[a];
        for (int a = 0; a < N; a++) {
            if (!mc->touch[a]) continue;
            mc->x_d = mc->x_swap = mc->x_f32 = mc->x_ra = mc->x_rb = 0.0;
            touch_term(mc, 1, a, -1, -1, c1[species_index(s, f->z[a])], fabs(c1[species_index(s, f->z[a])]));
            int nc = gather_candidates(&sc, &g, sc.pos + 3 * (size_t)a, &cd, &ccap);
            for (int c = 0; c < nc; c++)
                if (dist3(sc.pos + 3 * (size_t)a, sc.pos + 3 * (size_t)cd[c]) <= h * (1.0 + 1e-9)) mc->reach[cd[c] % N] = 1;
        }
        free(cd);
    }
    /* pair part */
    const double **pk = (const double **)malloc(sizeof(double *) * (size_t)(s->n_pairs + 1));
    const double **pc = (const double **)malloc(sizeof(double *) * (size_t)(s->n_pairs + 1));
    { const double *kp = s->pair_knots, *cp = c2;
      for (int p = 0; p < s->n_pairs; p++) { pk[p] = kp; pc[p] = cp; kp += s->pair_nk[p]; cp += s->pair_nk[p] - 4; } }
    int *cand = NULL, cap = 0;
    for (int i = 0; i < N; i++) {
        if (mc && !mc->reach[i]) continue;
        const double *ri = sc.pos + 3 * (size_t)i;
        int nc = gather_candidates(&sc, &g, ri, &cand, &cap);
        for (int c = 0; c < nc; c++) {
            int j = cand[c], p = pair_index(s, sc.z[i], sc.z[j]);
            if (p < 0) continue;
            if (mc && !(mc->touch[i] || mc->touch[j % N])) continue;
            const double *rj = sc.pos + 3 * (size_t)j;
            double d = dist3(ri, rj), rmin = s->pair_rmin[p] > 0 ? s->pair_rmin[p] : 0.0;
            if (!(d > rmin && d < s->pair_rmax[p])) continue;
            real dr = rdist3(ri, rj);
            int nb = s->pair_nk[p] - 4, first = searchsorted_left(pk[p], s->pair_nk[p], d) - 4;
            real phi = 0, dphi = 0, pa = 0, ga = 0, ha = 0, ddphi = 0, ta = 0;
            for (int a = 0; a < 4; a++) {
                int b = first + a;
                if (b < 0 || b >= nb) continue;
                phi += pc[p][b] * basis_element(pk[p] + b, d, dr, 0);
                dphi += pc[p][b] * basis_element(pk[p] + b, d, dr, 1);
                if (want_m) {
                    real a1, a2, ca = fabs(pc[p][b]);
                    basis_element_abs(pk[p] + b, d, dr, &a1, &a2);
                    pa += ca * basis_element(pk[p] + b, d, dr, 0); ga += ca * a1; ha += ca * a2;
                }
                if (sk && sk->H) {
                    ddphi += pc[p][b] * basis_element(pk[p] + b, d, dr, 2);
                    ta += (real)fabs(pc[p][b]) * basis_element_abs3(pk[p] + b, d, dr);
                }
            }
            e += phi;
            em += (double)(pa + dr * ga);
            real gm = 2.0 * ga + dr * ha;       /* |dphi|_abs + d |d(dphi w)/dd|_abs over |w|, as in two_body */
            if (forces) for (int k = 0; k < 3; k++) {
                forces[3 * i + k] += 2.0 * dphi * ((real)rj[k] - ri[k]) / dr;
                if (mf) mf[3 * i + k] += (double)(2.0 * gm * rabs((real)rj[k] - ri[k]) / dr);
            }
            if (virial6) strain_add(virial6, mv, dphi, gm, ri, rj, dr);
            if (sk) {
                term_t t = {.nl = 1, .ns = 2, .legs = {{0, 1}}, .r = {dr}, .rho = {dr}, .g = {dphi}, .K = {{ddphi}},
                            .ga = {ga}, .Ka = {{ha}}, .Ta = {{{ta}}}};
                int par[2] = {i, j % N};
                for (int c3 = 0; c3 < 3; c3++) t.d[0][c3] = (real)rj[c3] - ri[c3];
                if (mc) { mc->x_d = d; mc->x_swap = mc->x_f32 = mc->x_ra = mc->x_rb = 0.0; }
                sink_term(sk, i, par, &t, phi, pa + dr * ga);
            }
        }
    }
    /* trio part: real centres for the energy, all centres (ghost: real j) for the forces */
    if (T) {
        const double **tc = (const double **)malloc(sizeof(double *) * (size_t)T);
        { const double *cp = c3; for (int t = 0; t < T; t++) { tc[t] = cp; cp += (size_t)v[t].dim[0] * v[t].dim[1] * v[t].dim[2]; } }
        int *nbr = NULL, nbr_cap = 0; double *nbr_d = NULL;
        int n_centres = forces ? sc.m : N;
        for (int i = 0; i < n_centres; i++) {
            if (mc && !mc->reach[i % N]) continue;
            const double *ri = sc.pos + 3 * (size_t)i;
            int nc = gather_candidates(&sc, &g, ri, &cand, &cap), nn = 0;
            for (int c = 0; c < nc; c++) {
                double d = dist3(ri, sc.pos + 3 * (size_t)cand[c]);
                if (d > rmin3 && d <= rmax3) {
                    if (nn == nbr_cap) { nbr_cap = nbr_cap ? 2 * nbr_cap : 64; nbr = (int *)realloc(nbr, sizeof(int) * (size_t)nbr_cap); nbr_d = (double *)realloc(nbr_d, sizeof(double) * (size_t)nbr_cap); }
                    nbr[nn] = cand[c]; nbr_d[nn] = d; nn++;
                }
            }
            int ghost = i >= N;
            for (int a = 0; a < nn; a++) for (int b = 0; b < nn; b++) {
                int j = nbr[a], k = nbr[b];
                if (!(j < k)) continue;
                if (ghost && j >= N) continue;
                if (mc && !(mc->touch[i % N] || mc->touch[j % N] || mc->touch[k % N])) continue;
                double rij = nbr_d[a], rik = nbr_d[b];
                int zj = sc.z[j], zk = sc.z[k];
                if (zj > zk) { int ti = j; j = k; k = ti; ti = zj; zj = zk; zk = ti; double td = rij; rij = rik; rik = td; }
                int t = trio_index(s, sc.z[i], zj, zk);
                if (t < 0) continue;
                const double *rj = sc.pos + 3 * (size_t)j, *rk = sc.pos + 3 * (size_t)k;
                double rjk = dist3(rj, rk);
                const trio_view *tv = v + t;
                if (!(rij >= tv->k[0][0] && rij <= tv->k[0][tv->nk[0] - 1])) continue;
                if (!(rik >= tv->k[1][0] && rik <= tv->k[1][tv->nk[1] - 1])) continue;
                if (!(rjk >= tv->k[2][0] && rjk <= tv->k[2][tv->nk[2] - 1])) continue;
                double rd[3] = {rij, rik, rjk};
                real r[3] = {rdist3(ri, rj), rdist3(ri, rk), rdist3(rj, rk)};
                real val, gr[3], q[10];
                spline3_n(tv, tc[t], rd, r, &val, gr, want_m ? q : NULL, mc ? 4 : 10);
                if (!ghost) { e += val; if (want_m) em += (double)mag_value(q, r); }
                if (sk && !ghost) {
                    term_t tm = {.nl = 3, .ns = 3, .legs = {{0, 1}, {0, 2}, {1, 2}}, .r = {r[0], r[1], r[2]},
                                .rho = {r[0], r[1], r[0] + r[1]}, .g = {gr[0], gr[1], gr[2]}, .ga = {q[1], q[2], q[3]},
                                .Ka = {{q[4], q[5], q[6]}, {q[5], q[7], q[8]}, {q[6], q[8], q[9]}}};
                    int par[3] = {i, j % N, k % N};
                    for (int c3 = 0; c3 < 3; c3++) {
                        tm.d[0][c3] = (real)rj[c3] - ri[c3]; tm.d[1][c3] = (real)rk[c3] - ri[c3]; tm.d[2][c3] = (real)rk[c3] - rj[c3];
                    }
                    if (sk->H) spline3_d2(tv, tc[t], rd, r, &tm);
                    if (mc && mc->rec) {        /* the planted defects' variants of this triplet */
                        double rd_s[3] = {rd[1], rd[0], rd[2]}, rd_f[3] = {(double)(float)rd[0], rd[1], rd[2]};
                        real r_s[3] = {r[1], r[0], r[2]}, r_f[3] = {(real)rd_f[0], r[1], r[2]}, vx, gx[3];
                        mc->x_d = rjk; mc->x_ra = rij; mc->x_rb = rik;
                        spline3(tv, tc[t], rd_s, r_s, &vx, gx, NULL); mc->x_swap = (double)vx;
                        spline3(tv, tc[t], rd_f, r_f, &vx, gx, NULL); mc->x_f32 = (double)vx;
                    }
                    sink_term(sk, i, par, &tm, val, mag_value(q, r));
                }
                if (virial6 && !ghost) {          /* legs ij, ik, jk of the centre's own triplet */
                    strain_add(virial6, NULL, gr[0], 0.0, ri, rj, r[0]);
                    strain_add(virial6, NULL, gr[1], 0.0, ri, rk, r[1]);
                    strain_add(virial6, NULL, gr[2], 0.0, rj, rk, r[2]);
                    if (mv) for (int e6 = 0; e6 < 6; e6++) {
                        int ca = VOIGT[e6][0], cb = VOIGT[e6][1];
                        real wa[3] = {rabs(((real)rj[ca] - ri[ca]) * ((real)rj[cb] - ri[cb])) / r[0],
                                      rabs(((real)rk[ca] - ri[ca]) * ((real)rk[cb] - ri[cb])) / r[1],
                                      rabs(((real)rk[ca] - rj[ca]) * ((real)rk[cb] - rj[cb])) / r[2]};
                        mv[e6] += (double)mag_grad(q, wa, r);
                    }
                }
                if (forces) {
                    int idx[3] = {i, j, k};
                    for (int who = 0; who < 3; who++) {
                        int m = idx[who];
                        if (m >= N) continue;
                        for (int c3 = 0; c3 < 3; c3++) {
                            real dij = ((m == j) - (m == i)) * ((real)rj[c3] - ri[c3]) / r[0];
                            real dik = ((m == k) - (m == i)) * ((real)rk[c3] - ri[c3]) / r[1];
                            real djk = ((m == k) - (m == j)) * ((real)rk[c3] - rj[c3]) / r[2];
                            forces[3 * m + c3] -= dij * gr[0] + dik * gr[1] + djk * gr[2];
                            if (mf) { real wa[3] = {rabs(dij), rabs(dik), rabs(djk)}; mf[3 * m + c3] += (double)mag_grad(q, wa, r); }
                        }
                    }
                }
            }
        }
        free(nbr); free(nbr_d); free((void *)tc);
    }
    if (energy) *energy = e;
    if (me) *me = em;
    free(cand); free((void *)pk); free((void *)pc); if (v) free_trio_views(s, v);
    free_grid(&g); free_supercell(&sc);
    return 0;
}

/* (energy, forces, virial6 are `real`: double in libuf3oracle.so) */
int uf3o_eval(const uf3o_spec *s, const uf3o_frame *f, const double *c1, const double *c2, const double *c3,
              real *energy, real *forces) {
    return eval_worker(s, f, c1, c2, c3, energy, forces, NULL, NULL, NULL, NULL, NULL);
}

/* uf3o_eval plus the strain derivative virial6 [6] (eV, Voigt xx, yy, zz, yz, xz, xy; stress = virial6 / volume) */
int uf3o_eval_virial(const uf3o_spec *s, const uf3o_frame *f, const double *c1, const double *c2, const double *c3,
                     real *energy, real *forces, real *virial6) {
    return eval_worker(s, f, c1, c2, c3, energy, forces, virial6, NULL, NULL, NULL, NULL);
}

/* uf3o_eval_virial plus the magnitudes me [1], mf [N][3], mv [6] */
int uf3o_eval_x(const uf3o_spec *s, const uf3o_frame *f, const double *c1, const double *c2, const double *c3,
                real *energy, real *forces, real *virial6, double *me, double *mf, double *mv) {
    return eval_worker(s, f, c1, c2, c3, energy, forces, virial6, me, mf, mv, NULL);
}


/*
 * Site terms (uf3_flux.h's partition; the evaluator's own term loop with per-centre outputs): U [N] the one-body term of i, its
 * directed pair terms and the triplets it is the centre of; W [N][9], W_i[a][b] = sum_terms sum_s d_s[a] (dU_i / dr_s)[b] over the
 * neighbour images s of a term, d_s from the centre to the image; J [N][3] (with vel [N][3], else NULL), each centre's share of
 * J_pot = -sum_terms sum_s d_s (dU_i / dr_s . v_s), an image carrying its parent's velocity.  mU, mW, mJ: the magnitudes.
 * Also the frame's energy and its magnitude (energy, me: the sums the same loop makes).  sc_r: as uf3o_site_rows_x.
 */
int uf3o_site_terms_x(const uf3o_spec *s, const uf3o_frame *f, const double *c1, const double *c2, const double *c3, double sc_r,
                      const double *vel, real *U, real *W, real *J, double *mU, double *mW, double *mJ, real *energy, double *me) {
    int N = f->n_atoms;
    sink_t k = {.sc_r = sc_r, .n = N, .vel = vel, .U = U, .W = W, .J = vel ? J : NULL, .mU = mU, .mW = mW, .mJ = mJ};
    for (int q = 0; q < N; q++) { U[q] = 0.0; mU[q] = 0.0; }
    for (int q = 0; q < 9 * N; q++) { W[q] = 0.0; mW[q] = 0.0; }
    if (k.J) for (int q = 0; q < 3 * N; q++) { J[q] = 0.0; mJ[q] = 0.0; }
    return eval_worker(s, f, c1, c2, c3, energy, NULL, NULL, me, NULL, NULL, &k);
}

/*
 * Second derivatives of the evaluator's energy (uf3_hessian.h: real i with every image j in the pair range, real centres with
 * unordered pairs of their 3-body neighbours; an image moves with its parent, par = supercell index mod N): H [3N][3N],
 * mixed [3N][6] = d2E / dx dt_v, born [6][6] = d2E / dt_u dt_v at fixed fractional coordinates (t the strain of
 * uf3o_eval_virial), and their magnitudes.  mixed / born may be NULL (each with its magnitude).
 */
int uf3o_hessian_x(const uf3o_spec *s, const uf3o_frame *f, const double *c1, const double *c2, const double *c3, double sc_r,
                   real *H, real *mixed, real *born, double *mH, double *mL, double *mB) {
    size_t n3 = 3 * (size_t)f->n_atoms;
    sink_t k = {.sc_r = sc_r, .n = f->n_atoms, .H = H, .L = mixed, .B = born, .mH = mH, .mL = mL, .mB = mB};
    for (size_t q = 0; q < n3 * n3; q++) { H[q] = 0.0; mH[q] = 0.0; }
    if (mixed) for (size_t q = 0; q < n3 * 6; q++) { mixed[q] = 0.0; mL[q] = 0.0; }
    if (born) for (int q = 0; q < 36; q++) { born[q] = 0.0; mB[q] = 0.0; }
    return eval_worker(s, f, c1, c2, c3, NULL, NULL, NULL, NULL, NULL, NULL, &k);
}

/*
 * Energy differences of Monte Carlo moves on fixed positions (uf3_mc.h: mc_delta through k_mc_delta and k_mc_trials).
 * A move is a swap of the species of the real atoms i and j (mode 0; j_or_species holds j) or the transmutation of atom i to the
 * atomic number j_or_species (mode 1).  T = {i, j} or {i}, by real atom; z' is z after the move.
 *
 *     dE = E_touch(z') - E_touch(z),   E_touch = the sum of exactly those terms of eval_worker's term loop -- one-body terms, directed
 *          pair terms (real i, supercell j), triplets of real centres -- whose parent atoms, centre included, contain an atom of T.
 *
 * Every other term has the same value before and after the move, so dE is the difference of the two whole energies; it is never
 * formed from them.  The loop runs twice, once per species assignment, with the sink of touch_t.
 *
 * The magnitude.  An fp64 evaluation of dE by ANY bookkeeping (the device's weights 2 and 1 on pair entries, its lists of
 * affected centres) adds and subtracts the touched terms of both assignments, each computed from its own distances.  By the
 * definition at the top of this file each touched term t contributes |t|_abs + sum_r rho_r |dt/dr|_abs -- the mval the loop
 * already hands to its sinks -- whichever sign it enters with, and a term of z is as much an operand as a term of z':
 *
 *     M = M_touch(z') + M_touch(z),   M_touch = the sum of mval over the same terms as E_touch.
 *
 * The untouched terms cancel exactly before they are ever computed and must NOT enter M: with them M would be M_e(z) + M_e(z'),
 * of the order of the frame's energy, and the bound would again hide a missing term.  M <= M_e(z) + M_e(z') always, strictly for
 * every frame with an atom out of reach of T.
 *
 * A move with i == j, or between like species (a transmutation to the atom's own species), changes no term: dE = 0 and M = 0
 * exactly, without a walk.  Swapping (i, j) and (j, i) is the same T and the same z': the same bits.
 *
 * terms (may be NULL; only with n_moves == 1): [term_cap][UF3O_MC_TERM_W] the records of touch_t for both passes; n_terms [1] the
 * number of terms met (may exceed term_cap: call again).
 */
static int mc_worker(const uf3o_spec *s, const uf3o_frame *f, const double *c1, const double *c2, const double *c3,
                     int64_t n_moves, const int *mi, const int *mj, int mode, real *dE, double *M,
                     double *terms, int64_t term_cap, int64_t *n_terms) {
    int N = f->n_atoms, rc = 0;
    if (mode != 0 && mode != 1) return 3;
    if (terms && n_moves != 1) return 3;
    for (int64_t q = 0; q < n_moves; q++) {
        if (mi[q] < 0 || mi[q] >= N) return 3;
        if (mode == 0 ? (mj[q] < 0 || mj[q] >= N) : species_index(s, mj[q]) < 0) return 3;
    }
    unsigned char *touch = (unsigned char *)calloc((size_t)(N > 0 ? N : 1), 1), *reach = (unsigned char *)calloc((size_t)(N > 0 ? N : 1), 1);
    int *zn = (int *)malloc(sizeof(int) * (size_t)(N > 0 ? N : 1));
    if (n_terms) *n_terms = 0;
    for (int64_t q = 0; q < n_moves && !rc; q++) {
        int i = mi[q], j = mode == 0 ? mj[q] : -1;
        dE[q] = 0.0; M[q] = 0.0;
        if (mode == 0 ? (i == j || f->z[i] == f->z[j]) : f->z[i] == mj[q]) continue;
        memcpy(zn, f->z, sizeof(int) * (size_t)N);
        if (mode == 0) { zn[i] = f->z[j]; zn[j] = f->z[i]; } else zn[i] = mj[q];
        memset(touch, 0, (size_t)N);
        touch[i] = 1;
        if (j >= 0) touch[j] = 1;
        uf3o_frame fn = *f;
        fn.z = zn;
        touch_t t = {.touch = touch, .reach = reach, .rec = terms, .cap = term_cap};
        sink_t k = {.n = N, .mc = &t};
        real e[2] = {0.0, 0.0};
        double m[2] = {0.0, 0.0};
        for (int pass = 0; pass < 2 && !rc; pass++) {
            t.E = 0.0; t.M = 0.0; t.pass = pass;
            rc = eval_worker(s, pass ? &fn : f, c1, c2, c3, NULL, NULL, NULL, NULL, NULL, NULL, &k);
            e[pass] = t.E; m[pass] = t.M;
        }
        dE[q] = e[1] - e[0];
        M[q] = m[1] + m[0];
        if (n_terms) *n_terms = t.n_rec;
    }
    free(touch); free(reach); free(zn);
    return rc;
}

int uf3o_mc_delta_x(const uf3o_spec *s, const uf3o_frame *f, const double *c1, const double *c2, const double *c3,
                    int64_t n_moves, const int *i, const int *j_or_species, int mode, real *dE, double *M) {
    return mc_worker(s, f, c1, c2, c3, n_moves, i, j_or_species, mode, dE, M, NULL, 0, NULL);
}

/* one move with the records of its terms (touch_t) */
int uf3o_mc_terms_x(const uf3o_spec *s, const uf3o_frame *f, const double *c1, const double *c2, const double *c3,
                    int i, int j_or_species, int mode, real *dE, double *M, double *terms, int64_t term_cap, int64_t *n_terms) {
    return mc_worker(s, f, c1, c2, c3, 1, &i, &j_or_species, mode, dE, M, terms, term_cap, n_terms);
}
