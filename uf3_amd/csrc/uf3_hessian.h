// uf3_hessian.h -- analytic second derivatives of the UF3 energy of one frame (uf3_hessian[_dev]): the Hessian H [3R][3N] of
// the row atoms, the mixed position / strain derivatives and the clamped-ion (Born) strain term.  gfx950, fp64.
//
// Energy (the evaluator's): sum over real i and every image j of the pair term phi(r_ij), plus sum over real centres i and
// unordered pairs {j, k} of 3-body neighbours of V(r_ij, r_ik, r_jk); images move with their parent atom.  Each term is
// differentiated in leg space first (gradient g_l, symmetric leg Hessian K_ll', from the B-spline values, first and second
// derivatives), then the chain rule: dr/dx = +-u, d2r/dx2 = +-(I - uu^T) / r, dr/dt_v = d_a d_b / r.
//
// Traversal: row owner.  One thread owns row atom m and visits every (term, slot of m in the term) once: its pair bonds,
// its triplets as centre, and its triplets as a neighbour (through the lists of the centres in its own 3-body list).  It adds
// only the blocks of its own slot, so no two threads write the same element: no atomics, the rows are bitwise repeatable,
// and row slabs of a frame are the rows of the whole call.
#pragma once
#include "uf3_device.h"

// one neighbour image of an atom: vector from the atom to the image, its length, the parent atom, the packed integer image
// shift and flags (bit 0: inside the pair range of the two species, bit 1: 3-body neighbour).  The shift is that of the WRAPPED
// frame: with both atoms folded into the cell (hess_home_cell), the image of j that this entry is lies at wrapped(j) + shift .
// cell as seen from wrapped(i).  On a frame whose atoms lie inside their cell that is the shift applied to the positions as
// given; an atom outside its cell counts as its image inside, also where the shift decides a number (supercell_before on a
// symmetry-1 trio).  Reverse entries carry the negated shift either way (k_hessian's lookup).
struct __attribute__((aligned(16))) HessNbr {
    double dx, dy, dz, r;
    int j, shp, spec, flags;
};

struct HessArgs {
    const BasisDev *B;
    const double *pos;        // [N][3] as given (not wrapped)
    const int *spec;          // [N] species index
    int natoms;
    double cell[9];           // lattice rows
    double inv[9];            // inverse of the completed cell: frac_k = sum_j d_j inv[3j + k]
    int per[3], nimg[3];      // periodic flag; images tried per side around the nearest one
    int cap;                  // list capacity per atom
    int *cnt;                 // [N]
    int *bad;                 // set by the count pass when an image shift does not fit pack3's fields (|s| > 500)
    HessNbr *ent;             // [N][cap]
    const double *c2, *c3;    // pair coefficients (concatenated), full 3-body grids
    long long row_begin, row_end;
    long long ld;             // 3N: row stride of hess
    double *hess;             // [3R][3N], zeroed
    double *mixed;            // [3R][6], zeroed, or null
    double *born_part;        // [R][36], zeroed, or null: each row atom's share (its pair bonds and its triplets as centre)
};

// values, first and second derivatives of basis functions i-3 .. i at x (the de Boor triangle of bspline4, with the
// derivatives of the quadratic pieces carried one level further)
__device__ __forceinline__ void bspline4_d2(const KnotRec &k, double x, double *v, double *d, double *dd) {
    double l1 = x - k.t[2], l2 = x - k.t[1], l3 = x - k.t[0];
    double r1 = k.t[3] - x, r2 = k.t[4] - x, r3 = k.t[5] - x;
    const double n0 = r1 * k.r[0], n1 = l1 * k.r[0];
    double tmp = n0 * k.r[1];
    const double q0 = r1 * tmp;
    double saved = l2 * tmp;
    tmp = n1 * k.r[2];
    const double q1 = saved + r2 * tmp, q2 = l1 * tmp;
    tmp = q0 * k.r[3];
    v[0] = r1 * tmp; saved = l3 * tmp;
    tmp = q1 * k.r[4];
    v[1] = saved + r2 * tmp; saved = l2 * tmp;
    tmp = q2 * k.r[5];
    v[2] = saved + r3 * tmp;
    v[3] = l1 * tmp;
    const double a = 3.0 * q0 * k.r[3], b = 3.0 * q1 * k.r[4], c = 3.0 * q2 * k.r[5];
    d[0] = -a; d[1] = a - b; d[2] = b - c; d[3] = c;
    // quadratic pieces: q0' = -2 n0 r1, q1' = 2 n0 r1 - 2 n1 r2, q2' = 2 n1 r2
    const double dq0 = -2.0 * n0 * k.r[1], dq1 = 2.0 * n0 * k.r[1] - 2.0 * n1 * k.r[2], dq2 = 2.0 * n1 * k.r[2];
    const double a2 = 3.0 * dq0 * k.r[3], b2 = 3.0 * dq1 * k.r[4], c2 = 3.0 * dq2 * k.r[5];
    dd[0] = -a2; dd[1] = a2 - b2; dd[2] = b2 - c2; dd[3] = c2;
}

// The cell an atom lies in, per periodic axis: floor of its fractional coordinate.  An atom inside its cell or within
// HESS_FACE_EPS (fractional) of one of its faces stays where it is given, as the reference takes it: a coordinate that is 0 or 1
// up to rounding (an atom on a face of a skewed cell) must not hop to the neighbouring cell.
#define HESS_FACE_EPS 1e-9
__device__ __forceinline__ void hess_home_cell(const HessArgs &A, double x, double y, double z, int *w) {
    for (int k = 0; k < 3; k++) {
        const double f = x * A.inv[k] + y * A.inv[3 + k] + z * A.inv[6 + k];
        const bool stays = !A.per[k] || (f >= -HESS_FACE_EPS && f < 1.0 + HESS_FACE_EPS);
        w[k] = stays ? 0 : (int)fmin(fmax(floor(f), -1.0e6), 1.0e6);
    }
}

// ---- neighbour lists: one wave per atom, lanes over the other atoms, every image in reach of each -------------------------
// WRITE = false: counts only.  Entries in (atom, image, lane) order: the same lists on every call.  CHECK: flag image shifts
// beyond pack3's range.  A device function of one frame's arguments; its one kernel is k_flux_lists (uf3_flux.h), which puts a
// HessArgs together per frame of a batch on the device.  The Hessian's frame is a batch of one.
template <bool WRITE, bool CHECK>
__device__ __forceinline__ void hess_lists_atom(const HessArgs &A, int i, int lane) {
    const BasisDev *B = A.B;
    const double xi = A.pos[3 * (size_t)i], yi = A.pos[3 * (size_t)i + 1], zi = A.pos[3 * (size_t)i + 2];
    const int si = A.spec[i];
    int wi[3];
    hess_home_cell(A, xi, yi, zi, wi);
    const double s3_lo = B->s3_lo, s3_hi = B->s3_hi;
    const bool has3 = B->T > 0;
    const int n0 = A.per[0] ? A.nimg[0] : 0, n1 = A.per[1] ? A.nimg[1] : 0, n2 = A.per[2] ? A.nimg[2] : 0;
    int count = 0;
    HessNbr *out = A.ent + (size_t)i * A.cap;
    for (int j0 = 0; j0 < A.natoms; j0 += WAVE) {
        const int j = j0 + lane;
        const bool live = j < A.natoms;
        const int jj = live ? j : i;
        const double ex = A.pos[3 * (size_t)jj] - xi, ey = A.pos[3 * (size_t)jj + 1] - yi, ez = A.pos[3 * (size_t)jj + 2] - zi;
        const int sj = A.spec[jj];
        int base[3], wj[3];
        hess_home_cell(A, A.pos[3 * (size_t)jj], A.pos[3 * (size_t)jj + 1], A.pos[3 * (size_t)jj + 2], wj);
        for (int k = 0; k < 3; k++) {
            const double f = ex * A.inv[k] + ey * A.inv[3 + k] + ez * A.inv[6 + k];
            base[k] = A.per[k] ? -(int)rint(f) : 0;
            wj[k] -= wi[k];                                   // what the wrapped frame's shift has over the one applied here
        }
        const int p = B->pair_of[si * UF3_MAX_SPECIES + sj];
        const double p_lo = p >= 0 ? B->pairs[p].s_lo : 0.0, p_hi = p >= 0 ? B->pairs[p].s_hi : -1.0;
        for (int a = -n0; a <= n0; a++)
            for (int b = -n1; b <= n1; b++)
                for (int c = -n2; c <= n2; c++) {
                    const int S0 = base[0] + a, S1 = base[1] + b, S2 = base[2] + c;
                    const double dx = ex + S0 * A.cell[0] + S1 * A.cell[3] + S2 * A.cell[6];
                    const double dy = ey + S0 * A.cell[1] + S1 * A.cell[4] + S2 * A.cell[7];
                    const double dz = ez + S0 * A.cell[2] + S1 * A.cell[5] + S2 * A.cell[8];
                    const double s = norm3_sq_rn(dx, dy, dz);
                    const bool self = jj == i && S0 == 0 && S1 == 0 && S2 == 0;
                    const bool in2 = s > p_lo && s < p_hi;
                    const bool in3 = has3 && s > s3_lo && s <= s3_hi;
                    const bool ok = live && !self && (in2 || in3);
                    // (the reverse-shift lookup of k_hessian compares packed shifts: a shift beyond pack3's +-511 would alias)
                    const int T0 = S0 + wj[0], T1 = S1 + wj[1], T2 = S2 + wj[2];
                    if (CHECK && ok && (abs(S0) > 500 || abs(S1) > 500 || abs(S2) > 500 || abs(T0) > 500 || abs(T1) > 500 || abs(T2) > 500))
                        *A.bad = 1;
                    const unsigned long long mask = __ballot(ok);
                    if (WRITE && ok) {
                        const int slot = count + mbcnt(mask);
                        if (slot < A.cap) {
                            HessNbr e;
                            e.dx = dx; e.dy = dy; e.dz = dz; e.r = sqrt(s);
                            e.j = j; e.shp = pack3(T0, T1, T2); e.spec = sj; e.flags = (in2 ? 1 : 0) | (in3 ? 2 : 0);
                            out[slot] = e;
                        }
                    }
                    count += __popcll(mask);
                }
    }
    if (lane == 0) A.cnt[i] = count;
}

// ---- per-term derivatives -------------------------------------------------------------------------------------------------
// strain direction v applied to a vector d: (E_v d) with E_v = d eps / d t_v (eps_ab = eps_ba = t / 2 off the diagonal)
__device__ __forceinline__ void strain_dir(int v, const double *d, double *o) {
    o[0] = o[1] = o[2] = 0.0;
    if (v < 3) { o[v] = d[v]; return; }
    const int a = v == 3 ? 1 : 0, b = v == 5 ? 1 : 2;      // (yz, xz, xy)
    o[a] = 0.5 * d[b]; o[b] = 0.5 * d[a];
}
__device__ __forceinline__ void voigt_ab(int v, int &a, int &b) {
    if (v < 3) { a = b = v; return; }
    a = v == 3 ? 1 : 0; b = v == 5 ? 1 : 2;
}

// One term with NL legs (1: pair, 3: triplet), legs q from slot lf[q] to slot lt[q] with vectors d[q], lengths r[q], leg
// gradient g and leg Hessian K (row-major NL x NL).  Adds the blocks of slot s (row atom m) to the columns of the slots'
// parents par[], scaled by w; its mixed derivative, scaled by w, to mix[3][6]; with bo, the term's strain second derivative
// (unscaled) to bo[36].
template <int NL>
__device__ __forceinline__ void add_term(const HessArgs &A, double *Hm, double *mix, double *bo, int s, const int *par,
                                         const int *lf, const int *lt, const double (*d)[3], const double *r, const double *g,
                                         const double *K, double w) {
    constexpr int NS = NL == 1 ? 2 : 3;
    double u[NL][3], ir[NL], sg[NL][NS];
    for (int q = 0; q < NL; q++) {
        ir[q] = 1.0 / r[q];
        for (int k = 0; k < 3; k++) u[q][k] = d[q][k] * ir[q];
        for (int t = 0; t < NS; t++) sg[q][t] = (t == lt[q] ? 1.0 : 0.0) - (t == lf[q] ? 1.0 : 0.0);
    }
    // R[q'] = sum_q K_qq' sg_qs u_q
    double R[NL][3];
    for (int q2 = 0; q2 < NL; q2++)
        for (int k = 0; k < 3; k++) {
            double acc = 0.0;
            for (int q = 0; q < NL; q++) acc += K[q * NL + q2] * sg[q][s] * u[q][k];
            R[q2][k] = acc;
        }
    for (int t = 0; t < NS && Hm; t++) {
        double blk[3][3];
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                double acc = 0.0;
                for (int q = 0; q < NL; q++) {
                    acc += sg[q][t] * R[q][a] * u[q][b];
                    const double c = g[q] * sg[q][s] * sg[q][t] * ir[q];
                    acc += c * ((a == b ? 1.0 : 0.0) - u[q][a] * u[q][b]);
                }
                blk[a][b] = w * acc;
            }
        double *col = Hm + 3 * (size_t)par[t];
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) col[a * A.ld + b] += blk[a][b];
    }
    if (mix || bo) {
        // wq[q][v] = d r_q / d t_v
        double wq[NL][6];
        for (int q = 0; q < NL; q++)
            for (int v = 0; v < 6; v++) { int a, b; voigt_ab(v, a, b); wq[q][v] = d[q][a] * d[q][b] * ir[q]; }
        if (mix)
            for (int v = 0; v < 6; v++) {
                double acc[3] = {0.0, 0.0, 0.0};
                for (int q = 0; q < NL; q++) {
                    if (sg[q][s] == 0.0) continue;
                    double kw = 0.0;
                    for (int q2 = 0; q2 < NL; q2++) kw += K[q * NL + q2] * wq[q2][v];
                    double ed[3];
                    strain_dir(v, d[q], ed);
                    const double ue = u[q][0] * ed[0] + u[q][1] * ed[1] + u[q][2] * ed[2];
                    for (int k = 0; k < 3; k++) acc[k] += sg[q][s] * (u[q][k] * kw + g[q] * (ed[k] - u[q][k] * ue) * ir[q]);
                }
                for (int k = 0; k < 3; k++) mix[k * 6 + v] += w * acc[k];
            }
        if (bo)
            // d2 r / dt_u dt_v = (E_u d) . (E_v d) / r - w_u w_v / r  (the leg vector is linear in t)
            for (int v1 = 0; v1 < 6; v1++)
                for (int v2 = 0; v2 < 6; v2++) {
                    double acc = 0.0;
                    for (int q = 0; q < NL; q++) {
                        double kw = 0.0;
                        for (int q2 = 0; q2 < NL; q2++) kw += K[q * NL + q2] * wq[q2][v2];
                        double e1[3], e2[3];
                        strain_dir(v1, d[q], e1);
                        strain_dir(v2, d[q], e2);
                        const double dw = (e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2] - wq[q][v1] * wq[q][v2]) * ir[q];
                        acc += wq[q][v1] * kw + g[q] * dw;
                    }
                    bo[v1 * 6 + v2] += acc;
                }
    }
}

// value-free triplet derivatives: gradient g[3] and leg Hessian K[9] of V(rl, rm, rn); false outside the legs' supports
__device__ __forceinline__ bool trio_d2(const BasisDev *B, const double *c3, int trio, double rl, double rm, double rn, double *g,
                                        double *K) {
    const TrioDev *td = B->trios + trio;
    const LegDev l0 = td->leg[0], l1 = td->leg[1], l2 = td->leg[2];
    if (!((rl > l0.t0) & (rl < l0.tlast) & (rm > l1.t0) & (rm < l1.tlast) & (rn > l2.t0) & (rn < l2.tlast))) return false;
    KnotRec kl, km, kn;
    const int il = load_interval<0>(B->recs, l0, rl, kl), im = load_interval<0>(B->recs, l1, rm, km),
              in = load_interval<0>(B->recs, l2, rn, kn);
    double vl[4], dl[4], el[4], vm[4], dm[4], em[4], vn[4], dn[4], en[4];
    bspline4_d2(kl, rl, vl, dl, el);
    bspline4_d2(km, rm, vm, dm, em);
    bspline4_d2(kn, rn, vn, dn, en);
    const int dim_m = td->dim_m, dim_n = td->dim_n, mn = dim_m * dim_n;
    const double *c = c3 + td->lut_off + (size_t)(il - 3) * mn + (im - 3) * dim_n + (in - 3);
    double g0 = 0, g1 = 0, g2 = 0, k00 = 0, k01 = 0, k02 = 0, k11 = 0, k12 = 0, k22 = 0;
    for (int a = 0; a < 4; a++) {
        double s_vv = 0, s_dv = 0, s_vd = 0, s_ev = 0, s_dd = 0, s_ve = 0;   // over (m, n): v_m v_n, d_m v_n, v_m d_n, e_m v_n, d_m d_n, v_m e_n
        for (int b = 0; b < 4; b++) {
            const double *row = c + a * mn + b * dim_n;
            double sv = 0, sd = 0, se = 0;
            for (int w = 0; w < 4; w++) { sv += row[w] * vn[w]; sd += row[w] * dn[w]; se += row[w] * en[w]; }
            s_vv += vm[b] * sv; s_dv += dm[b] * sv; s_vd += vm[b] * sd; s_ev += em[b] * sv; s_dd += dm[b] * sd; s_ve += vm[b] * se;
        }
        g0 += dl[a] * s_vv; g1 += vl[a] * s_dv; g2 += vl[a] * s_vd;
        k00 += el[a] * s_vv; k01 += dl[a] * s_dv; k02 += dl[a] * s_vd;
        k11 += vl[a] * s_ev; k12 += vl[a] * s_dd; k22 += vl[a] * s_ve;
    }
    g[0] = g0; g[1] = g1; g[2] = g2;
    K[0] = k00; K[1] = k01; K[2] = k02; K[3] = k01; K[4] = k11; K[5] = k12; K[6] = k02; K[7] = k12; K[8] = k22;
    return true;
}

// the triplet of centre c with list entries ea, eb (positions ia != ib in c's list): legs in the evaluator's order
// (trio_swap_legs, uf3_device.h; NOT by list position where the order decides a number: the lists are in (atom, image offset
// around the nearest image) order), equal species on equal legs by list position as ever.  Slot of row atom m = the slot of
// entry `mine` (0: the centre itself)
__device__ __forceinline__ void hess_triplet(const HessArgs &A, double *Hm, double *mix, double *bo, int c, const HessNbr &ea, int ia,
                                             const HessNbr &eb, int ib, int mine) {
    const BasisDev *B = A.B;
    const bool swap = trio_swap_legs(B, A.spec[c], ea, eb, ia > ib);
    const HessNbr &ej = swap ? eb : ea, &ek = swap ? ea : eb;
    const int trio = B->trio_of[(A.spec[c] * UF3_MAX_SPECIES + ej.spec) * UF3_MAX_SPECIES + ek.spec];
    if (trio < 0) return;
    double d[3][3] = {{ej.dx, ej.dy, ej.dz}, {ek.dx, ek.dy, ek.dz}, {ek.dx - ej.dx, ek.dy - ej.dy, ek.dz - ej.dz}};
    double r[3] = {ej.r, ek.r, norm3_rn(d[2][0], d[2][1], d[2][2])};
    double g[3], K[9];
    if (!trio_d2(B, A.c3, trio, r[0], r[1], r[2], g, K)) return;
    const int par[3] = {c, ej.j, ek.j};
    const int lf[3] = {0, 0, 1}, lt[3] = {1, 2, 2};
    const int s = mine == 0 ? 0 : ((mine == 1) != swap ? 1 : 2);      // mine: 1 = entry ea, 2 = entry eb
    add_term<3>(A, Hm, mix, s == 0 ? bo : nullptr, s, par, lf, lt, d, r, g, K, 1.0);
}

__global__ void __launch_bounds__(64) k_hessian(HessArgs A) {
    const long long m = A.row_begin + (long long)blockIdx.x * 64 + threadIdx.x;
    if (m >= A.row_end) return;
    const BasisDev *B = A.B;
    const long long row = m - A.row_begin;
    double *Hm = A.hess + (size_t)row * 3 * A.ld;
    double *mix = A.mixed ? A.mixed + (size_t)row * 18 : nullptr;
    double *bo = A.born_part ? A.born_part + (size_t)row * 36 : nullptr;
    const int sm = A.spec[m];
    const int n = min(A.cnt[m], A.cap);
    const HessNbr *L = A.ent + (size_t)m * A.cap;
    // pairs: (m, image of j) with m in slot 0, and (j, image of m) with m in slot 1 -- the same block twice
    for (int e = 0; e < n; e++) {
        const HessNbr en = L[e];
        if (!(en.flags & 1)) continue;
        const int p = B->pair_of[sm * UF3_MAX_SPECIES + en.spec];
        const PairDev &pd = B->pairs[p];
        KnotRec kr;
        const int i = load_interval<0>(B->recs, pd.leg, en.r, kr);
        double v[4], dv[4], ddv[4];
        bspline4_d2(kr, en.r, v, dv, ddv);
        const double *cf = A.c2 + (B->pair_col[sm * UF3_MAX_SPECIES + en.spec] - B->S) + (i - 3);
        double g = 0, k = 0;
        for (int q = 0; q < 4; q++) { g += cf[q] * dv[q]; k += cf[q] * ddv[q]; }
        const double d[1][3] = {{en.dx, en.dy, en.dz}};
        const double r[1] = {en.r};
        const int par[2] = {(int)m, en.j}, lf[1] = {0}, lt[1] = {1};
        add_term<1>(A, Hm, mix, bo, 0, par, lf, lt, d, r, &g, &k, 2.0);      // (the Born share is not scaled: the directed term once)
    }
    if (B->T == 0) return;
    // triplets with m as centre
    for (int a = 0; a < n; a++) {
        const HessNbr ea = L[a];
        if (!(ea.flags & 2)) continue;
        for (int b = a + 1; b < n; b++) {
            const HessNbr eb = L[b];
            if (!(eb.flags & 2)) continue;
            hess_triplet(A, Hm, mix, bo, (int)m, ea, a, eb, b, 0);
        }
    }
    // triplets with an image of m as a neighbour: centre c = a 3-body neighbour of m, m's image there at the reverse shift
    for (int a = 0; a < n; a++) {
        const HessNbr ea = L[a];
        if (!(ea.flags & 2)) continue;
        const int c = ea.j;
        int s0, s1, s2;
        unpack3(ea.shp, s0, s1, s2);
        const int back = pack3(-s0, -s1, -s2);
        const int nc = min(A.cnt[c], A.cap);
        const HessNbr *Lc = A.ent + (size_t)c * A.cap;
        int me = -1;
        for (int e = 0; e < nc; e++)
            if (Lc[e].j == (int)m && Lc[e].shp == back) { me = e; break; }
        if (me < 0 || !(Lc[me].flags & 2)) continue;
        const HessNbr em = Lc[me];
        for (int f = 0; f < nc; f++) {
            if (f == me) continue;
            const HessNbr ef = Lc[f];
            if (!(ef.flags & 2)) continue;
            hess_triplet(A, Hm, mix, nullptr, c, em, me, ef, f, 1);
        }
    }
}

// B = sum of the row atoms' shares, in one fixed order: one workgroup per component, strided partial sums, a fixed tree
__global__ void __launch_bounds__(256) k_hess_born_sum(const double *part, long long n, double *out) {
    __shared__ double s[256];
    const int comp = blockIdx.x, t = threadIdx.x;
    double acc = 0.0;
    for (long long i = t; i < n; i += 256) acc += part[(size_t)i * 36 + comp];
    s[t] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) s[t] += s[t + w];
        __syncthreads();
    }
    if (t == 0) out[comp] = s[0];
}

// species index of every atom (-1 unknown) and a flag for the host
__global__ void __launch_bounds__(256) k_hess_species(const BasisDev *B, const int32_t *z, int n, int *spec, int *bad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int zz = z[i];
    const int s = (zz >= 0 && zz < 120) ? B->z2s[zz] : -1;
    spec[i] = s;
    if (s < 0) *bad = 1;
}
