// uf3_phonon.h -- phonons on a q-mesh (uf3_phonon_mesh / _dos / _thermo[_dev]): eigenvalues of the dynamical matrix D(q) at
// every q-point from the force-constant rows uf3_hessian writes, the density of states and the harmonic thermodynamics.
// gfx950, fp64.  Nothing here depends on the potential.
//
// D(q), per block (i, j) of primitive atoms: D_ij = sum over terms (i, p, n, w) with p mod N = j of
// w exp(2 pi i q.n) Phi[i, p] / sqrt(m_i m_j), then (D + D^H) / 2.  n is the integer lattice triple of the chosen image, q the
// reduced wave vector: q.n is reduced mod 1 axis by axis before sincospi, there is no Cartesian round trip.  The host sorts
// the terms by block (a stable counting sort), so that one owner sums a block in the caller's term order: no atomics, the
// eigenvalues are bitwise repeatable and do not depend on how a mesh is cut into calls.
//
// Two eigenvalue kernels, both cyclic complex Jacobi, stopped at off(D)_F <= 2^-52 |D|_F, PH_MAX_SWEEPS as a guard:
//   k_ph_mesh_lane<N>  3N <= 6: one lane per q-point, the upper triangle in registers, every index a compile-time constant
//   k_ph_mesh_wave     3N <= PH_MAX_DIM: one wave per q-point, D(q) in LDS (16 (3N)^2 bytes), round-robin pairing --
//                      floor(3N / 2) disjoint rotations per step, lanes over (rotation, row / column element)
// A pivot with |a_pq| <= 2^-52 |D|_F / 3N is left alone (threshold Jacobi): n^2 such entries pass the stopping test, and rotating
// an exactly degenerate diagonal pair by 45 degrees on a pivot that is rounding noise -- which crystal symmetry recreates in
// every sweep at zone-boundary points -- shuffles the large entries and turns quadratic convergence into halving per sweep.
// One rotation on the pivot (p, q), a_pq = b u with b = |a_pq|: J = diag(1, conj u) R, R the real Jacobi rotation that
// diagonalises [[a_pp, b], [b, a_qq]] (t = sgn(th) / (|th| + sqrt(th^2 + 1)), th = (a_qq - a_pp) / 2b); A <- J^H A J.
//
// Eigenvectors (uf3_phonon_mesh_vec / _pdos / _tdisp[_dev]): the <.., true> instances of both kernels start V
// at I, apply V <- V J for every rotation and permute the columns with the eigenvalue sort; their D side is the same statements
// in the same order, so lam and status have the bits of the eigenvalue-only instances.  The lane kernel keeps V in a lane's own
// column of LDS (N = 2: 36 KB a wave), the wave kernel keeps V^T beside D (32 (3N)^2 bytes and the rotation records: N <= 21,
// PH_VEC_MAX_ATOMS; larger cells are refused, there is no global-memory route).  Group velocities come from a second pass over
// the terms while V is at hand (ph_velocity), k_ph_pdos_part / _sum and k_ph_tdisp reduce V over the mesh in fixed order.
#pragma once
#include "uf3_device.h"

#define PH_MAX_ATOMS 32                  // 3N <= 96: 16 * 96^2 = 147 456 bytes of the CU's 160 KiB
#define PH_MAX_DIM (3 * PH_MAX_ATOMS)
#define PH_MAX_SWEEPS 30
#define PH_EPS 2.220446049250313e-16     // 2^-52
#define PH_THZ 15.633302                 // harmonic.THZ: sqrt(eV / (amu A^2)) / 2 pi in THz
#define PH_H 4.135667696e-3              // eV / THz   (CODATA 2018)
#define PH_KB 8.617333262e-5             // eV / K
#define PH_2PI 6.283185307179586
#define PH_VEC_MAX_ATOMS 21              // eigenvectors: V beside D in LDS, 32 (3N)^2 bytes: 3N = 63 is the last size within the CU's 160 KiB

struct __attribute__((aligned(16))) PhTerm {
    int p, n0, n1, n2;                   // supercell atom (column block of fc) and the integer lattice triple
};

struct PhMeshArgs {
    const double *fc;                    // [3N][ld]
    const double *inv_sqrt_mass;         // [N]
    const PhTerm *terms;                 // sorted by block (i, p mod N)
    const double *term_w;
    const int *block_off;                // [N * N + 1]
    const double *q;                     // [nq][3]
    double *lam;                         // [nq][3N]
    int *status;                         // [nq]
    long long nq, ld;
    int natoms;
    // the eigenvector instances only (k_ph_mesh_lane<N, true>, k_ph_mesh_wave<true>); either output may be null
    double *evec;                        // [nq][3N][3N][2]: row, mode, (re, im); column s belongs to lam[s]
    double *gvel;                        // [nq][3N][3]: THz A
    double cell[9];                      // rows: lattice vectors (A)
    double cutoff;                       // THz: modes with |f| <= cutoff get velocity 0
};

// w exp(2 pi i q.n): every product reduced mod 1 before the sum, the sum once more
__device__ __forceinline__ void ph_phase(const PhTerm &t, double w, double q0, double q1, double q2, double &re, double &im) {
    double x0 = q0 * (double)t.n0, x1 = q1 * (double)t.n1, x2 = q2 * (double)t.n2;
    x0 -= rint(x0); x1 -= rint(x1); x2 -= rint(x2);
    double x = x0 + x1 + x2;
    x -= rint(x);
    double s, c;
    sincospi(2.0 * x, &s, &c);
    re = w * c; im = w * s;
}

// the real rotation of the pivot: t, c, s from the diagonal pair and b = |a_pq| > 0
__device__ __forceinline__ void ph_rotation(double app, double aqq, double b, double &t, double &c, double &s) {
    const double th = (aqq - app) / (2.0 * b);
    t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
}

__device__ __forceinline__ double ph_freq(double lam) {
    return (lam > 0.0 ? 1.0 : (lam < 0.0 ? -1.0 : 0.0)) * sqrt(fabs(lam)) * PH_THZ;
}

// Group velocity of one mode from g_a = Re(v^H (dD / dq_a) v), dD / dq_a = sum w (2 pi i n_a) exp(2 pi i q.n) Phi / sqrt(m_i m_j)
// Hermitised like D (Hellmann-Feynman): d lam / d k_c = sum_a g_a cell[a][c], k the Cartesian wave vector without 2 pi, and
// v_c = THZ (d lam / d k_c) / (2 sqrt|lam|) in THz A; 0 for |f| <= cutoff (Gamma's acoustic modes).  Inside a degenerate cluster
// the diagonal depends on the basis the Jacobi sweeps ended in: only the cluster's sum is defined, and nothing here resolves it.
__device__ __forceinline__ void ph_velocity(const PhMeshArgs &A, double lam, double g0, double g1, double g2, double *out) {
    const bool keep = fabs(ph_freq(lam)) > A.cutoff;
    const double sc = keep ? PH_THZ / (2.0 * sqrt(fabs(lam))) : 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) out[c] = keep ? sc * (g0 * A.cell[c] + g1 * A.cell[3 + c] + g2 * A.cell[6 + c]) : 0.0;
}

// a volatile double in LDS: the address space is part of the type, or a volatile access becomes a flat one
typedef __attribute__((address_space(3))) volatile double PhLdsDouble;

// ---- 3N <= 6: one lane per q-point -------------------------------------------------------------------------------------------
// Only the entries r <= c of ar / ai are touched after the build, every index is a constant after unrolling: the arrays
// are registers, there is no scratch.
// VEC: V starts at I and takes V <- V J with every rotation (skipped pivots rotate nothing), its columns follow the sort; then the
// group velocities from a second pass over the terms, one reduced axis at a time (ph_velocity's comment).  The D side of the
// VEC instance is the same statements in the same order: lam and status have the bits of the eigenvalue-only instance.
template <int N, bool VEC = false>
__global__ void __launch_bounds__(64) k_ph_mesh_lane(PhMeshArgs A) {
    constexpr int n = 3 * N;
    const long long iq = (long long)blockIdx.x * 64 + threadIdx.x;
    if (iq >= A.nq) return;
    const double q0 = A.q[3 * iq], q1 = A.q[3 * iq + 1], q2 = A.q[3 * iq + 2];
    double ar[n][n], ai[n][n];
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) {
            double br[9], bi[9];
#pragma unroll
            for (int k = 0; k < 9; k++) br[k] = bi[k] = 0.0;
            const int lo = A.block_off[i * N + j], hi = A.block_off[i * N + j + 1];
            for (int e = lo; e < hi; e++) {
                const PhTerm t = A.terms[e];
                double pr, pi;
                ph_phase(t, A.term_w[e], q0, q1, q2, pr, pi);
                const double *f = A.fc + (size_t)(3 * i) * A.ld + 3 * (size_t)t.p;
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int b = 0; b < 3; b++) {
                        const double v = f[a * A.ld + b];
                        br[3 * a + b] += pr * v; bi[3 * a + b] += pi * v;
                    }
            }
            const double sc = A.inv_sqrt_mass[i] * A.inv_sqrt_mass[j];
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) { ar[3 * i + a][3 * j + b] = br[3 * a + b] * sc; ai[3 * i + a][3 * j + b] = bi[3 * a + b] * sc; }
        }
    // (D + D^H) / 2 into the upper triangle
    double tot = 0.0;
#pragma unroll
    for (int r = 0; r < n; r++) {
        ai[r][r] = 0.0;
        tot += ar[r][r] * ar[r][r];
#pragma unroll
        for (int c = r + 1; c < n; c++) {
            ar[r][c] = 0.5 * (ar[r][c] + ar[c][r]);
            ai[r][c] = 0.5 * (ai[r][c] - ai[c][r]);
            tot += 2.0 * (ar[r][c] * ar[r][c] + ai[r][c] * ai[r][c]);
        }
    }
    const double thr = PH_EPS * sqrt(tot) / n;
    // V: a lane's own column of LDS, sv[2 (r n + c) + (re | im)][lane] -- beside D's 184 registers at N = 2, 72 more for V spill
    // (154 registers, 620 bytes of scratch a lane); lanes never meet, so there is no barrier, every index is a constant and
    // consecutive lanes sit on consecutive banks.  Through a volatile LDS pointer (PhLdsDouble): 8-byte LDS reads stay single.
    __shared__ double ph_sv[VEC ? 2 * n * n : 1][64];
    PhLdsDouble *sv = (PhLdsDouble *)&ph_sv[0][threadIdx.x];
#define PH_VR(r, c) sv[64 * (2 * ((r) * n + (c)))]
#define PH_VI(r, c) sv[64 * (2 * ((r) * n + (c)) + 1)]
    if constexpr (VEC) {
#pragma unroll
        for (int r = 0; r < n; r++)
#pragma unroll
            for (int c = 0; c < n; c++) { PH_VR(r, c) = r == c ? 1.0 : 0.0; PH_VI(r, c) = 0.0; }
    }
    int sweeps = 0;
    for (;; sweeps++) {
        double off = 0.0;
#pragma unroll
        for (int r = 0; r < n; r++)
#pragma unroll
            for (int c = r + 1; c < n; c++) off += 2.0 * (ar[r][c] * ar[r][c] + ai[r][c] * ai[r][c]);
        if (off <= PH_EPS * PH_EPS * tot) break;
        if (sweeps == PH_MAX_SWEEPS) { sweeps = -1; break; }
#pragma unroll
        for (int p = 0; p < n - 1; p++)
#pragma unroll
            for (int q = p + 1; q < n; q++) {
                const double xr = ar[p][q], xi = ai[p][q];
                const double b = sqrt(xr * xr + xi * xi);
                if (b <= thr) continue;
                double t, c, s;
                ph_rotation(ar[p][p], ar[q][q], b, t, c, s);
                const double ur = xr / b, ui = xi / b;
                ar[p][p] -= t * b; ar[q][q] += t * b;
                ar[p][q] = 0.0; ai[p][q] = 0.0;
#pragma unroll
                for (int r = 0; r < n; r++) {
                    if (r == p || r == q) continue;
                    // A[r][p], A[r][q] from the upper triangle (conjugate of the stored entry below the diagonal)
                    const double er = r < p ? ar[r][p] : ar[p][r], ei = r < p ? ai[r][p] : -ai[p][r];
                    const double fr = r < q ? ar[r][q] : ar[q][r], fi = r < q ? ai[r][q] : -ai[q][r];
                    const double gr = ur * fr + ui * fi, gi = ur * fi - ui * fr;          // conj(u) A[r][q]
                    const double npr = c * er - s * gr, npi = c * ei - s * gi;
                    const double nqr = s * er + c * gr, nqi = s * ei + c * gi;
                    if (r < p) { ar[r][p] = npr; ai[r][p] = npi; } else { ar[p][r] = npr; ai[p][r] = -npi; }
                    if (r < q) { ar[r][q] = nqr; ai[r][q] = nqi; } else { ar[q][r] = nqr; ai[q][r] = -nqi; }
                }
                if constexpr (VEC) {
#pragma unroll
                    for (int r = 0; r < n; r++) {
                        const double er = PH_VR(r, p), ei = PH_VI(r, p), fr = PH_VR(r, q), fi = PH_VI(r, q);
                        const double gr = ur * fr + ui * fi, gi = ur * fi - ui * fr;          // conj(u) V[r][q]
                        PH_VR(r, p) = c * er - s * gr; PH_VI(r, p) = c * ei - s * gi;
                        PH_VR(r, q) = s * er + c * gr; PH_VI(r, q) = s * ei + c * gi;
                    }
                }
            }
    }
    double d[n];
#pragma unroll
    for (int r = 0; r < n; r++) d[r] = ar[r][r];
#pragma unroll
    for (int i = 0; i < n - 1; i++)
#pragma unroll
        for (int j = 0; j < n - 1 - i; j++) {
            const double lo = fmin(d[j], d[j + 1]), hi = fmax(d[j], d[j + 1]);
            if constexpr (VEC) {
                const bool sw = d[j] > d[j + 1];
#pragma unroll
                for (int r = 0; r < n; r++) {
                    const double xr = PH_VR(r, j), xi = PH_VI(r, j), yr = PH_VR(r, j + 1), yi = PH_VI(r, j + 1);
                    PH_VR(r, j) = sw ? yr : xr; PH_VI(r, j) = sw ? yi : xi;
                    PH_VR(r, j + 1) = sw ? xr : yr; PH_VI(r, j + 1) = sw ? xi : yi;
                }
            }
            d[j] = lo; d[j + 1] = hi;
        }
#pragma unroll
    for (int r = 0; r < n; r++) A.lam[(size_t)iq * n + r] = d[r];
    A.status[iq] = sweeps;
    if constexpr (VEC) {
        if (A.evec) {
            double *o = A.evec + 2 * (size_t)iq * n * n;
#pragma unroll
            for (int r = 0; r < n; r++)
#pragma unroll
                for (int c = 0; c < n; c++) { o[2 * (r * n + c)] = PH_VR(r, c); o[2 * (r * n + c) + 1] = PH_VI(r, c); }
        }
        if (!A.gvel) return;
        // dD / dq_a, a = 0, 1, 2 in turn: the build above with the factor 2 pi i n_a, Hermitised into the upper triangle (ar / ai
        // are free by now); g_s = v_s^H (dD / dq_a) v_s = sum_r H_rr |V_rs|^2 + 2 Re sum_{r < c} conj(V_rs) H_rc V_cs
        double g0[n], g1[n], g2[n];
#pragma unroll
        for (int s = 0; s < n; s++) g0[s] = g1[s] = g2[s] = 0.0;
#pragma unroll 1
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int i = 0; i < N; i++)
#pragma unroll
                for (int j = 0; j < N; j++) {
                    double br[9], bi[9];
#pragma unroll
                    for (int k = 0; k < 9; k++) br[k] = bi[k] = 0.0;
                    const int lo = A.block_off[i * N + j], hi = A.block_off[i * N + j + 1];
                    for (int e = lo; e < hi; e++) {
                        const PhTerm t = A.terms[e];
                        double cr, ci;
                        ph_phase(t, A.term_w[e], q0, q1, q2, cr, ci);
                        const double na = PH_2PI * (double)(a == 0 ? t.n0 : (a == 1 ? t.n1 : t.n2));
                        const double pr = -na * ci, pi = na * cr;
                        const double *f = A.fc + (size_t)(3 * i) * A.ld + 3 * (size_t)t.p;
#pragma unroll
                        for (int x = 0; x < 3; x++)
#pragma unroll
                            for (int y = 0; y < 3; y++) {
                                const double v = f[x * A.ld + y];
                                br[3 * x + y] += pr * v; bi[3 * x + y] += pi * v;
                            }
                    }
                    const double sc = A.inv_sqrt_mass[i] * A.inv_sqrt_mass[j];
#pragma unroll
                    for (int x = 0; x < 3; x++)
#pragma unroll
                        for (int y = 0; y < 3; y++) { ar[3 * i + x][3 * j + y] = br[3 * x + y] * sc; ai[3 * i + x][3 * j + y] = bi[3 * x + y] * sc; }
                }
#pragma unroll
            for (int r = 0; r < n; r++)
#pragma unroll
                for (int c = r + 1; c < n; c++) {
                    ar[r][c] = 0.5 * (ar[r][c] + ar[c][r]);
                    ai[r][c] = 0.5 * (ai[r][c] - ai[c][r]);
                }
#pragma unroll
            for (int s = 0; s < n; s++) {
                double wr[n], wi[n];
#pragma unroll
                for (int r = 0; r < n; r++) { wr[r] = PH_VR(r, s); wi[r] = PH_VI(r, s); }
                double acc = 0.0;
#pragma unroll
                for (int r = 0; r < n; r++) {
                    acc += ar[r][r] * (wr[r] * wr[r] + wi[r] * wi[r]);
#pragma unroll
                    for (int c = r + 1; c < n; c++) {
                        // conj(V_rs) V_cs
                        const double pr = wr[r] * wr[c] + wi[r] * wi[c], pi = wr[r] * wi[c] - wi[r] * wr[c];
                        acc += 2.0 * (ar[r][c] * pr - ai[r][c] * pi);
                    }
                }
                g0[s] = a == 0 ? acc : g0[s]; g1[s] = a == 1 ? acc : g1[s]; g2[s] = a == 2 ? acc : g2[s];
            }
        }
#pragma unroll
        for (int s = 0; s < n; s++) ph_velocity(A, d[s], g0[s], g1[s], g2[s], A.gvel + 3 * ((size_t)iq * n + s));
    }
}

#undef PH_VR
#undef PH_VI

// ---- 3N <= PH_MAX_DIM: one wave per q-point, D(q) in LDS -----------------------------------------------------------------------
struct __attribute__((aligned(16))) PhRot {
    int p, q;                            // p < q; q < 0: nothing to do (the padding index of an odd dimension, or a pivot below the threshold)
    double c, s, ur, ui;
};

__device__ __forceinline__ double ph_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// with vectors: V^T beside D, [n][n | 1] (column s of V is row s here, the odd leading dimension keeps lanes over s off one bank)
__host__ __device__ inline size_t ph_wave_lds(int n, bool vec = false) {
    return sizeof(double2) * (size_t)n * n + sizeof(PhRot) * (size_t)((n + 1) / 2) + (vec ? sizeof(double2) * (size_t)n * (n | 1) : 0);
}

// VEC: V starts at I and takes V <- V J with every step's rotations; V is held transposed, so the update of the columns p, q of V
// is the row phase's access pattern (lanes over (rotation, row of V), consecutive lanes on consecutive addresses) and rides in
// the row phase's loop.  Then lam's rank permutes the columns, and the group velocities come from a second pass over the terms:
// dD / dq_a is built into D's storage one reduced axis at a time and lane s sums v_s^H (dD / dq_a) v_s (3N <= 63: one mode a lane).
// The D side is the same statements in the same order: lam and status have the bits of the eigenvalue-only instance.
template <bool VEC = false>
__global__ void __launch_bounds__(64) k_ph_mesh_wave(PhMeshArgs A) {
    extern __shared__ __attribute__((aligned(16))) char ph_lds[];
    const int N = A.natoms, n = 3 * N, lane = threadIdx.x;
    const long long iq = blockIdx.x;
    double2 *D = (double2 *)ph_lds;                          // [n][n] row-major, (re, im)
    PhRot *rot = (PhRot *)(D + (size_t)n * n);
    const int ldv = n | 1;
    double2 *Vt = (double2 *)(rot + (n + 1) / 2);            // VEC: [n][ldv], Vt[s][r] = V[r][s]
    const double q0 = A.q[3 * iq], q1 = A.q[3 * iq + 1], q2 = A.q[3 * iq + 2];
    // build: one lane per block (i, j), its terms in order, the 3 x 3 sum in registers
    for (int blk = lane; blk < N * N; blk += WAVE) {
        const int i = blk / N, j = blk - i * N;
        double br[9], bi[9];
#pragma unroll
        for (int k = 0; k < 9; k++) br[k] = bi[k] = 0.0;
        const int lo = A.block_off[blk], hi = A.block_off[blk + 1];
        for (int e = lo; e < hi; e++) {
            const PhTerm t = A.terms[e];
            double pr, pi;
            ph_phase(t, A.term_w[e], q0, q1, q2, pr, pi);
            const double *f = A.fc + (size_t)(3 * i) * A.ld + 3 * (size_t)t.p;
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) {
                    const double v = f[a * A.ld + b];
                    br[3 * a + b] += pr * v; bi[3 * a + b] += pi * v;
                }
        }
        const double sc = A.inv_sqrt_mass[i] * A.inv_sqrt_mass[j];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) D[(3 * i + a) * n + 3 * j + b] = make_double2(br[3 * a + b] * sc, bi[3 * a + b] * sc);
    }
    if constexpr (VEC)
        for (int e = lane; e < n * ldv; e += WAVE) {
            const int s = e / ldv, r = e - s * ldv;
            Vt[e] = make_double2(s == r ? 1.0 : 0.0, 0.0);
        }
    __syncthreads();
    // (D + D^H) / 2: the owner of (r, c), r <= c, writes both
    double tot = 0.0;
    for (int e = lane; e < n * n; e += WAVE) {
        const int r = e / n, c = e - r * n;
        if (r > c) continue;
        const double2 x = D[r * n + c], y = D[c * n + r];
        const double vr = 0.5 * (x.x + y.x), vi = r == c ? 0.0 : 0.5 * (x.y - y.y);
        D[r * n + c] = make_double2(vr, vi);
        D[c * n + r] = make_double2(vr, -vi);
        tot += (r == c ? 1.0 : 2.0) * (vr * vr + vi * vi);
    }
    tot = ph_wave_sum(tot);
    __syncthreads();
    const int m = n + (n & 1), npairs = m / 2;
    const double thr = PH_EPS * sqrt(tot) / n;
    int sweeps = 0;
    for (;; sweeps++) {
        double off = 0.0;
        for (int e = lane; e < n * n; e += WAVE) {
            const int r = e / n, c = e - r * n;
            const double2 x = D[e];
            if (r != c) off += x.x * x.x + x.y * x.y;
        }
        off = ph_wave_sum(off);
        if (off <= PH_EPS * PH_EPS * tot) break;
        if (sweeps == PH_MAX_SWEEPS) { sweeps = -1; break; }
        for (int step = 0; step < m - 1; step++) {
            // round robin: index m - 1 stays, the others turn
            for (int k = lane; k < npairs; k += WAVE) {
                int a = k == 0 ? m - 1 : (step + k) % (m - 1), b = k == 0 ? step : (step - k + m - 1) % (m - 1);
                const int p = min(a, b), q = max(a, b);
                PhRot R;
                R.p = p; R.q = -1; R.c = 1.0; R.s = 0.0; R.ur = 1.0; R.ui = 0.0;
                if (q < n) {
                    const double2 x = D[p * n + q];
                    const double bb = sqrt(x.x * x.x + x.y * x.y);
                    if (bb > thr) {
                        double t;
                        ph_rotation(D[p * n + p].x, D[q * n + q].x, bb, t, R.c, R.s);
                        R.ur = x.x / bb; R.ui = x.y / bb; R.q = q;
                    }
                }
                rot[k] = R;
            }
            __syncthreads();
            // columns: A <- A J
            for (int e = lane; e < npairs * n; e += WAVE) {
                const int r = e / npairs, k = e - r * npairs;
                const PhRot R = rot[k];
                if (R.q < 0) continue;
                const double2 x = D[r * n + R.p], y = D[r * n + R.q];
                const double gr = R.ur * y.x + R.ui * y.y, gi = R.ur * y.y - R.ui * y.x;      // conj(u) y
                D[r * n + R.p] = make_double2(R.c * x.x - R.s * gr, R.c * x.y - R.s * gi);
                D[r * n + R.q] = make_double2(R.s * x.x + R.c * gr, R.s * x.y + R.c * gi);
            }
            __syncthreads();
            // rows: A <- J^H A
            for (int e = lane; e < npairs * n; e += WAVE) {
                const int k = e / n, c = e - k * n;
                const PhRot R = rot[k];
                if (R.q < 0) continue;
                const double2 x = D[R.p * n + c], y = D[R.q * n + c];
                const double gr = R.ur * y.x - R.ui * y.y, gi = R.ur * y.y + R.ui * y.x;      // u y
                D[R.p * n + c] = make_double2(R.c * x.x - R.s * gr, R.c * x.y - R.s * gi);
                D[R.q * n + c] = make_double2(R.s * x.x + R.c * gr, R.s * x.y + R.c * gi);
                if constexpr (VEC) {
                    // columns p, q of V <- V J: rows p, q of V^T, c the row of V
                    const double2 vx = Vt[R.p * ldv + c], vy = Vt[R.q * ldv + c];
                    const double hr = R.ur * vy.x + R.ui * vy.y, hi = R.ur * vy.y - R.ui * vy.x;  // conj(u) V[c][q]
                    Vt[R.p * ldv + c] = make_double2(R.c * vx.x - R.s * hr, R.c * vx.y - R.s * hi);
                    Vt[R.q * ldv + c] = make_double2(R.s * vx.x + R.c * hr, R.s * vx.y + R.c * hi);
                }
            }
            __syncthreads();
            // the pivots are zero and the diagonal is real by construction: say so exactly
            for (int k = lane; k < npairs; k += WAVE) {
                const PhRot R = rot[k];
                if (R.q < 0) continue;
                D[R.p * n + R.q] = make_double2(0.0, 0.0);
                D[R.q * n + R.p] = make_double2(0.0, 0.0);
                D[R.p * n + R.p].y = 0.0;
                D[R.q * n + R.q].y = 0.0;
            }
            __syncthreads();
        }
    }
    // ascending by rank (ties by index)
    for (int e = lane; e < n; e += WAVE) {
        const double v = D[e * n + e].x;
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const double u = D[j * n + j].x;
            rank += (u < v || (u == v && j < e)) ? 1 : 0;
        }
        A.lam[(size_t)iq * n + rank] = v;
        if constexpr (VEC) {
            // the rotation records are done with: perm[rank] = column of V, lams[rank] = its eigenvalue
            int *perm = (int *)rot;
            double *lams = (double *)(perm + ((n + 1) & ~1));
            perm[rank] = e; lams[rank] = v;
        }
    }
    if (lane == 0) A.status[iq] = sweeps;
    if constexpr (VEC) {
        const int *perm = (const int *)rot;
        const double *lams = (const double *)(perm + ((n + 1) & ~1));
        __syncthreads();
        if (A.evec) {
            double *o = A.evec + 2 * (size_t)iq * n * n;
            for (int e = lane; e < n * n; e += WAVE) {
                const int r = e / n, s = e - r * n;
                const double2 v = Vt[perm[s] * ldv + r];
                o[2 * e] = v.x; o[2 * e + 1] = v.y;
            }
        }
        if (!A.gvel) return;
        const int col = lane < n ? perm[lane] : 0;
        double g0 = 0.0, g1 = 0.0, g2 = 0.0;
        for (int a = 0; a < 3; a++) {
            // dD / dq_a: the build with the factor 2 pi i n_a, into D's storage (the diagonal was read above: first sync)
            for (int blk = lane; blk < N * N; blk += WAVE) {
                const int i = blk / N, j = blk - i * N;
                double br[9], bi[9];
#pragma unroll
                for (int k = 0; k < 9; k++) br[k] = bi[k] = 0.0;
                const int lo = A.block_off[blk], hi = A.block_off[blk + 1];
                for (int e = lo; e < hi; e++) {
                    const PhTerm t = A.terms[e];
                    double cr, ci;
                    ph_phase(t, A.term_w[e], q0, q1, q2, cr, ci);
                    const double na = PH_2PI * (double)(a == 0 ? t.n0 : (a == 1 ? t.n1 : t.n2));
                    const double pr = -na * ci, pi = na * cr;
                    const double *f = A.fc + (size_t)(3 * i) * A.ld + 3 * (size_t)t.p;
#pragma unroll
                    for (int x = 0; x < 3; x++)
#pragma unroll
                        for (int y = 0; y < 3; y++) {
                            const double v = f[x * A.ld + y];
                            br[3 * x + y] += pr * v; bi[3 * x + y] += pi * v;
                        }
                }
                const double sc = A.inv_sqrt_mass[i] * A.inv_sqrt_mass[j];
#pragma unroll
                for (int x = 0; x < 3; x++)
#pragma unroll
                    for (int y = 0; y < 3; y++) D[(3 * i + x) * n + 3 * j + y] = make_double2(br[3 * x + y] * sc, bi[3 * x + y] * sc);
            }
            __syncthreads();
            for (int e = lane; e < n * n; e += WAVE) {
                const int r = e / n, c = e - r * n;
                if (r > c) continue;
                const double2 x = D[r * n + c], y = D[c * n + r];
                const double hr = 0.5 * (x.x + y.x), hi = r == c ? 0.0 : 0.5 * (x.y - y.y);
                D[r * n + c] = make_double2(hr, hi);
                D[c * n + r] = make_double2(hr, -hi);
            }
            __syncthreads();
            if (lane < n) {
                const double2 *v = Vt + col * ldv;
                double acc = 0.0;
                for (int r = 0; r < n; r++) {
                    double tr = 0.0, ti = 0.0;
                    for (int c = 0; c < n; c++) {
                        const double2 d = D[r * n + c], w = v[c];
                        tr += d.x * w.x - d.y * w.y; ti += d.x * w.y + d.y * w.x;
                    }
                    const double2 w = v[r];
                    acc += w.x * tr + w.y * ti;                  // Re(conj(V_rs) (H v)_r)
                }
                g0 = a == 0 ? acc : g0; g1 = a == 1 ? acc : g1; g2 = a == 2 ? acc : g2;
            }
            __syncthreads();
        }
        if (lane < n) ph_velocity(A, lams[lane], g0, g1, g2, A.gvel + 3 * ((size_t)iq * n + lane));
    }
}

// ---- density of states -------------------------------------------------------------------------------------------------------

// sum of the q-weights (exact in int64 whatever the order): one workgroup
__global__ void __launch_bounds__(256) k_ph_wsum(const long long *wq, long long nq, long long *out) {
    __shared__ long long s[256];
    const int t = threadIdx.x;
    long long acc = 0;
    for (long long i = t; i < nq; i += 256) acc += wq ? wq[i] : 1;
    s[t] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) s[t] += s[t + w];
        __syncthreads();
    }
    if (t == 0) *out = s[0];
}

// numpy's bin rule: edges[b] <= f < edges[b + 1], the last bin closed; integer atomics (exact whatever the order)
__global__ void __launch_bounds__(256) k_ph_hist(const double *lam, const long long *wq, long long n_modes, int n3, const double *edges,
                                                 int n_bins, unsigned long long *counts) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_modes) return;
    const double f = ph_freq(lam[e]);
    if (!(f >= edges[0] && f <= edges[n_bins])) return;
    int lo = 0, hi = n_bins;                 // edges[lo] <= f, f < edges[hi] or f == edges[n_bins]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (f >= edges[mid]) lo = mid; else hi = mid;
    }
    atomicAdd(counts + lo, (unsigned long long)(wq ? wq[e / n3] : 1));
}

// Gaussian smearing: lanes over sample frequencies, a chunk of modes per workgroup streamed through LDS in tiles of 256; each
// lane sums a tile, then the tiles, in order.  part [n_chunks][n_samples].
#define PH_DOS_TILE 256
__global__ void __launch_bounds__(256) k_ph_dos_part(const double *lam, const long long *wq, long long n_modes, int n3, long long chunk,
                                                     const double *samples, int n_samples, double inv_sigma, double *part) {
    __shared__ double sf[PH_DOS_TILE], sw[PH_DOS_TILE];
    const int t = threadIdx.x;
    const int is = blockIdx.x * 256 + t;
    const long long lo = (long long)blockIdx.y * chunk, hi = min(lo + chunk, n_modes);
    const double fs = is < n_samples ? samples[is] : 0.0;
    double acc = 0.0;
    for (long long base = lo; base < hi; base += PH_DOS_TILE) {
        const long long e = base + t;
        __syncthreads();
        sf[t] = e < hi ? ph_freq(lam[e]) : 0.0;
        sw[t] = e < hi ? (double)(wq ? wq[e / n3] : 1) : 0.0;
        __syncthreads();
        const int cnt = (int)min((long long)PH_DOS_TILE, hi - base);
        double sub = 0.0;
        for (int k = 0; k < cnt; k++) {
            const double z = (fs - sf[k]) * inv_sigma;
            sub += sw[k] * exp(-0.5 * z * z);
        }
        acc += sub;
    }
    if (is < n_samples) part[(size_t)blockIdx.y * n_samples + is] = acc;
}

// g = sum of the chunks in order / (sigma sqrt(2 pi) sum w)
__global__ void __launch_bounds__(256) k_ph_dos_sum(const double *part, int n_chunks, int n_samples, double inv_sigma,
                                                    const long long *wsum, double *dos) {
    const int is = blockIdx.x * 256 + threadIdx.x;
    if (is >= n_samples) return;
    double acc = 0.0;
    for (int base = 0; base < n_chunks; base += 32) {
        double sub = 0.0;
        for (int k = base; k < min(base + 32, n_chunks); k++) sub += part[(size_t)k * n_samples + is];
        acc += sub;
    }
    dos[is] = acc * inv_sigma * 0.3989422804014327 / (double)*wsum;
}

// ---- harmonic thermodynamics -------------------------------------------------------------------------------------------------
// One workgroup per temperature, lanes over modes (stride 256), each lane in runs of 32 terms, then a fixed tree.  Modes with
// f <= cutoff are left out of every sum and counted (by weight).  out [nT][4] = F, U (eV), S, C_v (eV / K) per cell.
__global__ void __launch_bounds__(256) k_ph_thermo(const double *lam, const long long *wq, long long n_modes, int n3, const double *T,
                                                   double cutoff, const long long *wsum, double *out, double *zpe_out,
                                                   long long *excluded) {
    __shared__ double s[5][256];
    __shared__ long long sx[256];
    const int t = threadIdx.x;
    const double temp = T[blockIdx.x], kT = PH_KB * temp;
    double acc[5] = {0, 0, 0, 0, 0};
    long long nx = 0;
    for (long long base = t; base < n_modes; base += 256 * 32) {
        double sub[5] = {0, 0, 0, 0, 0};
        for (int k = 0; k < 32; k++) {
            const long long e = base + (long long)k * 256;
            if (e >= n_modes) break;
            const double f = ph_freq(lam[e]);
            const long long wi = wq ? wq[e / n3] : 1;
            if (!(f > cutoff)) { nx += wi; continue; }
            const double w = (double)wi, hf = PH_H * f;
            sub[4] += w * 0.5 * hf;
            if (temp > 0.0) {
                const double x = hf / kT;
                const double ex = exp(-x);                               // e^-x
                const double em = -expm1(-x);                            // 1 - e^-x
                const double l = x < 0.6931471805599453 ? log(em) : log1p(-ex);      // log(1 - e^-x), accurate at both ends
                const double bose = ex / em;                             // 1 / expm1(x)
                sub[0] += w * (0.5 * hf + kT * l);
                sub[1] += w * hf * (0.5 + bose);
                sub[2] += w * PH_KB * (x * bose - l);
                sub[3] += w * PH_KB * x * x * ex / (em * em);
            } else {
                sub[0] += w * 0.5 * hf;
                sub[1] += w * 0.5 * hf;
            }
        }
        for (int k = 0; k < 5; k++) acc[k] += sub[k];
    }
    for (int k = 0; k < 5; k++) s[k][t] = acc[k];
    sx[t] = nx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            for (int k = 0; k < 5; k++) s[k][t] += s[k][t + w];
            sx[t] += sx[t + w];
        }
        __syncthreads();
    }
    if (t < 4) out[4 * (size_t)blockIdx.x + t] = s[t][0] / (double)*wsum;
    if (t == 0 && blockIdx.x == 0) {
        *zpe_out = s[4][0] / (double)*wsum;
        *excluded = sx[0];
    }
}

// ---- projected density of states ---------------------------------------------------------------------------------------------
// g_c(f) = sum_q w_q sum_s |V_cs|^2 exp(-(f - f_s)^2 / 2 sigma^2) / (sigma sqrt(2 pi)) / sum_q w_q for the 3N channels c = 3 i + alpha.
// k_ph_dos_part's structure: lanes over sample frequencies, a chunk of modes per workgroup streamed through LDS in tiles of 256,
// each tile with the weights w_q |V_cs|^2 of a block of PH_PDOS_CH channels (blockIdx.z), each lane that many sums; a tile's sum,
// then the tiles, then (k_ph_pdos_sum) the chunks, all in order.  part [n_chunks][3N][n_samples].  Time reversal: V(-q) = conj V(q),
// the reduced mesh's integer weights apply unchanged.  The tile is read through volatile LDS pointers: 8-byte reads stay single.
#define PH_PDOS_CH 16
__global__ void __launch_bounds__(256) k_ph_pdos_part(const double *lam, const double *evec, const long long *wq, long long n_modes, int n3,
                                                      long long chunk, const double *samples, int n_samples, double inv_sigma, double *part) {
    __shared__ double sf[PH_DOS_TILE], sW[PH_PDOS_CH][PH_DOS_TILE];
    PhLdsDouble *vf = (PhLdsDouble *)sf, *vW = (PhLdsDouble *)&sW[0][0];
    const int t = threadIdx.x;
    const int is = blockIdx.x * 256 + t;
    const int c0 = blockIdx.z * PH_PDOS_CH, nc = min(PH_PDOS_CH, n3 - c0);
    const long long lo = (long long)blockIdx.y * chunk, hi = min(lo + chunk, n_modes);
    const double fs = is < n_samples ? samples[is] : 0.0;
    double acc[PH_PDOS_CH];
#pragma unroll
    for (int c = 0; c < PH_PDOS_CH; c++) acc[c] = 0.0;
    for (long long base = lo; base < hi; base += PH_DOS_TILE) {
        const long long e = base + t;
        __syncthreads();
        const bool in = e < hi;
        const long long iq = in ? e / n3 : 0;
        const int s = in ? (int)(e - iq * n3) : 0;
        const double w = in ? (double)(wq ? wq[iq] : 1) : 0.0;
        sf[t] = in ? ph_freq(lam[e]) : 0.0;
#pragma unroll
        for (int c = 0; c < PH_PDOS_CH; c++) {
            double v = 0.0;
            if (in && c < nc) {
                const double *x = evec + 2 * (((size_t)iq * n3 + c0 + c) * n3 + s);
                v = w * (x[0] * x[0] + x[1] * x[1]);
            }
            sW[c][t] = v;
        }
        __syncthreads();
        const int cnt = (int)min((long long)PH_DOS_TILE, hi - base);
        double sub[PH_PDOS_CH];
#pragma unroll
        for (int c = 0; c < PH_PDOS_CH; c++) sub[c] = 0.0;
        for (int k = 0; k < cnt; k++) {
            const double z = (fs - vf[k]) * inv_sigma;
            const double gk = exp(-0.5 * z * z);
#pragma unroll
            for (int c = 0; c < PH_PDOS_CH; c++) sub[c] += vW[c * PH_DOS_TILE + k] * gk;
        }
#pragma unroll
        for (int c = 0; c < PH_PDOS_CH; c++) acc[c] += sub[c];
    }
    if (is < n_samples)
#pragma unroll
        for (int c = 0; c < PH_PDOS_CH; c++)
            if (c < nc) part[((size_t)blockIdx.y * n3 + c0 + c) * n_samples + is] = acc[c];
}

// out [3N][n_samples]: the chunks in order / (sigma sqrt(2 pi) sum w); blockIdx.y the channel
__global__ void __launch_bounds__(256) k_ph_pdos_sum(const double *part, int n_chunks, int n3, int n_samples, double inv_sigma,
                                                     const long long *wsum, double *out) {
    const int is = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
    if (is >= n_samples) return;
    double acc = 0.0;
    for (int base = 0; base < n_chunks; base += 32) {
        double sub = 0.0;
        for (int k = base; k < min(base + 32, n_chunks); k++) sub += part[((size_t)k * n3 + c) * n_samples + is];
        acc += sub;
    }
    out[(size_t)c * n_samples + is] = acc * inv_sigma * 0.3989422804014327 / (double)*wsum;
}

// ---- thermal displacement tensors --------------------------------------------------------------------------------------------
// U_i^{ab}(T) = (1 / sum w_q) sum_q w_q sum_s E_s(T) / (m_i lam_s) Re(V_{3i+a,s} conj V_{3i+b,s}) in A^2 (eV / (amu eV / (amu A^2))),
// E_s = h f_s (1 / 2 + 1 / (e^x - 1)), x = h f_s / k_B T, in k_ph_thermo's forms (e^-x / -expm1(-x)); T = 0: the zero-point term.
// One workgroup per (temperature, atom), lanes over modes (stride 256) in runs of 32, then a fixed tree: k_ph_thermo's sums.
// out [nT][N][6] = xx, yy, zz, yz, xz, xy.  Modes with f <= cutoff are left out and their weight is reported.
__global__ void __launch_bounds__(256) k_ph_tdisp(const double *lam, const double *evec, const long long *wq, long long n_modes, int n3,
                                                  const double *inv_sqrt_mass, const double *T, double cutoff, const long long *wsum,
                                                  double *out, long long *excluded) {
    __shared__ double s[6][256];
    __shared__ long long sx[256];
    const int t = threadIdx.x, ia = blockIdx.y;
    const double temp = T[blockIdx.x], kT = PH_KB * temp;
    const double inv_m = inv_sqrt_mass[ia] * inv_sqrt_mass[ia];
    double acc[6] = {0, 0, 0, 0, 0, 0};
    long long nx = 0;
    for (long long base = t; base < n_modes; base += 256 * 32) {
        double sub[6] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 32; k++) {
            const long long e = base + (long long)k * 256;
            if (e >= n_modes) break;
            const double l = lam[e], f = ph_freq(l);
            const long long iq = e / n3;
            const int m = (int)(e - iq * n3);
            const long long wi = wq ? wq[iq] : 1;
            if (!(f > cutoff)) { nx += wi; continue; }
            const double hf = PH_H * f;
            double en = 0.5 * hf;
            if (temp > 0.0) {
                const double x = hf / kT;
                en = hf * (0.5 + exp(-x) / -expm1(-x));
            }
            const double coef = (double)wi * en * inv_m / l;
            const double *v = evec + 2 * (((size_t)iq * n3 + 3 * ia) * n3 + m);
            const double xr = v[0], xi = v[1], yr = v[2 * n3], yi = v[2 * n3 + 1], zr = v[4 * n3], zi = v[4 * n3 + 1];
            sub[0] += coef * (xr * xr + xi * xi);
            sub[1] += coef * (yr * yr + yi * yi);
            sub[2] += coef * (zr * zr + zi * zi);
            sub[3] += coef * (yr * zr + yi * zi);
            sub[4] += coef * (xr * zr + xi * zi);
            sub[5] += coef * (xr * yr + xi * yi);
        }
        for (int k = 0; k < 6; k++) acc[k] += sub[k];
    }
    for (int k = 0; k < 6; k++) s[k][t] = acc[k];
    sx[t] = nx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            for (int k = 0; k < 6; k++) s[k][t] += s[k][t + w];
            sx[t] += sx[t + w];
        }
        __syncthreads();
    }
    if (t < 6) out[6 * ((size_t)blockIdx.x * gridDim.y + ia) + t] = s[t][0] / (double)*wsum;
    if (t == 0 && blockIdx.x == 0 && ia == 0) *excluded = sx[0];
}
