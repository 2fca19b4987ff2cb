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
#pragma once
#include "uf3_device.h"

#define PH_MAX_ATOMS 32                  // 3N <= 96: 16 * 96^2 = 147 456 bytes of the CU's 160 KiB
#define PH_MAX_DIM (3 * PH_MAX_ATOMS)
#define PH_MAX_SWEEPS 30
#define PH_EPS 2.220446049250313e-16     // 2^-52
#define PH_THZ 15.633302                 // harmonic.THZ: sqrt(eV / (amu A^2)) / 2 pi in THz
#define PH_H 4.135667696e-3              // eV / THz   (CODATA 2018)
#define PH_KB 8.617333262e-5             // eV / K

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

// ---- 3N <= 6: one lane per q-point -------------------------------------------------------------------------------------------
// Only the entries r <= c of ar / ai are touched after the build, every index is a constant after unrolling: the arrays
// are registers, there is no scratch.
template <int N>
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
            d[j] = lo; d[j + 1] = hi;
        }
#pragma unroll
    for (int r = 0; r < n; r++) A.lam[(size_t)iq * n + r] = d[r];
    A.status[iq] = sweeps;
}

// ---- 3N <= PH_MAX_DIM: one wave per q-point, D(q) in LDS -----------------------------------------------------------------------
struct __attribute__((aligned(16))) PhRot {
    int p, q;                            // p < q; q < 0: nothing to do (the padding index of an odd dimension, or a pivot below the threshold)
    double c, s, ur, ui;
};

__device__ __forceinline__ double ph_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__host__ __device__ inline size_t ph_wave_lds(int n) {
    return sizeof(double2) * (size_t)n * n + sizeof(PhRot) * (size_t)((n + 1) / 2);
}

__global__ void __launch_bounds__(64) k_ph_mesh_wave(PhMeshArgs A) {
    extern __shared__ __attribute__((aligned(16))) char ph_lds[];
    const int N = A.natoms, n = 3 * N, lane = threadIdx.x;
    const long long iq = blockIdx.x;
    double2 *D = (double2 *)ph_lds;                          // [n][n] row-major, (re, im)
    PhRot *rot = (PhRot *)(D + (size_t)n * n);
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
    }
    if (lane == 0) A.status[iq] = sweeps;
}

// ---- density of states -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ph_freq(double lam) {
    return (lam > 0.0 ? 1.0 : (lam < 0.0 ? -1.0 : 0.0)) * sqrt(fabs(lam)) * PH_THZ;
}

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
