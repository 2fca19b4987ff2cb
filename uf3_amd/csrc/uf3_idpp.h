// uf3_idpp.h -- the image dependent pair potential on the device (uf3_idpp_create, include/uf3_hip.h): the energy / force source of
// a uf3_neb handle that needs no model (Smidstrup et al., J. Chem. Phys. 140, 214106; ASE's idpp_interpolate).  A band of M images
// of n atoms with end points R^0 and R^{M-1}; for image k, lambda = k / (M - 1):
//
//   d_ij(R)  = |D_ij(R)|, D_ij the nearest-image vector x_j - x_i (below)
//   t_ij     = (1 - lambda) d_ij(R^0) + lambda d_ij(R^{M-1})          (this form: both end points are reproduced exactly)
//   S        = sum_{i<j} (t_ij - d_ij)^2 / d_ij^4                      (1 / A^2)
//   F_i      = -dS/dx_i = sum_{j != i} c_ij D_ij / d_ij,   c_ij = -2 (t - d) (d + 2 (t - d)) / d^5      (ASE's IDPP force)
//
// over all pairs with one image each (no cut-off); fixed atoms count in every sum (the NEB kernels drop their forces).
//
// Nearest-image vector: the fractional difference along the periodic axes (rows of the inverse of the cell completed for
// non-periodic axes as neb._axes does; the host passes them in) is rounded (half to even) and the rounding subtracted, as lattice
// vectors; among the 3^p shifts s in {-1, 0, 1} on the p periodic axes around that result the shortest vector is taken, ties to
// the first in the order s_a, s_b, s_c = -1, 0, 1 with s_c running fastest.  That is exact for every cell whose true nearest image
// lies within one cell of the rounded one (the skewed and turned cells of the drivers' tests).  For a band whose periodic cell
// rows are mutually orthogonal (exact zeros) rounding alone gives the same vectors and the host's per-frame flag skips the search,
// there and only there.  A pair at exactly half a cell is a kink of S: two images are equally near and F jumps between them.
//
//   k_idpp      one 256-thread workgroup per chunk of <= 256 atoms of one image (the drivers' ChunkTable), thread <-> atom i, its
//               position in the image and in both end points in registers.  The workgroup walks the image's atoms in tiles of 256,
//               staged in LDS with the same atoms of the two end-point frames (frames frame0 and frame0 + n_img - 1 of the same
//               position buffer: they never move, nothing is copied and no n x n table kept) as nine arrays of 256 doubles
//               (18 KB; every read is an 8-byte broadcast, never a 16-byte access at an 8-byte-aligned address).  Every ordered
//               pair is computed once from each side: the price of no atomics.  F_i goes to frc, the thread's half of S through
//               an LDS tree to one partial per chunk.  End-point images write zeros without walking.
//   k_idpp_sum  one thread per frame: the frame's partials added in chunk order -> energies
//
// A band's numbers depend on that band alone and two runs give the same bits.  Coincident atoms (d = 0) give a non-finite S and F,
// which k_neb_partial / k_neb_band turn into status nonfinite for that band alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uf3_neb.h"

struct IdppCell {                           // one frame's cell as k_idpp takes it (host: idpp_cells)
    double h[9];                            // rows: the lattice vectors (rows of non-periodic axes unused)
    double g[9];                            // g[3 k + c]: fraction along axis k = sum_c D_c g[3 k + c] (the completed cell's inverse)
    int per[3];                             // the axis is periodic
    int search;                             // 0: periodic rows mutually orthogonal, rounding alone is exact
};

struct IdppArgs {
    const double *pos;                      // [N][3]
    const int *blk_frame;                   // [n_blocks]
    const long long *blk_lo;                // [n_blocks]
    const int *blk_n;                       // [n_blocks]
    const int *frame_blk;                   // [n_frames + 1]
    const int *frame_band;                  // [n_frames]
    const long long *offsets;               // [n_frames + 1]
    const NebBand *bands;
    const IdppCell *cells;                  // [n_frames]
    double *frc;                            // [N][3]
    double *partial;                        // [n_blocks]: the chunk's share of S
    double *energies;                       // [n_frames] (k_idpp_sum)
    int n_frames;
};

// |D|^2 of the nearest-image vector of (x, y, z), which it replaces
__device__ __forceinline__ double idpp_nearest(double &x, double &y, double &z, const IdppCell &C) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (C.per[k]) {
            const double n = rint(x * C.g[3 * k] + y * C.g[3 * k + 1] + z * C.g[3 * k + 2]);
            x -= n * C.h[3 * k]; y -= n * C.h[3 * k + 1]; z -= n * C.h[3 * k + 2];
        }
    }
    if (!C.search) return x * x + y * y + z * z;
    const int la = C.per[0] ? 1 : 0, lb = C.per[1] ? 1 : 0, lc = C.per[2] ? 1 : 0;
    double best = __builtin_inf(), bx = x, by = y, bz = z;
    for (int sa = -la; sa <= la; sa++) {
        const double ax = x + sa * C.h[0], ay = y + sa * C.h[1], az = z + sa * C.h[2];
        for (int sb = -lb; sb <= lb; sb++) {
            const double cx = ax + sb * C.h[3], cy = ay + sb * C.h[4], cz = az + sb * C.h[5];
            for (int sc = -lc; sc <= lc; sc++) {
                const double vx = cx + sc * C.h[6], vy = cy + sc * C.h[7], vz = cz + sc * C.h[8];
                const double v2 = vx * vx + vy * vy + vz * vz;
                if (v2 < best) { best = v2; bx = vx; by = vy; bz = vz; }     // (strict: ties keep the first)
            }
        }
    }
    x = bx; y = by; z = bz;
    return best;
}

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_idpp(IdppArgs A) {
    __shared__ double tile[9 * UF3_RELAX_THREADS];      // [frame: image, first, last][x, y, z][256]; the tree's 2 x 256 afterwards
    const int b = blockIdx.x, t = threadIdx.x;
    const int f = A.blk_frame[b];
    const NebBand *B = A.bands + A.frame_band[f];
    const int f0 = B->frame0, M = B->n_img;
    const long long i = A.blk_lo[b] + t;
    const bool mine = t < A.blk_n[b];
    if (f == f0 || f == f0 + M - 1) {                   // an end point: S = 0, F = 0
        if (mine) {
#pragma unroll
            for (int k = 0; k < 3; k++) A.frc[3 * i + k] = 0.0;
        }
        if (t == 0) A.partial[b] = 0.0;
        return;
    }
    const IdppCell &C = A.cells[f];
    const long long lo = A.offsets[f], lo0 = A.offsets[f0], lo1 = A.offsets[f0 + M - 1];
    const int na = (int)(A.offsets[f + 1] - lo);
    const int me = (int)(i - lo);                       // the atom's index within the image
    const double lam = (double)(f - f0) / (double)(M - 1), oml = 1.0 - lam;
    double xi[3] = {0.0, 0.0, 0.0}, x0[3] = {0.0, 0.0, 0.0}, x1[3] = {0.0, 0.0, 0.0};
    if (mine) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            xi[k] = A.pos[3 * (lo + me) + k];
            x0[k] = A.pos[3 * (lo0 + me) + k];
            x1[k] = A.pos[3 * (lo1 + me) + k];
        }
    }
    double F[3] = {0.0, 0.0, 0.0}, S = 0.0;
    for (int jb = 0; jb < na; jb += UF3_RELAX_THREADS) {
        const int nj = na - jb < UF3_RELAX_THREADS ? na - jb : UF3_RELAX_THREADS;
        if (t < nj) {
            const long long j = jb + t;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                tile[(0 + k) * UF3_RELAX_THREADS + t] = A.pos[3 * (lo + j) + k];
                tile[(3 + k) * UF3_RELAX_THREADS + t] = A.pos[3 * (lo0 + j) + k];
                tile[(6 + k) * UF3_RELAX_THREADS + t] = A.pos[3 * (lo1 + j) + k];
            }
        }
        __syncthreads();
        if (mine) {
            for (int jj = 0; jj < nj; jj++) {
                if (jb + jj == me) continue;
                double dx = tile[0 * UF3_RELAX_THREADS + jj] - xi[0], dy = tile[1 * UF3_RELAX_THREADS + jj] - xi[1],
                       dz = tile[2 * UF3_RELAX_THREADS + jj] - xi[2];
                double ax = tile[3 * UF3_RELAX_THREADS + jj] - x0[0], ay = tile[4 * UF3_RELAX_THREADS + jj] - x0[1],
                       az = tile[5 * UF3_RELAX_THREADS + jj] - x0[2];
                double bx = tile[6 * UF3_RELAX_THREADS + jj] - x1[0], by = tile[7 * UF3_RELAX_THREADS + jj] - x1[1],
                       bz = tile[8 * UF3_RELAX_THREADS + jj] - x1[2];
                const double d2 = idpp_nearest(dx, dy, dz, C);
                const double d0 = sqrt(idpp_nearest(ax, ay, az, C)), d1 = sqrt(idpp_nearest(bx, by, bz, C));
                const double d = sqrt(d2);
                const double w = (oml * d0 + lam * d1) - d;                 // t - d
                const double i2 = 1.0 / d2, i4 = i2 * i2;
                S += w * w * i4;
                const double c = -2.0 * w * (d + 2.0 * w) * i4 * i2;        // c_ij / d
                F[0] += c * dx; F[1] += c * dy; F[2] += c * dz;
            }
        }
        __syncthreads();
    }
    if (mine) {
#pragma unroll
        for (int k = 0; k < 3; k++) A.frc[3 * i + k] = F[k];
    }
    double s[2] = {mine ? 0.5 * S : 0.0, 0.0};          // every pair was met from both sides
    relax_block_reduce<2>(s, tile);
    if (t == 0) A.partial[b] = s[0];
}

__global__ void k_idpp_sum(IdppArgs A) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= A.n_frames) return;
    double e = 0.0;
    for (int c = A.frame_blk[f]; c < A.frame_blk[f + 1]; c++) e += A.partial[c];    // chunk order
    A.energies[f] = e;
}
