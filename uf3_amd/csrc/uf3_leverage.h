// uf3_leverage.h -- leverage of feature rows against the system the fit solved: q = x^T (G + R^T R)^-1 x = |W x|^2.
//
//   k_leverage   q[g] = sum over the rows r of group g, over k, of ( sum_{j <= k} W[k][j] X[r][j] )^2       (fp64)
//                X [n_rows][ld] row-major, the first n_feat columns used (the padding is never read into the result);
//                W [n_feat][n_feat] row-major, lower triangular: the inverse of the Cholesky factor of the system matrix, with
//                exact zeros above the diagonal (the host's promise -- the kernel does not mask inside a diagonal tile);
//                group 1 or 3 consecutive rows per output (3: one number per atom from its three force rows).
//
// Z = X W^T never exists in memory.  A workgroup of four waves owns LV_ROWS = 48 rows outright (three 16-row MFMA tiles;
// 48 = 16 * 3 so that both group sizes tile) and produces Z^T for them 16 x 16 tile by tile on the fp64 matrix cores:
//     D[k][r] (+)= A[k][j] B[j][r],   A = W (16 rows k x 4 columns j per v_mfma_f64_16x16x4_f64),  B = X^T (4 x 16 rows r)
// so that an X row is a COLUMN of the accumulator: on the hardware's layout a lane then holds four k of ONE row, and the sum of
// squares over k is a sum inside the lane plus one reduction at the very end.  (Which (k, r) a lane's four values are is read
// from the context's k_mfma_probe table, not assumed: the final reduction goes through the table's inverse.)
//
// Staging.  The 48 x n_feat block does not fit the LDS beside anything else at n_feat = 434, so it goes through in slabs of
// LV_SLAB = 64 columns j ([48][66] doubles, 25 KB: the stride 66 puts the 32 (row, j) pairs of a half-wave's operand read on
// 32 distinct 8-byte bank pairs), coalesced 512-byte row pieces, the next slab in flight in registers while the current one
// is multiplied (k_gram_tiled's scheme).  W is read straight from the L2 into the A operand: each wave owns k tiles of its own,
// so within a workgroup every element of W's triangle is read by exactly one wave, once per pass -- an LDS copy would only be
// read once as well.  A 16 x 16 piece of W is four loads a lane, issued a piece ahead of the twelve MFMAs that consume them.
//
// Passes.  The accumulators of all k tiles of a wide matrix do not fit the registers (n_feat = 1798: 113 tiles), so the k tiles
// go in passes of 4 waves x LV_KT = 4 tiles (256 columns of Z; 4 x 3 tiles x 4 doubles = 96 accumulator registers a lane); a pass
// walks the slabs 0 .. its last column and squares its tiles into the lane's running sums.  Pass p re-stages the slabs the
// earlier passes staged (n_feat = 434: 4 + 7 slab stages instead of 7, from the L2).
//
// The triangle.  Tile k-range [16 kt, 16 kt + 16) needs j < 16 kt + 16 only.  An MFMA step covers 4 j x 16 k, and 16 kt + 16 is a
// multiple of 4: a step is either wholly above the diagonal (4 j0 >= 16 kt + 16) or needed, never split -- so the cut is a trip
// count (pieces of four steps; a tile's last piece is its diagonal piece, all four steps of which hold some j <= k) and costs
// no instruction inside the loop.  That is the factor of two over the dense product.
//
// No atomics, no scratch in HBM: lane sums -> LDS -> one thread per row adds them in a fixed order -> plain stores.  The same
// call twice is bit-identical; q is a sum of squares (>= 0), exactly 0.0 for a row of zeros.
// Ragged ends: unconditional loads from a clamped address, zeroed by a select (k_gram_mfma's idiom).
#pragma once
#include "uf3_kernels.h"

#define LV_ROWS 48        // rows of X per workgroup
#define LV_SLAB 64        // columns j per slab
#define LV_LDW 66         // slab row stride (doubles)
#define LV_KT 4           // k tiles per wave and pass

__global__ void __launch_bounds__(256, 2)
k_leverage(const double *x, int64_t n_rows, int n_feat, int64_t ld, const double *w, int group, const int *frag_rowcol, double *q) {
    // one LDS object: the slab while multiplying; at the end the lanes' sums [3][4][256], then the row sums [48]
    __shared__ double lds[LV_ROWS * LV_LDW + 256 / 2];
    int *inv = (int *)(lds + LV_ROWS * LV_LDW);                     // [16 r][16 k] -> lane * 4 + v  (inverse of the probe table)
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t r0 = (int64_t)blockIdx.x * LV_ROWS;
    {
        const int fr = frag_rowcol[2 * t], fc = frag_rowcol[2 * t + 1];   // t = lane * 4 + v of a wave's accumulator
        inv[fc * 16 + fr] = t;
    }
    // staging role: column (t & 63) of the slab, rows (t >> 6) + 4 i
    const int sc = t & 63, sr = t >> 6;
    int64_t srow[LV_ROWS / 4];
    bool svalid[LV_ROWS / 4];
#pragma unroll
    for (int i = 0; i < LV_ROWS / 4; i++) {
        const int64_t row = r0 + sr + 4 * i;
        svalid[i] = row < n_rows;
        srow[i] = (svalid[i] ? row : 0) * ld;
    }
    double gq[LV_ROWS / 4];
    auto fetch = [&](int s) {
        const int col = s * LV_SLAB + sc;
        const bool vc = col < n_feat;
        const double *p = x + (vc ? col : 0);
#pragma unroll
        for (int i = 0; i < LV_ROWS / 4; i++) gq[i] = p[srow[i]];
#pragma unroll
        for (int i = 0; i < LV_ROWS / 4; i++) gq[i] = (vc && svalid[i]) ? gq[i] : 0.0;
    };
    auto store = [&]() {
#pragma unroll
        for (int i = 0; i < LV_ROWS / 4; i++) lds[(sr + 4 * i) * LV_LDW + sc] = gq[i];
    };
    // operand roles of the lane: A = W[16 kt + (lane & 15)][j0 + (lane >> 4)], B = X[16 m + (lane & 15)][j0 + (lane >> 4)]
    const int li = lane & 15, lk = lane >> 4;
    const double *xb = lds + li * LV_LDW + lk;
    double sq[3][4];
    int fk[4];                                                       // k (within a tile) of the lane's four accumulator values
#pragma unroll
    for (int v = 0; v < 4; v++) fk[v] = frag_rowcol[(lane * 4 + v) * 2];
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int v = 0; v < 4; v++) sq[m][v] = 0.0;
    const int nt = (n_feat + 15) >> 4;                               // k tiles
    const int n_pass = (nt + 4 * LV_KT - 1) / (4 * LV_KT);
    for (int pass = 0; pass < n_pass; pass++) {
        double4_t acc[LV_KT][3];
        const double *wrow[LV_KT];
        int kt[LV_KT];
#pragma unroll
        for (int u = 0; u < LV_KT; u++) {
#pragma unroll
            for (int m = 0; m < 3; m++) acc[u][m] = double4_t{0, 0, 0, 0};
            kt[u] = pass * 4 * LV_KT + 4 * u + wave;                 // interleaved: the waves' shares of the triangle stay close
            const int k = kt[u] * 16 + li;
            wrow[u] = w + (size_t)(k < n_feat ? k : 0) * n_feat;
        }
        const int kt_last = min(nt, (pass + 1) * 4 * LV_KT) - 1;    // the pass's last tile decides how many slabs it walks
        const int n_slab = (kt_last * 16 + 16 + LV_SLAB - 1) / LV_SLAB;
        __syncthreads();                                             // (the previous pass's last slab is still being read)
        fetch(0);
        store();
        __syncthreads();
        for (int s = 0; s < n_slab; s++) {
            if (s + 1 < n_slab) fetch(s + 1);
#pragma unroll
            for (int u = 0; u < LV_KT; u++) {
                // pieces of 16 j of this slab that tile kt[u] needs: j0 < 16 kt + 16
                const int np = kt[u] < nt ? min(LV_SLAB / 16, max(0, kt[u] + 1 - s * (LV_SLAB / 16))) : 0;
                double a[4];
                auto load_w = [&](int pc) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int j = s * LV_SLAB + pc * 16 + 4 * e + lk;
                        a[e] = wrow[u][j < n_feat ? j : 0];
                    }
                };
                if (np > 0) load_w(0);
                for (int pc = 0; pc < np; pc++) {
                    // (no select on the data here: a column j >= n_feat meets the slab's zeros, a row k >= n_feat is dropped
                    // when the tile is squared.  What is left of vector work per piece is the address clamp of the four W
                    // loads -- a compare and a select each, needed in the matrix's last slab only, beside twelve MFMAs)
                    const double ac[4] = {a[0], a[1], a[2], a[3]};
                    load_w(pc + 1 < np ? pc + 1 : pc);              // (the last trip re-reads its own piece: nothing conditional)
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const double *bp = xb + pc * 16 + 4 * e;
#pragma unroll
                        for (int m = 0; m < 3; m++)
                            acc[u][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[e], bp[m * 16 * LV_LDW], acc[u][m], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
            if (s + 1 < n_slab) {
                store();
                __syncthreads();
            }
        }
#pragma unroll
        for (int u = 0; u < LV_KT; u++)
#pragma unroll
            for (int m = 0; m < 3; m++)
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const double z = kt[u] * 16 + fk[v] < n_feat ? acc[u][m][v] : 0.0;
                    sq[m][v] += z * z;
                }
    }
    // the lanes' sums through LDS: part[m][wave][lane * 4 + v]; thread (m, r) adds the 4 x 16 values of row 16 m + r in a
    // fixed order (waves, then k)
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int v = 0; v < 4; v++) lds[(m * 4 + wave) * 256 + lane * 4 + v] = sq[m][v];
    __syncthreads();
    double rs = 0.0;
    if (t < LV_ROWS) {
        const int m = t >> 4, r = t & 15;
        for (int wq = 0; wq < 4; wq++)
            for (int k = 0; k < 16; k++) rs += lds[(m * 4 + wq) * 256 + inv[r * 16 + k]];
    }
    __syncthreads();
    if (t < LV_ROWS) lds[t] = rs;
    __syncthreads();
    if (group == 1) {
        if (t < LV_ROWS && r0 + t < n_rows) q[r0 + t] = rs;
    } else if (t < LV_ROWS / 3) {
        const int64_t g = r0 / 3 + t;                                // (r0 and n_rows are multiples of 3)
        if (3 * g < n_rows) q[g] = (lds[3 * t] + lds[3 * t + 1]) + lds[3 * t + 2];
    }
}
