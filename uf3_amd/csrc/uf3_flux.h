// uf3_flux.h -- per-atom resolution of the UF3 energy (uf3_site_terms[_dev], uf3_heat_flux[_dev], uf3_md_run_flux): site
// energies, site virials and the heat current of a batch of frames.  gfx950, fp64.
//
// Site energy   U_i = the evaluator's own partition (what uf3_eval_atoms(i, i + 1) returns): the one-body term of i's species,
//               the directed pair terms phi(r_ij) of i over every image j in the pair range, and every triplet
//               V(r_ij, r_ik, r_jk) with i as the centre, over unordered pairs {j, k} of its 3-body neighbours.
//               sum_i U_i = uf3_eval's frame energy.
// Images        move with their parent atom and carry its velocity.
// Site virial   for a slot s of a term of U_i (a neighbour image), d_s = the vector from the centre to that image:
//               W_i[a][b] = sum_terms sum_s d_s[a] (dU_i / dr_s)[b]; nine components, row-major.  sum_i W_i, symmetrised, in
//               Voigt order (xx, yy, zz, yz, xz, xy) = uf3_eval_virial's dE / d(strain).
// Heat current  e_i = 1/2 m_i v_i^2 + U_i;  J = J_conv + J_pot (extensive, eV Angstrom / fs),
//               J_conv = sum_i e_i v_i,   J_pot = - sum_i sum_terms sum_s d_s (dU_i / dr_s . v_s)
//               = d/dt sum_i r_i e_i with Newton's equations put in (exact in a cluster; in a periodic cell term by term with
//               the image vectors in place of r_s - r_i).
// Derivatives   pair: dU_i / dr_j = phi'(r_ij) u_ij.  Triplet with legs ij, ik, jk and leg gradient g:
//               d / dr_j = g_ij u_ij - g_jk u_jk,   d / dr_k = g_ik u_ik + g_jk u_jk   (u_jk the unit vector from j to k).
//
//   k_flux_lists   the per-atom image lists (hess_lists_atom, uf3_hessian.h) of a batch: one wave per atom, its frame's
//                  arguments put together from a per-frame table.  O(N^2 images) per frame.  The one list kernel: the
//                  Hessian's frame is a batch of one.
//   k_flux_site_terms  one wave per centre: lanes over its pair entries, then over the (j, k) pairs of its 3-body
//                  neighbours, in strides of 64; U (1), J_pot (3) and W (9) in registers, combined by the evaluator's DPP tree (wave_sum),
//                  lane 0 writes the record.  Values and leg gradients come from trio_value and the evaluator's pair code
//                  (load_interval + bspline4): the same knot records, coefficient windows and support tests.
//   k_flux_frame   one workgroup per frame: J_conv and J_pot from the per-atom records, strided partial sums + the LDS tree
//                  of k_md_thermo (md_block_sum).
// No atomics: every record has one writer and every sum a fixed order that depends on the centre's entries alone, taken in a
// canonical order (by image vector), so the results repeat bit for bit, do not depend on the batch around a frame, and do not
// depend on the numbering of the atoms or on the choice of the periodic cell where that leaves the image vectors' bits alone.
// (Except on a symmetry-1 trio: there the reference's energy itself depends on both, through which of two neighbours of one
// species takes leg l -- supercell_before, uf3_device.h; DESIGN.md section 7.  The ORDER of the sums stays canonical.)
#pragma once
#include "uf3_hessian.h"
#include "uf3_md.h"

// one frame of a batch for k_flux_lists: the geometry of its HessArgs (hess_geometry) and where its atoms start
struct FluxFrame {
    double cell[9], inv[9];
    int per[3], nimg[3];
    long long lo;             // first atom of the frame in the batch
    int natoms, pad;
};

struct FluxArgs {
    const BasisDev *B;
    const FluxFrame *frames;  // [n_frames]
    const int64_t *offsets;   // [n_frames + 1]
    int n_frames;
    long long n;              // atoms of the batch
    const double *pos;        // [n][3]
    const double *vel;        // [n][3] or null (no current)
    const double *mass;       // [n] amu (k_flux_frame)
    const int *spec;          // [n]
    int cap;                  // list capacity per atom
    int *cnt;                 // [n]
    int *flags;               // [0]: an image shift beyond pack3's range; [1]: a list longer than cap
    HessNbr *ent;             // [n][cap]
    const double *c1, *c2, *c3;
    double *u;                // [n] site energies
    double *w;                // [n][9] site virials, or null
    double *jp;               // [n][3] each centre's share of J_pot, or null
    double *flux;             // [n_frames][6]: J_conv, J_pot (k_flux_frame)
};

// the frame of atom i: the last f with offsets[f] <= i (no frame is empty)
__device__ __forceinline__ int flux_frame_of(const int64_t *offsets, int n_frames, long long i) {
    int lo = 0, hi = n_frames - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <bool WRITE>
__global__ void __launch_bounds__(64) k_flux_lists(FluxArgs F) {
    const long long i = blockIdx.x;
    if (i >= F.n) return;
    const FluxFrame *fr = F.frames + flux_frame_of(F.offsets, F.n_frames, i);
    HessArgs A;
    const long long lo = fr->lo;
    A.B = F.B; A.pos = F.pos + 3 * (size_t)lo; A.spec = F.spec + lo; A.natoms = fr->natoms;
    for (int k = 0; k < 9; k++) { A.cell[k] = fr->cell[k]; A.inv[k] = fr->inv[k]; }
    for (int k = 0; k < 3; k++) { A.per[k] = fr->per[k]; A.nimg[k] = fr->nimg[k]; }
    A.cap = F.cap; A.cnt = F.cnt + lo; A.bad = F.flags; A.ent = F.ent + (size_t)lo * F.cap;
    hess_lists_atom<WRITE, true>(A, (int)(i - lo), threadIdx.x);
}

// (a, b), a < b, of the p-th unordered pair in the order (0,1) (0,2) (1,2) (0,3) ...
__device__ __forceinline__ void flux_pair_of(int p, int &a, int &b) {
    int t = (int)((1.0 + sqrt(1.0 + 8.0 * (double)p)) * 0.5);
    while (t * (t - 1) / 2 > p) t--;
    while ((t + 1) * t / 2 <= p) t++;
    b = t; a = p - t * (t - 1) / 2;
}

// a before b in the canonical order of a centre's entries: by the image vector (dx, dy, dz), then by the list position.
// The order is a property of the geometry, not of how the atoms are numbered or which image of the cell holds them.
__device__ __forceinline__ bool flux_before(const HessNbr &a, int ia, const HessNbr &b, int ib) {
    if (a.dx != b.dx) return a.dx < b.dx;
    if (a.dy != b.dy) return a.dy < b.dy;
    if (a.dz != b.dz) return a.dz < b.dz;
    return ia < ib;
}

// dynamic LDS: [cap] ints -- first the centre's entries in canonical order (list positions), then, compacted in place
// behind the read front, those of its 3-body neighbours
template <bool WANT_W, bool WANT_J>
__global__ void __launch_bounds__(64) k_flux_site_terms(FluxArgs F) {
    extern __shared__ int idx3[];
    const long long m = blockIdx.x;
    const int lane = threadIdx.x;
    if (m >= F.n) return;
    const BasisDev *B = F.B;
    const long long lo = F.offsets[flux_frame_of(F.offsets, F.n_frames, m)];
    const int sm = F.spec[m];
    const int full = F.cnt[m];
    if (full > F.cap) {                       // the list was cut: the host grows the capacity and runs the sample again
        if (lane == 0) F.flags[1] = 1;
        return;
    }
    const int n = full;
    const HessNbr *L = F.ent + (size_t)m * F.cap;
    const int S = B->S;
    double u = 0.0, jp[3] = {0.0, 0.0, 0.0}, w[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (lane == 0) u = F.c1[sm];
    // the canonical order: entry e goes to the place given by the number of entries before it (the entries are finite and
    // the order is total, so the places are a permutation of 0 .. n - 1)
    for (int e = lane; e < n; e += WAVE) {
        const HessNbr en = L[e];
        int place = 0;
        for (int f = 0; f < n; f++) place += flux_before(L[f], f, en, e) ? 1 : 0;
        idx3[place] = e;
    }
    __syncthreads();
    // pair entries, and the compaction of the 3-body neighbours (canonical order kept; slot n3 + mbcnt <= e0 + lane, and
    // the wave has read its 64 places before it writes: in place)
    int n3 = 0;
    for (int e0 = 0; e0 < n; e0 += WAVE) {
        const bool live = e0 + lane < n;
        const int e = live ? idx3[e0 + lane] : 0;
        const HessNbr en = L[e];
        const bool is3 = live && (en.flags & 2);
        const unsigned long long mask3 = __ballot(is3);
        if (is3) idx3[n3 + mbcnt(mask3)] = e;
        n3 += __popcll(mask3);
        if (live && (en.flags & 1)) {
            const int pair_idx = sm * UF3_MAX_SPECIES + en.spec;
            const LegDev leg = B->pairs[B->pair_of[pair_idx]].leg;
            KnotRec kr;
            const int i = load_interval<1>(B->recs, leg, en.r, kr);
            double v[4], dv[4];
            bspline4<true>(kr, en.r, v, dv);
            const double *cf = F.c2 + (B->pair_col[pair_idx] - S) + (i - 3);
            double phi = 0, dphi = 0;
            for (int q = 0; q < 4; q++) { phi += cf[q] * v[q]; dphi += cf[q] * dv[q]; }
            u += phi;
            const double t = dphi / en.r;
            const double d[3] = {en.dx, en.dy, en.dz};
            if (WANT_W)
                for (int a = 0; a < 3; a++)
                    for (int b = 0; b < 3; b++) w[3 * a + b] += d[a] * (t * d[b]);
            if (WANT_J) {
                const double *vj = F.vel + 3 * (size_t)(lo + en.j);
                const double gv = t * (d[0] * vj[0] + d[1] * vj[1] + d[2] * vj[2]);
                for (int a = 0; a < 3; a++) jp[a] -= d[a] * gv;
            }
        }
    }
    __syncthreads();
    // triplets with m as the centre, walked in canonical order; legs in the evaluator's order (trio_swap_legs, uf3_device.h),
    // equal species on equal legs in canonical order, which keeps the bits independent of numbering and cell (test_tiling)
    if (B->T > 0) {
        const int npair = n3 * (n3 - 1) / 2;
        for (int p0 = 0; p0 < npair; p0 += WAVE) {
            const int p = p0 + lane;
            if (p >= npair) continue;
            int a, b;
            flux_pair_of(p, a, b);
            const HessNbr ea = L[idx3[a]], eb = L[idx3[b]];
            const bool swap = trio_swap_legs(B, sm, ea, eb, false);
            const HessNbr &ej = swap ? eb : ea, &ek = swap ? ea : eb;
            const int trio = B->trio_of[(sm * UF3_MAX_SPECIES + ej.spec) * UF3_MAX_SPECIES + ek.spec];
            const double dj[3] = {ej.dx, ej.dy, ej.dz}, dk[3] = {ek.dx, ek.dy, ek.dz};
            const double djk[3] = {dk[0] - dj[0], dk[1] - dj[1], dk[2] - dj[2]};
            const double rn = norm3_rn(djk[0], djk[1], djk[2]);
            double val, g[3];
            if (!trio_value(B, F.c3, trio, ej.r, ek.r, rn, true, val, g)) continue;
            u += val;
            const double tl = g[0] / ej.r, tm = g[1] / ek.r, tn = g[2] / rn;
            double gj[3], gk[3];          // dU_i / dr_j, dU_i / dr_k
            for (int q = 0; q < 3; q++) { gj[q] = tl * dj[q] - tn * djk[q]; gk[q] = tm * dk[q] + tn * djk[q]; }
            if (WANT_W)
                for (int x = 0; x < 3; x++)
                    for (int y = 0; y < 3; y++) w[3 * x + y] += dj[x] * gj[y] + dk[x] * gk[y];
            if (WANT_J) {
                const double *vj = F.vel + 3 * (size_t)(lo + ej.j), *vk = F.vel + 3 * (size_t)(lo + ek.j);
                const double pj = gj[0] * vj[0] + gj[1] * vj[1] + gj[2] * vj[2];
                const double pk = gk[0] * vk[0] + gk[1] * vk[1] + gk[2] * vk[2];
                for (int q = 0; q < 3; q++) jp[q] -= dj[q] * pj + dk[q] * pk;
            }
        }
    }
    // (every lane is back here: the DPP tree reads all 64)
    u = wave_sum(u);
    if (lane == 0) F.u[m] = u;
    if (WANT_W)
        for (int q = 0; q < 9; q++) { const double s = wave_sum(w[q]); if (lane == 0) F.w[9 * (size_t)m + q] = s; }
    if (WANT_J)
        for (int q = 0; q < 3; q++) { const double s = wave_sum(jp[q]); if (lane == 0) F.jp[3 * (size_t)m + q] = s; }
}

// [J_conv (3), J_pot (3)] of every frame
__global__ void __launch_bounds__(UF3_MD_THREADS) k_flux_frame(FluxArgs F) {
    __shared__ double lds[6 * UF3_MD_THREADS];
    const int f = blockIdx.x;
    const long long lo = F.offsets[f], hi = F.offsets[f + 1];
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (long long i = lo + threadIdx.x; i < hi; i += UF3_MD_THREADS) {
        const double vx = F.vel[3 * i], vy = F.vel[3 * i + 1], vz = F.vel[3 * i + 2];
        const double e = 0.5 * F.mass[i] * UF3_MD_KE * (vx * vx + vy * vy + vz * vz) + F.u[i];
        s[0] += e * vx; s[1] += e * vy; s[2] += e * vz;
        s[3] += F.jp[3 * i]; s[4] += F.jp[3 * i + 1]; s[5] += F.jp[3 * i + 2];
    }
    md_block_sum<6>(s, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < 6; k++) F.flux[6 * (size_t)f + k] = s[k];
}
