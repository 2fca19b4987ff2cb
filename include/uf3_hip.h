/*
 * uf3_hip.h -- C ABI of the MI355X-native UF3 hot path (libuf3hip.so).
 *
 * The reference (uf3 v0.4.0) is pure Python and has no FFI; the boundary it
 * offers is its object API.  Each entry point below replaces the arithmetic
 * behind one of those Python surfaces, so that the classes in uf3_amd/ (same
 * names and signatures as the reference's) are thin ctypes shims:
 *
 *   uf3_basis_create      <- uf3/representation/bspline.py:20-88   (BSplineBasis tables)
 *   uf3_featurize[_dev]   <- uf3/representation/process.py:293-506 (evaluate_configuration,
 *                            featurize_{energy,force}_{2B,3B}); distances.py:19-143,
 *                            angles.py:17-232, bspline.py:810-895
 *   uf3_gram[_dev]        <- uf3/regression/least_squares.py:716-760 (X^T X, X^T y)
 *   uf3_eval[_dev]        <- uf3/forcefield/calculator.py:156-343  (energy, forces)
 *   uf3_neighbors_debug   <- distances.py:48-69 / angles.py:289-346 index semantics
 *   uf3_pair_geometry, uf3_distance_matrix, uf3_direction_cosines
 *                         <- the free functions of distances.py:19-143, 212-235, 331-364 and angles.py:289-346
 *   uf3_pair_histogram[_dev] <- uf3/data/analyze.py (DataAnalyzer.get_distances, update_histograms),
 *                            distances.py:367-442 (summarize_distances)
 *
 * Conventions
 *   - every function returns 0 on success, a non-zero UF3_E* code otherwise;
 *     uf3_last_error(ctx) gives the message (ctx may be NULL for create failures);
 *   - the caller owns all buffers; the library allocates only inside the opaque
 *     handles (grow-only device workspace) and frees in *_destroy;
 *   - a ctx is bound to one HIP device and one stream; calls on one ctx must be
 *     serialised by the caller (one ctx per device / per Python thread);
 *   - "_dev" entries take HBM pointers for the bulk arrays and enqueue on the ctx
 *     stream without synchronising; the plain entries take host pointers, copy in
 *     and out, and synchronise before returning.  Frame metadata (offsets, cells,
 *     pbc) is always host memory: it is a few hundred bytes per frame.
 *     uf3_featurize_dev synchronises only while a context is still learning its
 *     neighbour capacities (the first calls); afterwards the kernels' status words
 *     travel to pinned host memory behind the launches and are looked at by the next
 *     call on the context and by uf3_ctx_synchronize, which then report
 *     UF3_ESPECIES / UF3_EINVAL / UF3_ERETRY for the EARLIER call;
 *   - all floating point data is IEEE double, C-contiguous; positions in Angstrom.
 */
#ifndef UF3_HIP_H
#define UF3_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct uf3_ctx uf3_ctx;
typedef struct uf3_basis uf3_basis;

enum {
    UF3_OK = 0,
    UF3_EINVAL = 1,     /* bad argument / unsupported basis */
    UF3_ESPECIES = 2,   /* a frame contains an element outside the basis (process.py:321-330) */
    UF3_EHIP = 3,       /* HIP runtime error */
    UF3_ENOMEM = 4,
    UF3_EOVERFLOW = 5,  /* internal capacity exceeded after retries */
    UF3_ERETRY = 6      /* an earlier asynchronous uf3_featurize_dev call ran with neighbour capacities that turned
                           out too small, or met atoms given far outside their periodic cell (their 3-body force
                           rows need the launches that carry the reference's image-range rule): its outputs (and
                           whatever was derived from them) are invalid; the context has adapted -- repeat the work
                           since the last uf3_ctx_synchronize */
};

/* Flat description of a BSplineBasis (host memory, copied by uf3_basis_create). */
typedef struct uf3_basis_spec {
    int32_t n_species;            /* S */
    const int32_t *species_z;     /* [S] ascending atomic numbers */
    int32_t n_pairs;              /* S(S+1)/2 pair blocks in column order */
    const int32_t *pair_z;        /* [P][2], z0 <= z1 */
    const int32_t *pair_nk;       /* [P] knots per pair (4-fold ends included) */
    const double *pair_knots;     /* concatenated */
    const double *pair_rmin;      /* [P] r_min_map */
    const double *pair_rmax;      /* [P] r_max_map */
    const int32_t *pair_col;      /* [P] first column of the block (1-body columns count) */
    int32_t lead2, trail2;        /* trimmed basis functions of every pair block */
    int32_t n_trios;              /* 0 for a 2-body basis */
    const int32_t *trio_z;        /* [T][3] centre, n1 <= n2 */
    const int32_t *trio_nk;       /* [T][3] knots of the l (ij), m (ik), n (jk) legs */
    const double *trio_knots;     /* concatenated l, m, n per trio */
    const int32_t *trio_col;      /* [T] first column of the compressed block */
    const int32_t *trio_ncol;     /* [T] compressed block width */
    const int32_t *trio_lut;      /* concatenated [L*M*N] raw bin -> column within block, or -1
                                     (symmetry fold, template mask and trims already applied) */
    int32_t n_feat;               /* F = total columns, y excluded */
    double r_cut;                 /* BSplineBasis.r_cut: image range of the reference supercell */
} uf3_basis_spec;

/* A batch of frames.  All three arrays live in HOST memory. */
typedef struct uf3_frames {
    int32_t n_frames;
    const int64_t *atom_offsets;  /* [n_frames+1], atom_offsets[0] = 0 */
    const double *cells;          /* [n_frames][3][3], rows = lattice vectors */
    const uint8_t *pbc;           /* [n_frames][3] */
} uf3_frames;

int uf3_ctx_create(int device, uf3_ctx **out);
void uf3_ctx_destroy(uf3_ctx *ctx);
/* enqueue on an existing hipStream_t, e.g. torch's current stream; NULL = HIP's null stream (torch's
 * default).  Until this is called the ctx uses a private non-blocking stream, which is NOT ordered with
 * work the caller enqueues elsewhere: callers of the _dev entries should always set their stream. */
int uf3_ctx_set_stream(uf3_ctx *ctx, void *hip_stream);
/* back to the ctx's private stream (what a temporary user of uf3_ctx_set_stream does when it is done) */
int uf3_ctx_use_own_stream(uf3_ctx *ctx);
int uf3_ctx_synchronize(uf3_ctx *ctx);
const char *uf3_last_error(const uf3_ctx *ctx);
/* Which sources this binary was compiled from: the first 16 hex digits of the sha256 over uf3_hip.hip, uf3_kernels.h,
 * uf3_feat3.h, uf3_virial_rows.h, uf3_device.h, uf3_md.h, uf3_hessian.h, uf3_relax.h, uf3_phonon.h, uf3_npt.h, uf3_neb.h, uf3_idpp.h, uf3_mc.h, uf3_flux.h and this header, concatenated in that order (the Makefile passes it in; "unknown" for a build
 * outside it).  __graft_entry__.build() rebuilds when it differs from the tree's, smoke() prints it. */
const char *uf3_build_id(void);
/* timing of the dominant kernel: (re)start / read accumulated HIP-event time in ms and launches */
int uf3_ctx_timing_reset(uf3_ctx *ctx, int enable);
int uf3_ctx_timing_read(uf3_ctx *ctx, double *featurize_ms, int64_t *featurize_launches,
                        double *neighbor_ms, double *gram_ms, double *eval_ms);

/* MD route of the evaluator (round 5).  The reference's calculator rebuilds supercell, distances and neighbour pairs on every
 * call (uf3/forcefield/calculator.py:124-153, 183-343).  With skin > 0 (Angstrom; 0 = off, the default) the whole-batch
 * energy + force entries (uf3_eval[_virial][_dev] on a basis with 3-body terms) keep, per atom, every neighbour image within
 * r_cut + skin in device memory -- sorted by (species, reference supercell index), no geometry -- and each call filters that
 * list by the true distances of ITS positions: the surviving pairs and 3-body lists are the reference's, in a fixed order, so
 * results do not depend on when the lists were built.  They are rebuilt when the batch layout (offsets, cells, pbc), the basis
 * or a species changes, and when an atom has moved more than skin / 2 from where they were built (checked on the device in
 * every call; past 0.7 of that the next call rebuilds first, past all of it the call repeats itself on new lists).
 * uf3_ctx_md_stats: list builds | calls served from lists | calls repeated because an atom outran the skin. */
int uf3_ctx_md_skin(uf3_ctx *ctx, double skin);
int uf3_ctx_md_stats(uf3_ctx *ctx, int64_t *builds, int64_t *steps, int64_t *redone);

/*
 * The fit's accumulation with HOST arrays in (round 5; SURVEY 8b's `uf3_gram_accumulate`): what the reference does as
 * BasisFeaturizer.evaluate -> HDF5 tables -> WeightedLinearModel.fit_from_file (uf3/representation/process.py:121-291,
 * uf3/regression/least_squares.py:355-483), without the rows ever leaving the GPU and without anything but this library between
 * the caller's arrays and the normal equations.  uf3_fit_add takes one pointer per frame (positions [N][3], atomic numbers [N] as
 * int64 or int32, force targets [N][3]; total energies per frame) -- no concatenation on the caller's side --, packs chunks of
 * <= max_atoms_per_chunk atoms into pinned staging (two sets, one transfer per chunk on a copy stream beside the previous chunk's
 * kernels), featurizes, normalises the energy rows and targets per atom (least_squares.py:697-700), accumulates
 * [G_e | G_f | o_e | o_f | m_e | m_f] over all F columns on the device and returns without waiting for the GPU.  A neighbour
 * capacity that overflowed in an earlier chunk surfaces as UF3_ERETRY from a later uf3_fit_add or from uf3_fit_pack: uf3_fit_reset
 * and add everything again (capacities only grow).  uf3_fit_pack folds the frozen columns out, optionally sums the packed pieces
 * over the ranks of the context's communicator (uf3_comm_init) and copies the 2 n_keep^2 + 2 n_keep + 6 doubles to the host:
 * what WeightedLinearModel.fit_from_pieces solves.  frozen_idx / frozen_c: the columns fixed by the basis (bspline.py:577-635)
 * and their coefficients; keep: the others.
 */
typedef struct uf3_fit uf3_fit;
int uf3_fit_create(uf3_basis *basis, int with_forces, int64_t max_atoms_per_chunk /* <= 0: 320000 */, const int64_t *frozen_idx,
                   const double *frozen_c, int32_t n_frozen, uf3_fit **out);
void uf3_fit_destroy(uf3_fit *fit);
int uf3_fit_reset(uf3_fit *fit);
int uf3_fit_add(uf3_fit *fit, int32_t n_frames, const int64_t *atom_counts, const double *const *positions, const void *const *z,
                int z_is_int64, const double *cells /*[n_frames][9]*/, const uint8_t *pbc /*[n_frames][3]*/, const double *energies,
                const double *const *forces /* NULL: a fit without forces */);
int uf3_fit_pack(uf3_fit *fit, const int64_t *keep, int32_t n_keep, int allreduce, double *out_host);
int uf3_fit_info(const uf3_fit *fit, int64_t *n_chunks, double *n_energy_rows, double *n_force_rows);
/* the pieces into a device buffer of the caller's (2 F^2 + 2 F + 6 doubles; zeroed by uf3_fit_reset, not here) instead of the
 * accumulator's own: frames given as host arrays and batches already resident in HBM then add up in one place.  NULL: undo. */
int uf3_fit_use_flat(uf3_fit *fit, double *d_flat);
/* a call's first chunk holds this fraction of max_atoms_per_chunk and the following ones double it up to the limit (default
 * 0.125: the GPU starts after a short pack and later packs hide behind the previous chunk's kernels; 1: equal chunks) */
int uf3_fit_first_chunk(uf3_fit *fit, double fraction);
/* The chunk plan uf3_fit_add makes for these frames, computed on the host alone (no device, no context; test surface):
 * n_chunks chunks, chunk k ending behind frame chunk_ends[k] (room for n_frames entries; NULL: the count only).  A chunk
 * holds at most max_atoms atoms (<= 0: 320000) unless it is a single frame. */
int uf3_fit_plan_debug(int32_t n_frames, const int64_t *atom_counts, int64_t max_atoms, double first_fraction,
                       int32_t *chunk_ends, int32_t *n_chunks);
/* The plan the evaluator makes for one launch of its centre / gather kernel, computed on the host alone (no device, no context;
 * test surface): from the 3-body list capacity, the route (two_pass, md_step), the basis' sizes (n2 pair coefficients, n_recs knot
 * records, cw_bytes of window table), whether the basis allows the per-bond-table instances (tab_ok) and the context holds its
 * window table (has_window), the device's LDS grant lds_max and the switches (bit 0 UF3_EVAL_NO_TAB, 1 UF3_EVAL_NO_CW,
 * 2 UF3_EVAL_NO_CAP16).  Out: instance (bit 0 CW, 1 WIN, 2 TAB, 3 capacity 16 as a constant), the dynamic LDS of a workgroup,
 * the per-wave part of it (CW only, else 0) and fits (0: the launch would be refused, list too long for LDS). */
int uf3_eval_plan_debug(int32_t cap, int two_pass, int md_step, int64_t n2, int64_t n_recs, int64_t cw_bytes, int tab_ok,
                        int has_window, int32_t lds_max, int switches, int32_t *instance, int64_t *lds, int64_t *lds_per_wave,
                        int32_t *fits);

/* The plan uf3_basis_create makes of a spec -- every table it uploads and every fact its launches read --, computed on the host
 * alone (no device, no context; test surface).  switches: bit 0 UF3_NO_MFMA_FEAT, bit 1 UF3_NO_FEAT3.  table: 0 the summary
 * below; 1 the host mirror (BasisDev, its device pointers null); 2 knot records with the grouped layouts' window rows behind them;
 * 3 lut; 4 colsrc; 5 dsrc; 6 gsrc; 7 trios (TrioDev); 8 / 9 / 10 k_featurize3's window rows, fold tables and per-trio offsets
 * (empty unless feat3_ok); 11 the per-species column lists; 12 block_bounds; 13 / 14 the evaluator's cw_lut_off and cw_dim_l.
 * *len: the table's bytes; out (NULL: the length only) receives them, cap its room.  A spec uf3_basis_create refuses is refused
 * here with the same message (uf3_last_error(NULL)). */
typedef struct uf3_basis_plan_summary {
    int64_t c2_len, c3_len, n_recs, n_pair_recs, trio_rec_lo, wrow_lo, n_dsrc, n_gsrc;
    double r_cut;
    double f3_leg[2][3];          /* k_featurize3's centre leg | leg n: t0, tlast, inv_h */
    int32_t f3_leg_nk[2], f3_leg_row0[2];
    int32_t n_wrows, modes, vmodes, all_grouped7, all_banded9, feat3_ok, eval_tab_ok, eval_cw_ok;
    int32_t cw_lo, cw_ext, cw_dim_m, cw_dim_n, cw_zero, cw_bytes;
    int32_t f3_lo_p, f3_ext_p, f3_lo_n, f3_ext_n, f3_nr, n_f3rows, n_f3src;
    int32_t pairs_uniform, trio_legs_uniform;
    int32_t sp_ncols[8];
    int32_t dense_stride[16], dense_stride_f[16], dense_grouped[16], dense_dump[16];
} uf3_basis_plan_summary;
int uf3_basis_plan_debug(const uf3_basis_spec *spec, int switches, int table, void *out, int64_t cap, int64_t *len);

/* RCCL behind the C ABI (round 5; SURVEY 8b's `uf3_gram_allreduce`).  One process per GPU.  The one exchange of the path is
 * the SUM over the ranks of the packed normal-equation pieces [G_e | G_f | o_e | o_f | m_e | m_f] (and, for a decomposed
 * frame, of [forces | energy | strain derivative]); the reference returns per-chunk results to the parent process and adds them
 * there (uf3/representation/process.py:196-254, uf3/regression/least_squares.py:391-412).  Rank 0 draws an id
 * (uf3_comm_unique_id, UF3_COMM_ID_BYTES bytes), the host gets it to the other ranks by any channel it has (MPI, a file,
 * torch.distributed's store), every rank joins with uf3_comm_init -- a collective call --; uf3_allreduce_sum_f64 then sums a
 * device buffer in place over xGMI, on the context's stream, asynchronously.  librccl is opened at run time (the copy already in
 * the process, else UF3_RCCL_PATH, else the system's): the library itself links against nothing but HIP. */
#define UF3_COMM_ID_BYTES 128
int uf3_comm_unique_id(uf3_ctx *ctx, void *id);
int uf3_comm_init(uf3_ctx *ctx, int n_ranks, int rank, const void *id);
int uf3_comm_destroy(uf3_ctx *ctx);
int uf3_comm_info(const uf3_ctx *ctx, int32_t *n_ranks, int32_t *rank);     /* 0 / -1 without a communicator */
int uf3_allreduce_sum_f64(uf3_ctx *ctx, double *d_buf, int64_t n);
int uf3_gram_allreduce(uf3_ctx *ctx, double *d_packed, int64_t n);           /* the same call under SURVEY 8b's name */

int uf3_basis_create(uf3_ctx *ctx, const uf3_basis_spec *spec, uf3_basis **out);
void uf3_basis_destroy(uf3_basis *basis);
/* Diagnostics: which featurizer specialisations the basis uses.  Bit 0: one-body + pair blocks (the launch that also
 * builds the 3-body neighbour lists); bits 1..5: 3-body blocks on the generic output-stationary kernels ((symmetry images,
 * 64-column chunks) = (1,1) (1,2) (2,1) (2,2) (6,1)); bits 6..9: 3-body blocks whose window of non-trimmed bins runs on the
 * fp64 matrix cores, rows (component, l) x columns (n, m) in 16 x 16 tiles: (row tiles, column tiles) = (1,1) (1,2) (1,<=4)
 * (<=2,<=6).  Within bit 7 the 3 x 3 x <=9 windows of the reference's default trims stage grouped n windows, within bit 9
 * the wide windows run banded; both are chosen per block by uf3_basis_create.  Bit 12 (round 4): the
 * basis qualifies for k_featurize3 -- one window layout on all trios, centre legs alike, 3 x <= 9 up to 6 x <= 13 kept bins,
 * symmetric folds for equal neighbour species --, which then writes the 3-body FORCE (and with them energy) rows of every block
 * by bond factorisation on the fp64 vector units (uf3_amd/csrc/uf3_feat3.h); the launches of bits 1..9 remain for energy-only
 * calls, for batches with atoms far outside their cell and for every other basis.  Setting UF3_NO_FEAT3 in the environment
 * before uf3_basis_create switches k_featurize3 off, UF3_NO_MFMA_FEAT keeps every block on the generic kernels (used by the
 * tests to compare the three paths). */
int uf3_basis_featurizer_modes(const uf3_basis *basis, int32_t *mask);

/*
 * Feature rows of a batch of frames (y column excluded).
 *   x_e [n_frames][F]   energy rows: element counts | 2-body | 3-body      (NULL: skip)
 *   x_f [sum N][3][F]   force rows of atom a, component c at ((a*3)+c)*F   (NULL: skip)
 */
int uf3_featurize(uf3_basis *basis, const uf3_frames *frames, const double *pos /*[sumN][3]*/,
                  const int32_t *z /*[sumN]*/, double *x_e, double *x_f);
int uf3_featurize_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos,
                      const int32_t *d_z, double *d_x_e, double *d_x_f);
/*
 * Virial rows: the strain derivative of the (unnormalised) energy row, six more rows of the design matrix per frame
 * (uf3_amd/csrc/uf3_virial_rows.h).
 *   x_v [n_frames][6][F]   Voigt order xx, yy, zz, yz, xz, xy, the convention of uf3_eval_virial: d x_e / d t for the strain
 *                          eps_aa = t, or eps_ab = eps_ba = t / 2 off the diagonal, applied to cell and positions alike;
 *                          x_v[f] @ c is what uf3_eval_virial returns for the coefficients c.  One-body columns and every
 *                          column the energy row leaves at zero are zero.
 * x_e and x_f may be NULL; when given they are what uf3_featurize[_dev] writes, by the same launches.  A batch with an atom
 * far outside its cell (the batches whose 3-body force rows take the reference's image-range rule) is refused with
 * UF3_EINVAL: wrap the atoms first.  Capacity overflow as in uf3_featurize: the host entry grows and repeats, the device entry
 * reports UF3_ERETRY at a later call once the context knows its capacities (and the refusal above likewise, then).
 * With UF3_DEBUG_LDS set every launch reports "uf3 virial rows mode M: lds .. B, rows in lds|hbm ..." on stderr.
 */
int uf3_featurize_virial(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z,
                         double *x_e, double *x_f, double *x_v /* [n_frames][6][F] */);
int uf3_featurize_virial_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const int32_t *d_z,
                             double *d_x_e, double *d_x_f, double *d_x_v);
/* The same with the force rows `ld` doubles apart (ld >= F; columns F .. ld of a row are left alone), the layout uf3_gram_dev
 * and uf3_gram_force_rows_dev read through their own `ld`: with ld a multiple of 16 every row starts on a 128-byte line --
 * rows of F = 434 or 1798 doubles do not, and the partial lines at the ends of a row's column segments are written twice
 * (WRITE_SIZE 1.15 x the rows at F = 434, profiles/round5_hbm_counters.json). */
int uf3_featurize_ld_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_positions, const int32_t *d_z,
                         double *d_x_e, double *d_x_f, int64_t ld);

/*
 * Normal-equation pieces of a row block: gram[F][F] (+)= X^T X, ord[F] (+)= X^T y, with
 * X [n_rows][ld] row-major (first F columns used).  accumulate = 0 overwrites.  y or ord may be NULL:
 * then X^T y is not formed, and ord (when given) is zeroed by accumulate = 0 and left as it is by accumulate = 1.
 * With UF3_DEBUG_LDS set every launch reports its kernel on stderr ("uf3: gram kernel=mfma|small|tiled|tiled_sub ...").
 */
int uf3_gram(uf3_ctx *ctx, const double *x, const double *y, int64_t n_rows, int32_t n_feat,
             int64_t ld, int accumulate, double *gram, double *ord);
int uf3_gram_dev(uf3_ctx *ctx, const double *d_x, const double *d_y, int64_t n_rows,
                 int32_t n_feat, int64_t ld, int accumulate, double *d_gram, double *d_ord);
/*
 * The same pieces for the FORCE rows of a featurized batch (d_x_f as uf3_featurize_dev wrote it, [3 n_atoms][ld]; d_z the
 * atomic numbers the batch was featurized with).  The rows of an atom of species s are zero outside the blocks s takes part
 * in -- in the reference's dense X^T X (least_squares.py:19-67) those zeros are multiplied like everything else --: with two
 * or more species the rows are listed by species on the device and each list is multiplied on its own columns only.  The
 * result equals uf3_gram_dev's up to the order of summation; one species, narrow matrices and small batches go there.
 */
int uf3_gram_force_rows_dev(uf3_basis *basis, const double *d_x_f, const double *d_y_f, const int32_t *d_z,
                            int64_t n_atoms, int64_t ld, int accumulate, double *d_gram, double *d_ord);

/*
 * Leverage of feature rows against the system a linear fit solved (uf3_amd/csrc/uf3_leverage.h):
 *   q[g] = sum over the rows r of group g, over k, of ( sum_{j <= k} W[k][j] X[r][j] )^2  =  sum_r x_r^T (G + R^T R)^-1 x_r
 * for W = inv(cholesky(G + R^T R)).
 *   X      [n_rows][ld] row-major fp64; the first n_feat columns are used, columns n_feat .. ld never reach the result
 *          (they may hold anything, NaN included).
 *   W      [n_feat][n_feat] row-major, lower triangular with EXACT zeros above the diagonal (the caller's promise: the kernel
 *          skips every 16 x 4 matrix-core step that lies wholly above the diagonal and does not mask the others); frozen
 *          columns are whole zero rows and zero columns.
 *   group  1 or 3: how many consecutive rows are summed into one output (3: one number per atom from its three force rows).
 *          Any other value, or n_rows % group != 0, is UF3_EINVAL.
 *   q      [n_rows / group], written with plain stores by the one workgroup that owns the rows: no atomics, no Z = X W^T in
 *          memory, no scratch proportional to n_rows.  The same call twice gives bit-identical q; q >= 0, and exactly 0.0 for
 *          an all-zero row.
 * n_rows == 0 is allowed and launches nothing (q is left alone).  The _dev entry takes device pointers, runs on the context's
 * stream and does not synchronise -- after the context's first matrix-core call: that one (this entry's or uf3_gram_dev's) probes
 * the accumulator layout and waits for the answer, so make it before capturing a graph.  The host entry stages x and w, runs
 * and copies q back.
 * With UF3_DEBUG_LDS set every launch reports its configuration on stderr ("uf3: leverage kernel=k_leverage rows=.. ...").
 */
int uf3_leverage(uf3_ctx *ctx, const double *x, int64_t n_rows, int32_t n_feat, int64_t ld,
                 const double *w, int32_t group, double *q /* [n_rows / group] */);
int uf3_leverage_dev(uf3_ctx *ctx, const double *d_x, int64_t n_rows, int32_t n_feat, int64_t ld,
                     const double *d_w, int32_t group, double *d_q);

/*
 * The bookkeeping around the Gram pieces of a device-resident fit (what the reference does on the host in
 * dataframe_to_tuples, least_squares.py:666-713, freeze_columns / VarianceRecorder, :19-67, :296-304, :817-890), on the
 * context's stream, nothing synchronises:
 *   uf3_fit_rows_dev   energy rows of a batch divided by their frames' atom counts (per-atom normalisation, :697-700; in
 *                      place), and the target moments: moments[1..2] += (sum, sum of squares) of the FROZEN energies
 *                      y_e - x_e[:, frozen] . c_frozen, moments[4..5] += those of the force targets (y_f may be NULL).
 *                      moments[0] / [3] (the counts) are the caller's.  The energy rows are PACKED: row f starts at
 *                      d_x_e + f * n_feat (no leading dimension, unlike uf3_gram_dev: pass unpadded rows).
 *   uf3_fit_pack_dev   flat [G_e (F x F) | G_f (F x F) | o_e (F) | o_f (F) | m_e (3) | m_f (3)] over all F columns ->
 *                      the same layout over the n_keep unfrozen columns, frozen columns folded out on the Gram level
 *                      (o_keep -= G[keep, frozen] . c_frozen): the additive pieces one rank hands to the all-reduce.
 *                      n_keep == 0 (every column frozen) is allowed: the six moments are then the whole packed buffer.
 * keep / frozen are int64 column indices in HBM, c_frozen the frozen coefficients in HBM.
 */
int uf3_fit_rows_dev(uf3_ctx *ctx, int32_t n_frames, int32_t n_feat, double *d_x_e, const double *d_atom_counts,
                     const double *d_y_e, const double *d_y_f, int64_t n_y_f, const int64_t *d_frozen,
                     const double *d_c_frozen, int32_t n_frozen, double *d_moments /*[6]*/);
int uf3_fit_pack_dev(uf3_ctx *ctx, int32_t n_feat, const double *d_flat, const int64_t *d_keep, int32_t n_keep,
                     const int64_t *d_frozen, const double *d_c_frozen, int32_t n_frozen, double n_energy_rows,
                     double n_force_rows, double *d_packed);

/*
 * Energy and forces of a fitted model on a batch of frames.
 *   c1 [S]; c2 concatenated pair coefficient vectors (nk-4 each, all basis functions);
 *   c3 concatenated full L*M*N grids per trio (BSplineBasis.decompress_3B output).
 *   energies [n_frames]; forces [sum N][3] (NULL: energies only).
 *
 * The leg rule of the whole evaluator family (uf3_eval*, uf3_eval_atoms, uf3_eval_centres, the MD / relax / NEB / NPT drivers,
 * uf3_hessian, uf3_site_terms, uf3_heat_flux, uf3_mc_*):
 *   - The energy of a triplet is the reference's.  Leg l takes the neighbour of lower atomic number; of two neighbours of one
 *     species, the one with the lower reference supercell index AS SEEN FROM THE REAL COPY OF THE CENTRE (image rank with b
 *     slowest, a middle, c fastest, each axis in the order 0, +1, -1, +2, ...; then the atom's index in the frame).
 *     The tie-break decides a number only where the two legs differ (a symmetry-1 trio); on equal l and m legs either
 *     assignment is the same function, and every kernel keeps the order it always had there (and with it its bits).
 *   - Every other quantity is the exact derivative or partition of that energy: forces, virials, site energies and site
 *     virials, the heat current, the Hessian with its mixed rows and Born term, the MC energy differences.
 * Two properties of a basis with a symmetry-1 trio (two neighbours of one species on UNEQUAL l and m legs) follow:
 *   1. The forces are not the reference calculator's.  Its force loop numbers ghost-centred triplets differently from its
 *      energy loop, so its forces are not the gradient of its energy there; the evaluator's are.  (The featurizer's force rows
 *      stay the reference's.)
 *   2. The energy depends on the numbering of the atoms and on which cell image holds an atom (wrap a frame and it may change).
 *      That is the reference's property; nothing here is invariant under renumbering or lattice translations of single atoms
 *      on such a basis.
 */
int uf3_eval(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z,
             const double *c1, const double *c2, const double *c3, double *energies, double *forces);
int uf3_eval_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const int32_t *d_z,
                 const double *c1, const double *c2, const double *c3 /* host */,
                 double *d_energies, double *d_forces);

/*
 * Same, plus the analytic strain derivative of the energy per frame: virials [n_frames][6] = dE/d(eps) in
 * Voigt order (xx, yy, zz, yz, xz, xy), eV; stress = virial / cell volume.  Row N3 of SURVEY section 8f: the
 * reference only offers finite differences (calculator.py:399-404).
 */
int uf3_eval_virial(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z,
                    const double *c1, const double *c2, const double *c3, double *energies, double *forces,
                    double *virials);
int uf3_eval_virial_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const int32_t *d_z,
                        const double *c1, const double *c2, const double *c3 /* host */,
                        double *d_energies, double *d_forces, double *d_virials);

/*
 * The share of atoms [atom_begin, atom_end) (indices into the concatenated batch) of the same quantities: the
 * one-body, pair and centre-role triplet energies of those atoms, their force rows (the other rows of `forces`
 * are zero on return from the host variant and untouched by the _dev variant) and their share of the strain
 * derivative.  Every atom gathers its own force, so shares over disjoint ranges add up to uf3_eval_virial's
 * results: the spatial decomposition of ONE large frame over GPUs is a range per rank + one sum-reduce (SURVEY
 * section 8f row N4; not in the reference, whose calculator is single-process).  forces / virials may be NULL.
 */
int uf3_eval_atoms(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z,
                   const double *c1, const double *c2, const double *c3, int64_t atom_begin, int64_t atom_end,
                   double *energies, double *forces, double *virials);
int uf3_eval_atoms_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const int32_t *d_z,
                       const double *c1, const double *c2, const double *c3 /* host */, int64_t atom_begin,
                       int64_t atom_end, double *d_energies, double *d_forces, double *d_virials);

/*
 * The share of the CENTRES [atom_begin, atom_end): their one-body, pair and centre-role triplet energies and strain
 * derivative (as above), their pair forces, and what their triplets put on EVERY atom -- each triplet is evaluated once, at
 * its centre; rows of atoms inside the range or in its halo (the atoms its 3-body lists mention) come back non-zero, all
 * others zero.  Shares over disjoint ranges add up to uf3_eval_virial's results like those of uf3_eval_atoms, at a third
 * of the triplet work: what a rank of a decomposed frame computes before the one sum-reduce of
 * [energy | strain derivative | forces] (uf3_amd/parallel.py: sharded_evaluate).  forces / virials may be NULL.
 * Both variants write EVERY row of `forces` (the _dev variant zeroes the whole array on the stream before it adds the
 * shares): the caller does not clear the buffer between calls.
 */
int uf3_eval_centres(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z,
                     const double *c1, const double *c2, const double *c3, int64_t atom_begin, int64_t atom_end,
                     double *energies, double *forces, double *virials);
int uf3_eval_centres_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const int32_t *d_z,
                         const double *c1, const double *c2, const double *c3 /* host */, int64_t atom_begin,
                         int64_t atom_end, double *d_energies, double *d_forces, double *d_virials);

/*
 * Neighbour indices in the reference's supercell numbering (ghost index =
 * image_rank * N + atom, geometry.py:108-149), single frame, host buffers.
 *   pair_ij [P][pair_cap][2]  2-body (i, j) per pair block, row-major sorted; pair_count [P]
 *   n3_ij   [n3_cap][2]       3-body neighbour pairs of real centres;         n3_count [1]
 * Pass caps of 0 (and NULL arrays) to obtain the counts only.
 */
int uf3_neighbors_debug(uf3_basis *basis, const uf3_frames *frame, const double *pos, const int32_t *z,
                        int64_t *pair_count, int64_t *pair_ij, int64_t pair_cap,
                        int64_t *n3_count, int64_t *n3_ij, int64_t n3_cap);
/* The 3-body neighbour lists the LAST featurizer / evaluator call on the basis' context built and consumed (the product path's
 * own lists, not the separate walk behind uf3_neighbors_debug): counts [natoms] and, per atom, the reference supercell index
 * (image_rank * N + atom) of every entry in list order, sidx [natoms][sidx_cap] with sidx_cap >= *cap_out (pass sidx = NULL to
 * learn the capacity first).  Test infrastructure (reference: uf3/representation/angles.py:289-346 identify_ij): valid only
 * straight after a synchronised single-frame call and before anything else runs on the context. */
int uf3_n3_lists_debug(uf3_basis *basis, int64_t natoms, int64_t *cap_out, int32_t *counts, int32_t *sidx, int64_t sidx_cap);

/*
 * The same 2-body pairs with their geometry: pair_geo [P][pair_cap][4] = distance, then (R_j - R_i) / distance -- what
 * distances_by_interaction / derivatives_by_interaction (distances.py:19-143) select out of the dense distance matrix
 * and what compute_direction_cosines (:331-364) divides, as lists, in the order of pair_ij.  Caps of 0: counts only.
 */
int uf3_pair_geometry(uf3_basis *basis, const uf3_frames *frame, const double *pos, const int32_t *z,
                      int64_t *pair_count, int64_t *pair_ij, double *pair_geo, int64_t pair_cap);

/*
 * Pair-distance histograms of a batch of frames: what DataAnalyzer.get_distances + update_histograms (uf3/data/analyze.py) and
 * summarize_distances (uf3/representation/distances.py:367-442) build from cdist of each frame against its explicit supercell
 * (geometry.get_supercell with r_cut = the basis' r_cut; a non-periodic frame against itself), without the n x 27 n matrix.
 * Every ordered (centre i of the frame, image j of the supercell) pair whose distance d satisfies r_min < d <= r_max
 * (upper_inclusive != 0, the analyzer's mask) or r_min < d < r_max (upper_inclusive == 0, summarize_distances'), with the
 * range of the pair block of the two species, adds one to bin k of that pair: edges[k] <= d < edges[k+1], the last bin closed,
 * d outside [edges[0], edges[n_bins]] not counted (np.histogram on an edge array).
 *   basis      species and ranges: RawDeviceBasis-style, every pair at (r_min, r_max) and r_cut = the supercell's range
 *   edges      [n_bins + 1] host, strictly increasing, edges[0] >= 0
 *   noise      [n_noise][3] host or NULL: added to the supercell positions by reference supercell index (image_rank * N + atom,
 *              block 0 = the frame itself) -- ase.Atoms.rattle of the supercell (analyze.py:get_distances): the centres stay put
 *              and every atom also meets its own image at |noise|.  n_noise must cover the supercell of every frame
 *   per_frame  0: out [P][n_bins] summed over the frames;  1: out [n_frames][P][n_bins]
 *   out        int64 counts, overwritten; pair blocks in the basis' order
 * UF3_EINVAL for n_bins < 1, edges not strictly increasing or starting below 0, a noise array shorter than a frame's supercell,
 * null pointers.  The host entry reports UF3_ESPECIES for an element outside the basis; the _dev entry enqueues everything on the
 * context's stream and waits for nothing (edges and noise are read before it returns), so its caller must pass species of the
 * basis.
 */
int uf3_pair_histogram(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z, int32_t n_bins,
                       const double *edges, int upper_inclusive, const double *noise, int64_t n_noise, int per_frame,
                       int64_t *out);
int uf3_pair_histogram_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const int32_t *d_z, int32_t n_bins,
                           const double *edges, int upper_inclusive, const double *noise, int64_t n_noise, int per_frame,
                           int64_t *d_out);

/*
 * Batched fp64 solve-and-score of a cut-off / regulariser scan (uf3_amd.regression.optimize.CutoffScan).  Device buffers,
 * everything enqueued on the context's stream, nothing waited for.
 *   slots      [n_folds][2 n^2 + 2 n + 6]: one uf3_fit_pack_dev buffer per fold, G_e | G_f | o_e | o_f | m_e | m_f over the
 *              n = n_cols unfrozen columns of the large basis (1 <= n_folds <= 32)
 *   cols       column maps of the lower bases, concatenated: basis b has m_b = col_off[b+1] - col_off[b] columns, cols[col_off[b]
 *              + i] the position of its column i among the n (int32)
 *   reg_rc, reg_v, reg_off   per lower basis the unit regulariser pieces P_k = R_k^T R_k (k = ridge 1b, 2b, 3b, curvature 2b,
 *              3b) in COO over its m_b columns: entries reg_off[b] .. reg_off[b+1], (row, col) int32 pairs, 5 values each; one
 *              entry per (row, col)
 *   sys        [n_sys][6] int64: basis, held-out fold (-1: none), workspace offset (doubles), solution offset (doubles), first
 *              row (the prefix sum of m over the systems before it; total_rows = the sum over all), unused
 *   sys_w      [n_sys][7]: alpha_e, alpha_f, lambda[5]
 *   ws         ws_len doubles; system s uses m*m + 2m of them from its offset: A (row-major; on return L in the lower triangle,
 *              A's strict upper triangle untouched), the diagonal of A, the right-hand side b
 *   x          x_len doubles: the solution of system s at its offset
 *   sse        [n_sys][4]: squared errors of the solution, energy (per-atom rows) and force, on the training slots and on the
 *              held-out slot: c^T G c - 2 c^T o + sum y^2, unclamped (zero for the held-out pair when fold = -1; NaN on failure)
 *   status     [n_sys]: 0, or j + 1 where j is the first pivot <= 0 or not finite; -1 / -2 / -3 for a workspace or solution
 *              offset out of range, a column outside [0, n), m above 4096
 * A = alpha_e sum_{f != fold} G_e,f[cols, cols] + alpha_f sum_{f != fold} G_f,f[cols, cols] + sum_k lambda_k P_k, b likewise from
 * the ordinates; solved by Cholesky (trailing updates on the fp64 matrix cores).
 */
int uf3_scan_solve_dev(uf3_ctx *ctx, int32_t n_cols, int32_t n_folds, const double *d_slots, const int32_t *d_cols,
                       const int64_t *d_col_off, const int32_t *d_reg_rc, const double *d_reg_v, const int64_t *d_reg_off,
                       int32_t n_sys, int64_t total_rows, const int64_t *d_sys, const double *d_sys_w, double *d_ws,
                       int64_t ws_len, double *d_x, int64_t x_len, double *d_sse, int32_t *d_status);

/*
 * Molecular dynamics on the device (uf3_amd.forcefield.md.MolecularDynamics; kernels in uf3_md.h).  The object owns positions
 * (kept UNWRAPPED), velocities, forces, inverse masses and species of a batch of frames
 * in HBM and steps them with velocity Verlet (friction 0) or BAOAB Langevin dynamics; the forces come from the evaluator
 * (uf3_eval[_virial]_dev's code path) between two fused integrator launches.  Units: Angstrom, fs, amu, eV, K.
 * Atoms outside the cell: the evaluator bins wrapped copies for its cell lists, but it takes the reference's finite image range
 * (-fac .. fac cells per axis) around the positions AS GIVEN, as uf3_eval does on the same frame.  An atom that has drifted out of
 * its cell loses the interactions that range no longer reaches from where it is: the energy and forces of every step are uf3_eval's
 * of the unwrapped positions the object holds, which are the wrapped frame's only while every atom is inside its cell.  Nothing in
 * the object wraps unless uf3_md_set_wrap (below) has turned wrapping on, which is the repair for runs in which atoms may cross
 * a cell face (diffusion, a melt); without it such a run is to be stopped and continued from wrapped positions
 * (uf3_md_set_state) before that happens.  The same holds for uf3_relax_* and uf3_neb_*, which keep positions
 * unwrapped for the same reason (tests/test_gpu_redescribed.py holds the rule).
 *   uf3_md_create          copies frames, positions [N][3], velocities [N][3] (NULL: zero), species, masses [N] and the model
 *                          (c1 / c2 / c3 as for uf3_eval) into the object; no evaluation yet.  Masses positive and finite.
 *   uf3_md_set_state       host arrays in; NULL keeps that part.  New positions invalidate the forces.
 *   uf3_md_get_state       host arrays out; NULL skips.  Forces / energies of positions set since the last evaluation are
 *                          evaluated first.
 *   uf3_md_init_velocities Maxwell-Boltzmann velocities at temperature_K from the Philox stream (draws 2, 3 of the current
 *                          step), each frame's centre-of-mass velocity removed; exact_temperature: each frame rescaled to
 *                          exactly temperature_K with 3N degrees of freedom (a frame whose kinetic energy is 0 stays at rest).
 *   uf3_md_run             n_steps steps of dt_fs; friction_per_fs > 0: Langevin at temperature_K, 0: NVE.  Normals of atom i
 *                          in the step opened at absolute step s: Philox4x32-10, counter (i, s lo, s hi, 0 / 1), key (seed lo,
 *                          seed hi), Box-Muller -- run(a); run(b) equals run(a + b).  The context's MD skin is `skin` for the
 *                          run and the caller's again on return (also on errors); the change drops the neighbour lists, so
 *                          every run starts with one list build.  A 2-body-only basis never takes the MD route and rebuilds its
 *                          lists on every step.  thermo_every > 0: one record per frame after every thermo_every-th step of the
 *                          run, [PE, KE] or, with_stress, [PE, KE, W (6), K (6)] (W = dE/d(strain), Voigt order; K = sum m v (x) v,
 *                          eV); thermo must then hold n_steps / thermo_every records (NULL when none is due).  A force call that
 *                          fails returns its code; the step counter then counts the completed steps and the state is that of
 *                          the failed step's drift.
 *   uf3_md_info            absolute step counter, atoms, frames.
 *   uf3_md_run_npt         n_steps steps at constant pressure (kernels in uf3_npt.h): isotropic Martyna-Tobias-
 *                          Klein dynamics, every frame its own piston.  A frame's cell is s * (the cell it was created with);
 *                          v_eps = d ln s / dt.  pressure_eV_A3: the target P0; barostat_time_fs: tau_p of the piston mass
 *                          W_p = (3N + 3) k_B piston_temperature_K tau_p^2 (piston_temperature_K > 0 always; the Python layer
 *                          passes temperature_K unless told otherwise).  friction_per_fs and barostat_friction_per_fs both 0:
 *                          NPH, which conserves H = KE + PE + P0 V + W_p v_eps^2 / 2; otherwise the atoms get uf3_md_run's O-step
 *                          and the piston v_eps = c_p v_eps + sqrt((1 - c_p^2) k_B temperature_K / W_p) xi (pure damping at
 *                          temperature_K = 0).  Random numbers: the atoms' counters are uf3_md_run's, (i, s lo, s hi, 0 / 1) with
 *                          i < 2^28; the piston of frame f draws from counter (2^31 | f, s lo, s hi, 0), which no atom's
 *                          counter can equal.  run(a); run(b) does the arithmetic of run(a + b).  Every frame must be periodic
 *                          along all three axes.  For its own duration the call puts the context's MD state into a "cells
 *                          live on the device" mode next to the run's skin: the evaluator's list key stops comparing cells, its
 *                          kernels read the frame's current cell rows from the device copy the integrator updates, and the
 *                          displacement test is made against reference positions that are scaled along with the cell, with the
 *                          per-frame limit (s (skin + r_cut) - r_cut) / 2, s relative to the build; a scale outside the range
 *                          over which the build's image ranges hold voids the lists.  The host reads the cells back in front of
 *                          a list build and at the end of the run only.  Skin and mode are the caller's again on return, also on
 *                          errors.  Records, when thermo_every > 0: [PE, KE, W (6), K (6), V, s, H] (17 doubles) per frame.
 *   uf3_md_get_cells       the current cells [n_frames][9], scales s [n_frames] and strain rates v_eps [n_frames] (1/fs); NULL
 *                          skips.  Before the first constant-pressure run: the cells of uf3_md_create, 1 and 0.
 *   uf3_ctx_md_live        1 while the context's MD state is in the "cells live on the device" mode (tests), else 0.
 *   uf3_philox_debug       Philox4x32-10 on the device for caller-given counters [n][4] and keys [n][2] (tests).
 */
typedef struct uf3_md uf3_md;
int uf3_md_create(uf3_basis *basis, const uf3_frames *frames, const double *pos, const double *vel, const int32_t *z,
                  const double *masses, const double *c1, const double *c2, const double *c3, uf3_md **out);
void uf3_md_destroy(uf3_md *md);
int uf3_md_set_state(uf3_md *md, const double *pos, const double *vel);
int uf3_md_get_state(uf3_md *md, double *pos, double *vel, double *forces, double *energies /*[n_frames]*/);
int uf3_md_init_velocities(uf3_md *md, double temperature_K, uint64_t seed, int exact_temperature);
int uf3_md_run(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs, uint64_t seed, double skin,
               int64_t thermo_every, int with_stress, double *thermo);
int uf3_md_info(const uf3_md *md, int64_t *step, int64_t *n_atoms, int32_t *n_frames);
int uf3_md_run_npt(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs, double pressure_eV_A3,
                   double barostat_time_fs, double barostat_friction_per_fs, double piston_temperature_K, uint64_t seed,
                   double skin, int64_t thermo_every, double *thermo);
int uf3_md_get_cells(uf3_md *md, double *cells, double *scales, double *strain_rates);
int uf3_ctx_md_live(uf3_ctx *ctx, int32_t *live);
/* uf3_md_run with heat-current samples (uf3_flux.h; the definitions stand in front of uf3_site_terms below): what uf3_md_run does,
 * and after every flux_every-th step of the run one record [n_frames][6] = J_conv (3), J_pot (3) (eV Angstrom / fs) of the closed
 * state -- velocities at integer time, the positions the forces belong to.  flux must hold n_steps / flux_every records (NULL
 * when none is due; flux_every = 0 is uf3_md_run call for call).  The launch that closes a sampled step does not open the next
 * one, which is the split a run boundary makes anyway: the trajectory and the thermo records keep their bits, and run(a); run(b)
 * gives the records of run(a + b).  The lists of the samples are the state's own (sized at its first sample with a quarter of
 * headroom; a sample whose lists overflow is redone with a larger capacity); one stream synchronisation per sample.  There is
 * no such entry for uf3_md_run_npt: the heat current is sampled at constant volume only (the Python layer refuses the pair with
 * UF3_EINVAL). */
int uf3_md_run_flux(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs, uint64_t seed,
                    double skin, int64_t thermo_every, int with_stress, double *thermo, int64_t flux_every, double *flux);
/* uf3_md_run with grade samples (uf3_site_rows.h; the definitions stand in front of uf3_site_rows below): what uf3_md_run does,
 * and after every grade_every-th step of the run one record [n_frames][2] = (the frame's largest site grade, the frame-local
 * index of its atom as a double) of the closed state, placed exactly as uf3_md_run_flux places a heat-current sample: the
 * trajectory and the thermo records keep their bits, and run(a); run(b) gives the records of run(a + b).  d_w: uf3_leverage's W
 * [n_feat][n_feat] ON THE DEVICE.  grades must hold n_steps / grade_every records (NULL when none is due).  grade_stop > 0: the
 * run ends after the first sample in which any frame's maximum exceeds grade_stop; *steps_done is the number of completed steps of
 * this call, the state is that of a run of *steps_done steps bit for bit (a later run continues from it), and only the thermo and
 * grade records due up to that sample are filled.  grade_stop <= 0: never.  The whole batch stops, not the one frame.  The
 * samples' lists are the state's own, as for the flux; one stream synchronisation per sample.  The grades describe the WRAPPED
 * frame, as uf3_site_terms does.  No constant-pressure variant, and no entry that samples grades and the heat current in one run
 * (the Python layer refuses both pairs). */
int uf3_md_run_grade(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs, uint64_t seed,
                     double skin, int64_t thermo_every, int with_stress, double *thermo, const double *d_w, int64_t grade_every,
                     double grade_stop, double *grades, int64_t *steps_done);
/* Periodic wrapping with image counts, opt-in (k_md_wrap, uf3_md.h).  Off -- the default -- nothing above
 * changes: no launch, no buffer, no bit.  On, the object stores pos and int32 img [N][3] and its position is pos + img . cell
 * with the frame's CURRENT cell (rows are lattice vectors; under uf3_md_run_npt the cell the integrator has just written).
 * k_md_wrap takes n = floor(fractional coordinate) on periodic axes, pos -= n . cell, img += n; axes that are not periodic and
 * frames without a periodic axis are left alone bit for bit.  It runs in front of every neighbour-list build made for the
 * object (the first of a run, the early-warning rebuild, the "lists outrun" repeat) and in front of every evaluation on the
 * rebuild-everything route (skin 0, 2-body bases), never between a list build and the steps on its lists.  Invariant: an
 * evaluation of a wrapping object never sees an atom farther outside its cell than that atom has moved since the last wrap
 * (at most skin / 2, or the constant-pressure limit), so the evaluator's image-range rule and the samplers' nearest-image rule
 * describe the same crystal and the hazard above does not arise.  A wrap rounds (pos - n . cell is not exact): with wrapping
 * on, the last bits of a trajectory depend on where the lists were built (the skin, the run boundaries); it stays deterministic
 * for a given sequence of calls, and run(a); run(b) agrees with run(a + b) to rounding, not bit for bit.
 *   uf3_md_set_wrap     on: wraps now and from then on as described; off: folds img into pos and zeroes it.  Either drops
 *                       the evaluator's lists and the object's forces only if a position changed.
 *   uf3_md_get_state    keeps its meaning: positions UNWRAPPED, pos + img . cell formed on the device.
 *   uf3_md_get_wrapped  the stored pair: pos [N][3] and img [N][3] (zeros while wrapping has never been on); NULL skips.
 *   uf3_md_set_state    positions are taken as given and img becomes zero.
 * Mean-squared displacement (k_md_msd_partial, k_md_msd_frame):
 *   uf3_md_msd_origin   the origin [N][3] of the displacements; NULL: the current unwrapped positions.  A run that samples
 *                       without one takes the positions it starts from.
 *   uf3_md_run_msd      what uf3_md_run does, and after every msd_every-th step one record [n_frames][4 S + 4] of the closed
 *                       state, S the basis' species count: per species sum |dr|^2, sum dx, sum dy, sum dz over its atoms with
 *                       dr = pos + img . cell - origin, then sum m dr (3) and sum m over the frame.  Placed as uf3_md_run_flux
 *                       places its samples: the trajectory and the thermo records keep their bits.  No atomics: the order of
 *                       the sums depends on the atom counts alone and records repeat bit for bit.  msd must hold
 *                       n_steps / msd_every records (NULL when none is due).  Constant volume only, and one sampler per run
 *                       (the Python layer refuses msd_every at a pressure or next to flux_every / grade_every). */
int uf3_md_set_wrap(uf3_md *md, int on);
int uf3_md_get_wrapped(uf3_md *md, double *pos, int32_t *images);
int uf3_md_msd_origin(uf3_md *md, const double *origin);
int uf3_md_run_msd(uf3_md *md, int64_t n_steps, double dt_fs, double temperature_K, double friction_per_fs, uint64_t seed,
                   double skin, int64_t thermo_every, int with_stress, double *thermo, int64_t msd_every, double *msd);
/* Switching runs: molecular dynamics on H(lambda) = K + lambda U_uf3 + (1 - lambda) U_E with lambda moving during the run
 * (non-equilibrium thermodynamic integration; kernels in uf3_ti.h).  U_E = 1/2 sum_i k_i |x_i - x0_i|^2 is an
 * Einstein crystal on the reference sites x0 (Angstrom) with per-atom springs k_i (eV / Angstrom^2); all k_i = 0 leaves the
 * scaled model alone (reversible scaling).
 *   uf3_md_set_reference  ref_pos [N][3], finite; NULL: the current positions.  spring [N], finite and >= 0; NULL: all zero.
 *                         Allocates the feature's device memory: an object that never switches has none of it.
 *   uf3_md_run_switch     n_steps steps of the scheme of uf3_md_run (velocity Verlet; BAOAB when friction_per_fs > 0, 1/fs)
 *                         with dt_fs (fs), every frame at its own temperature temperatures_K [n_frames] (K, >= 0) and its own
 *                         lambda_f(j) = lambda_a[f] + (lambda_b[f] - lambda_a[f]) schedule[j] for the states j = 0 .. n_steps
 *                         of the run; lambda_a, lambda_b [n_frames] and schedule [n_steps + 1] finite and in [0, 1].  Step
 *                         j -> j + 1 kicks with F_i(j) = lambda_f(j) F_uf3,i - (1 - lambda_f(j)) k_i (x_i - x0_i), drifts,
 *                         evaluates, and kicks with F(j + 1).  With D_f = U_uf3,f - U_E,f the work is
 *                         W_f += (lambda_f(j + 1) - lambda_f(j)) (D_f(j) + D_f(j + 1)) / 2 (eV), summed on the device in step
 *                         order; work [n_frames] receives the work of THIS call, so a switch made in two calls on the two
 *                         halves of a schedule adds up to one call's.  fix_com != 0 keeps every frame's momentum where it is:
 *                         the mixed force loses m_i / M_f times its sum over the frame, and the O-step's noise dv_i = sig_i xi_i
 *                         loses sum_j m_j dv_j / M_f.  every > 0: records [n_steps / every][n_frames][5] =
 *                         [lambda, U_uf3, U_E, KE, W so far] (eV) of the closed state after every every-th step; every = 0:
 *                         records NULL.  seed, skin and the absolute step counter are uf3_md_run's: the normals are those of
 *                         (atom, absolute step, draws 0 / 1), and a switch goes on from where a run stopped.  No atomics; the
 *                         order of every sum depends on the atom counts alone: work and records repeat bit for bit.
 * UF3_EINVAL with a message: an object that wraps (a spring needs the unwrapped displacement; solids do not diffuse), an
 * object that runs at a pressure, uf3_md_run_switch before uf3_md_set_reference, and any argument outside the above (checked
 * in parameter order). */
int uf3_md_set_reference(uf3_md *md, const double *ref_pos, const double *spring);
int uf3_md_run_switch(uf3_md *md, int64_t n_steps, double dt_fs, const double *temperatures_K, double friction_per_fs, uint64_t seed,
                      double skin, const double *lambda_a, const double *lambda_b, const double *schedule, int fix_com,
                      int64_t every, double *records, double *work);
int uf3_philox_debug(uf3_ctx *ctx, int64_t n, const uint32_t *counters, const uint32_t *keys, uint32_t *out);

/*
 * Batched structure relaxation on the device (uf3_amd.forcefield.relax.Relaxation; kernels in uf3_relax.h): FIRE in ASE's
 * formulation (N_min 5, f_inc 1.1, f_dec 0.5, alpha_start 0.1, f_alpha 0.99; mass-free), every frame its own optimiser.  The
 * object owns positions (kept UNWRAPPED), velocities, forces and the per-frame state in HBM; the forces come from the evaluator.
 *   uf3_relax_create     copies frames, positions [N][3], species, an optional per-atom fixed mask [N] (0 / 1; NULL: none;
 *                        refused with relax_cell) and the model (c1 / c2 / c3 as for uf3_eval); no evaluation yet.  relax_cell:
 *                        frames periodic along all three axes also relax their cell (x = q D, cell = cell0 D, cell coordinates
 *                        n D; force on them -D^-T W / n, W the strain derivative of uf3_eval_virial); other frames positions only.
 *   uf3_relax_run        evaluations 0 .. max_steps; after each, a frame still running is tested -- converged when every atom's
 *                        |F_i| < fmax (and, with the cell, every row of D^-T W / n) -- and, but after the last, moved by one FIRE
 *                        step (dt: the first step's time step; dt_max; maxstep: the trust radius over the frame's whole step,
 *                        cell rows included).  Non-finite forces, energy or strain derivative freeze the frame (status 2);
 *                        converged frames (status 1) are never moved again; status 0: still running.  The FIRE state carries
 *                        over between runs.  The context's MD skin is `skin` for a positions-only run and 0 for a cell run,
 *                        the caller's again on return (also on errors).  The host looks at the device every check_every
 *                        steps and stops when no frame runs; cell runs wait for the new cells every step.  record_every > 0:
 *                        records [max_steps / record_every + 1][n_frames][2] (energy, criterion) of evaluations 0,
 *                        record_every, ...; rows after a stop repeat each frame's final values (NULL when record_every is 0).
 *   uf3_relax_get_state  host arrays out, NULL skips: positions [N][3], cells [n_frames][9], forces [N][3] (Cartesian) and
 *                        energies [n_frames] of the current positions (evaluated first if they moved since), status, steps
 *                        (moves made) and the last criterion [n_frames] (NaN before the first run).
 */
typedef struct uf3_relax uf3_relax;
int uf3_relax_create(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z, const uint8_t *fixed,
                     const double *c1, const double *c2, const double *c3, int relax_cell, uf3_relax **out);
void uf3_relax_destroy(uf3_relax *r);
int uf3_relax_run(uf3_relax *r, int64_t max_steps, double fmax, double dt, double dt_max, double maxstep, double skin,
                  int64_t check_every, int64_t record_every, double *records);
int uf3_relax_get_state(uf3_relax *r, double *pos, double *cells /*[n_frames][9]*/, double *forces, double *energies,
                        int32_t *status, int64_t *steps, double *fmax /*[n_frames]*/);

/*
 * Batched nudged elastic bands on the device (uf3_amd.forcefield.neb.NudgedElasticBand; kernels in uf3_neb.h).  A band is M >= 3
 * consecutive frames (images) of equal atom count, species, cell and pbc; images 0 and M - 1 are end points: evaluated for their
 * energies, never moved.  Interior image i: t+ = R_{i+1} - R_i, t- = R_i - R_{i-1} as stored (positions are kept UNWRAPPED, no
 * minimum image), the improved tangent of Henkelman & Jonsson (2000) from the neighbours' energies, g = F - (F.tau^) tau^ +
 * k (|t+| - |t-|) tau^; with climb the interior image of highest energy at that evaluation (ties: the lowest index) has
 * g = F - 2 (F.tau^) tau^ instead.  Rows of fixed atoms are 0 in t+, t- and g.  One FIRE (uf3_relax_run's constants and rules,
 * maxstep over the whole vector) per band over all its interior images; criterion: the largest per-atom |g|.
 *   uf3_neb_create     copies frames, positions [N][3], species, an optional fixed mask [N] (0 / 1; NULL: none), the model, the
 *                      bands (band b: frames band_first_frame[b] .. band_first_frame[b + 1] - 1; [0] = 0, [n_bands] = n_frames)
 *                      and one spring constant per band (eV / A^2).  UF3_EINVAL: a band of fewer than 3 images; images of a band
 *                      that differ in atom count, species, cell, pbc or fixed mask; neighbouring images with identical
 *                      positions; a spring that is not positive and finite.
 *   uf3_neb_run        evaluations 0 .. max_steps; after each, a band still running is tested -- converged (status 1) when its
 *                      criterion < fmax; frozen (status 2) on a non-finite energy or force anywhere in the band, |tau| = 0 or
 *                      a non-finite sum -- and, but after the last, moved by one FIRE step.  State carries over between runs;
 *                      a converged band is tested again by the next run (its fmax and climb may differ) and moves only if it
 *                      fails that test; a frozen band stays frozen.
 *                      The context's MD skin is `skin` during the run, the caller's again on return (also on errors).  The
 *                      host looks at the device every check_every steps.  record_every > 0: records
 *                      [max_steps / record_every + 1][n_frames + 2 n_bands] of evaluations 0, record_every, ...: the energy of
 *                      every frame, then per band (criterion, climbing image as a double, -1: none); rows after a stop repeat
 *                      the final values (NULL when record_every is 0).
 *   uf3_neb_get_state  host arrays out, NULL skips: positions, true forces and NEB forces g [N][3] (0 on end points, fixed
 *                      atoms and images whose tangent vanishes; tangents as in the last run) and energies [n_frames] of the current positions (evaluated first if
 *                      they moved since); per band status, steps (moves made), the last criterion (NaN before the first run)
 *                      and the image that climbed at the last evaluation (index within the band, or -1).
 */
typedef struct uf3_neb uf3_neb;
int uf3_neb_create(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z, const uint8_t *fixed,
                   const double *c1, const double *c2, const double *c3, int32_t n_bands,
                   const int32_t *band_first_frame /*[n_bands + 1]*/, const double *spring /*[n_bands]*/, uf3_neb **out);
void uf3_neb_destroy(uf3_neb *neb);
int uf3_neb_run(uf3_neb *neb, int64_t max_steps, double fmax, double dt, double dt_max, double maxstep, double skin, int climb,
                int64_t check_every, int64_t record_every, double *records);
int uf3_neb_get_state(uf3_neb *neb, double *pos, double *forces, double *neb_forces, double *energies, int32_t *status,
                      int64_t *steps, double *criterion, int32_t *climbing /*[n_bands]*/);

/*
 * IDPP band initialisation on the device (uf3_amd.forcefield.neb.IDPP / idpp_interpolate; kernels in uf3_idpp.h): bands relaxed on
 * the image dependent pair potential (Smidstrup et al., J. Chem. Phys. 140, 214106; ASE's idpp_interpolate), an artificial surface
 * built from interpolated pair distances that keeps atoms of a band apart where a linear band drives them through each other.
 * Image k of a band of M images, lambda = k / (M - 1), over all pairs with one image each (no cut-off):
 *     d_ij = |D_ij|, D_ij the nearest-image vector x_j - x_i;   t_ij = (1 - lambda) d_ij(R^0) + lambda d_ij(R^{M-1});
 *     S = sum_{i<j} (t_ij - d_ij)^2 / d_ij^4  (1 / A^2);   F_i = -dS/dx_i = sum_{j != i} c_ij D_ij / d_ij,
 *     c_ij = -2 (t - d) (d + 2 (t - d)) / d^5.
 * Nearest-image vector: the fractional difference along the periodic axes (the cell completed by unit vectors orthogonal to its
 * periodic rows for the other axes) has its rounding subtracted; among the 3^p shifts in {-1, 0, 1} on the p periodic axes around
 * that result the shortest vector is taken, ties to the first in a fixed order.  Exact for every cell whose true nearest image
 * lies within one cell of the rounded one; where the periodic cell rows are mutually orthogonal rounding alone is exact and the
 * search is skipped.  A pair at exactly half a cell is a kink of S.
 *   uf3_idpp_create    uf3_neb_create's arguments and refusals without a basis and a model (spring: 1 / A^4).  The handle is a
 *                      uf3_neb whose energies are S and whose forces are F; uf3_neb_run (skin is accepted and unused: no lists
 *                      are built and the context's MD skin is not touched; climb = 1 is UF3_EINVAL), uf3_neb_get_state and
 *                      uf3_neb_destroy serve it.  Fixed atoms count in every sum and feel no force.  Coincident atoms make S
 *                      non-finite: that band ends with status 2.
 */
int uf3_idpp_create(uf3_ctx *ctx, const uf3_frames *frames, const double *pos, const int32_t *z, const uint8_t *fixed,
                    int32_t n_bands, const int32_t *band_first_frame /*[n_bands + 1]*/, const double *spring /*[n_bands]*/,
                    uf3_neb **out);

/*
 * Nudged elastic bands whose images differ in cell (solid-state NEB; uf3_amd.forcefield.neb.CellNudgedElasticBand; the <true>
 * instances of uf3_neb.h's kernels): the band of uf3_neb_create in uf3_relax_create's generalised coordinates.  C0 is the cell of a band's image 0;
 * image i has D_i = C0^-1 C_i, q_i = x_i D_i^-1 and the vector u_i = (q_i [n][3], Y_i = kappa D_i [3][3]) of 3 n + 9 numbers; its
 * true force is (F D_i^T, G_i = -D_i^-T W_i / kappa), W the strain derivative of uf3_eval_virial.  t+ = u_{i+1} - u_i and
 * t- = u_i - u_{i-1} as stored over all 3 n + 9 entries (no minimum image); tangent, spring term, climbing image, the one FIRE
 * per band (its velocity has a 3 x 3 cell part per image; maxstep over the band's whole vector) and the statuses are
 * uf3_neb_run's.  Criterion: the largest row norm of g over every atom row and the three cell rows of every interior image.
 * A move: q += dr_q, D += dr_Y / kappa, x = q D, C = C0 D; end images never move and their cells are never written.
 *   uf3_ssneb_create        uf3_neb_create's arguments without a fixed mask, and cell_factor [n_bands] (kappa; NULL: the atom
 *                           count of an image, uf3_relax_run's convention).  UF3_EINVAL: uf3_neb_create's refusals except that
 *                           the cells of a band's images may differ; a frame that is not periodic along all three axes; a
 *                           cell without volume (|det| <= 1e-12 of the product of its row lengths); a cell_factor that is not positive and finite.  The handle is a uf3_neb:
 *                           uf3_neb_run, uf3_neb_get_state and uf3_neb_destroy serve it.  uf3_neb_run freezes a band (status 2)
 *                           also on a non-finite strain derivative and on a singular or non-finite D; its skin is accepted and
 *                           unused: the context's MD skin is 0 during the run (every step rebuilds the lists: the cells change)
 *                           and the caller's again on return; the new cells are waited for after every step.
 *                           uf3_neb_get_state's forces and neb_forces are the atom rows F D^T and those of g.
 *   uf3_neb_get_cell_state  host arrays out, NULL skips: the current cells [n_frames][9], the strain derivatives
 *                           [n_frames][6] (xx, yy, zz, yz, xz, xy), the cell forces G and the cell part of g [n_frames][9]
 *                           (0 on end points; tangents as in the last run) of the current state (evaluated first if it moved
 *                           since).  UF3_EINVAL on a handle that uf3_ssneb_create did not make.
 */
int uf3_ssneb_create(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z, const double *c1,
                     const double *c2, const double *c3, int32_t n_bands, const int32_t *band_first_frame /*[n_bands + 1]*/,
                     const double *spring /*[n_bands]*/, const double *cell_factor /*[n_bands] or NULL*/, uf3_neb **out);
int uf3_neb_get_cell_state(uf3_neb *neb, double *cells, double *virials, double *cell_forces, double *neb_cell_forces);

/*
 * Batched species-swap Monte Carlo on fixed positions (uf3_amd.forcefield.mc.MonteCarlo; kernels in uf3_mc.h): every frame its own
 * Markov chain over WHICH species sits on which site -- canonical swaps or semi-grand-canonical transmutations.  The object owns
 * positions, species (atomic numbers), a neighbour table and the per-frame counters in HBM.  A trial costs the energy terms that
 * contain the one or two atoms it touches, not an evaluation of the frame.
 *   uf3_mc_create         copies frames, positions [N][3], species, an optional per-atom mask swappable [N] (0 / 1; NULL: every
 *                         atom) and the model (c1 / c2 / c3 as for uf3_eval), and builds the neighbour table: per atom the
 *                         entries (real atom, image displacement) within the largest pair r_max and within the 3-body range, from
 *                         the positions alone -- no species in it.  The table is built on the host, O(N^2 images) per frame, once
 *                         per geometry.  UF3_EINVAL: a frame of more than 49 152 atoms (a frame's species sit in LDS, one byte
 *                         each), an atom with more than 512 neighbours in the 3-body range (the affected centres of a trial sit
 *                         in LDS; there is no global-memory fallback), non-finite positions or cells, a mask entry above 1, null
 *                         pointers; UF3_ESPECIES: an element outside the basis.  Atoms outside the cell: the table holds the
 *                         evaluator's candidate set, the images -fac .. fac of the reference's range around the positions AS
 *                         GIVEN.  Every dE and running energy is uf3_eval's on those positions; like uf3_eval's it lacks the terms
 *                         of an atom outside its cell that the range no longer reaches.  Wrap first for the wrapped frame's.
 *   uf3_mc_run            n_trials trials of every frame still running, in launches of at most 1024 trials (no launch is
 *                         open-ended), one workgroup per frame.  Trial t (absolute: the counter lives in the object and goes on
 *                         across runs) of frame f: Philox4x32-10 with counter (f, t lo, t hi, 0) and key (seed lo, seed hi) gives
 *                         r0 .. r3.  mode 0 (swap): i = (r0 N) >> 32, j = (r1 N) >> 32 over the frame's N atoms; null trial
 *                         (counted, never accepted) when i == j, z_i == z_j or either atom is not swappable.  mode 1 (transmute):
 *                         i as above, new species the k-th of the allowed species other than z_i in the basis' species order,
 *                         k = (r1 (S_allowed - 1)) >> 32; allowed: mu [S] finite (-inf excludes a species; mu is required in mode
 *                         1 and refused in mode 0); null when i is not swappable, z_i is not allowed or nothing else is.  dE is
 *                         the sum of every energy term of the evaluator that contains a touched atom, new species minus old, in a
 *                         fixed order (no atomics); dE' = dE - (mu_new - mu_old).  Accepted when dE' <= 0 or
 *                         u < exp(-dE' / k_B T_f), u = ((r2 << 32 | r3) >> 11) + 0.5) 2^-53; temperatures_K [n_frames] >= 0, 0
 *                         accepts dE' <= 0 only.  An accepted trial writes the species and adds dE (not the mu term) to the
 *                         frame's running energy, which starts from the evaluator's.  A non-finite dE freezes the frame (status
 *                         2; the trial is not counted).  record_every > 0: records [n_trials / record_every][n_frames][3 + S]
 *                         after every record_every-th trial of the run: energy, accepted so far, trials so far, atoms of each
 *                         species; rows a frozen frame did not reach repeat its last row of the run (NULL when record_every is
 *                         0).  run(a); run(b) equals run(a + b) bit for bit, and a frame's chain does not depend on the batch
 *                         around it.  The context's MD skin and lists are not touched.
 *   uf3_mc_delta          dE [n] of n caller-given proposals on the current species, nothing applied: frame, atom i within the
 *                         frame, and the second atom j within the frame (mode 0) or the new atomic number (mode 1).  A swap of
 *                         like atoms gives exactly 0.  A triplet's legs follow the evaluator's rule (above uf3_eval) for the
 *                         species it has before and after the move: a change of species can move a neighbour onto the other leg
 *                         and a triplet in or out of its trio's ranges.  UF3_EINVAL: an index outside its frame; UF3_ESPECIES: an unknown element.
 *   uf3_mc_set_positions  new positions [N][3]: the table is rebuilt, the running energies are evaluated again on next need.
 *   uf3_mc_get_state      host arrays out, NULL skips: species [N] (atomic numbers), running energies, accepted and counted
 *                         trials, status (0 running, 2 frozen) [n_frames].
 */
typedef struct uf3_mc uf3_mc;
int uf3_mc_create(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z, const uint8_t *swappable,
                  const double *c1, const double *c2, const double *c3, uf3_mc **out);
void uf3_mc_destroy(uf3_mc *mc);
int uf3_mc_run(uf3_mc *mc, int64_t n_trials, int mode, const double *temperatures_K /*[n_frames]*/, const double *mu /*[S] or NULL*/,
               uint64_t seed, int64_t record_every, double *records);
int uf3_mc_delta(uf3_mc *mc, int64_t n, const int32_t *frame, const int32_t *i, const int32_t *j_or_species, int mode, double *dE);
int uf3_mc_set_positions(uf3_mc *mc, const double *pos);
int uf3_mc_get_state(uf3_mc *mc, int32_t *z, double *energies, int64_t *accepted, int64_t *trials, int32_t *status);

/*
 * The energy uf3_eval computes, resolved per atom, for a batch of frames (uf3_flux.h).
 *   Site energy   U_i: the evaluator's own partition, what uf3_eval_atoms(i, i + 1) returns as the share of atom i -- the
 *                 one-body term of i's species, the directed pair terms phi(r_ij) of i over every image j in the pair range,
 *                 and every triplet V(r_ij, r_ik, r_jk) with i as the centre, over unordered pairs {j, k} of its 3-body
 *                 neighbours.  sum_i U_i = uf3_eval's energy of the WRAPPED frame: the lists take every image in reach around
 *                 the nearest one, so U, W and J do not change when an atom is moved by a lattice vector, whereas uf3_eval
 *                 takes the reference's finite image range around the positions as given and loses terms of an atom outside its
 *                 cell.  The two agree when every atom lies inside its cell (wrap first); uf3_md_run_flux samples on the
 *                 object's unwrapped positions and so keeps describing the wrapped frame after uf3_md_run's forces no longer do.
 *   Images        move with their parent atom and carry its velocity.
 *   Site virial   W_i[a][b] = sum_terms sum_s d_s[a] (dU_i / dr_s)[b], s the slots of a term of U_i (neighbour images), d_s the
 *                 vector from the centre to the image; [N][9] row-major.  sum_i W_i, symmetrised, in Voigt order = uf3_eval_virial's
 *                 dE / d(strain).
 *   Heat current  e_i = 1/2 m_i v_i^2 + U_i;  J = J_conv + J_pot, extensive, eV Angstrom / fs (velocities Angstrom / fs, masses amu):
 *                 J_conv = sum_i e_i v_i,  J_pot = - sum_i sum_terms sum_s d_s (dU_i / dr_s . v_s)  (= d/dt sum_i r_i e_i with
 *                 Newton's equations; exact in a cluster, term by term with image vectors in a periodic cell).  Pair:
 *                 dU_i / dr_j = phi'(r_ij) u_ij; triplet with legs ij, ik, jk and leg gradient g: d / dr_j = g_ij u_ij - g_jk u_jk,
 *                 d / dr_k = g_ik u_ik + g_jk u_jk (u_jk from j to k).
 *   Legs          the evaluator's rule (above uf3_eval): of two neighbours of one species the lower reference supercell index
 *                 as seen from the centre takes leg l.  The order in which a centre's terms are ADDED is another matter (by image
 *                 vector: see below) and does not decide any term.
 *   uf3_site_terms   site_energies [N] and / or site_virials [N][9] (NULL skips one).
 *   uf3_heat_flux    flux [n_frames][6] = J_conv (3), J_pot (3); site_energies [N] or NULL.
 * The neighbour lists are the call's own (every image in reach of every atom, O(N^2 images) per frame; skin 0): the context's MD
 * lists and its evaluator state are left as they were.  No atomics: one wave per centre, a fixed reduction tree -- results repeat
 * bit for bit and a frame's do not depend on the batch around it.  A 2-body-only basis is allowed.  Errors: bad frames, null
 * pointers, masses not positive and finite or velocities not finite (host entries, nothing launched), atoms more than 500 cells
 * apart along a periodic axis, a cell far thinner than the cut-off (UF3_EINVAL); an element outside the basis (UF3_ESPECIES).
 * _dev: device pos, vel, z, masses and outputs (coefficients on the host, as uf3_eval_dev); the host entries stage both ways.
 */
int uf3_site_terms(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z, const double *c1,
                   const double *c2, const double *c3, double *site_energies, double *site_virials);
int uf3_site_terms_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const int32_t *d_z, const double *c1,
                       const double *c2, const double *c3, double *d_site_energies, double *d_site_virials);
int uf3_heat_flux(uf3_basis *basis, const uf3_frames *frames, const double *pos, const double *vel, const int32_t *z,
                  const double *masses, const double *c1, const double *c2, const double *c3, double *flux, double *site_energies);
int uf3_heat_flux_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const double *d_vel, const int32_t *d_z,
                      const double *d_masses, const double *c1, const double *c2, const double *c3, double *d_flux,
                      double *d_site_energies);

/*
 * Site rows and extrapolation grades (uf3_site_rows.h): how far an ATOM lies from the fit.
 *   Site row   rows[i][0 .. F) . c == U_i, uf3_site_terms' site energy, for EVERY flat coefficient vector c (the featurizer's
 *              column order, length n_feat, frozen columns included: what the calculator expands into c1 / c2 / c3).  The same
 *              partition, the same leg rule (on a symmetry-1 trio the supercell-index tie-break decides which column a product
 *              lands in), the same nearest-image lists; the fold from (trio, bin triple) to column is the table the
 *              featurizer's energy row uses.  The sum of a frame's rows is uf3_featurize's energy row of the wrapped frame.
 *   Grade      grade[i] = |W b_i|^2 = b_i^T (G + R^T R)^-1 b_i with uf3_leverage's W (lower triangular with exact zeros above
 *              the diagonal, frozen columns as zero rows and columns): the predictive variance of the site energy up to the
 *              noise scale.
 *   uf3_site_rows    rows [N][ld], ld >= n_feat; columns n_feat .. ld are not written.  Takes no coefficients.  The grades
 *                    describe the WRAPPED frame, as uf3_site_terms does: an atom outside its cell counts as its image inside,
 *                    also in the symmetry-1 tie-break (the wrapped image's place in the reference supercell decides the column).
 *   uf3_site_grade   grade [N]; frame_max / frame_argmax [n_frames] (either may be NULL): the largest grade of each frame and
 *                    the frame-local index of its atom, the lowest index on ties, from a fixed reduction tree.  Here, and
 *                    here only, a frame may be empty: it gives 0 and -1.  The grades describe the WRAPPED frame, as
 *                    uf3_site_terms does.  A tile of 16 rows is built in LDS and multiplied by W on the fp64 matrix cores;
 *                    where 16 rows of this basis and the lists' index arrays do not fit 80 KB of LDS (n_feat above about 600)
 *                    the entry goes through chunks of site rows in a context-owned scratch of at most 64 MB and uf3_leverage's
 *                    kernel instead: the same numbers within uf3_leverage's summation-order bound.
 * One wave per centre, the row accumulated in LDS, plain stores, no global atomics: results repeat bit for bit and a frame's do
 * not depend on the batch around it.  A 2-body-only basis is allowed.  Errors as uf3_site_terms: bad frames, null pointers, atoms
 * more than 500 cells apart along a periodic axis, a cell far thinner than the cut-off, a list or a row too long for LDS
 * (UF3_EINVAL); an element outside the basis (UF3_ESPECIES).  _dev: device pos, z, w and outputs.
 */
int uf3_site_rows(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z, double *rows, int64_t ld);
int uf3_site_rows_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const int32_t *d_z, double *d_rows, int64_t ld);
int uf3_site_grade(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z, const double *w, double *grade,
                   double *frame_max, int32_t *frame_argmax);
int uf3_site_grade_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const int32_t *d_z, const double *d_w,
                       double *d_grade, double *d_frame_max, int32_t *d_frame_argmax);

/*
 * Analytic second derivatives of the energy uf3_eval computes on the WRAPPED frame, for ONE frame (uf3_hessian.h; the Gamma-point
 * force constants of the frame, periodic images folded onto their parent atom).  The lists take every image in reach around the
 * nearest one: H, mixed and born do not change when an atom is moved by a lattice vector, whereas uf3_eval takes the reference's
 * finite image range around the positions as given -- with an atom outside its cell they are the derivatives of the wrapped
 * frame's energy, not of what uf3_eval returns for the positions passed in.  Rows m in [row_begin, row_end) (R rows), all N atoms as columns.
 *   hess  [3R][3N]  d2E / dx_{m,a} dx_{p,b}
 *   mixed [3R][6]   d2E / dx_{m,a} dt_v (NULL: not formed): t_v the strain of uf3_eval_virial (Voigt xx, yy, zz, yz, xz, xy;
 *                   eps_ab = eps_ba = t / 2 off the diagonal; cell and positions map through I + eps); = -dF_{m,a} / dt_v
 *   born  [6][6]    d2E / dt_u dt_v at fixed fractional coordinates (clamped ions; NULL: not formed; whole frame only)
 * Every triplet's legs follow the evaluator's rule (above uf3_eval), also where the row atom is a neighbour of the triplet: H,
 * mixed and born are the second derivatives of uf3_eval's energy (of the wrapped frame) on every basis, symmetry-1 trios included.
 * The neighbour lists are the call's own (skin 0): the context's MD lists and its evaluator state are left as they were.
 * Every row is written by one thread in a fixed order: the results are bitwise repeatable, and the rows of a slab are the
 * rows of the whole call.  Errors: more than one frame, an empty or out-of-range row span, born with a partial span
 * (UF3_EINVAL); atoms more than 500 cells apart along a periodic axis (UF3_EINVAL: wrap them first); an element outside the
 * basis (UF3_ESPECIES).  uf3_hessian: host buffers; _dev: device pos, z and outputs
 * (coefficients on the host, as uf3_eval_dev).
 */
int uf3_hessian(uf3_basis *basis, const uf3_frames *frames, const double *pos, const int32_t *z, const double *c1,
                const double *c2, const double *c3, int64_t row_begin, int64_t row_end, double *hess, double *mixed, double *born);
int uf3_hessian_dev(uf3_basis *basis, const uf3_frames *frames, const double *d_pos, const int32_t *d_z, const double *c1,
                    const double *c2, const double *c3, int64_t row_begin, int64_t row_end, double *d_hess, double *d_mixed,
                    double *d_born);

/*
 * Phonons on a q-mesh (uf3_phonon.h): eigenvalues of the dynamical matrix at many wave vectors, the density of states and the
 * harmonic thermodynamics.  They take a context and no basis: nothing here depends on the potential.  Units: eV, Angstrom,
 * amu, THz, K.  Every entry exists twice -- host buffers, or (_dev) device buffers for the large arrays, enqueued on the
 * context's stream without waiting; the small descriptive arrays (terms, term_w, edges, samples, temps) are host arrays in
 * both, checked before anything is launched.
 *
 * uf3_phonon_mesh: lam [nq][3N], the eigenvalues of D(q) in ascending order (eV / (amu A^2)), and status [nq], the number of
 * Jacobi sweeps taken or -1 where the cap of 30 sweeps was reached (lam of that q is then not converged).
 *   fc [3N][3 n_sc_atoms]  force-constant rows of the cell's N atoms against the atoms of a supercell, atom p of the supercell
 *                          an image of atom p mod N: what uf3_hessian writes for rows [0, N) of an n^3 supercell
 *   inv_sqrt_mass [N]      1 / sqrt(amu)
 *   terms [n_terms][5]     (i, p, n0, n1, n2): block row i < N, supercell atom p, integer lattice triple n of the chosen image;
 *   term_w [n_terms]       its weight (1 / multiplicity of equivalent images)
 *   q [nq][3]              reduced wave vectors
 * D_ij(q) = sum over the terms (i, p) with p mod N = j of w exp(2 pi i q.n) fc[i, p] / sqrt(m_i m_j), then (D + D^H) / 2; q.n is
 * reduced mod 1 before the sine and cosine.  Every sum has one order (the caller's term order within a block) and nothing is
 * accumulated atomically: lam is bitwise repeatable, and a mesh cut into several calls gives the bits of one call.  N <= 2 runs
 * one lane per q-point with the matrix in registers, larger cells one wave per q-point with D(q) in LDS (16 (3N)^2 bytes): the
 * limit is N <= 32 (3N = 96, 147 456 bytes of the 160 KiB of a CU).  Errors (UF3_EINVAL, nothing launched): N < 1 or above the
 * limit, nq < 1, n_sc_atoms not a multiple of N, a term whose atom indices lie outside [0, N) x [0, n_sc_atoms), null pointers.
 *
 * uf3_phonon_dos: from lam [nq][n_modes] and integer q-weights wq [nq] (NULL: all 1), with f = sign(lam) sqrt|lam| * 15.633302
 * THz (imaginary modes negative).  Either output may be NULL, not both:
 *   counts [n_bins]   int64 weighted histogram over edges [n_bins + 1] (THz, strictly increasing), numpy's rule: bins half open,
 *                     the last one closed, values outside dropped
 *   dos [n_samples]   g(f_s) = sum_q w_q sum_modes exp(-(f_s - f)^2 / 2 sigma^2) / (sigma sqrt(2 pi)) / sum_q w_q, in fixed-order
 *                     partial sums (no floating-point atomics: bitwise repeatable)
 * Errors (UF3_EINVAL): nq < 1, both outputs NULL, edges not strictly increasing, sigma <= 0, missing edges / samples.
 *
 * uf3_phonon_thermo: per primitive cell, out [n_temps][4] = F, U (eV), S, C_v (eV / K) at temps [n_temps] (K, >= 0), *zpe the
 * zero-point energy (eV) and *excluded the summed weight of the modes with f <= cutoff_thz, which are left out of every sum
 * (imaginary modes among them).  Per mode, x = h f / k_B T: F = hf / 2 + k_B T log(1 - e^-x), U = hf (1 / 2 + 1 / (e^x - 1)),
 * S = k_B (x / (e^x - 1) - log(1 - e^-x)), C_v = k_B x^2 e^x / (e^x - 1)^2; T = 0: F = U = zpe, S = C_v = 0; each sum divided by
 * sum_q w_q.  h = 4.135667696e-3 eV / THz, k_B = 8.617333262e-5 eV / K.  Fixed-order sums.  Errors (UF3_EINVAL): nq < 1, a
 * negative or non-finite temperature or cut-off, null pointers.
 *
 * Eigenvectors on the mesh.
 * uf3_phonon_mesh_vec: uf3_phonon_mesh's arguments, lam and status (bit for bit what uf3_phonon_mesh writes: the same rotations in
 * the same order), plus the cell [3][3] (rows: lattice vectors, A; a host array in both entries), cutoff_thz and
 *   evec [nq][3N][3N][2]   V(q): row (3 i + alpha), mode, (re, im); column s is an orthonormal eigenvector of lam[s].  V starts at
 *                          I and takes every Jacobi rotation, diag(1, conj u) included; skipped pivots rotate nothing
 *   gvel [nq][3N][3]       group velocities d f / d k in THz A (1 THz A = 100 m / s), k the Cartesian wave vector without 2 pi:
 *                          g_a = Re(v_s^H (dD / dq_a) v_s) with dD / dq_a = sum w (2 pi i n_a) exp(2 pi i q.n) fc / sqrt(m_i m_j)
 *                          Hermitised like D (same terms, owners and order), d lam / d k_c = sum_a g_a cell[a][c],
 *                          v_c = 15.633302 (d lam / d k_c) / (2 sqrt|lam_s|); modes with |f_s| <= cutoff_thz get 0
 * Either output may be NULL, not both; the cell and the cut-off are looked at only with gvel.  Inside a degenerate cluster of
 * modes the diagonal g depends on the basis the Jacobi sweeps ended in: only the cluster's SUM of velocities is defined, and
 * nothing resolves it.  Both outputs are bitwise repeatable and do not depend on how a mesh is cut into calls.  V lives beside D
 * in LDS (32 (3N)^2 bytes): the limit with vectors is N <= 21 (3N = 63, 127 KB); larger cells are refused, there is no
 * global-memory route.  Errors (UF3_EINVAL): uf3_phonon_mesh's, N above 21, both outputs NULL, and with gvel a cell that is
 * singular or not finite or a cut-off that is negative or not finite.
 *
 * uf3_phonon_pdos: out [n_modes][n_samples], g_c(f) = sum_q w_q sum_s |V_cs|^2 exp(-(f - f_s)^2 / 2 sigma^2) / (sigma sqrt(2 pi)) /
 * sum_q w_q for every channel c = 3 i + alpha, from lam [nq][n_modes] and evec as uf3_phonon_mesh_vec writes it.  Fixed-order
 * partial sums, bitwise repeatable; V(-q) = conj V(q), so a mesh reduced by time reversal takes its integer weights unchanged.
 * Errors (UF3_EINVAL): n_modes not a multiple of 3 in [3, 63], nq < 1, sigma <= 0, missing samples, null pointers.
 *
 * uf3_phonon_tdisp: out [n_temps][N][6], the mean-square displacement tensors in A^2 (xx, yy, zz, yz, xz, xy):
 * U_i^{ab}(T) = (1 / sum w_q) sum_q w_q sum_s E_s(T) / (m_i lam_s) Re(V_{3i+a,s} conj V_{3i+b,s}), E_s = h f_s (1 / 2 + 1 / (e^x - 1)),
 * x = h f_s / k_B T (uf3_phonon_thermo's constants and forms; T = 0: the zero-point term).  inv_sqrt_mass [N] is a host array in
 * both entries.  Modes with f <= cutoff_thz are left out and *excluded is their summed weight.  Fixed-order sums.  Errors
 * (UF3_EINVAL): N outside [1, 21], nq < 1, a negative or non-finite temperature or cut-off, masses not positive, null pointers.
 */
int uf3_phonon_mesh(uf3_ctx *ctx, int32_t n_atoms, int64_t n_sc_atoms, const double *fc, const double *inv_sqrt_mass,
                    int64_t n_terms, const int32_t *terms, const double *term_w, int64_t nq, const double *q, double *lam,
                    int32_t *status);
int uf3_phonon_mesh_dev(uf3_ctx *ctx, int32_t n_atoms, int64_t n_sc_atoms, const double *d_fc, const double *d_inv_sqrt_mass,
                        int64_t n_terms, const int32_t *terms, const double *term_w, int64_t nq, const double *d_q, double *d_lam,
                        int32_t *d_status);
int uf3_phonon_dos(uf3_ctx *ctx, int32_t n_modes, int64_t nq, const double *lam, const int64_t *wq, int32_t n_bins,
                   const double *edges, int64_t *counts, int32_t n_samples, const double *samples, double sigma, double *dos);
int uf3_phonon_dos_dev(uf3_ctx *ctx, int32_t n_modes, int64_t nq, const double *d_lam, const int64_t *d_wq, int32_t n_bins,
                       const double *edges, int64_t *d_counts, int32_t n_samples, const double *samples, double sigma, double *d_dos);
int uf3_phonon_thermo(uf3_ctx *ctx, int32_t n_modes, int64_t nq, const double *lam, const int64_t *wq, int32_t n_temps,
                      const double *temps, double cutoff_thz, double *out, double *zpe, int64_t *excluded);
int uf3_phonon_thermo_dev(uf3_ctx *ctx, int32_t n_modes, int64_t nq, const double *d_lam, const int64_t *d_wq, int32_t n_temps,
                          const double *temps, double cutoff_thz, double *d_out, double *d_zpe, int64_t *d_excluded);
int uf3_phonon_mesh_vec(uf3_ctx *ctx, int32_t n_atoms, int64_t n_sc_atoms, const double *fc, const double *inv_sqrt_mass,
                        int64_t n_terms, const int32_t *terms, const double *term_w, int64_t nq, const double *q, double *lam,
                        int32_t *status, const double *cell, double cutoff_thz, double *evec, double *gvel);
int uf3_phonon_mesh_vec_dev(uf3_ctx *ctx, int32_t n_atoms, int64_t n_sc_atoms, const double *d_fc, const double *d_inv_sqrt_mass,
                            int64_t n_terms, const int32_t *terms, const double *term_w, int64_t nq, const double *d_q,
                            double *d_lam, int32_t *d_status, const double *cell, double cutoff_thz, double *d_evec, double *d_gvel);
int uf3_phonon_pdos(uf3_ctx *ctx, int32_t n_modes, int64_t nq, const double *lam, const double *evec, const int64_t *wq,
                    int32_t n_samples, const double *samples, double sigma, double *out);
int uf3_phonon_pdos_dev(uf3_ctx *ctx, int32_t n_modes, int64_t nq, const double *d_lam, const double *d_evec, const int64_t *d_wq,
                        int32_t n_samples, const double *samples, double sigma, double *d_out);
int uf3_phonon_tdisp(uf3_ctx *ctx, int32_t n_atoms, int64_t nq, const double *lam, const double *evec, const int64_t *wq,
                     const double *inv_sqrt_mass, int32_t n_temps, const double *temps, double cutoff_thz, double *out,
                     int64_t *excluded);
int uf3_phonon_tdisp_dev(uf3_ctx *ctx, int32_t n_atoms, int64_t nq, const double *d_lam, const double *d_evec, const int64_t *d_wq,
                         const double *inv_sqrt_mass, int32_t n_temps, const double *temps, double cutoff_thz, double *d_out,
                         int64_t *d_excluded);

/*
 * Dense helpers behind the module-level functions of uf3.representation.distances / angles, for frames small enough
 * for an n x m matrix (the reference's own limit).  Host buffers.
 *   uf3_distance_matrix     out [na][nb] = |a_i - b_j| in scipy cdist's order of operations (get_distance_matrix,
 *                           distances.py:212-235; identify_ij's matrix, angles.py:289-346)
 *   uf3_direction_cosines   out [n_atoms][3][n_d] = ((m == j) - (m == i)) (R_j - R_i) / r_ij (distances.py:331-364)
 */
int uf3_distance_matrix(uf3_ctx *ctx, const double *a, int64_t na, const double *b, int64_t nb, double *out);
int uf3_direction_cosines(uf3_ctx *ctx, const double *sup_pos, int64_t n_sup, const int64_t *i_where,
                          const int64_t *j_where, const double *rij, int64_t n_d, int64_t n_atoms, double *out);

#ifdef __cplusplus
}
#endif
#endif /* UF3_HIP_H */
