/*
 * gf2bv_hip.h -- C ABI of libgf2bv_hip.so, the MI355X (gfx950) GF(2) solver that sits where
 * gf2bv's `_internal.c` calls M4RI.
 *
 * Plain C: pointers, sizes, opaque handles.  No torch / HIP types in any signature (a HIP
 * stream or device pointer crosses as `void*`).  Reference interface each entry point
 * replaces is cited as file:line relative to maple3142/gf2bv.
 *
 * Matrix layout everywhere ("augmented words"): row-major uint64, `stride` words per row,
 * column c of A = bit (c % 64) of word (c / 64), the right-hand side b is column `cols`
 * (so a row needs ceil((cols+1)/64) words).  This is M4RI's mzd_t bit order
 * (_internal.c:398-426 fills it with mzd_write_bit) and int.to_bytes(...,'little').
 *
 * Solution vectors: ceil(cols/64) words, bit j = variable j (_internal.c:32-39).
 *
 * Threading: every call owns its device buffers and stream; no global mutable state except
 * the last-error string, which is thread-local, and a thread-safe pool that recycles idle
 * device buffers, streams and events between calls (small buffers up to 512 MiB in total,
 * plus up to six large working buffers per device, at most a sixth of the device's memory and
 * never more than 48 GiB; GF2BV_KEEP_BIG=0 in the environment keeps none (every GF2BV_* variable the
 * library reads is listed in DESIGN.md, "Environment switches"); gf2bv_pool_trim()
 * returns all of them to the device, and an allocation the device refuses -- the library's own or
 * gf2bv_device_alloc -- frees them and is repeated once).  Matches the reference releasing the GIL around the
 * whole factor/solve/kernel section (_internal.c:429-492).
 * Handles: a gf2bv_factor may be used from several threads; its calls -- solves, appends, copies and the getters (rank, rows,
 * pivots, device_bytes) -- take a mutex inside the handle and run one at a time, so a getter beside an append sees the state
 * before or after it, never a mixture.  gf2bv_factor_free waits for a call that is running, but racing it against other calls on
 * the same handle is a caller error (a call that arrives after it uses freed memory).  gf2bv_space and gf2bv_slab handles have no
 * lock and own one set of device and pinned buffers each: they belong to one thread at a time (different handles on different
 * threads are fine).  gf2bv_result handles are immutable once returned.  No GF2BV_* environment variable may change while another
 * thread is inside the library.
 */
#ifndef GF2BV_HIP_H
#define GF2BV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF2BV_OK            0
#define GF2BV_ERR_ARG       1   /* bad argument (the binding maps these to ValueError/TypeError) */
#define GF2BV_ERR_NODEVICE  2   /* no usable gfx950 device: the product path fails loudly, no CPU fallback */
#define GF2BV_ERR_HIP       3   /* a HIP runtime call failed, see gf2bv_last_error() */
#define GF2BV_ERR_NOMEM     4

#define GF2BV_MODE_SINGLE        0   /* _internal.h:25 SOLVE_MODE_SINGLE       */
#define GF2BV_MODE_AFFINE_SPACE  1   /* _internal.h:26 SOLVE_MODE_AFFINE_SPACE */

#define GF2BV_STATUS_SOLVED        0
#define GF2BV_STATUS_INCONSISTENT  1   /* _internal.c:440-446 -> Python None */

typedef struct gf2bv_result gf2bv_result;     /* owns origin / basis / pivots of one solve */

typedef struct gf2bv_stats {
	int64_t rows, cols, stride_words;
	int64_t rank, dimension;
	int32_t status;
	int32_t n_panels;          /* 64-column panels processed                                  */
	int32_t n_sweeps;          /* bulk-update passes over the trailing matrix that did work    */
	int32_t panels_per_sweep;  /* G: 64-column panels fused into one pass                      */
	int32_t tables_per_sweep;  /* G*T: grease tables applied per row per pass                  */
	int32_t table_bits;        /* k: index bits of the widest table                            */
	int32_t tile_words;        /* 64-bit words of one row segment handled by a lane group      */
	int32_t gang_systems;      /* systems that shared this solve's kernel launches (1: a solve of its own)    */
	double  sweep_words;       /* sum over sweeps of rows_swept x active_words  (unit of work) */
	double  row_xors;          /* sum over sweeps of rows_swept x T                            */
	float   ms_pack;           /* digits/words -> device matrix (H2D + pack kernel)            */
	float   ms_eliminate;      /* forward elimination, all panels (HIP events)                 */
	float   ms_sweep;          /* time inside the bulk-update kernels (HIP events): the sum over passes; launches that run side by side
	                            * (the two halves of an outer pass of the two-level elimination, the inner updates beside them) count once */
	float   ms_backsub;        /* consistency check + back-substitution + kernel basis         */
	float   ms_export;         /* D2H of origin / basis                                        */
	float   ms_total;          /* host wall clock of the whole call                            */
	int32_t search_handovers;  /* panels whose first search unit stopped waiting for the rest of its launch and
	                              left publishing to the last arriver (co-residency is not assumed)           */
	int32_t fast_blocks;       /* blocks of 4 panels factorised by the one-launch dense block search (k_block_fast)     */
	/* round 3 (two-level elimination): sweep_words above counts one word per word and BLOCK applied (the unit of the
	 * roofline, whatever kernel applied it); an outer pass applies K blocks per trip through HBM, so what the bulk kernels
	 * actually read + wrote is less: */
	double  hbm_words;         /* 64-bit words the bulk-update launches moved (each read once and written once)       */
	int32_t bulk_launches;     /* k_update16 + k_update16k launches that had pivots to apply                          */
	int32_t outer_blocks;      /* blocks applied through outer passes (0: one-level schedule)                         */
	int32_t handover_retries;  /* 1: a stream hand-over gate expired on the device and this is the result of the SECOND attempt,
	                              made with events (the device stays on events for this process); 0 normally        */
	int32_t small_path;        /* 1: solved by the one-launch kernel for systems that fit the LDS of one workgroup (k_small_solve; the
	                              phase times and sweep counters above are then 0 except ms_total); GF2BV_SMALL=0 disables that path */
	/* the one-launch block search of sparse systems (k_block_sparse; single systems whose first block the dense search refuses): which
	 * of its branches ran.  All 0 when it never ran (GF2BV_SPARSE_FAST=0, gangs, two-level plans, dense systems). */
	int32_t sparse_blocks[3];        /* blocks it factorised, by the size of its candidate pool: 1024 / 4096 / 6144 rows (fast_blocks counts
	                                    these and the dense search's)                                                                   */
	int32_t sparse_panels_first64;   /* panels of those blocks whose 64 pivot rows were the first 64 pool rows with a bit in the panel     */
	int32_t sparse_panels_absorb;    /* ... that needed more of the first 512 such rows (at least one find_absorb chunk)                   */
	int32_t sparse_panels_rounds;    /* ... that were selected by the rounds over the whole pool                                           */
	int32_t sparse_giveups;          /* blocks the host handed back to the general panel steps after the search gave up on them (behind the
	                                    probed first block of a pool size or after everything was submitted, alike); the third switches
	                                    the search off for the rest of the solve                                                          */
	int32_t sparse_giveup_why[5];    /* the search's give-ups by reason 1..5: [0] not a full block, [1] fewer than 256 rows with a non-zero
	                                    window in reach, [2] the pool lacks 64 independent rows for a panel, [3] the chosen rows were not
	                                    independent after all, [4] fewer than 64 pool rows have a bit in a panel                           */
	int32_t sparse_nz_max;           /* the most alive rows with a non-zero window one of its launches counted (above the pool size: that
	                                    pool was truncated)                                                                             */
	/* the general panel search (search_panel of k_panel_step: every panel no one-launch search took): which way each panel was
	 * published.  Functions of the system alone -- who did the writing is timing and is counted by search_handovers only.  All 0
	 * where that search never ran (the small path; blocks taken by k_block_fast / k_block_sparse: 4 x fast_blocks panels).
	 * general_unit0 + general_adopted + general_merged = the panels it published. */
	int32_t general_unit0;           /* panels whose basis is the first search unit's (complete on its own; the alive bound comes from it)  */
	int32_t general_adopted;         /* ... is another unit's complete record or, on a two-level arrival, a group's complete record        */
	int32_t general_merged;          /* ... was rebuilt from the units' (or the groups') source-row lists: no record was complete; every
	                                    rank-deficient panel                                                                              */
	int32_t general_wide;            /* panels searched by every unit (the panel before was hard: merged, or its record took > 8 chunks)   */
	int32_t general_two_level;       /* wide panels of more than 16 units: groups of 16 units form a record each, the publisher chooses
	                                    among those                                                                                       */
	int32_t general_group_adopted;   /* group records that are a complete member's                                                        */
	int32_t general_group_merged;    /* group records merged from the members' lists                                                      */
	int32_t general_gj_kept;         /* unit0 / adopted panels whose record's first chunk went through the column-wise elimination
	                                    (gj_columns: >= 48 of 64 candidates with > 12 bits) and kept its result (>= 56 pivots)             */
	int32_t general_gj_redone;       /* ... and redid the chunk row-wise                                                                  */
	int32_t general_chunks;          /* 64-row chunks scanned by the units behind the unit0 / adopted panels' records (a group's adopted
	                                    member included; merges add nothing)                                                              */
	/* the one-launch small solve (k_small_solve): which branches its passes took.  Both 0 where small_path is 0.  A pass takes up to 64
	 * candidate rows of a panel, whichever wavefronts' atomicAdd arrive first, so for random systems both depend on timing; they are
	 * functions of the data only for systems built so that every arrival order gives the same passes (tests/small_cases.py). */
	int32_t small_passes;            /* passes that ran, over all panels (a pass that finds no candidate ends its panel and is not counted)   */
	int32_t small_pass_kinds;        /* bit mask over those passes: 1 a panel's first pass found at most 4 new pivots (bit loops on the rows),
	                                    2 a panel's first pass found more (nibble tables), 4 / 8 the same for a later pass of a panel,
	                                    16 a pass saw more than 64 candidates (the rest were left out), 32 a pass saw fewer than 64            */
} gf2bv_stats;

/* ---- library / device ------------------------------------------------------------------ */
int         gf2bv_version(void);
const char *gf2bv_build_id(void);              /* content hash of the HIP sources this binary was compiled from (build.py) */
int         gf2bv_device_count(void);          /* 0 when no HIP device is visible */
const char *gf2bv_last_error(void);            /* thread-local, never NULL */

/* ---- solve: replaces the body of m4ri_solve, gf2bv/_internal.c:398-489 -------------------- */

/* Equations as raw CPython `int` digit arrays (the binding memcpy's ob_digit, the device
 * pack kernel does what _internal.c:403-426 does bit by bit under the GIL):
 * row r occupies digits[digit_off[r] .. digit_off[r+1]), little-endian digits of
 * `bits_per_digit` payload bits (30 on 64-bit CPython) in uint32; sign already dropped;
 * bit 0 = affine term, bit k = coefficient of variable k-1; bits above `cols` ignored.
 * digit_off[0] must be 0 (offsets are relative to `digits`); GF2BV_ERR_ARG otherwise.
 * Requires rows >= cols > 0 (_internal.c:372-395). */
int gf2bv_solve_digits(const uint32_t *digits, const int64_t *digit_off, int bits_per_digit,
                       int64_t rows, int64_t cols, int mode, int device, gf2bv_result **out);

/* Same system, already packed as augmented words in HOST memory (not modified). */
int gf2bv_solve_words(const uint64_t *aug, int64_t rows, int64_t cols, int64_t stride_words,
                      int mode, int device, gf2bv_result **out);

/* Same, matrix resident in DEVICE memory (row-major augmented words, left untouched: the solver
 * first copies it into its own tile-major working layout, one extra pass over the matrix).
 * d_aug must be 16-byte aligned and stride_words even.  `stream` is a HIP stream handle or NULL: the solve is
 * enqueued on it (so it is ordered after whatever produced the matrix there) and the call returns when
 * the result is on the host.
 * `time_kernels` != 0 brackets every bulk-update launch with HIP events (fills ms_sweep). */
int gf2bv_solve_device(void *d_aug, int64_t rows, int64_t cols, int64_t stride_words,
                       int mode, int device, void *stream, int time_kernels, gf2bv_result **out);

/* ---- many right-hand sides of ONE matrix, one elimination (gf2bv/_internal.c:398-455) ------------------------------------
 * The reference builds A (rows x cols) and B (rows x 1) as separate mzd_t, factors A alone (_mzd_pluq, :429-433) and only then
 * solves against B (:438-455): pivots, the origin rule (free variables 0) and the kernel basis depend on A only.  These entries
 * eliminate A once with every right-hand side carried along as an extra column (right-hand side j = column cols + j of the
 * working matrix, ceil((cols + nrhs) / 64) words per row), then decide each system's consistency and back-substitute all of them
 * in one pass over U (mode 1: the kernel basis is computed once, when at least one system is consistent).
 * rhs: nrhs rows of rhs_words >= ceil(rows/64) uint64; bit r of row j = affine term of equation r in system j (bits >= rows
 * ignored).  The affine term of the matrix input (digit bit 0 / column `cols`) is ignored.  out[0..nrhs) receives one handle
 * per system, each identical to what gf2bv_solve_digits/_words/_device returns for that system alone (status, rank, pivots,
 * dimension, origin, basis); every handle carries the shared solve's stats.
 * Argument errors (null pointers, nrhs < 1, rhs_words < ceil(rows/64), the shape rules of the single entries) return
 * GF2BV_ERR_ARG before any device is touched; a widened matrix that does not fit on the device returns GF2BV_ERR_NOMEM.
 * Scope: one system on one device -- no gangs, no column slabs; every size takes the blocked path (no one-launch small path). */
int gf2bv_solve_rhs_digits(const uint32_t *digits, const int64_t *digit_off, int bits_per_digit, int64_t rows, int64_t cols,
                           const uint64_t *rhs, int64_t nrhs, int64_t rhs_words, int mode, int device, gf2bv_result **out);
int gf2bv_solve_rhs_words(const uint64_t *aug, int64_t rows, int64_t cols, int64_t stride_words,
                          const uint64_t *rhs, int64_t nrhs, int64_t rhs_words, int mode, int device, gf2bv_result **out);
/* d_aug as in gf2bv_solve_device (16-byte aligned, even stride_words); d_rhs: device memory, 8-byte aligned, read after
 * everything enqueued on `stream` before the call. */
int gf2bv_solve_rhs_device(void *d_aug, int64_t rows, int64_t cols, int64_t stride_words, const void *d_rhs, int64_t nrhs,
                           int64_t rhs_words, int mode, int device, void *stream, int time_kernels, gf2bv_result **out);

/* ---- a kept factorization: factor A once, solve right-hand sides against it later (gf2bv/_internal.c:431-447) -----------
 * The reference's two steps -- _mzd_pluq on A, _mzd_pluq_solve_left on B -- with the factorization kept in a handle.  The matrix
 * arguments follow gf2bv_solve_rhs_*; column `cols` (the affine term) is ignored.  Each gf2bv_factor_solve* takes right-hand sides
 * in the format of gf2bv_solve_rhs_*, and result j is bit-identical to what gf2bv_solve_rhs_words returns for the same matrix and
 * right-hand side j (status, rank, pivots, dimension, origin, basis), for every call on the handle, in any order.  More than 64
 * right-hand sides run in passes of 64.  Calls on one handle are serialised by a mutex inside it.
 * Device memory: the handle keeps the eliminated matrix [U | 64 slot columns | T] until gf2bv_factor_free, where T (rows x rows
 * bits) is what the row operations made of the identity: about twice the matrix for square systems (16 GiB at 262144^2).
 * gf2bv_pool_trim does not take it.  A factorization that does not fit returns GF2BV_ERR_NOMEM.
 * A result's stats: ms_pack = upload of the right-hand sides, ms_eliminate = forming T b (the replay of the elimination),
 * ms_backsub / ms_export / ms_total as usual; the elimination counters (n_panels, fast_blocks, outer_blocks, ...) are the
 * factorization's (they count the T columns as well).
 * Argument errors (null pointers, nrhs < 1, rhs_words < ceil(rows/64), the shape rules of the single entries) return
 * GF2BV_ERR_ARG before any device is touched.  Scope: one system on one device; a handle stays on the device it was made on. */
typedef struct gf2bv_factor gf2bv_factor;
int gf2bv_factor_digits(const uint32_t *digits, const int64_t *digit_off, int bits_per_digit, int64_t rows, int64_t cols,
                        int mode, int device, gf2bv_factor **out);
int gf2bv_factor_words(const uint64_t *aug, int64_t rows, int64_t cols, int64_t stride_words, int mode, int device,
                       gf2bv_factor **out);
/* d_aug as in gf2bv_solve_device; read after everything enqueued on `stream` (NULL = the null stream) before the call */
int gf2bv_factor_device(void *d_aug, int64_t rows, int64_t cols, int64_t stride_words, int mode, int device, void *stream,
                        gf2bv_factor **out);
/* out[0..nrhs) receives one result handle per right-hand side (free each with gf2bv_result_free) */
int gf2bv_factor_solve(gf2bv_factor *h, const uint64_t *rhs, int64_t nrhs, int64_t rhs_words, gf2bv_result **out);
/* d_rhs: device memory, 8-byte aligned, read after everything enqueued on `stream` (NULL = the null stream) before the call;
 * time_kernels is accepted for symmetry with gf2bv_solve_rhs_device (the phase times are always measured) */
int gf2bv_factor_solve_device(gf2bv_factor *h, const void *d_rhs, int64_t nrhs, int64_t rhs_words, void *stream,
                              int time_kernels, gf2bv_result **out);
int64_t gf2bv_factor_rank(const gf2bv_factor *h);
/* Writes the handle's pivot columns, `rank` entries, in one locked copy.  An append on another thread can raise the rank between
 * gf2bv_factor_rank and this call, so `out` must have room for cols entries (the rank never exceeds cols); a caller that shares the
 * handle pre-fills it with -1 and counts what was written -- that count and those entries are one state of the handle. */
int     gf2bv_factor_pivots(const gf2bv_factor *h, int32_t *out);
int64_t gf2bv_factor_device_bytes(const gf2bv_factor *h);              /* device memory the handle holds */
void    gf2bv_factor_free(gf2bv_factor *h);
/* Equations appended to a kept factorization.  After appending B1, ..., Bm to a handle made from A, the handle behaves as
 * gf2bv_factor_words on the row-stacked matrix [A; B1; ...; Bm] in that order: every later solve, rank, pivots and mode-1 basis is
 * bit-identical to gf2bv_solve_rhs_words on the stacked matrix, and a right-hand side then has ceil(total_rows / 64) words (bit r =
 * the constant of stacked row r).  The appended matrices have the handle's cols; their column `cols` is ignored; rows may be fewer
 * than cols (rows >= 1; the total stays within the size limits of the single entries).  Appends and solves interleave in any
 * order.  The cost is that of the new rows against the kept U and T, not a new factorization; the handle grows in steps of 1024
 * rows of capacity.  GF2BV_ERR_ARG (before the device is touched) and GF2BV_ERR_NOMEM (the grown handle or the append's buffers
 * do not fit; all are taken before the kept state changes) leave the handle as it was.  GF2BV_ERR_HIP means the append failed
 * after it had started to change the handle (a device error, or a refused allocation of the mode-1 basis's back-substitution):
 * the handle is then unusable -- rank and rows return -1, every other call GF2BV_ERR_ARG -- and only gf2bv_factor_free remains.
 * Forms as in gf2bv_factor_words / _digits / _device (d_aug 16-byte aligned, even stride_words, read after everything enqueued
 * on `stream` (NULL = the null stream) before the call). */
int gf2bv_factor_append_words(gf2bv_factor *h, const uint64_t *aug, int64_t rows, int64_t stride_words);
int gf2bv_factor_append_digits(gf2bv_factor *h, const uint32_t *digits, const int64_t *digit_off, int bits_per_digit,
                               int64_t rows);
int gf2bv_factor_append_device(gf2bv_factor *h, const void *d_aug, int64_t rows, int64_t stride_words, void *stream);
int64_t gf2bv_factor_rows(const gf2bv_factor *h);                     /* the stacked row count (-1: null or unusable handle) */
/* An independent handle with the same state: a device-to-device copy of the kept matrix and records (no factorization).  Appends
 * to either leave the other as it is.  Free it with gf2bv_factor_free. */
int     gf2bv_factor_copy(gf2bv_factor *h, gf2bv_factor **out);

/* Batch of `nsys` independent equal-shape systems resident on one device
 * (system s starts at d_aug + s*sys_stride_words words); out[0..nsys) receives handles.
 * The systems run in lock-step "gangs": one set of kernel launches eliminates a whole gang
 * (grid dimension y = system), so the latency-bound panel path is paid once per gang and the bulk
 * updates of all its systems fill the chip; results are identical to nsys separate calls.  In the
 * stats of a gang member ms_eliminate is the gang's elimination time, and ms_sweep (with
 * `time_kernels` != 0) the time inside the GANG's bulk-update launches (one launch serves all its
 * systems), not a per-system share.
 * Ordering: the gangs run on the library's own streams; they start after everything that was
 * enqueued on `stream` (a HIP stream handle, NULL = the null stream) when the call is made -- the stream
 * that produced the matrices -- and the call returns when all systems are solved.
 * Independent systems are the unit that bench.py shards across GPUs (BASELINE configs[3]).
 * Layout: the form of gf2bv_solve_device per system (d_aug 16-byte aligned, even stride_words covering cols+1 bits), and an
 * even sys_stride_words of at least rows*stride_words.  On any non-zero return every out[s] is null (results of gangs that
 * had finished are freed), and after the first failing gang no further gang is started. */
int gf2bv_solve_batch_device(void *d_aug, int64_t nsys, int64_t sys_stride_words,
                             int64_t rows, int64_t cols, int64_t stride_words,
                             int mode, int device, void *stream, int time_kernels, gf2bv_result **out);

/* Batch of `nsys` independent equal-shape systems given as digit arrays (see gf2bv_solve_digits):
 * row r of system s is entry s*rows + r of digit_off (nsys*rows + 1 entries).  One upload, lock-step
 * gangs as in gf2bv_solve_batch_device.  This is what a batched m4ri_solve binds
 * (gf2bv_amd._internal.m4ri_solve_many).  The offsets are absolute (they need not start at 0) and must not decrease;
 * digits may be null only when there are none.  On any non-zero return every out[s] is null. */
int gf2bv_solve_batch_digits(const uint32_t *digits, const int64_t *digit_off, int bits_per_digit,
                             int64_t nsys, int64_t rows, int64_t cols, int mode, int device,
                             gf2bv_result **out);

/* The same batch over SEVERAL devices of the node, from one process and without any collective: entry k of
 * devices[0..ndevices) takes the k-th contiguous share of the systems (floor(nsys*k/ndevices) ..) on its own host thread,
 * uploads only its share of the digits and runs it as lock-step gangs there; out[] is in input order and identical to
 * what the one-device call returns.  A device may be listed more than once (its shares then run as concurrent gangs).
 * The reference solves one system per m4ri_solve call (gf2bv/_internal.c:359-502): independent systems -- one per
 * output bit / per instance in the recovery examples -- are the natural shard unit; this is what
 * m4ri_solve_many(..., devices) binds: devices=None = the module's default device (as m4ri_solve: a process pinned to one
 * GPU stays on it), devices="all" = every visible device, or an explicit list.  The arguments are checked as in
 * gf2bv_solve_batch_digits before any device is; on any non-zero return every out[s] is null. */
int gf2bv_solve_batch_digits_multi(const uint32_t *digits, const int64_t *digit_off, int bits_per_digit,
                                   int64_t nsys, int64_t rows, int64_t cols, int mode,
                                   const int *devices, int ndevices, gf2bv_result **out);

/* ---- result accessors (AffineSpace getters, gf2bv/_internal.c:206-240) -------------------- */
int     gf2bv_result_status(const gf2bv_result *r);      /* GF2BV_STATUS_* */
int64_t gf2bv_result_rank(const gf2bv_result *r);
int64_t gf2bv_result_dimension(const gf2bv_result *r);   /* cols - rank (mode 1), basis rows */
int64_t gf2bv_result_words(const gf2bv_result *r);       /* ceil(cols/64) */
/* origin: the solution with every free variable 0 (_internal.c:438-455) */
int     gf2bv_result_origin(const gf2bv_result *r, uint64_t *out_words);
/* basis: dimension x words, M4RI kernel order (_internal.c:309-357, :475-489) */
int     gf2bv_result_basis(const gf2bv_result *r, uint64_t *out_words);
/* pivot columns c_0 < c_1 < ... (column rank profile), `rank` entries */
int     gf2bv_result_pivots(const gf2bv_result *r, int32_t *out);
int     gf2bv_result_stats(const gf2bv_result *r, gf2bv_stats *out);
void    gf2bv_result_free(gf2bv_result *r);

/* ---- AffineSpace arithmetic on host word vectors (tiny; gf2bv/_internal.c:242-273, :101-122) */
/* out = origin ^ XOR_{i: bit i of selector words set} basis[i]   (AffineSpace.get) */
void gf2bv_space_combine(const uint64_t *origin, const uint64_t *basis, int64_t dimension,
                         int64_t words, const uint64_t *selector, int64_t selector_words,
                         uint64_t *out);

/* ---- column-slab solve: ONE system over the GPUs of a node (replaces the single _mzd_pluq call of
 * gf2bv/_internal.c:431-433 for systems one GPU should not solve alone) --------------------------------------------
 * One process per GPU.  Rank r of `world` owns the column tiles t with t % world == r (gf2bv_slab_tiles(cols) tiles
 * of 8 words).  The caller owns the working matrix (d_work: gf2bv_slab_work_words(rows, cols) uint64, tile-major: tile
 * t is the contiguous slab d_work[t * slab_words .. (t+1) * slab_words), slab_words = work_words / tiles) and ALL the
 * communication:
 *     for b in range(gf2bv_slab_blocks(h)):
 *         if gf2bv_slab_owner(h, b) == rank: gf2bv_slab_factor(h, b, payload)    # panel path of the block, records out
 *         broadcast(payload, src = gf2bv_slab_owner(h, b))                       # ONE collective per block (RCCL over xGMI)
 *         gf2bv_slab_apply(h, b, payload)                                        # TRSM + bulk update of the own tiles
 *     gf2bv_slab_finish_local(h); gather every rank's tiles of d_work on rank 0; gf2bv_slab_solve(h, &result) there
 * payload: gf2bv_slab_payload_bytes(h) bytes of device memory (block records + rows x 32 bytes of multipliers).
 * Results are bit-identical to gf2bv_solve_device on the same matrix (the elimination is the same; only who applies
 * it to which columns differs).  d_aug: the full row-major system on every rank (left untouched); gf2bv_slab_open takes no
 * stream and reads it on the library's own stream, so d_aug must be complete on the device when the call is made (the caller
 * synchronizes the stream that produced it first). */
typedef struct gf2bv_slab gf2bv_slab;
int64_t gf2bv_slab_work_words(int64_t rows, int64_t cols);
int64_t gf2bv_slab_tiles(int64_t cols);
int     gf2bv_slab_open(void *d_aug, int64_t rows, int64_t cols, int64_t stride_words, void *d_work, int64_t work_words,
                        int world, int rank, int device, gf2bv_slab **out);
int64_t gf2bv_slab_blocks(const gf2bv_slab *h);
int     gf2bv_slab_owner(const gf2bv_slab *h, int block);
int64_t gf2bv_slab_payload_bytes(const gf2bv_slab *h);
int     gf2bv_slab_factor(gf2bv_slab *h, int block, void *d_payload);
int     gf2bv_slab_apply(gf2bv_slab *h, int block, const void *d_payload);
/* The same two steps ordered against the caller's collective stream instead of the host (`stream`: the HIP stream the
 * broadcast of d_payload is enqueued on).  The caller alternates TWO payload buffers: block b uses buffer b & 1 on every
 * rank.  _factor_on exports the records with one launch on the library's panel stream, makes `stream` wait for it and
 * returns at once: a broadcast enqueued on `stream` afterwards sends finished records, and the panel stream never waits
 * for the collective.  _apply_on imports what `stream` holds when it is called (non-owners), and orders `stream` behind the
 * import of the PREVIOUS block (whose buffer the next collective will write).  No call waits for the device: the broadcast
 * of block b + 1 overlaps the bulk update of block b on every rank.  At world size 1 nothing is exported at all.
 * (gf2bv_amd/slab.py runs this form.) */
int     gf2bv_slab_factor_on(gf2bv_slab *h, int block, void *d_payload, void *stream);
int     gf2bv_slab_apply_on(gf2bv_slab *h, int block, const void *d_payload, void *stream);
int     gf2bv_slab_finish_local(gf2bv_slab *h);
int     gf2bv_slab_solve(gf2bv_slab *h, gf2bv_result **out);
void    gf2bv_slab_close(gf2bv_slab *h);

/* ---- AffineSpace on the device: bulk enumeration (gf2bv/_internal.c:101-122 Gray walk, :63-91 binary walk) ---- */
/* The reference yields one element per call: one row XOR and one int export each.  Here a whole range of elements is
 * materialised by one kernel: element g of the walk = origin ^ XOR of basis[i] over the set bits i of code(g), with
 * code(g) = g ^ (g >> 1) for gray != 0 (AffineSpaceIterator, dimension <= 64) and code(g) = g otherwise
 * (AffineSpaceIteratorSlow, AffineSpace.get).  gf2bv_space_open uploads origin (words) and basis (dimension x words)
 * once; gf2bv_space_enumerate writes elements first .. first+count-1 (count x words uint64) to out_words (host
 * memory) -- or, with out_words == NULL, leaves them in the handle's own pinned buffer, valid until the next
 * enumerate / close (gf2bv_space_buffer): the iterators of the CPython binding slice their ints straight out of it. */
typedef struct gf2bv_space gf2bv_space;
int  gf2bv_space_open(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int device,
                      gf2bv_space **out);
int  gf2bv_space_enumerate(gf2bv_space *space, uint64_t first, int64_t count, int gray, uint64_t *out_words);
const uint64_t *gf2bv_space_buffer(const gf2bv_space *space);
void gf2bv_space_close(gf2bv_space *space);

/* ---- quadratic search: the consistent points of a linearised quadratic system's solution space ----------------------------
 * A space of QuadraticSystem unknowns: coordinates 0..n_lin-1 are linear, pair (i, j), j < i, is at n_lin + i(i-1)/2 + j;
 * `words` must cover those n_lin + n_lin(n_lin-1)/2 columns.  A point is consistent when every pair coordinate equals the
 * product of its two linear bits (QuadraticSystem.convert_sol).  The space is reduced to quadratic forms in r_eff variables
 * whose common zeros are exactly the consistent points (r: the rank of the space's projection onto the linear coordinates,
 * at most 256 is reduced).
 * gf2bv_quad_search: *count = the number of consistent points; the first min(count, max_solutions) of them, in the order in
 * which AffineSpace iteration meets them, are written to out_words (count x words).  *count = -1: the search gave up (r above
 * 256, or r_eff above max_enum and relinearisation makes no progress); *lin_rank = r in every case.  max_enum: 0..40.
 * More than 2^22 consistent points are counted, not collected: GF2BV_ERR_NOMEM when max_solutions > 0.  Argument errors
 * return GF2BV_ERR_ARG before any device is touched.
 * gf2bv_quad_search_alloc: the same search, the points in a buffer the library allocates for exactly min(count, max_solutions)
 * points (*out_words = NULL when that is 0), released with gf2bv_quad_free.
 * gf2bv_quad_plan (host only, touches no device): r, r_eff (-1: r above 256, no forms), m forms of form_words words each in
 * the equation-int layout of a QuadraticSystem of r_eff unknowns (bit 0 = constant, bit 1 + v = variable v, bit
 * 1 + r_eff + i(i-1)/2 + j = the product of variables i and j, j < i), written when forms != NULL and m <= forms_cap.  No
 * consistent point at all: r_eff = 0 and the single form 1.
 * gf2bv_quad_plan_device: the same plan with the forms built by the device kernel of gf2bv_quad_search (k_quad_forms) instead of
 * its host twin, so that the two can be compared; argument errors return GF2BV_ERR_ARG before any device is touched.
 * gf2bv_quad_points (host only): the points (words each) that nys common zeros ys (y_words each) of those forms stand for.
 * gf2bv_quad_forms_search: every common zero of m forms (that layout, r_eff <= 40) by the device search, ascending;
 * *count = their number, the first max_out written.
 * gf2bv_quad_last_times: this thread's last gf2bv_quad_search in ms -- reduction, forms build, affine elimination, device
 * search, relinearised solves, total -- then the number of levels and of first-pass candidates. */
int  gf2bv_quad_search(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                       int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t *out_words);
int  gf2bv_quad_search_alloc(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                             int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t **out_words);
void gf2bv_quad_free(uint64_t *words);
int  gf2bv_quad_plan(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                     int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms, int64_t forms_cap);
int  gf2bv_quad_plan_device(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin, int device,
                            int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms, int64_t forms_cap);
int  gf2bv_quad_points(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                       const uint64_t *ys, int64_t nys, int64_t y_words, uint64_t *out_words);
int  gf2bv_quad_forms_search(const uint64_t *forms, int64_t m, int64_t r_eff, int device, int64_t max_out, int64_t *count,
                             uint64_t *out);
void gf2bv_quad_last_times(double *out8);

/* ---- cubic search: the consistent points of a solution space over the degree-3 columns ----------------------------------------
 * A space over the columns of degree-3 XL and of PackedCubicSystem: coordinates 0..n_lin-1 are linear, pair (i, j), j < i, is at
 * n_lin + C(i,2) + j, triple (i, j, l), l < j < i, at n_lin + C(n_lin,2) + C(i,3) + C(j,2) + l; n_lin 1..2000 and `words` must
 * cover those columns.  A point is consistent when every pair and triple coordinate equals the product of its linear bits.  The
 * space is reduced to CUBIC forms in r_eff variables whose common zeros are exactly the consistent points.
 * The entries mirror the quadratic ones above one for one -- same arguments, same results, same order of the points, the same
 * 2^22 cap on collected points, max_enum 0..40, points released with gf2bv_quad_free -- with these differences:
 *  - r (the rank of the projection onto the linear coordinates) is reduced up to kFormsMaxRank = 64: a point of the forms is one word.
 *    Above it gf2bv_cubic_search gives up (*count = -1) and gf2bv_cubic_plan says r_eff = -1.
 *  - There is no relinearisation level: r_eff > max_enum gives up.  (r_eff <= r <= n_lin: with n_lin <= max_enum it never does.)
 *  - The forms are the equation ints of a PackedCubicSystem of r_eff unknowns: bit 0 the constant, bit 1 + k unknown k, bit
 *    1 + r_eff + C(i,2) + j the product of unknowns j < i, bit 1 + r_eff + C(r_eff,2) + C(i,3) + C(j,2) + l that of l < j < i;
 *    form_words = ceil((1 + r_eff + C(r_eff,2) + C(r_eff,3)) / 64).  Zero forms are dropped; none of those left is affine.
 *  - Memory: one build holds C(n_lin,2) + C(n_lin,3) product forms and up to as many forms of form_words(r) words each, on the
 *    host (gf2bv_cubic_plan) or on the device; a search holds m forms of 2 + r_eff + C(r_eff,2) words.  Above 1 GiB either returns
 *    GF2BV_ERR_NOMEM without attempting the allocation.
 *  - gf2bv_cubic_points: y_words >= 1; an assignment is the first word of each.
 *  - gf2bv_cubic_last_times: the relinearisation entry is 0 and `levels` counts the rounds of the affine elimination. */
int  gf2bv_cubic_search(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                        int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t *out_words);
int  gf2bv_cubic_search_alloc(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                              int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t **out_words);
int  gf2bv_cubic_plan(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                      int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms, int64_t forms_cap);
int  gf2bv_cubic_plan_device(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin, int device,
                             int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms, int64_t forms_cap);
int  gf2bv_cubic_points(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                        const uint64_t *ys, int64_t nys, int64_t y_words, uint64_t *out_words);
int  gf2bv_cubic_forms_search(const uint64_t *forms, int64_t m, int64_t r_eff, int device, int64_t max_out, int64_t *count,
                              uint64_t *out);
void gf2bv_cubic_last_times(double *out8);

/* ---- quartic search: the consistent points of a solution space over the degree-4 columns --------------------------------------
 * A space over the columns of degree-4 XL and of PackedQuarticSystem: the cubic layout above followed by the quadruples, (i, j, l, p),
 * p < l < j < i, at n_lin + C(n_lin,2) + C(n_lin,3) + C(i,4) + C(j,3) + C(l,2) + p; n_lin 1..450 and `words` must cover those
 * columns.  A point is consistent when every pair, triple and quadruple coordinate equals the product of its linear bits.  The space
 * is reduced to QUARTIC forms in r_eff variables whose common zeros are exactly the consistent points.  The
 * entries mirror the cubic ones above one for one -- r reduced up to 64, no relinearisation level (r_eff > max_enum gives up),
 * max_enum 0..40, y_words >= 1, the same order and cap of the points, gf2bv_quad_free -- with these differences:
 *  - The forms are the equation ints of a PackedQuarticSystem of r_eff unknowns: the cubic form layout followed by the product of
 *    unknowns p < l < j < i at bit 1 + r_eff + C(r_eff,2) + C(r_eff,3) + C(i,4) + C(j,3) + C(l,2) + p;
 *    form_words = ceil((1 + r_eff + C(r_eff,2) + C(r_eff,3) + C(r_eff,4)) / 64): 648 at r_eff = 32, 1297 at 38.
 *  - Memory: one build holds S = C(n_lin,2) + C(n_lin,3) + C(n_lin,4) product forms and up to as many forms of form_words(r) words
 *    each; a search holds m forms of 2 + r_eff + C(r_eff,2) + C(r_eff,3) words.  Above 1 GiB either returns GF2BV_ERR_NOMEM without
 *    attempting the allocation.  A space of full rank r = n_lin always fits up to n_lin = 35 (at most 0.83 GiB) and never from 40 on
 *    (the product forms alone take 1.21 GiB); at 36..39 it fits when few enough product coordinates are left as forms. */
int  gf2bv_quartic_search(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                          int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t *out_words);
int  gf2bv_quartic_search_alloc(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                                int max_enum, int64_t max_solutions, int device, int64_t *count, int64_t *lin_rank, uint64_t **out_words);
int  gf2bv_quartic_plan(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                        int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms, int64_t forms_cap);
int  gf2bv_quartic_plan_device(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin, int device,
                               int64_t *r, int64_t *r_eff, int64_t *m, int64_t *form_words, uint64_t *forms, int64_t forms_cap);
int  gf2bv_quartic_points(const uint64_t *origin, const uint64_t *basis, int64_t dimension, int64_t words, int64_t n_lin,
                          const uint64_t *ys, int64_t nys, int64_t y_words, uint64_t *out_words);
int  gf2bv_quartic_forms_search(const uint64_t *forms, int64_t m, int64_t r_eff, int device, int64_t max_out, int64_t *count,
                                uint64_t *out);
void gf2bv_quartic_last_times(double *out8);

/* ---- quadratic expansion: factored quadratic equations -> linearised rows, on the device ---------------------------------
 * A quadratic equation in n_lin unknowns kept FACTORED: a linear form plus products of two linear forms, every form
 * Wl = ceil((n_lin + 1) / 64) words in the equation-int order (bit 0 = constant, bit 1 + g = unknown g; bits above n_lin ignored).
 *   lin[rows_live][Wl]        the linear part of each row,
 *   term_off[rows_live + 1]   int64, starts at 0, never decreases: row r owns the products ta[t] * tb[t], t in term_off[r] .. term_off[r+1],
 *   ta[T][Wl], tb[T][Wl]      the operands, T = term_off[rows_live] (may be null when T is 0, host forms only).
 * (Arrays with entries for all `rows` rows are fine: what lies behind rows_live is not read.)
 * Row r of the output is e = lin[r] ^ XOR_t mul(ta[t], tb[t]) in the augmented-words layout for cols = n_lin + n_lin(n_lin-1)/2:
 * column c = bit c + 1 of e, column `cols` = bit 0 of e, every bit from cols + 1 to the end of the stride zero.  mul(a, b) is
 * QuadraticSystem._mul_bit (gf2bv/__init__.py:334-338): constant and linear bits a & b (x^2 = x; no constant x linear cross terms),
 * pair (i, j), j < i, at bit 1 + n_lin + i(i-1)/2 + j iff a_i b_j ^ a_j b_i with a_i = bit 1 + i of a.  Rows rows_live .. rows - 1
 * are written as zeros (the padding up to rows >= cols).
 * gf2bv_quad_expand_device: everything in device memory; the kernel is enqueued on `stream` (a HIP stream handle or NULL) and
 * the call returns, as gf2bv_synth_device does: gf2bv_solve_device / gf2bv_factor_device / gf2bv_factor_append_device on the same
 * stream consume d_aug with no synchronisation in between.  d_aug 16-byte aligned, stride_words even and >= ceil((cols + 1) / 64).
 * The offsets cannot be checked there: a row whose offsets decrease or are negative is expanded as its linear part.
 * gf2bv_quad_expand_words: host pointers in, rows x stride_words words back in host memory (upload, kernel, download).
 * gf2bv_solve_quad_terms: upload, expansion into a buffer of the pool, gf2bv_solve_device on the same stream; needs rows >= cols.
 * Argument errors (null pointers, n_lin < 1 or cols >= 2^31 - 64, rows_live outside 0..rows, offsets that do not start at 0 or
 * decrease, rows < cols for the solve entry, a bad stride or mode) return GF2BV_ERR_ARG before any device is touched. */
int gf2bv_quad_expand_device(const void *d_lin, const void *d_term_off, const void *d_ta, const void *d_tb, int64_t rows_live,
                             int64_t rows, int64_t n_lin, void *d_aug, int64_t stride_words, int device, void *stream);
int gf2bv_quad_expand_words(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t rows_live,
                            int64_t rows, int64_t n_lin, uint64_t *out_aug, int64_t stride_words, int device);
int gf2bv_solve_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t rows_live,
                           int64_t rows, int64_t n_lin, int mode, int device, gf2bv_result **out);

/* ---- cubic expansion: factored cubic equations -> linearised rows over the monomials of degree <= 3, on the device ----------
 * A cubic equation in n_lin unknowns kept FACTORED: a linear form plus products of two and products of three affine forms, every
 * form Wl = ceil((n_lin + 1) / 64) words in the equation-int order (bit 0 = constant, bit 1 + g = unknown g; bits above n_lin ignored).
 *   lin[rows_live][Wl]           the linear part of each row,
 *   off2[rows_live + 1]          int64, starts at 0, never decreases: row r owns the products ta[t] * tb[t], t in off2[r] .. off2[r+1],
 *   ta[T2][Wl], tb[T2][Wl]       their operands, T2 = off2[rows_live] (may be null when T2 is 0, host forms only),
 *   off3[rows_live + 1]          the same for the products ua[u] * ub[u] * uc[u], u in off3[r] .. off3[r+1],
 *   ua[T3][Wl], ub, uc           their operands, T3 = off3[rows_live] (may be null when T3 is 0, host forms only).
 * Row r of the output is e = lin[r] ^ XOR_t ta[t] tb[t] ^ XOR_u ua[u] ub[u] uc[u], the products being the EXACT products of
 * GF(2)[x] / (x_i^2 + x_i): constants multiply like anything else.  (This is NOT the mul of the quadratic expansion above, which
 * follows QuadraticSystem._mul_bit and has no constant x linear cross terms.)  The layout is degree-3 XL's augmented-words row over
 * cols3 = n_lin + C(n_lin,2) + C(n_lin,3): column c < n_lin unknown c, pair (i, j), j < i, at n_lin + C(i,2) + j, triple (i, j, l),
 * l < j < i, at cols2 + C(i,3) + C(j,2) + l, the constant at column cols3, every bit behind it up to the end of the stride zero.
 * Rows rows_live .. rows - 1 are written as zeros.
 * gf2bv_cubic_expand_device: everything in device memory; the kernel is enqueued on `stream` (a HIP stream handle or NULL) and the
 * call returns: gf2bv_solve_device on the same stream consumes d_aug with no synchronisation in between.  d_aug 16-byte aligned,
 * stride_words even and >= ceil((cols3 + 1) / 64).  The offsets cannot be checked there: a row whose offsets (of either kind)
 * decrease or are negative is expanded as its linear part.
 * gf2bv_cubic_expand_words: host pointers in, rows x stride_words words back in host memory (upload, kernel, download).
 * gf2bv_solve_cubic_terms: upload, expansion into a buffer of the pool, gf2bv_solve_device on the same pool stream; rows >= cols3.
 * Argument errors (null pointers, n_lin < 1 or cols3 >= 2^31 - 64, rows_live outside 0..rows, either offset array not starting at 0
 * or decreasing, rows < cols3 for the solve entry, a bad stride or mode, operands that do not fit the kernel's 64 KiB of LDS) return
 * GF2BV_ERR_ARG before any device is touched; an expansion that does not fit on the device returns GF2BV_ERR_NOMEM.
 * gf2bv_cubic_chunks (pure, no device): how many quadratic and how many cubic terms of a row one pass of the kernel holds in LDS at
 * this n_lin; a row with more of either takes several passes. */
int gf2bv_cubic_expand_device(const void *d_lin, const void *d_off2, const void *d_ta, const void *d_tb, const void *d_off3,
                              const void *d_ua, const void *d_ub, const void *d_uc, int64_t rows_live, int64_t rows, int64_t n_lin,
                              void *d_aug, int64_t stride_words, int device, void *stream);
int gf2bv_cubic_expand_words(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                             const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, int64_t rows_live, int64_t rows,
                             int64_t n_lin, uint64_t *out_aug, int64_t stride_words, int device);
int gf2bv_solve_cubic_terms(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                            const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, int64_t rows_live, int64_t rows,
                            int64_t n_lin, int mode, int device, gf2bv_result **out);
int gf2bv_cubic_chunks(int64_t n_lin, int32_t *quad_chunk, int32_t *cubic_chunk);

/* ---- quartic expansion: factored quartic equations -> linearised rows over the monomials of degree <= 4, on the device --------
 * A quartic equation in n_lin unknowns kept FACTORED: the cubic expansion's form with products of four affine forms too, every form
 * Wl = ceil((n_lin + 1) / 64) words in the equation-int order (bit 0 = constant, bit 1 + g = unknown g; bits above n_lin ignored).
 *   lin, off2, ta, tb, off3, ua, ub, uc   as for the cubic expansion,
 *   off4[rows_live + 1]                   int64, starts at 0, never decreases: row r owns the products va[v] * vb[v] * vc[v] * vd[v],
 *                                         v in off4[r] .. off4[r+1],
 *   va[T4][Wl], vb, vc, vd                their operands, T4 = off4[rows_live] (may be null when T4 is 0, host forms only).
 * Row r of the output is e = lin[r] ^ XOR_t ta[t] tb[t] ^ XOR_u ua[u] ub[u] uc[u] ^ XOR_v va[v] vb[v] vc[v] vd[v], the products being
 * the EXACT products of GF(2)[x] / (x_i^2 + x_i), constants included.  The layout is degree-4 XL's augmented-words row over
 * cols4 = n_lin + C(n_lin,2) + C(n_lin,3) + C(n_lin,4): column c < n_lin unknown c, pairs and triples where the cubic expansion puts
 * them, quadruple (i, j, l, p), p < l < j < i, at cols3 + C(i,4) + C(j,3) + C(l,2) + p, the constant at column cols4, every bit behind
 * it up to the end of the stride zero.  Rows rows_live .. rows - 1 are written as zeros.
 * gf2bv_quartic_expand_device: everything in device memory; the kernel (k_quartic_expand) is enqueued on `stream` (a HIP stream
 * handle or NULL) and the call returns: gf2bv_solve_device on the same stream consumes d_aug with no synchronisation in between.
 * d_aug 16-byte aligned, stride_words even and >= ceil((cols4 + 1) / 64).  The offsets cannot be checked there: a row whose offsets
 * (of any kind) decrease or are negative is expanded as its linear part.
 * gf2bv_quartic_expand_words: host pointers in, rows x stride_words words back in host memory (upload, kernel, download).
 * gf2bv_solve_quartic_terms: upload, expansion into a buffer of the pool, gf2bv_solve_device on the same pool stream; rows >= cols4.
 * Argument errors (null pointers, n_lin < 1 or cols4 >= 2^31 - 64, rows_live outside 0..rows, any of the three offset arrays not
 * starting at 0 or decreasing, rows < cols4 for the solve entry, a bad stride or mode, operands and staged rows that do not fit the
 * kernel's LDS -- it stages cubic rows of ceil((cols3 + 1) / 64) words there, which 160 KiB hold up to n_lin of about 157) return
 * GF2BV_ERR_ARG before any device is touched; an expansion that does not fit on the device returns GF2BV_ERR_NOMEM.
 * gf2bv_quartic_chunks (pure, no device): how many quadratic, cubic and quartic terms of a row one pass of the kernel holds in LDS
 * at this n_lin; a row with more of any takes several passes. */
int gf2bv_quartic_expand_device(const void *d_lin, const void *d_off2, const void *d_ta, const void *d_tb, const void *d_off3,
                                const void *d_ua, const void *d_ub, const void *d_uc, const void *d_off4, const void *d_va,
                                const void *d_vb, const void *d_vc, const void *d_vd, int64_t rows_live, int64_t rows, int64_t n_lin,
                                void *d_aug, int64_t stride_words, int device, void *stream);
int gf2bv_quartic_expand_words(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                               const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, const int64_t *off4, const uint64_t *va,
                               const uint64_t *vb, const uint64_t *vc, const uint64_t *vd, int64_t rows_live, int64_t rows,
                               int64_t n_lin, uint64_t *out_aug, int64_t stride_words, int device);
int gf2bv_solve_quartic_terms(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                              const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, const int64_t *off4, const uint64_t *va,
                              const uint64_t *vb, const uint64_t *vc, const uint64_t *vd, int64_t rows_live, int64_t rows,
                              int64_t n_lin, int mode, int device, gf2bv_result **out);
int gf2bv_quartic_chunks(int64_t n_lin, int32_t *quad_chunk, int32_t *cubic_chunk, int32_t *quartic_chunk);

/* The factored form in front of the entries that keep a factorization, share one elimination or batch: each uploads the term
 * arrays (host pointers, as gf2bv_solve_quad_terms takes them), expands them into a buffer of the pool and runs the device entry
 * named on the same pool stream; the host waits only where that entry waits, and the buffers are back in the pool on return.
 * Results are those of that entry on gf2bv_quad_expand_words of the same arrays.  Argument errors -- the rules of
 * gf2bv_solve_quad_terms and of the entry underneath -- return GF2BV_ERR_ARG before any device is touched; an expansion that does
 * not fit on the device returns GF2BV_ERR_NOMEM.
 * gf2bv_factor_quad_terms: gf2bv_factor_device on the expansion (rows >= cols; the handle keeps its own copy).
 * gf2bv_factor_append_quad_terms: gf2bv_factor_append_device on the handle's device; all `rows` >= 1 rows are live; n_lin must be
 *   the one the handle was made with (n_lin + n_lin(n_lin-1)/2 = its cols).  The failure contract of gf2bv_factor_append_* holds:
 *   the uploaded terms and the expansion are taken before the kept state changes, GF2BV_ERR_ARG and GF2BV_ERR_NOMEM leave the
 *   handle as it was.
 * gf2bv_solve_rhs_quad_terms: gf2bv_solve_rhs_device; rhs in host memory, in the format of gf2bv_solve_rhs_words.  As in every rhs
 *   entry the constant of the matrix input -- what the expansion leaves in column `cols` -- is ignored: rhs holds the constants.
 * gf2bv_solve_batch_quad_terms: nsys independent systems over the same n_lin as ONE concatenated term set; system s owns the
 *   factored rows sys_row_off[s] .. sys_row_off[s + 1] (nsys + 1 int64, from 0, never decreasing; term_off has one entry per row of
 *   the whole set and one more, its offsets absolute).  A system's live rows may not exceed `rows`, and rows >= cols: one launch
 *   expands every system (grid y = system) into rows x stride words each, the rows behind its live ones as zeros -- the host pads
 *   nothing --, and gf2bv_solve_batch_device solves them as lock-step gangs.  On any non-zero return every out[s] is null.
 * gf2bv_quad_expand_batch_words: that expansion alone, brought back to the host: out_aug holds nsys x rows x stride_words words. */
int gf2bv_factor_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t rows_live,
                            int64_t rows, int64_t n_lin, int mode, int device, gf2bv_factor **out);
int gf2bv_factor_append_quad_terms(gf2bv_factor *h, const uint64_t *lin, const int64_t *term_off, const uint64_t *ta,
                                   const uint64_t *tb, int64_t rows, int64_t n_lin);
int gf2bv_solve_rhs_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t rows_live,
                               int64_t rows, int64_t n_lin, const uint64_t *rhs, int64_t nrhs, int64_t rhs_words, int mode, int device,
                               gf2bv_result **out);
int gf2bv_solve_batch_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb,
                                 const int64_t *sys_row_off, int64_t nsys, int64_t rows, int64_t n_lin, int mode, int device,
                                 gf2bv_result **out);
int gf2bv_quad_expand_batch_words(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb,
                                  const int64_t *sys_row_off, int64_t nsys, int64_t rows, int64_t n_lin, uint64_t *out_aug,
                                  int64_t stride_words, int device);

/* ---- degree-3 XL: quadratic equations multiplied by 1 and by every unknown, on the device --------------------------------------
 * Input: m quadratic rows in n_lin unknowns in the augmented-words layout for cols2 = n_lin + n_lin(n_lin-1)/2 -- what
 * gf2bv_quad_expand_* writes: column c < n_lin unknown c, column n_lin + i(i-1)/2 + j the pair (i, j), j < i, column cols2 the
 * constant --, quad_stride_words >= ceil((cols2 + 1) / 64) words apart.
 * Output: `rows` >= m(n_lin + 1) rows over cols3 = cols2 + n_lin(n_lin-1)(n_lin-2)/6 columns: the first cols2 as in the input, the
 * triple (i, j, l), l < j < i, at column cols2 + i(i-1)(i-2)/6 + j(j-1)/2 + l, the constant at column cols3, every bit from cols3 + 1
 * to the end of the stride zero.  Equation e gives the rows e(n_lin+1) .. e(n_lin+1) + n_lin: row e(n_lin+1) is f_e itself, row
 * e(n_lin+1) + 1 + k is x_k f_e with x^2 = x.  For f = c + sum l_i x_i + sum q_ij x_i x_j that product has the constant 0, unknown k
 * = c ^ l_k, pair {k, i} = l_i ^ q_ki, the triple T containing k = q of the other two members of T, everything else 0.  Rows
 * m(n_lin+1) .. rows - 1 are written as zeros (the padding up to rows >= cols3).
 * gf2bv_xl3_expand_device: everything in device memory; the kernel is enqueued on `stream` (a HIP stream handle or NULL) and the
 * call returns, as gf2bv_quad_expand_device does: gf2bv_solve_device / gf2bv_factor_device on the same stream consume d_aug with no
 * synchronisation in between, and d_quad may be what gf2bv_quad_expand_device wrote on that stream.  d_aug 16-byte aligned,
 * stride_words even and >= ceil((cols3 + 1) / 64).
 * gf2bv_xl3_expand_words: host pointers in, rows x stride_words words back in host memory (upload, kernel, download).
 * gf2bv_solve_xl3_words: upload, expansion into a buffer of the pool with rows = max(m(n_lin+1), cols3), gf2bv_solve_device on the
 * same pool stream: a result over cols3 columns.
 * gf2bv_solve_xl3_quad_terms: the factored form of gf2bv_solve_quad_terms (all m rows live): the quadratic rows are expanded on the
 * device with no padding, multiplied there on the same stream and solved; quadratic rows and expansion are held at once.
 * Argument errors (null pointers, n_lin < 1, cols3 or m(n_lin+1) or rows >= 2^31 - 64, rows < m(n_lin+1), a short stride, for the
 * device entry an odd stride_words or a misaligned d_aug, a quadratic row above the kernel's LDS budget of 64 KiB -- n_lin > 1023 --,
 * a bad mode, the offset rules of gf2bv_solve_quad_terms) return GF2BV_ERR_ARG before any device is touched; an expansion that does
 * not fit on the device returns GF2BV_ERR_NOMEM. */
int gf2bv_xl3_expand_device(const void *d_quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int64_t rows, void *d_aug,
                            int64_t stride_words, int device, void *stream);
int gf2bv_xl3_expand_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int64_t rows, uint64_t *out_aug,
                           int64_t stride_words, int device);
int gf2bv_solve_xl3_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int mode, int device,
                          gf2bv_result **out);
int gf2bv_solve_xl3_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t m,
                               int64_t n_lin, int mode, int device, gf2bv_result **out);

/* ---- hybrid XL: guess unknowns, solve every assignment's degree-3 XL system as one batch ------------------------------------
 * With fewer than about n^2/6 independent quadratic equations degree-3 XL leaves a large space.  Fixing f unknowns in all 2^f ways
 * leaves 2^f quadratic systems in n' = n_lin - f unknowns with the same m equations each, which need about n'^2/6: independent
 * systems of one shape, solved as lock-step gangs (gf2bv_solve_batch_device).
 * Source rows: m quadratic rows over n_lin unknowns in the layout gf2bv_quad_expand_* writes (column c < n_lin unknown c, column
 * n_lin + i(i-1)/2 + j pair (i, j), j < i, the constant at column cols2).
 * Guess: nguess distinct unknown indices g_0 .. g_{nguess-1} in the caller's order (a host int32 array in every entry),
 * 0 <= nguess <= min(n_lin - 1, 30).  Assignment index a sets x_{g_t} to bit t of a.  R is the other unknowns in increasing index,
 * renumbered 0 .. n'-1.
 * Specialised row of assignment a: the same layout over n' unknowns, W2' = ceil((cols2' + 1) / 64) words:
 *   q'(i', j') = q(R[i'], R[j'])                                           (the pair block does not depend on a)
 *   l'(i')     = l(R[i']) ^ XOR_{t: a_t = 1} q(R[i'], g_t)
 *   c'         = c ^ XOR_{t: a_t = 1} l(g_t) ^ XOR_{t < u: a_t = a_u = 1} q(g_t, g_u)
 * A row may become 0 or the constant 1; it stays in and the solver reports the inconsistency.
 * System of assignment a: the degree-3 XL expansion of its m specialised rows exactly as gf2bv_xl3_expand_* defines it for n',
 * padded with zero rows to rows' = max(m(n'+1), cols3(n')).
 * gf2bv_quad_specialise_device (k_quad_specialise): the rows of assignments a0 .. a0 + na - 1; system s = a - a0 gets m rows
 * out_stride_words apart at d_out + s * sys_stride_words, every bit behind column cols2' written as zero.  out_stride_words >= W2',
 * sys_stride_words >= m * out_stride_words; 16-byte stores where both strides are even and d_out is 16-byte aligned, 8-byte stores
 * otherwise.  Enqueued on `stream`, the call returns: the ordering contract of gf2bv_xl3_expand_device.
 * gf2bv_quad_specialise_words: host pointers; out holds na x m x out_stride_words words.
 * gf2bv_xl3_expand_batch_device (k_xl3_expand_batch): nsys systems of m quadratic rows each, system s at
 * d_quad + s * quad_sys_stride_words, expanded to `rows` rows each at d_aug + s * sys_stride_words; d_aug 16-byte aligned,
 * stride_words and sys_stride_words even, sys_stride_words >= rows * stride_words, quad_sys_stride_words >= m * quad_stride_words.
 * gf2bv_xl3_expand_batch_words: the same with host pointers (no parity or alignment rule; the words of out_aug between a system's
 * rows and the next system are left as they are).
 * gf2bv_solve_xl3_guess_words / _quad_terms: on one pool stream the upload (or the quadratic expansion with no padding), the
 * specialisation, the batched expansion and gf2bv_solve_batch_device over cols3(n') columns; out[a - a0] is assignment a's result.
 * Held at once: the quadratic rows, na x m specialised rows and na x rows' expanded rows, plus what the gangs take.  On a non-zero
 * return every out[s] is NULL.
 * GF2BV_ERR_ARG, before any device is touched: null pointers, n_lin < 1, nguess < 0 or > min(n_lin - 1, 30), a guess out of range or
 * repeated, a0 < 0, na < 0, a0 + na > 2^nguess, na * m or na * rows' or nsys * rows >= 2^31 - 64, short strides, the rules of the XL
 * and batch entries underneath, a source row that does not fit the specialisation kernel's LDS together with its specialised form
 * and the guess vectors (64 KiB), a bad mode.  GF2BV_ERR_NOMEM: the staging does not fit.
 * gf2bv_xl3_guess_chunk (pure, no device): the largest count c <= 2^nguess whose specialised rows plus expansions take at most a
 * quarter of free_bytes (the solver keeps a tile-major copy of about the size of every system it has in a gang: expansion plus copy
 * stay below half of what was free) and whose rows together stay below 2^31 - 64; 0 when one system does not fit, -1 for a bad
 * shape.  gf2bv_xl3_guess_chunk_device reads the free memory of `device` (and what the library's pool holds idle there). */
int gf2bv_quad_specialise_device(const void *d_quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess,
                                 int64_t nguess, int64_t a0, int64_t na, void *d_out, int64_t out_stride_words, int64_t sys_stride_words,
                                 int device, void *stream);
int gf2bv_quad_specialise_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess,
                                int64_t nguess, int64_t a0, int64_t na, uint64_t *out, int64_t out_stride_words, int device);
int gf2bv_xl3_expand_batch_device(const void *d_quad, int64_t nsys, int64_t quad_sys_stride_words, int64_t m, int64_t quad_stride_words,
                                  int64_t n_lin, int64_t rows, void *d_aug, int64_t stride_words, int64_t sys_stride_words, int device,
                                  void *stream);
int gf2bv_xl3_expand_batch_words(const uint64_t *quad, int64_t nsys, int64_t quad_sys_stride_words, int64_t m, int64_t quad_stride_words,
                                 int64_t n_lin, int64_t rows, uint64_t *out_aug, int64_t stride_words, int64_t sys_stride_words, int device);
int gf2bv_solve_xl3_guess_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess,
                                int64_t nguess, int64_t a0, int64_t na, int mode, int device, gf2bv_result **out);
int gf2bv_solve_xl3_guess_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t m,
                                     int64_t n_lin, const int32_t *guess, int64_t nguess, int64_t a0, int64_t na, int mode, int device,
                                     gf2bv_result **out);
int64_t gf2bv_xl3_guess_chunk(int64_t m, int64_t n_lin, int64_t nguess, int64_t free_bytes);
int gf2bv_xl3_guess_chunk_device(int64_t m, int64_t n_lin, int64_t nguess, int device, int64_t *chunk);

/* ---- degree-4 XL: quadratic equations multiplied by 1, by every unknown and by every pair of unknowns, on the device ----------------
 * The xl4 entries are the xl3 entries above with the same arguments, stream-ordering and staging contracts; only the layout differs.
 * Input: m quadratic rows as for degree 3.
 * Columns: cols4 = cols3 + C(n_lin,4).  The first cols3 columns are exactly degree 3's; the quadruple (i, j, l, p), p < l < j < i, is at
 * column cols3 + C(i,4) + C(j,3) + C(l,2) + p; the constant at column cols4; every bit from cols4 + 1 to the end of the stride zero.
 * Rows: equation e owns R4 = 1 + n_lin + C(n_lin,2) rows from e * R4: f_e itself; x_k f_e at offset 1 + k, k = 0 .. n_lin - 1;
 * x_a x_b f_e, b < a, at offset 1 + n_lin + C(a,2) + b.  Rows m * R4 .. rows - 1 are written as zeros; the solve entries use
 * rows = max(m * R4, cols4).
 * Products, for f = c + sum l_i x_i + sum q_ij x_i x_j and S = {a, b}: x_a x_b f has the constant and every unknown 0, the pair S
 * = c ^ l_a ^ l_b ^ q_ab and every other pair 0, the triple S + {i} = l_i ^ q_ia ^ q_ib, the quadruple S + {i, j} = q_ij, and every
 * monomial that does not contain S 0.  The rows f and x_k f are degree 3's with zero quadruple columns.
 * Rank: the multipliers reach the equations' own degree, so f_i f_j and f_j f_i coincide and f_i f_i = f_i: before saturation the
 * rank of the m * R4 rows is m * R4 - m - C(m,2).
 * gf2bv_xl4_expand_device / _words (k_xl4_expand), gf2bv_solve_xl4_words, gf2bv_solve_xl4_quad_terms, gf2bv_xl4_expand_batch_device /
 * _words (k_xl4_expand_batch), gf2bv_solve_xl4_guess_words / _quad_terms (gf2bv_quad_specialise_device's rows over n' = n_lin - nguess
 * unknowns, expanded to degree 4 and solved as one batch over cols4(n') columns), gf2bv_xl4_guess_chunk / _chunk_device: as their xl3
 * twins.  GF2BV_ERR_ARG before any device is touched for the same reasons, with cols4 in place of cols3 and m * R4 in place of
 * m(n_lin + 1): every store of the kernels lands inside rows x stride_words.
 * gf2bv_xl4_quartic_root: the kernel's index function on the host -- the largest i >= 3 with C(i,4) <= u, -1 for u < 0 -- for checks. */
int gf2bv_xl4_expand_device(const void *d_quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int64_t rows, void *d_aug,
                            int64_t stride_words, int device, void *stream);
int gf2bv_xl4_expand_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int64_t rows, uint64_t *out_aug,
                           int64_t stride_words, int device);
int gf2bv_solve_xl4_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, int mode, int device,
                          gf2bv_result **out);
int gf2bv_solve_xl4_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t m,
                               int64_t n_lin, int mode, int device, gf2bv_result **out);
int gf2bv_xl4_expand_batch_device(const void *d_quad, int64_t nsys, int64_t quad_sys_stride_words, int64_t m, int64_t quad_stride_words,
                                  int64_t n_lin, int64_t rows, void *d_aug, int64_t stride_words, int64_t sys_stride_words, int device,
                                  void *stream);
int gf2bv_xl4_expand_batch_words(const uint64_t *quad, int64_t nsys, int64_t quad_sys_stride_words, int64_t m, int64_t quad_stride_words,
                                 int64_t n_lin, int64_t rows, uint64_t *out_aug, int64_t stride_words, int64_t sys_stride_words, int device);
int gf2bv_solve_xl4_guess_words(const uint64_t *quad, int64_t m, int64_t quad_stride_words, int64_t n_lin, const int32_t *guess,
                                int64_t nguess, int64_t a0, int64_t na, int mode, int device, gf2bv_result **out);
int gf2bv_solve_xl4_guess_quad_terms(const uint64_t *lin, const int64_t *term_off, const uint64_t *ta, const uint64_t *tb, int64_t m,
                                     int64_t n_lin, const int32_t *guess, int64_t nguess, int64_t a0, int64_t na, int mode, int device,
                                     gf2bv_result **out);
int64_t gf2bv_xl4_guess_chunk(int64_t m, int64_t n_lin, int64_t nguess, int64_t free_bytes);
int gf2bv_xl4_guess_chunk_device(int64_t m, int64_t n_lin, int64_t nguess, int device, int64_t *chunk);
int64_t gf2bv_xl4_quartic_root(int64_t u);

/* ---- degree-4 XL on cubic equations: cubic rows multiplied by 1 and by every unknown, on the device (k_xl4_cubic_expand) ------------
 * Input: m cubic rows over n_lin unknowns as gf2bv_cubic_expand_* writes them, cubic_stride_words apart: column c < n_lin the unknown
 * l_c, pair (i, j), j < i, at n_lin + C(i,2) + j (q_ij), triple (i, j, l), l < j < i, at cols2 + C(i,3) + C(j,2) + l (t_ijl), the
 * constant c at cols3.  W3 = ceil((cols3 + 1) / 64) words of a row are read; bits behind the constant column are ignored.
 * Output: degree-4 XL's columns (cols4 of them, the constant at cols4, every bit behind it up to the stride zero).
 * Rows: equation e owns the n_lin + 1 rows from e(n_lin + 1): f_e itself (its cols3 columns, no quadruple), then x_k f_e,
 * k = 0 .. n_lin - 1, with x^2 = x.  Rows m(n_lin + 1) .. rows - 1 are written as zeros; the solve entries use
 * rows = max(m(n_lin + 1), cols4).
 * Products: a monomial M of x_k f is f[M] ^ f[M - {k}] where M contains k and 0 elsewhere -- the unknown k = c ^ l_k, the pair {k, i}
 * = l_i ^ q_ki, the triple {k, a, b} = q_ab ^ t_kab, a quadruple containing k = t of its other three; the constant 0.
 * Rank: the multipliers (degree 1) stay below the equations' degree, so there is no forced relation among the rows as at degree 4 on
 * quadratic rows: about cols4 / (n_lin + 1) equations give full rank.
 * gf2bv_xl4_cubic_expand_device: everything in device memory; the kernel is enqueued on `stream` and the call returns.  d_aug needs
 * 16-byte alignment and an even stride_words covering cols4 + 1 bits.
 * gf2bv_xl4_cubic_expand_words: host pointers in, rows x stride_words words back (upload, kernel, download).
 * gf2bv_solve_xl4_cubic_words: expanded cubic rows in, multiplied and solved on the device.
 * gf2bv_solve_xl4_cubic_terms: the factored form of gf2bv_solve_cubic_terms (m live rows, no padding) uploaded, expanded by
 * k_cubic_expand, multiplied by k_xl4_cubic_expand and handed to gf2bv_solve_device, all on one pool stream: no row of either
 * expansion exists on the host.
 * GF2BV_ERR_ARG before any device is touched: null pointers, n_lin < 1 or cols4 >= 2^31 - 64, m(n_lin + 1) >= 2^31 - 64,
 * rows < m(n_lin + 1), a cubic row beyond the kernel's LDS (W3 * 8 > 64 KiB: n_lin above 146), cubic_stride_words < W3, a stride
 * that does not cover cols4 + 1 bits, a bad mode, and for the factored form what gf2bv_solve_cubic_terms refuses. */
int gf2bv_xl4_cubic_expand_device(const void *d_cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, int64_t rows, void *d_aug,
                                  int64_t stride_words, int device, void *stream);
int gf2bv_xl4_cubic_expand_words(const uint64_t *cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, int64_t rows,
                                 uint64_t *out_aug, int64_t stride_words, int device);
int gf2bv_solve_xl4_cubic_words(const uint64_t *cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, int mode, int device,
                                gf2bv_result **out);
int gf2bv_solve_xl4_cubic_terms(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                                const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, int64_t m, int64_t n_lin, int mode,
                                int device, gf2bv_result **out);

/* ---- hybrid degree-4 XL on cubic equations: guess unknowns, solve every assignment's system as one batch ---------------------------
 * The hybrid entries above one degree up: with fewer than about cols4 / (n_lin + 1) cubic equations, f unknowns are fixed in all 2^f
 * ways, which leaves 2^f cubic systems in n' = n_lin - f unknowns with the same m equations each; they need about cols4(n') / (n' + 1).
 * Source rows: m cubic rows over n_lin unknowns as gf2bv_cubic_expand_* writes them (the layout of the section above), W3 words read.
 * Guess, assignment index and R: as for gf2bv_quad_specialise_device.
 * Specialised row of assignment a, in the same layout over n' unknowns, W3' = ceil((cols3' + 1) / 64) words, with l, q, t taken over
 * unordered sets:
 *   t'(i', j', k') = t(R[i'], R[j'], R[k'])                                 (the triple block does not depend on a)
 *   q'(i', j')     = q(R[i'], R[j']) ^ XOR_{u: a_u = 1} t(R[i'], R[j'], g_u)
 *   l'(i')         = l(R[i']) ^ XOR_{u: a_u = 1} q(R[i'], g_u) ^ XOR_{u < v: a_u = a_v = 1} t(R[i'], g_u, g_v)
 *   c'             = c ^ XOR_{u} l(g_u) ^ XOR_{u < v} q(g_u, g_v) ^ XOR_{u < v < w} t(g_u, g_v, g_w)      (over the set bits of a)
 * A row may become 0 or the constant 1; it stays in and the solver reports the inconsistency.
 * gf2bv_cubic_specialise_device / _words (k_cubic_specialise): arguments, strides, store widths and the ordering contract of
 * gf2bv_quad_specialise_device / _words, with out_stride_words >= W3' and every bit behind column cols3' written as zero; bits
 * behind the source's constant column are ignored.
 * gf2bv_xl4_cubic_expand_batch_device / _words (k_xl4_cubic_expand_batch): gf2bv_xl3_expand_batch_device / _words on nsys systems of
 * m cubic rows each, every system expanded exactly as gf2bv_xl4_cubic_expand_* defines it.
 * gf2bv_solve_xl4_cubic_guess_words: expanded cubic rows in; upload, specialisation, batched multiply and gf2bv_solve_batch_device
 * over cols4(n') columns on one pool stream, rows' = max(m(n' + 1), cols4(n')) a system; out[a - a0] is assignment a's result.
 * gf2bv_solve_xl4_cubic_guess_terms: the factored form of gf2bv_solve_cubic_terms (m live rows, no padding) uploaded and expanded
 * by k_cubic_expand in front of the same chain: no row of any expansion exists on the host.  On a non-zero return every out[s] is NULL.
 * gf2bv_xl4_cubic_guess_chunk / _chunk_device: gf2bv_xl3_guess_chunk / _chunk_device for these systems (m W3' + rows' W4' words each).
 * GF2BV_ERR_ARG before any device is touched: what the quadratic hybrid entries refuse, with cols3 for cols2 in the source and cols4(n')
 * for cols3(n') in the systems; the cubic row, its specialised form and the guess vectors beyond the specialisation kernel's LDS
 * (8 (W3 + W3' + f ceil(cols2' / 64) + C(f,2) (ceil(n' / 64) + 1) + 1 + f) + 4 n' bytes > 64 KiB); what gf2bv_xl4_cubic_expand_* and,
 * for the factored form, gf2bv_solve_cubic_terms refuse. */
int gf2bv_cubic_specialise_device(const void *d_cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, const int32_t *guess,
                                  int64_t nguess, int64_t a0, int64_t na, void *d_out, int64_t out_stride_words, int64_t sys_stride_words,
                                  int device, void *stream);
int gf2bv_cubic_specialise_words(const uint64_t *cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, const int32_t *guess,
                                 int64_t nguess, int64_t a0, int64_t na, uint64_t *out, int64_t out_stride_words, int device);
int gf2bv_xl4_cubic_expand_batch_device(const void *d_cubic, int64_t nsys, int64_t cubic_sys_stride_words, int64_t m,
                                        int64_t cubic_stride_words, int64_t n_lin, int64_t rows, void *d_aug, int64_t stride_words,
                                        int64_t sys_stride_words, int device, void *stream);
int gf2bv_xl4_cubic_expand_batch_words(const uint64_t *cubic, int64_t nsys, int64_t cubic_sys_stride_words, int64_t m,
                                       int64_t cubic_stride_words, int64_t n_lin, int64_t rows, uint64_t *out_aug, int64_t stride_words,
                                       int64_t sys_stride_words, int device);
int gf2bv_solve_xl4_cubic_guess_words(const uint64_t *cubic, int64_t m, int64_t cubic_stride_words, int64_t n_lin, const int32_t *guess,
                                      int64_t nguess, int64_t a0, int64_t na, int mode, int device, gf2bv_result **out);
int gf2bv_solve_xl4_cubic_guess_terms(const uint64_t *lin, const int64_t *off2, const uint64_t *ta, const uint64_t *tb, const int64_t *off3,
                                      const uint64_t *ua, const uint64_t *ub, const uint64_t *uc, int64_t m, int64_t n_lin,
                                      const int32_t *guess, int64_t nguess, int64_t a0, int64_t na, int mode, int device,
                                      gf2bv_result **out);
int64_t gf2bv_xl4_cubic_guess_chunk(int64_t m, int64_t n_lin, int64_t nguess, int64_t free_bytes);
int gf2bv_xl4_cubic_guess_chunk_device(int64_t m, int64_t n_lin, int64_t nguess, int device, int64_t *chunk);

/* ---- composition: affine maps substituted into affine forms, and powers of a self-map, on the device (k_compose) -----------
 * Every form is in the equation-int order: bit 0 the constant, bit 1 + g unknown g, little-endian 64-bit words.
 *   a[ra][>= Wa]   forms over n unknowns, Wa = ceil((n + 1) / 64); bits above n are ignored,
 *   b[n][>= Wb]    images over nb unknowns, Wb = ceil((nb + 1) / 64): row g is the affine form that replaces unknown g; bits
 *                  above nb are ignored and come out zero.
 * out[r] = (bit 0 of a[r]) x 1 ^ XOR over the g with bit 1 + g of a[r] set, of b[g]: ra rows of Wb words over nb unknowns -- the
 * GF(2) matrix product a x b~, b~ = b with the unit form (bit 0 alone) in front as row 0.  The entries supply the unit row
 * themselves.  Words Wb .. out_stride - 1 of every output row are written as zero.  ra == 0 is legal and writes nothing.
 * gf2bv_compose_words: host pointers; upload, kernel, download on a stream of the pool.
 * gf2bv_compose_device: everything in device memory; the kernel is enqueued on `stream` (a HIP stream handle or NULL) and the call
 * returns, as gf2bv_quad_expand_device does; no pointer is kept.  d_a, d_b, d_out 16-byte aligned, their strides even; d_out must
 * not overlap d_a or d_b.
 * gf2bv_compose_power_*: b a self-map (n rows over n unknowns); out = the n image rows of b substituted into itself k times -- k = 0
 * the identity (image g = unknown g), k = 1 b itself with its bits above n dropped.  k = k_words[0 .. k_nwords), little-endian.
 * Square-and-multiply on the device: three (n + 1) x stride buffers of the pool stay resident, nothing comes back to the host
 * between the products, bit_length(k) - 1 + popcount(k) of them.  gf2bv_compose_power_device works on `stream` behind what is
 * queued there, copies d_b first (d_out may be d_b) and WAITS for the stream before it returns: its buffers go back to the pool.
 * gf2bv_compose_shape (no device): out[0] the bits of `a` per table slice, out[1] the rows of a workgroup, out[2] the words of a
 * column tile, out[3] the kernel's LDS bytes.
 * gf2bv_compose_last_times: this thread's last composition entry -- ms[0] upload, ms[1] kernels, ms[2] download (milliseconds; zero
 * for gf2bv_compose_device, which waits for nothing), ms[3] the number of products.
 * gf2bv_compose_unroll_*: a model stepped on the device.  b a self-map as for the power entries, a[ra] forms over its n unknowns;
 * out has count x ra rows, time-major: row i x ra + r = a[r] with b substituted start + i x step times (a o b^(start + i x step)),
 * i = 0 .. count - 1.  start >= 0 and step >= 1 are little-endian word arrays as k is.  count == 0 or ra == 0 is legal and writes
 * nothing.  The schedule is fixed: block 0 = a o b^start (start = 0: a copied with its bits above n cleared, no product; otherwise
 * b^start by square-and-multiply and one product), S = b^step (step = 1: b, no product), then doubling with P = S, h = 1: the rows
 * of the times [h, min(2h, count)) = the rows of the times [0, min(h, count - h)) o P, written straight to their place in out, and
 * P = P o P while 2h < count.  With pw(k) = bit_length(k) - 1 + popcount(k), pw(0) = 0, that is
 * (step > 1 ? pw(step) : 0) + (start > 0 ? pw(start) + 1 : 0) + (count >= 2 ? 2 ceil(log2 count) - 1 : 0) products.  Power's three
 * buffers and, for gf2bv_compose_unroll_words, the count x ra output rows stay resident; nothing comes back to the host between the
 * products and the count is not cut into chunks.  gf2bv_compose_unroll_device works on `stream` behind what is queued there, copies
 * d_b before anything else and WAITS for the stream before it returns; its blocks are read from and written to d_out, which must not
 * overlap d_a or d_b.
 * Argument errors (null pointers, ra < 0, count < 0, n < 1 or nb < 1, n + 1 or nb + 1 >= 2^31 - 64, a stride below its width, an odd
 * or unaligned device matrix, k_nwords, start_nwords or step_nwords < 1, step = 0, a largest block of the schedule that is no legal
 * product) return GF2BV_ERR_ARG before any device is touched; buffers that do not fit are GF2BV_ERR_NOMEM with nothing left
 * allocated. */
int gf2bv_compose_words(const uint64_t *a, int64_t ra, int64_t a_stride, int64_t n, const uint64_t *b, int64_t b_stride, int64_t nb,
                        uint64_t *out, int64_t out_stride, int device);
int gf2bv_compose_device(const void *d_a, int64_t ra, int64_t a_stride, int64_t n, const void *d_b, int64_t b_stride, int64_t nb,
                         void *d_out, int64_t out_stride, int device, void *stream);
int gf2bv_compose_power_words(const uint64_t *b, int64_t b_stride, int64_t n, const uint64_t *k_words, int64_t k_nwords, uint64_t *out,
                              int64_t out_stride, int device);
int gf2bv_compose_power_device(const void *d_b, int64_t b_stride, int64_t n, const uint64_t *k_words, int64_t k_nwords, void *d_out,
                               int64_t out_stride, int device, void *stream);
int gf2bv_compose_unroll_words(const uint64_t *a, int64_t ra, int64_t a_stride, int64_t n, const uint64_t *b, int64_t b_stride,
                               const uint64_t *start_words, int64_t start_nwords, const uint64_t *step_words, int64_t step_nwords,
                               int64_t count, uint64_t *out, int64_t out_stride, int device);
int gf2bv_compose_unroll_device(const void *d_a, int64_t ra, int64_t a_stride, int64_t n, const void *d_b, int64_t b_stride,
                                const uint64_t *start_words, int64_t start_nwords, const uint64_t *step_words, int64_t step_nwords,
                                int64_t count, void *d_out, int64_t out_stride, int device, void *stream);
int gf2bv_compose_shape(int32_t out[4]);
void gf2bv_compose_last_times(double ms[4]);

/* ---- synthetic systems + independent residual check (bench / tests) ----------------------- */
/* word w of row r = mix64(mix64(seed) ^ ((r<<20)|w)); planted solution = pseudo-row 0xFFFFF;
 * RHS = <row, planted>.  Writes rows x stride_words words at d_aug. */
/* (asynchronous: the generator kernel is enqueued on `stream` and the call returns) */
int gf2bv_synth_device(void *d_aug, int64_t rows, int64_t cols, int64_t stride_words,
                       uint64_t seed, int device, void *stream);
/* counts rows i with <A_i, x> != b_i on an (untouched) device matrix; x in host memory */
int gf2bv_residual_device(const void *d_aug, int64_t rows, int64_t cols, int64_t stride_words,
                          const uint64_t *x_words, int device, void *stream, int64_t *bad_rows);

/* Practical HBM ceilings of this device, measured with plain streaming kernels on a scratch buffer of
 * `bytes` bytes (use >= 1 GiB, well past the 256 MiB Infinity Cache): rmw_gbs = in-place 16-byte
 * read-XOR-write (the access pattern of the bulk update; read + written bytes per second),
 * read_gbs = read-only.  Reported by bench.py next to the 8 TB/s spec peak. */
int gf2bv_stream_ceiling_device(int device, int64_t bytes, double *rmw_gbs, double *read_gbs);

/* Shader clock of this device under an LDS-bound load (every CU issuing ds_read_b128 back to back for ~5 ms), from the
 * shader-clock and the 100 MHz real-time counters inside the kernel, and the LDS bytes per clock and CU that load reached
 * (MI355X_MICROARCH.md: 256 B/clk/CU for ds_read_b128).  bench.py prices the table lookups of the K-fused outer pass
 * (k_update16k, LDS-bound) against CUs x 256 B x this clock. */
int gf2bv_lds_clock_device(int device, double *shader_mhz, double *lds_bytes_per_clk_cu);

/* Registers per lane and static LDS bytes of the kernels that must fit on a compute unit TOGETHER -- the panel path of
 * block b+1 runs beside the bulk update of block b, and a panel kernel that does not fit next to an update workgroup
 * (two wavefronts per SIMD, 128 KiB of tables) silently waits for one to retire: out[0..1] the default bulk-update
 * instance, then k_block_fast, k_narrow_all, k_prio_window, k_panel_step (registers, LDS each; n >= 10).  A test holds the
 * budget: registers <= 512 - 2 x round_up(update's, 8), LDS <= 160 KiB - update's.  With n >= 13: out[10..12] = registers,
 * LDS and SCRATCH bytes per lane of k_update16k, the outer pass of the two-level elimination (it keeps 16 row segments per
 * lane in registers: scratch must be 0).  With n >= 15: out[13..14] = registers, LDS of k_block_fast_narrow.  With n >= 17:
 * out[15..16] = registers, LDS of k_block_sparse<256, 4> (the sparse block search, first pool size: beside the bulk update like
 * every panel kernel). */
int gf2bv_kernel_resources(int device, int32_t *out, int n);

/* plain device buffer helpers so a host language without a HIP binding can stage data.  gf2bv_device_alloc: when the device
 * is out of memory the pool's idle buffers are freed and the allocation is repeated once. */
int gf2bv_device_alloc(int device, int64_t bytes, void **d_ptr);
int gf2bv_device_free(int device, void *d_ptr);
int gf2bv_device_upload(int device, void *d_dst, const void *h_src, int64_t bytes);
int gf2bv_device_download(int device, void *h_dst, const void *d_src, int64_t bytes);


/* Page-locked host staging for bindings that assemble their input on the host (the CPython shim gathers every equation's digit
 * array -- gf2bv/_internal.c:403-426 walks them bit by bit instead -- into ONE buffer before gf2bv_solve_digits): the
 * host-to-device copy out of such a buffer is a single DMA, and the buffers are recycled between calls (up to four idle ones,
 * GF2BV_HOST_POOL_MB MiB in all, default 4608 -- DESIGN.md, "Environment switches"; gf2bv_host_pool_trim frees the idle ones and returns their bytes).  Any host
 * pointer remains valid input for every entry point; this is an optimisation, not a requirement. */
int  gf2bv_host_alloc(int64_t bytes, void **h_ptr);
void gf2bv_host_free(void *h_ptr);
int64_t gf2bv_host_pool_trim(void);

/* ---- the buffer pool (see "Threading" at the top) ----------------------------------------------- */
/* Frees every IDLE buffer the pool keeps on `device` (large working buffers and the small-buffer cache; nothing a running
 * solve holds).  Returns the bytes given back to the device, -1 without a usable device.  A caller that shares the GPU
 * (a tensor framework, another library) calls this between jobs; the library calls it itself when hipMalloc reports out of memory. */
int64_t gf2bv_pool_trim(int device);
/* Bytes of idle buffers the pool currently keeps on `device` (what gf2bv_pool_trim would free). */
int64_t gf2bv_pool_idle_bytes(int device);
/* What the pool has handed out on `device` and not yet got back: out[0] buffers, out[1] streams, out[2] events.  An entry gives back
 * everything it took before it returns, so between calls these count only what kept handles (gf2bv_factor, gf2bv_space, gf2bv_slab)
 * own; while another thread is inside the library they are a snapshot of its work.  Returns 0, or -1 for device < 0 or a null
 * `out`; no device is touched. */
int gf2bv_pool_in_use(int device, int64_t out[3]);
/* The gang size gf2bv_solve_batch_* would choose for `nsys` systems of rows x cols with `free_bytes` of device memory free: a pure
 * function, no device is touched (bench.py --dry-run-ranks: every rank's plan of the multi-GPU batch job, testable without GPUs). */
int64_t gf2bv_plan_gang(int64_t nsys, int64_t rows, int64_t cols, int64_t free_bytes);
/* The GF2BV_* environment switches as a solve entered now would parse them ("Environment switches"): one "NAME=value\n"
 * line per variable into buf (n bytes, NUL-terminated), the value after defaults and clamps, "unset" where a variable that is not
 * set leaves the choice to the solve.  No device is touched.  GF2BV_ERR_ARG when buf is null or too small (2048 bytes suffice). */
int gf2bv_knob_dump(char *buf, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* GF2BV_HIP_H */
