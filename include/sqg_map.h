/*
 * sqg_map.h -- subsequence dynamic time warping of event rows against the genome's expected level track, on the device (an addition to
 * sqg_scale.h and sqg_pileup.h).
 *
 * Every consumer call so far is handed what a real tool has to work out first: which stretch of the reference a read came from.
 * sqg_batch_align aligns rows to the read's own true events, the pileups take their keys from the sampler's origin.  The step in front of
 * all that -- finding a read's signal in the reference -- is subsequence DTW (sDTW) of the read's first events against the expected levels
 * of both strands: SquiggleFilter and DTWax map this way, RawHash and Sigmap in their chaining-free modes, and every Read-Until /
 * adaptive-sampling decision rests on it.  A simulator is the one place where the answer is known for every read: map_key0 and map_step
 * below compare directly with sqg_pileup.h's origin {key0, step}.
 *
 * The rule below is the contract: exact integers throughout, no floating point.
 *
 * HIP backend only, like every consumer call; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * Contexts.  DNA without SQG_PREFIX, with SQG_METH or without.  Anything else returns SQG_EINVAL, and sqg_last_error names the flag.
 *   sqg_map_track needs a loaded genome (sqg_genome_load*), else SQG_ESEQUENCE.  sqg_batch_map needs only the track's arrays: the rows of
 *   a staged batch can be mapped against a track built earlier, or against a synthetic one.  For uniformity it takes the lifetime rule of
 *   sqg_batch_align: the batch has been run and still owns its device results and its dwells, else SQG_ESEQUENCE.
 *
 * ---- sqg_map_track ----
 *
 * [lo, hi) is a window of forward-strand coordinates of the loaded genome, contigs laid end to end as in sqg_pileup.h: 0 <= lo <= hi <=
 * genome length and hi - lo <= 2^24 (SQG_MAP_MAX_WINDOW).  levels is a caller-owned device array of int32, [4^k] ([5^k] under SQG_METH):
 * the level of every pore-table row in 1/256 ADC code.  It is device memory, which the host cannot refuse, so a value is CLAMPED to
 * +-2^23, as sqg_call.h clamps its inputs.  fwd and rev are caller-owned device arrays of int32, [hi - lo], OVERWRITTEN; either may be NULL.
 *
 * For every g in [lo, hi):
 *     fwd[g - lo] = levels[row(G[g .. g+k))]
 *     rev[g - lo] = levels[row(revcomp(G[g .. g+k)))]
 *   row is sqg_targets.h's kmer rule: 2 bits per base, base-5 digits under SQG_METH -- of the plain bases, no 'M' is ever put in.
 *   Case.  The genome's bytes are taken as the sampler takes them (k_sampler.h: k_copy_reads).  A '+' read is a copy of the bytes as they
 *   stand, so fwd ranks them as they stand: without SQG_METH a lower-case base ranks as its upper case, under SQG_METH a lower-case byte
 *   has digit 0, as it has in a sampled read.  A '-' read goes through the complement table, which answers in upper case for either case,
 *   so rev ranks the upper-case complement (reversed) with or without SQG_METH.
 *   A position has no level -- BOTH entries are SQG_MAP_NONE (INT32_MIN) -- when g + k runs past the end of g's contig, when g + k >
 *   genome length, or when any of the k bytes is not one of A C G T a c g t, an 'N' among them.  The k-mer may run past hi: the window
 *   bounds the starting positions, not the bytes that are read.
 *
 * ---- sqg_batch_map ----
 *
 * Rows.  row_off is a HOST array [n_reads+1] as for sqg_batch_align, in->sum and in->len are sqg_align_in_t, the optional scale is
 *   sqg_align_scale_t.  Read r maps the rows i = 0 .. m-1 with
 *       m = clamp(row_off[r+1] - row_off[r] - cfg.row_first, 0, cfg.row_count)
 *   and row i is row row_off[r] + cfg.row_first + i of the caller's arrays.  Its value q[i] is sqg_scale.h's q0 -- that floor, that product
 *   modulo 2^64, that clamp to +-2^26 -- and with a scale that header's q, with its shift and its clamps, gain[r] and shift[r] CLAMPED into
 *   their ranges.
 *
 * cfg       stay_pen    added when a row stays on the position of the row before it, 0 .. 1<<17
 *           skip_pen    added when a row skips one position, 0 .. 1<<17
 *           cost_cap    a cell's cost is capped here, 1 .. 1<<17
 *           row_first   the first row of every read that is mapped, >= 0
 *           row_count   at most this many rows are mapped, 1 .. 4096 (SQG_MAP_MAX_ROWS)
 *           strands     bit 0 (SQG_MAP_PLUS): '+', bit 1 (SQG_MAP_MINUS): '-'; at least one, no other bit
 *   With these ranges D < 4096 * 2^17 + 4095 * 2^17 < 2^30: a cell is 32 bits.
 *
 * Track.  track->lo, hi, fwd, rev as sqg_map_track wrote them, or synthetic: int32 [hi - lo] each, a value other than SQG_MAP_NONE CLAMPED
 *   to +-2^23.  fwd is read only for '+', rev only for '-'; the one a strand asked for needs must not be NULL.  W = hi - lo <= 2^24.
 *
 * Programme.  Per strand the positions are u = 0 .. W-1.
 *     '+'   u stands for g = lo + u,      Lv[u] = fwd[u]
 *     '-'   u stands for g = hi - 1 - u,  Lv[u] = rev[hi - 1 - lo - u]          (a '-' read walks the forward coordinate downwards)
 *   Cell cost.  c(i,u) = cost_cap where Lv[u] is SQG_MAP_NONE, else min(|q[i] - Lv[u]|, cost_cap).
 *   Row 0:      D[0][u] = c(0,u), S[0][u] = u: the free start.
 *   Row i >= 1: three candidates, in this order:
 *                 step  D[i-1][u-1]
 *                 stay  D[i-1][u]   + stay_pen
 *                 skip  D[i-1][u-2] + skip_pen
 *               a candidate with a negative index is absent; the FIRST candidate with the smallest value wins, D[i][u] is that value
 *               plus c(i,u), and S[i][u] is the winner's S.  The start of the path travels with the cell: there is no traceback and no
 *               trace memory.
 *   End.        e is the lowest u at which D[m-1][u] is smallest.  The read's strand is the one with the smaller end cost; a tie goes
 *               to '+'.
 *
 * Outputs, [n_reads] each.  map_cost: the winning strand's D[m-1][e].  map_step: +1 / -1.  map_key0, map_key1: the g of S[m-1][e] and of
 *   e -- the forward coordinate of the k-mer under row 0 and under the last row; on '-' key0 >= key1.  map_cost_other: the other strand's
 *   end cost, -1 if that strand was not asked for.  m == 0 or W == 0: map_cost = -1, map_step = 0, both keys INT64_MIN, map_cost_other = -1.
 *
 * Limit.  Time is m * W per strand and read.  This is a mapper for a virus, an amplicon panel or a target region -- SquiggleFilter's and
 *   Read-Until's case --, not for a 3-Gb genome, which needs seeding first; that is not here.
 *
 * SQG_MAP_DEFAULT takes SQG_ALIGN_DEFAULT's penalties, clipped to the ranges above, 256 rows and both strands.  It is a starting point
 * and is not measured.
 *
 * The recommended levels, made by the binding's map_levels() from the context's own pore model and not part of the kernel's rule:
 *     levels = (int32)rint(256 * (double)level_mean * digitisation / range)
 *   and the recommended scale for rows in stored ADC codes, the binding's Batch.map_shift(): gain 65536, shift = rint(256 * offset[r]).
 */
#ifndef SQG_MAP_H
#define SQG_MAP_H

#include "sqg_scale.h"
#include "sqg_pileup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SQG_MAP_NONE        INT32_MIN     /* a track entry without a level                                          */
#define SQG_MAP_MAX_WINDOW  (1 << 24)     /* hi - lo                                                                */
#define SQG_MAP_MAX_ROWS    4096          /* cfg.row_count                                                          */
#define SQG_MAP_PLUS        1u
#define SQG_MAP_MINUS       2u

typedef struct {
    int32_t  stay_pen;        /* added when a row stays on the position of the row before it, 0 .. 1<<17            */
    int32_t  skip_pen;        /* added when a row skips one position, 0 .. 1<<17                                    */
    int32_t  cost_cap;        /* a cell's cost is capped here, 1 .. 1<<17                                           */
    int32_t  row_first;       /* the first row of every read that is mapped, >= 0                                   */
    int32_t  row_count;       /* at most this many rows, 1 .. SQG_MAP_MAX_ROWS                                      */
    uint32_t strands;         /* SQG_MAP_PLUS | SQG_MAP_MINUS, at least one                                         */
} sqg_map_cfg_t;

#define SQG_MAP_DEFAULT { 4096, 4096, 65536, 0, 256, 3u }

typedef struct {              /* the window and its levels: what sqg_map_track wrote, or synthetic                  */
    int64_t lo, hi;           /* [lo, hi), hi - lo <= SQG_MAP_MAX_WINDOW                                            */
    const int32_t *fwd;       /* DEVICE, caller-owned, [hi - lo]; needed for '+'                                    */
    const int32_t *rev;       /* DEVICE, caller-owned, [hi - lo]; needed for '-'                                    */
} sqg_map_track_t;

typedef struct {              /* DEVICE, caller-owned, [n_reads], OVERWRITTEN; any may be NULL = not wanted          */
    int32_t *map_cost;        /* the winning strand's end cost; -1: none                                            */
    int8_t  *map_step;        /* +1 / -1; 0: none                                                                   */
    int64_t *map_key0;        /* forward coordinate of the k-mer under row 0; INT64_MIN: none                       */
    int64_t *map_key1;        /* ... under the last row                                                             */
    int32_t *map_cost_other;  /* the other strand's end cost; -1: not asked for, or none                            */
} sqg_map_out_t;

/* device: the level track of [lo, hi) of the loaded genome into fwd and rev, those that are not NULL; returns when they are complete.
 * SQG_EINVAL, sqg_last_error naming the cause: a NULL ctx or levels; a context as above; lo < 0, hi < lo, hi > genome length,
 * hi - lo > SQG_MAP_MAX_WINDOW.  SQG_ESEQUENCE: no genome is loaded.  hi == lo succeeds and writes nothing.  Works on the context's
 * stream and waits for it. */
int sqg_map_track(sqg_ctx_t *ctx, int64_t lo, int64_t hi, const int32_t *levels, int32_t *fwd, int32_t *rev);

/* device: maps the first rows of every read of the batch against the track and fills the outputs of *out that are not NULL; returns when
 * they are complete.  row_off is HOST memory, [n_reads+1].  SQG_EINVAL, sqg_last_error naming the field: a NULL ctx, batch, cfg, row_off,
 * in, in->sum, in->len, track or out; a cfg field outside the ranges above; a scale with a NULL gain or shift (scale NULL: none);
 * track->hi < track->lo or hi - lo > SQG_MAP_MAX_WINDOW; a NULL fwd with SQG_MAP_PLUS or a NULL rev with SQG_MAP_MINUS while hi > lo; a
 * row_off that does not start at 0 or is not non-decreasing, or a read of 2^31 rows or more; a context as above.  SQG_ESEQUENCE: the
 * lifetime rule above.  An empty batch succeeds and writes nothing.  Works on the context's stream and waits for it; the caller's arrays
 * must not be in use by another stream meanwhile. */
int sqg_batch_map(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_map_cfg_t *cfg, const int64_t *row_off, const sqg_align_in_t *in,
                  const sqg_align_scale_t *scale, const sqg_map_track_t *track, const sqg_map_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
