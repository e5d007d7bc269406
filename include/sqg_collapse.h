/*
 * sqg_collapse.h -- event rows summed per true event they are assigned to, and the pileup of those sums (an addition to sqg_pileup.h).
 *
 * sqg_batch_events is the table the simulator knows, sqg_batch_pileup its sum across reads; sqg_batch_detect is the table a tool finds in
 * the samples, sqg_batch_align the assignment of the found rows to the read's k-mers.  What m6Anet, xPore, Nanocompore and
 * `nanopolish train` ingest lies one step further: the aligned rows merged per k-mer position (f5c `eventalign --collapse-events`,
 * Nanocompore `eventalign_collapse`), then those merged rows summed by reference position or by k-mer.  The two calls here make that
 * join on the device.  sqg_batch_collapse gives the OBSERVED event table: the caller's rows summed per true event, mean / sd by the
 * event table's own formulas.  sqg_batch_pileup_rows adds that observed table into the arrays sqg_batch_pileup adds the truth to, under
 * the same rules: "observed minus true" per site or per pore-table row is a subtraction of two pileups.
 *
 * The rule below is the contract: exact integers throughout, except mean / sd, which are sqg_events.h's formulas with one rounding per
 * operation.
 *
 * HIP backend only, like every consumer call; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * Contexts.  All that sqg_batch_events takes.  The rows are plain device arrays of the caller's: the detector's (sum, sumsq, dt_len,
 * det_off) with the aligner's al_ev or the detector's true_ev, the true table's own, or any other.
 *
 * Which rows count.  Row i of read r has row_off[r] <= i < row_off[r+1].  It counts iff ev_off[r] <= ev[i] < ev_off[r+1] with the
 *   batch's own ev_off: its event is one of its read's.  Every other value of ev[i] -- -1 (the aligner's "none"), an event of another
 *   read -- DROPS the row: a dropped row adds 1 to rd_dropped[r] and to nothing else.  No order of ev within a read is assumed.
 *
 * Sums.  For event e, over the rows that count with ev[i] == e, in any order:
 *     ob_rows[e]  = their number, modulo 2^32
 *     ob_len[e]   = sum of max(len[i], 0)
 *     ob_sum[e]   = sum of sum[i]         over the rows with len[i] >= 1
 *     ob_sumsq[e] = sum of sumsq[i]       over the rows with len[i] >= 1
 *   The last three are two's-complement and wrap modulo 2^64: np.add.at in wrapping arithmetic, as in sqg_pileup.h.  A row with
 *   len < 1 adds to ob_rows only.  An event that no row is assigned to has zeros in all four.
 *
 * mean, sd.  With ob_len[e] > 0: sqg_events.h's expressions with len = (double)ob_len[e], sum = (double)ob_sum[e] and
 *   sumsq = (double)ob_sumsq[e], for the read of event e; norm and trim as in sqg_event_cfg_t (PA: the read's offset; MEDMAD: med2 and
 *   inv of the span trim selects).  ob_len[e] == 0: mean = sd = 0.0f.  For ob_len < 2^31 the result is bit-equal to what
 *   sqg_batch_events derives from the same sums.
 *
 * Observed pileup.  An event e is ELIGIBLE, and has its key and plane, exactly as sqg_pileup.h says for event e (by, split, segs, the
 *   origin and the sampler's origin).  Eligible with ob_rows[e] == 0: `unseen`, adds nothing.  Eligible, seen, key outside [lo, hi):
 *   `outside`.  Otherwise `counted`, and it adds
 *     n += 1                                         one per observed event, not one per row
 *     ob_len > 0:  dwell += ob_len, dwell_sq += ob_len * ob_len modulo 2^64,
 *                  mean_sum, mean_sq, sd_sum from q(mean), q(sd) of the collapse's floats under the cfg's norm and trim
 *     ob_len == 0: n only.
 *   q is sqg_pileup.h's; it is defined for |mean| * 4096 < 2^63, which the samples of a batch never leave and a caller's sums may: beyond it
 *   the arithmetic of q alone is undefined, never the memory the call touches.
 *   dropped: the sum of rd_dropped.  With rows that are the true table itself (ev = 0 .. n_events-1, sum, sumsq, ev_len) the call adds
 *   bit for bit what sqg_batch_pileup adds and reports the same counted and outside, unseen == dropped == 0.
 */
#ifndef SQG_COLLAPSE_H
#define SQG_COLLAPSE_H

#include "sqg_pileup.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t norm;           /* SQG_CHUNK_MEDMAD | SQG_CHUNK_PA, as sqg_event_cfg_t.norm                     */
    int32_t  trim;           /* as sqg_event_cfg_t.trim                                                     */
} sqg_collapse_cfg_t;

typedef struct {             /* DEVICE memory of the context's device, owned by the caller, [n_rows], each at its element's natural alignment */
    const int64_t *ev;       /* the row of sqg_batch_events each row is assigned to (al_ev, true_ev, or the caller's own) */
    const int64_t *sum;      /* sum of the row's samples                                                    */
    const int64_t *sumsq;    /* sum of their squares; may be NULL only if neither ob_sumsq, sd nor (pileup) sd_sum is wanted */
    const int32_t *len;      /* samples of the row                                                          */
} sqg_collapse_in_t;

typedef struct {             /* DEVICE, caller-owned, OVERWRITTEN; any may be NULL = not wanted                */
    uint32_t *ob_rows;       /* [n_events] rows assigned to the event                                       */
    int64_t  *ob_len;        /* [n_events] sum of their len (rows with len < 1 add 0)                       */
    int64_t  *ob_sum;        /* [n_events] sum of their sum                                                 */
    int64_t  *ob_sumsq;      /* [n_events] sum of their sumsq                                               */
    float    *mean, *sd;     /* [n_events] sqg_events.h's formulas on (ob_sum, ob_sumsq, ob_len)            */
    int32_t  *rd_dropped;    /* [n_reads]  rows of the read that were dropped                               */
} sqg_collapse_out_t;

/* device: sums the rows [row_off[r], row_off[r+1]) of *in per event of read r, for every read of the batch, and fills the outputs of *out
 * that are not NULL; returns when they are complete.  n_rows = row_off[n_reads]; row_off is HOST memory, [n_reads+1].  The lifetime rule
 * of sqg_batch_events: the batch must have been run and still own its device results AND its dwells, else SQG_ESEQUENCE.  A NULL ctx,
 * batch, cfg, row_off, in, in->ev, in->sum, in->len or out; an unknown norm, a trim that is neither 0 nor 1; a row_off that does not start
 * at 0 or is not non-decreasing, or a read of 2^31 rows or more; a NULL in->sumsq while ob_sumsq or sd is wanted: SQG_EINVAL,
 * sqg_last_error names the field.  An empty batch succeeds and writes nothing; n_rows == 0 on a batch that is not empty zero-fills the
 * outputs.  Works on the context's stream and waits for it. */
int sqg_batch_collapse(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_collapse_cfg_t *cfg, const int64_t *row_off,
                       const sqg_collapse_in_t *in, const sqg_collapse_out_t *out);

typedef struct { int64_t counted, outside, unseen, dropped; } sqg_pileup_rows_stat_t;   /* host; may be NULL */

/* device: adds the observed events of the rows of *in to the outputs of *out that are not NULL (sqg_pileup.h's arrays: ADDED TO); returns
 * when the adds are complete.  Every error of sqg_batch_collapse's inputs and every cfg / origin error of sqg_batch_pileup applies; a
 * NULL in->sumsq while sd_sum is wanted is SQG_EINVAL.  An empty batch succeeds and adds nothing; n_rows == 0 adds nothing (every
 * eligible event is unseen). */
int sqg_batch_pileup_rows(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_pileup_cfg_t *cfg, const sqg_pileup_origin_t *origin,
                          const int64_t *row_off, const sqg_collapse_in_t *in, const sqg_pileup_out_t *out, sqg_pileup_rows_stat_t *stat);

#ifdef __cplusplus
}
#endif
#endif
