/*
 * sqg_detect.h -- the two-window t-statistic event detector on a batch's signal, on the device (an addition to sqg_events.h).
 *
 * sqg_batch_events hands out the truth: the event boundaries the simulator knows exactly.  A user of real reads recovers them only
 * approximately, and the first step of every tool that does so is the event detector of scrappie, which nanopolish, f5c, UNCALLED,
 * Sigmap and RawHash carry with the same five parameters: two sliding t-statistics (a short and a long window) and a peak machine on
 * each.  A raw-signal mapper run on this simulator's output sees the DETECTED table, not the true one; this call makes the detected
 * table on the device, next to the true one, so that the step can be scored (true_ev below).
 *
 * The rule below is the contract.  It is modelled on the scrappie detector with two deliberate changes:
 *   - The window sums are exact integers.  The tools keep running float32 sums, which lose precision along a long read.
 *   - Boundaries are recorded in strictly ascending order.  The tools keep them in emission order.
 * Results are therefore CLOSE to f5c's on the same signal, NOT bit-equal.
 *
 * HIP backend only, like the events; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * Contexts.  All that sqg_batch_events takes.  The detector runs over the STORED samples of a read in stored order, as a tool reading
 * the BLOW5 file would: for RNA that is the reversed array (src/gensig.c:348-354).  Prefix, stall and adaptor samples are included.
 *
 * cfg       w_short, w_long          the two windows, 1 <= w_short < w_long <= 64
 *           thr_short, thr_long      the thresholds a peak of either detector must exceed, finite and >= 0
 *           peak_height              how far a statistic must rise above a minimum to open a peak, and fall below the peak to close
 *                                    it; finite and >= 0
 *           norm, trim               as in sqg_event_cfg_t.  They bear only on mean, sd, med2 and mad4.
 *           SQG_DETECT_DNA is {3, 6, 1.4, 9.0, 0.2} and SQG_DETECT_RNA {7, 14, 2.5, 9.0, 1.0} (the doubles nearest those decimals),
 *           norm and trim, not named by the initialisers, are 0 behind them: SQG_CHUNK_MEDMAD, the whole read.
 *
 * t-statistic.  Per read with stored samples x[0..n), for each window w of the two:
 *   t_w[i] = 0 for i < w or i > n - w.  Otherwise, with S1 the sum of x[i-w .. i), S2 the sum of x[i .. i+w) and Q the sum of x
 *   squared over [i-w, i+w):
 *     N = w (S2 - S1)^2        D = w Q - S1^2 - S2^2        t_w[i] = sqrt((double)N / (double)(D > 0 ? D : 1))
 *   in exact integers up to the two conversions.  D >= 0 always.  With w <= 64, N < 2^51 and D < 2^44, so both conversions are exact;
 *   the division and the square root are IEEE double, one rounding each, as for mean / sd of sqg_events.h.  That is why w_long is
 *   capped at 64.
 *
 * Peak machine.  One machine per detector, k = 0 short and k = 1 long, with state pos = -1, val = +inf, valid = false, masked = 0;
 * the two share last = 0.  W, TH and h are the cfg's windows, thresholds and peak height:
 *
 *   for i in 0 .. n-1:  for k in 0, 1:
 *       if masked[k] >= i: continue
 *       cur = t_{W[k]}[i]
 *       if pos[k] < 0:
 *           if cur < val[k]: val[k] = cur
 *           elif cur - val[k] > h: val[k] = cur; pos[k] = i
 *       else:
 *           if cur > val[k]: val[k] = cur; pos[k] = i
 *           if k == 0 and val[0] > TH[0]: masked[1] = pos[0] + W[0]; pos[1] = -1; val[1] = +inf; valid[1] = false
 *           if val[k] - cur > h and val[k] > TH[k]: valid[k] = true
 *           if valid[k] and i - pos[k] > W[k] / 2:          (integer division)
 *               if pos[k] > last: record boundary pos[k]; last = pos[k]
 *               pos[k] = -1; val[k] = cur; valid[k] = false
 *
 *   All comparisons are strict and in double.  The `pos[k] > last` guard is what keeps the boundaries ascending; a search over several
 *   thousand small random signals and cfgs found no input on which it drops a boundary, so the tests assert the order and do not
 *   claim to exercise the guard.
 *
 * Rows.  Boundaries b_1 < ... < b_m give m + 1 rows per read: [0, b_1), ..., [b_m, n).  A read shorter than 2 w_short samples has one
 * row.  The rows of read r are [det_off[r], det_off[r+1]) of the plan, in ascending order of dt_start.
 *   dt_read    r.
 *   dt_start   the first stored sample of the row within its read.
 *   dt_len     its samples.
 *   sum, sumsq, vmin, vmax, mean, sd
 *              exactly the formulas of sqg_events.h over [dt_start, dt_start + dt_len), with len = dt_len.
 *   true_ev    the row of sqg_batch_events (batch-wide index) whose [ev_start, ev_start + ev_len), with ev_len >= 1, contains the
 *              row's first sample.  torch.unique(true_ev) against n_events scores under-segmentation, repeats of a value
 *              over-segmentation.
 * Per read:
 *   med2, mad4 as in sqg_event_out_t, over the span trim selects.
 */
#ifndef SQG_DETECT_H
#define SQG_DETECT_H

#include "sqg_events.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t  w_short;     /* samples of the short window, 1 .. w_long - 1                                  */
    int32_t  w_long;      /* samples of the long window, w_short + 1 .. 64                                 */
    double   thr_short;   /* threshold of the short detector                                               */
    double   thr_long;    /* threshold of the long detector                                                */
    double   peak_height; /* rise that opens a peak, fall that closes it                                   */
    uint32_t norm;        /* SQG_CHUNK_MEDMAD | SQG_CHUNK_PA: mean, sd                                     */
    int32_t  trim;        /* 0: statistics over the whole read; 1: over its insert (sqg_segments.h)        */
} sqg_detect_cfg_t;

#define SQG_DETECT_DNA { 3,  6, 1.4, 9.0, 0.2 }      /* norm and trim are left 0: SQG_CHUNK_MEDMAD, the whole read */
#define SQG_DETECT_RNA { 7, 14, 2.5, 9.0, 1.0 }

typedef struct {          /* all DEVICE memory of the context's device, owned by the caller, each at its element's natural alignment; any may be NULL = not wanted */
    int32_t  *dt_read;    /* [n_rows] read index within the batch                                          */
    int64_t  *dt_start;   /* [n_rows] first stored sample of the row within its read                       */
    int32_t  *dt_len;     /* [n_rows] samples of the row                                                   */
    int64_t  *sum;        /* [n_rows] sum of the row's int16 samples                                       */
    int64_t  *sumsq;      /* [n_rows] sum of their squares                                                 */
    int16_t  *vmin;       /* [n_rows] the smallest of them                                                 */
    int16_t  *vmax;       /* [n_rows] the largest of them                                                  */
    float    *mean;       /* [n_rows] mean of the row's samples, normalised by cfg->norm                   */
    float    *sd;         /* [n_rows] their standard deviation on the same scale                           */
    int64_t  *true_ev;    /* [n_rows] the row of sqg_batch_events that holds the row's first sample        */
    int32_t  *med2;       /* [n_reads] twice the median of the samples of the span cfg->trim selects       */
    int32_t  *mad4;       /* [n_reads] four times their median absolute deviation                          */
} sqg_detect_out_t;

/* device work and a copy-back of the per-read counts, like sqg_site_plan: det_off (HOST, [n_reads+1], may be NULL) gets the first row
 * of every read, *n_rows their number.  The lifetime rule and the errors of sqg_batch_detect; an empty batch gives det_off[0] = 0 and
 * *n_rows = 0.  A NULL n_rows: SQG_EINVAL. */
int sqg_detect_plan(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_detect_cfg_t *cfg, int64_t *det_off, int64_t *n_rows);

/* device: fills the outputs of *out that are not NULL, the rows numbered as the plan numbers them; returns when they are complete.  The
 * batch must have been run and still own its device results AND its dwells (sqg.h: until two more batches have been run), else
 * SQG_ESEQUENCE.  A NULL ctx, batch, cfg or out, or a cfg field outside the ranges above: SQG_EINVAL, sqg_last_error names the field.
 * An empty batch succeeds and writes nothing.  Works on the context's stream and waits for it. */
int sqg_batch_detect(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_detect_cfg_t *cfg, const sqg_detect_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
