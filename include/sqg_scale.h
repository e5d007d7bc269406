/*
 * sqg_scale.h -- a per-read shift and scale estimated from event rows, and the aligner under a per-read scaling (an addition to sqg_align.h).
 *
 * sqg_batch_align compares a row's level with the k-mers' as they stand: it works on rows in the simulator's own units.  A tool does not
 * know a read's calibration.  f5c / nanopolish estimate a per-read shift and scale by the method of moments, align under it, re-estimate
 * both by least squares over the aligned events (recalibrate_model) and align again.  The two calls here are those two steps, on the
 * device: sqg_batch_scale makes either estimate from the caller's rows, sqg_batch_align_scaled is sqg_batch_align under a per-read gain and
 * shift the caller supplies.  The truth of a simulated read is gain 1, shift 0: the estimate a tool would make stands next to it, and the
 * loop "moments -> align -> fit -> align" runs and is scored without a row leaving the device.
 *
 * The rule below is the contract: exact integers for every sum, then doubles with one rounding per written operation, the discipline of
 * sqg_events.h's mean / sd (the library is built without floating-point contraction; double division and square root are correctly
 * rounded on the device).
 *
 * HIP backend only, like every consumer call; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * Contexts.  All that sqg_batch_align takes.  The rows are plain device arrays of the caller's, as there.
 *
 * ---- sqg_batch_scale ----
 *
 * Row value.     y[i] = clamp(floor(16 * sum[i] / max(len[i], 1)), -2^20, 2^20), floor toward minus infinity: the row's level in 1/16 ADC
 *                code.  The product 16 * sum[i] is taken modulo 2^64 (two's complement): it is the true product for |sum| < 2^59.
 * Target value.  x[j] = 16 * level_raw of the read's true event j: sqg_events.h's level_raw, as in sqg_align.h.  The sums below do not
 *                depend on the order of the targets.
 * The unit.      1/16 code, not the aligner's 1/256, so that the sums of squares stay exact in 64 bits: |y|, |x| <= 2^20 makes every sum
 *                exact for a read of fewer than 2^22 rows.  Beyond that the sums wrap modulo 2^64, as in sqg_collapse.h.
 *
 * SQG_SCALE_MOMENTS.  Read r has m = row_off[r+1] - row_off[r] rows and T = ev_off[r+1] - ev_off[r] targets.
 *     n = m,   sy = sum of y,   syy = sum of y * y     over all m rows
 *     nx = T,  sx = sum of x,   sxx = sum of x * x     over all T targets
 *     sxy = 0, rd_dropped = 0.   in->ev is not read.
 * SQG_SCALE_FIT.  Row i of read r COUNTS iff ev_off[r] <= ev[i] < ev_off[r+1]: sqg_collapse.h's rule, -1 and an event of another read
 *     drop the row.  rd_dropped[r] is the number of dropped rows.  Over the rows that count, with x_i = 16 * level_raw[ev[i]]:
 *     n = nx = their number,   sy, syy over y_i,   sx, sxx over x_i,   sxy = sum of x_i * y_i.
 *
 * Derived.  Doubles, one rounding per operation written here; (double) of a 64-bit sum is one rounding to nearest-even.
 *     n == 0 or nx == 0:  gain = 65536, shift = 0.  Otherwise
 *     my = (double)sy / (double)n            mx = (double)sx / (double)nx
 *     vy = (double)syy / (double)n - my * my vx = (double)sxx / (double)nx - mx * mx
 *     MOMENTS:  g = (vy > 0 && vx > 0) ? sqrt(vx / vy) : 1.0
 *     FIT:      cxy = (double)sxy / (double)n - mx * my
 *               g = vy > 0 ? cxy / vy : 1.0
 *     g = min(max(g, 2^-16), 16.0)
 *     s = mx - g * my
 *     gain  = (int32)rint(g * 65536.0)                                  Q16
 *     shift = (int32)min(max(rint(s * 16.0), -2^26), 2^26)              in 1/256 code, the aligner's unit
 *   rint rounds half to even.  The mapping is row -> model: a model value is about g * row + s, so the aligner's costs and
 *   SQG_ALIGN_DEFAULT keep their meaning under sqg_batch_align_scaled.
 *
 * ---- sqg_batch_align_scaled ----
 *
 * sqg_align.h's rule with one change, to the row values:
 *     q0[i] = clamp(floor(256 * sum[i] / max(len[i], 1)), -2^26, 2^26)      (the clamp sqg_batch_align applies too: invisible there, since
 *                                                                            |Lv| <= 2^23 and cost_cap <= 2^24)
 *     q[i]  = clamp(((int64)gain[r] * q0[i] >> 16) + shift[r], -2^26, 2^26)  (>> is an arithmetic shift: a floor)
 *   gain[r] must lie in 1 .. 2^20 and shift[r] in -2^26 .. 2^26.  The two arrays are device memory, which the host cannot refuse: a value
 *   outside its range is CLAMPED into it by the kernel.  That is undefined behaviour of neither arithmetic nor memory.
 *   With gain = 65536 and shift = 0 for every read every output is bit-equal to sqg_batch_align's.
 */
#ifndef SQG_SCALE_H
#define SQG_SCALE_H

#include "sqg_align.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SQG_SCALE_MOMENTS 0u   /* rows against ALL targets of the read, no assignment needed            */
#define SQG_SCALE_FIT     1u   /* least squares of target on row over the rows in->ev assigns           */

typedef struct {
    uint32_t mode;           /* SQG_SCALE_MOMENTS | SQG_SCALE_FIT                                        */
} sqg_scale_cfg_t;

typedef struct {             /* DEVICE memory of the context's device, owned by the caller, [n_rows], each at its element's natural alignment */
    const int64_t *sum;      /* sum of the row's samples                                                 */
    const int32_t *len;      /* samples of the row; a value < 1 is taken as 1                            */
    const int64_t *ev;       /* FIT only: the row of sqg_batch_events each row is assigned to (al_ev, true_ev, or the caller's own) */
} sqg_scale_in_t;

typedef struct {             /* DEVICE, caller-owned, [n_reads], OVERWRITTEN; any may be NULL = not wanted  */
    int64_t *n, *nx;         /* rows and targets the sums run over                                       */
    int64_t *sy, *syy;       /* sum of y, of y * y                                                       */
    int64_t *sx, *sxx;       /* sum of x, of x * x                                                       */
    int64_t *sxy;            /* sum of x * y (FIT; MOMENTS: 0)                                           */
    int32_t *gain, *shift;   /* the estimate: Q16, and 1/256 code                                        */
    int32_t *rd_dropped;     /* rows of the read that were dropped (FIT; MOMENTS: 0)                     */
} sqg_scale_out_t;

typedef struct {             /* DEVICE memory of the context's device, owned by the caller, [n_reads]     */
    const int32_t *gain;     /* Q16, 1 .. 1<<20 (clamped)                                                */
    const int32_t *shift;    /* 1/256 code, -(1<<26) .. 1<<26 (clamped)                                  */
} sqg_align_scale_t;

/* device: the sums and the estimate of every read of the batch from the rows [row_off[r], row_off[r+1]) of *in, into the outputs of *out
 * that are not NULL; returns when they are complete.  n_rows = row_off[n_reads]; row_off is HOST memory, [n_reads+1].  The lifetime rule
 * of sqg_batch_align: the batch must have been run and still own its device results AND its dwells, else SQG_ESEQUENCE.  A NULL ctx,
 * batch, cfg, row_off, in, in->sum, in->len or out; an unknown mode; SQG_SCALE_FIT with a NULL in->ev; a row_off that does not start at 0
 * or is not non-decreasing, or a read of 2^31 rows or more: SQG_EINVAL, sqg_last_error names the field.  An empty batch succeeds and
 * writes nothing; n_rows == 0 on a batch that is not empty reads no target either: it writes 0 to every sum and to rd_dropped (nx, sx and
 * sxx included), gain = 65536 and shift = 0.  Works on the context's stream and waits for it. */
int sqg_batch_scale(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_scale_cfg_t *cfg, const int64_t *row_off,
                    const sqg_scale_in_t *in, const sqg_scale_out_t *out);

/* device: sqg_batch_align under the per-read scaling of *scale.  Every argument, error and lifetime rule of sqg_batch_align; a NULL scale,
 * scale->gain or scale->shift is SQG_EINVAL as well.  An empty batch succeeds and writes nothing. */
int sqg_batch_align_scaled(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_align_cfg_t *cfg, const int64_t *row_off,
                           const sqg_align_in_t *in, const sqg_align_scale_t *scale, const sqg_align_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
