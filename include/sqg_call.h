/*
 * sqg_call.h -- per-read CpG methylation calls of a batch, scored on the device from event rows (an addition to sqg_scale.h and sqg_pileup.h).
 *
 * The library simulates --meth-freq: reads carry 'M', the pore table has 5^k rows, sqg_batch_sites hands out labelled windows.  It also
 * rebuilds what an event-based tool does to a read: detect, align, calibrate, collapse, pile up.  What such a tool does LAST was missing:
 * nanopolish / f5c call-methylation score, per read and per CpG, the event means over the site's k-mers under the methylated and the
 * unmethylated rows of the pore model -- a log-likelihood ratio per site and read -- and calculate_methylation_frequency sums those
 * into a called frequency per genome position.  sqg_batch_call does both where the rows are: from the true table's sums
 * (sqg_batch_events), from the observed table's (sqg_batch_collapse over detected and aligned rows), under a per-read calibration or
 * without one.  The truth stands next to every result: the label per site, the frequency byte per position.
 *
 * The rule below is the contract.  Everything is exact integer arithmetic (level_raw is sqg_events.h's expression, one value per row).
 *
 * HIP backend only, like every consumer call; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * Contexts.  DNA, without SQG_PREFIX, with SQG_METH.  Anything else returns SQG_EINVAL, and sqg_last_error names the flag.  With or
 * without SQG_IDEAL*.  Lifetime is that of sqg_batch_events: the batch has been run and still owns its device results and its dwells,
 * else SQG_ESEQUENCE.
 *
 * Sites.  Read r has bytes read[0..len) and ne = len - k + 1 events.  A candidate is sqg_sites.h's candidate in an SQG_METH context:
 *   p + 1 < len, read[p+1] == 'G', read[p] is 'C' or 'M'.  Upper case only.  A 'C' that ends one read and a 'G' that begins the next
 *   are no candidate.  Every candidate of a read with len >= k is a site.  A read shorter than a k-mer has no sites.  Sites are numbered
 *   in read order, then by ascending p.  sqg_call_plan returns the per-read offsets and the number of sites.  It does device work plus
 *   a copy-back of the per-read counts, like sqg_site_plan.
 *
 * Span.  The span of a site is the events whose k-mer holds base p: e = max(0, p-k+1) ... min(p, ne-1).  The span is never empty.
 *
 * Hypothesis rows.  For h in {C (digit 1), M (digit 3)} and event e of the span: R_h(e) = sum over i < k of dg(e+i) * 5^(k-1-i).
 *   dg(j) is the base-5 digit that sqg_targets.h's kmer rule gives read[j].  The exceptions depend on cfg.neigh:
 *     SQG_CALL_NEIGH_READ (0)   Only j == p takes h.  The other CpGs in the k-mer stay as the read has them.
 *     SQG_CALL_NEIGH_SAME (1)   Every j in e ... e+k-1 that is a candidate of the read takes h.  Its 'G' may lie at e+k, outside the
 *                               k-mer.  This is nanopolish's all-or-none group, at k-mer scope.
 *
 * Observed value.  x = ev_off[r] + e.  in->sum[x] is int64.  L = in->len64[x] or in->len32[x].  Exactly one of the two pointers is
 *   non-NULL.  The two types exist because collapse's ob_len is int64 while the true table's ev_len is int32.  L < 1: the event is
 *   unobserved and skipped.  Otherwise q0 is sqg_scale.h's q0, with that >> and those clamps (the product 256 * sum modulo 2^64, as
 *   there).  With a scale, q is its q (gain and shift CLAMPED into their ranges, as there).  Without one, q = q0.
 *
 * Term.  Lv = 256 * level_raw(R_h, r), by sqg_events.h's level_raw expression for pore-table row R_h and read r's offset.
 *     d  = clamp(q - Lv, -2^19, 2^19)
 *     W  = clamp(model->w[R_h], 0, 2^24)
 *     Cc = clamp(model->c[R_h], -2^20, 2^20)
 *     t  = min((W * d * d) >> 32, cfg.term_cap), with 64-bit arithmetic throughout
 *     nll_h += Cc + t
 *   model->w and model->c are caller-owned device arrays of int32, [5^k].  They are device memory, which the host cannot refuse, so
 *   they are clamped as sqg_scale.h clamps its inputs.  w is Q24 of 1/(2 sd^2) per code^2 (d is in 1/256 code: d*d carries 2^16, W 2^24,
 *   and >> 32 leaves 2^8).  c is 256 * ln(sd).  Both hypotheses therefore score in 1/256 nat.  term_cap is 0 ... 2^26, so nine terms
 *   fit int32.
 *
 * Per site.  n_obs is the number of events of the span that were used.  nll_c and nll_m are int32, both 0 when n_obs == 0.
 *   llr = nll_c - nll_m.  label = (read[p] == 'M').  site_read and site_pos identify the site.
 *   call: 0 if n_obs < cfg.min_obs or |llr| < cfg.llr_min, with llr_min >= 0.  Otherwise 2 if llr > 0, else 1.
 *
 * Key.  The origin is {key0, step}, as in sqg_pileup.h.  NULL takes the sampler's origin.  A NULL origin on a batch that was not
 *   sampled, while site_key or freq is wanted, is SQG_EINVAL.  The key is the forward-strand coordinate of the C of the CpG:
 *     step = +1: site_key = key0 + p.
 *     step = -1: site_key = key0 + k - 2 - p.
 *   Both strands of one CpG have one key.  It is the index of that CpG's byte in sqg_genome_set_meth's freq.
 *   step = 0: site_key = INT64_MIN, and the site counts as outside.
 *
 * Frequency.  freq holds lo and hi, and four uint32 arrays, [hi - lo], on the device.  They are ADDED TO and persist from batch to
 *   batch.  Integer atomics only.  Any array may be NULL.  A site with key in [lo, hi) adds:
 *     cov += 1      truth += label      called += (call != 0)      meth += (call == 2)
 *
 * Stat (host).  sites; outside: with a freq, the sites whose key is not in [lo, hi) -- those of a read whose step is 0 among them --,
 *   without one 0; called: the sites with call != 0; agree: those of them with (call == 2) == label.
 *
 * SQG_CALL_DEFAULT: the all-or-none group, a term capped at 50 nat, a call at |llr| >= 2 nat from one event on.  These are nanopolish's
 * conventions (its group, its 2.0 threshold of calculate_methylation_frequency), not measured here.
 *
 * The recommended model, made by the binding's call_model() from the context's own pore model and not part of the kernel's rule:
 *     sdc = (double)level_stdv * digitisation / range            the row's standard deviation in ADC codes
 *     w   = clip(rint(2^24 / (2 * sdc * sdc)), 0, 2^24)
 *     c   = clip(rint(256 * ln(sdc)), -2^20, 2^20)
 */
#ifndef SQG_CALL_H
#define SQG_CALL_H

#include "sqg_scale.h"
#include "sqg_pileup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SQG_CALL_NEIGH_READ 0u   /* only the site's own base takes the hypothesis                                   */
#define SQG_CALL_NEIGH_SAME 1u   /* every candidate inside the event's k-mer takes it                               */

typedef struct {
    uint32_t neigh;           /* SQG_CALL_NEIGH_READ | SQG_CALL_NEIGH_SAME                                          */
    int32_t  term_cap;        /* an event's squared term is capped here, 0 .. 1<<26 (1/256 nat)                     */
    int32_t  llr_min;         /* a site with |llr| below this is not called, 0 .. INT32_MAX (1/256 nat)             */
    int32_t  min_obs;         /* nor one with fewer events used than this, 0 .. 1<<20                               */
} sqg_call_cfg_t;

#define SQG_CALL_DEFAULT { SQG_CALL_NEIGH_SAME, 256 * 50, 256 * 2, 1 }

typedef struct {              /* DEVICE memory of the context's device, owned by the caller, [n_events]: one row per row of sqg_batch_events */
    const int64_t *sum;       /* sum of the event's samples (sqg_event_out_t.sum, sqg_collapse_out_t.ob_sum)        */
    const int64_t *len64;     /* their number as int64 (ob_len) ...                                                 */
    const int32_t *len32;     /* ... or as int32 (ev_len): exactly one of the two; a value < 1: unobserved          */
} sqg_call_in_t;

typedef struct {              /* DEVICE, caller-owned, [5^k], values outside their range are clamped                 */
    const int32_t *w;         /* Q24 of 1 / (2 sd^2) per code^2, 0 .. 1<<24                                         */
    const int32_t *c;         /* 256 * ln(sd), -(1<<20) .. 1<<20                                                    */
} sqg_call_model_t;

typedef struct {              /* DEVICE, caller-owned, [n_sites], OVERWRITTEN; any may be NULL = not wanted          */
    int32_t *site_read;       /* read index within the batch                                                        */
    int32_t *site_pos;        /* p, the site's base within its read                                                 */
    uint8_t *label;           /* 1: the read carries 'M' there                                                      */
    int64_t *site_key;        /* forward-strand coordinate of the CpG's C; INT64_MIN: the read's step is 0          */
    int32_t *n_obs;           /* events of the span that were used                                                  */
    int32_t *nll_c;           /* the span's score under C, 1/256 nat                                                */
    int32_t *nll_m;           /* ... and under M                                                                    */
    int32_t *llr;             /* nll_c - nll_m: positive speaks for M                                               */
    uint8_t *call;            /* 0 none, 1 unmethylated, 2 methylated                                               */
} sqg_call_out_t;

typedef struct {              /* the called frequency per position; the whole struct may be NULL = none             */
    int64_t  lo, hi;          /* the key window [lo, hi)                                                            */
    uint32_t *cov;            /* DEVICE, caller-owned, [hi - lo], ADDED TO; any may be NULL: sites                  */
    uint32_t *truth;          /* ... of them with label 1                                                           */
    uint32_t *called;         /* ... with call != 0                                                                 */
    uint32_t *meth;           /* ... with call == 2                                                                 */
} sqg_call_freq_t;

typedef struct { int64_t sites, outside, called, agree; } sqg_call_stat_t;   /* host; may be NULL */

/* site_off [n_reads+1] (host memory, may be NULL): the first site of every read; *n_sites their number.  Device work plus a copy-back
 * of the per-read counts, like sqg_site_plan.  A context that is not DNA with SQG_METH and without SQG_PREFIX, or a NULL n_sites:
 * SQG_EINVAL.  The lifetime rule above: else SQG_ESEQUENCE. */
int sqg_call_plan(sqg_ctx_t *ctx, sqg_batch_t *b, int64_t *site_off, int64_t *n_sites);

/* device: scores every site of the batch, sites numbered as sqg_call_plan numbers them, into the outputs of *out that are not NULL and
 * adds them to *freq; returns when both are complete.  scale NULL: none; origin NULL: the sampler's; freq NULL: none; stat NULL ok.
 * SQG_EINVAL, sqg_last_error naming the field: a NULL ctx, batch, cfg, in, in->sum, model, model->w, model->c or out; both or neither
 * of in->len64 and in->len32; an unknown neigh; term_cap, llr_min or min_obs outside the ranges above; a scale with a NULL gain or
 * shift; freq->hi < freq->lo; an origin with a NULL member or a step outside {-1, 0, +1}; a NULL origin on a batch that was not
 * sampled while site_key or freq is wanted; a context as for sqg_call_plan.  SQG_ESEQUENCE: the lifetime rule above.  An empty batch or
 * a batch without sites succeeds and writes nothing (stat: zeros).  Works on the context's stream and waits for it; the caller's arrays
 * must not be in use by another stream meanwhile. */
int sqg_batch_call(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_call_cfg_t *cfg, const sqg_call_in_t *in, const sqg_call_model_t *model,
                   const sqg_align_scale_t *scale, const sqg_pileup_origin_t *origin,
                   const sqg_call_out_t *out, const sqg_call_freq_t *freq, sqg_call_stat_t *stat);

#ifdef __cplusplus
}
#endif
#endif
