/*
 * sqg_events.h -- the per-event signal table of a batch, made on the device (an addition to sqg_segments.h).
 *
 * The four other views of a run batch -- chunks, per-sample targets, segments, CpG windows -- are shaped for networks that eat raw
 * samples.  The other large family of nanopore signal consumers takes no samples at all: one row per k-mer event with where the event
 * starts, how long it dwells, and the mean and spread of the current -- the eventalign / resquiggle table m6Anet, xPore, Nanocompore
 * and Remora's per-base metrics are trained and validated on.  A user of real reads gets it by basecalling, mapping and running an
 * event aligner, which recovers approximately the boundaries a simulator knows exactly.  Everything needed is on the device once a
 * batch has run: the per-event dwells, the reads' bytes, the pore table, the reads' offsets and the signal.  The outputs are
 * caller-owned device arrays, so nothing crosses to the host.
 *
 * HIP backend only, like the chunks; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * Contexts.  All of them: DNA and RNA; with SQG_PREFIX or without (the RNA stall chain and the five stand-in events of a read shorter
 * than a k-mer, src/gensig.c:242-245, included); with SQG_METH or without; with SQG_IDEAL_TIME / SQG_IDEAL or without.  No plan call:
 * the table has exactly one row per event of the batch in the order of the dwells (aln->ss, sqg_fetch_dwell) -- sqg_result_t.n_events
 * rows, those of read r being [ev_off[r], ev_off[r+1]), which the host has.
 *
 * cfg       norm   SQG_CHUNK_MEDMAD | SQG_CHUNK_PA, as in sqg_chunk_cfg_t
 *           trim   0: med2 / mad4 and the MEDMAD constants are taken over the whole read.  1: over the read's insert, the stored
 *                  samples [seg[3], seg[4]) of sqg_segments.h, as the trimmed chunk calls take them.  The rows are all events either
 *                  way.  On a context without SQG_PREFIX both give the same bytes.
 *
 * Per read r with n stored samples raw[0..n) (RNA: stored reversed, src/gensig.c:348-354): its events e = 0 .. ne0 + ne1 - 1 are chain
 * 0's events, then chain 1's (the RNA stall of an SQG_PREFIX context: sqg_segments.h); d[e] their dwells (each (int)dwell_mean in a
 * constant-dwell context); E their exclusive prefix sum over both chains, in generation order.  Row ev_off[r] + e:
 *   ev_read    r.
 *   ev_start   the first stored sample of the event within its read.  DNA: E[e].  RNA: n - E[e] - d[e].  The rows of a read tile [0, n)
 *              without gap or overlap: ascending for DNA, descending for RNA.
 *   ev_len     d[e].
 *   sum, sumsq the sum of raw and of raw squared over the event's stored samples [ev_start, ev_start + ev_len): exact integers.
 *   vmin, vmax the smallest and the largest of them.
 *   kmer       the pore-table row of the event's k-mer within its own chain: sqg_targets.h's kmer rule (base-5 digits in an SQG_METH
 *              context) on the chain's bases.  Chain 0 is the read with its attached prefix, or the stand-in sequence of a read
 *              shorter than a k-mer.
 *   level_raw  sqg_targets.h's clean_raw for that k-mer and the read's offset.  It is NOT lowered in the RNA adaptor's level-shift
 *              range, which follows no event boundary: sqg_batch_segments' shift says which stored samples the generator lowered, and
 *              sqg_segments.h by how much.
 *   seg        0 stall, 1 adaptor, 2 poly-A, 3 insert: the event ranges of sqg_segments.h -- an event belongs to the segment of the
 *              FIRST base of its k-mer; chain 1 is stall.  Without SQG_PREFIX every event is 3, and so is every event of a read shorter
 *              than a k-mer.  The ev_len of a segment's events sum to the difference of sqg_batch_segments' seg bounds.
 *   mean, sd   from sum, sumsq and len = ev_len in double arithmetic, one rounding per operation (no fused multiply-add), then one
 *              conversion to float:
 *                m = (double)sum / (double)len
 *                v = ((double)sumsq - (double)sum * m) / (double)len;  v = v < 0 ? 0 : v;  s = sqrt(v)
 *                PA       mean = (float)(((m + offset) * range) / digitisation)      sd = (float)((s * range) / digitisation)
 *                MEDMAD   mean = (float)((m - med2 * 0.5) * (double)inv)             sd = (float)(s * (double)inv)
 *              with inv the float of sqg_chunks.h and med2 / mad4 over the span trim selects.
 * Per read:
 *   med2, mad4 as in sqg_chunk_out_t, over the span trim selects.  Written for every read whenever asked for.
 */
#ifndef SQG_EVENTS_H
#define SQG_EVENTS_H

#include "sqg_segments.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t norm;        /* SQG_CHUNK_MEDMAD | SQG_CHUNK_PA                                               */
    int32_t  trim;        /* 0: statistics over the whole read; 1: over its insert (sqg_segments.h)        */
} sqg_event_cfg_t;

typedef struct {          /* all DEVICE memory of the context's device, owned by the caller, each at its element's natural alignment; any may be NULL = not wanted */
    int32_t  *ev_read;    /* [n_events] read index within the batch                                        */
    int64_t  *ev_start;   /* [n_events] first stored sample of the event within its read                   */
    int32_t  *ev_len;     /* [n_events] samples of the event: its dwell                                    */
    int64_t  *sum;        /* [n_events] sum of the event's int16 samples                                   */
    int64_t  *sumsq;      /* [n_events] sum of their squares                                               */
    int16_t  *vmin;       /* [n_events] the smallest of them                                               */
    int16_t  *vmax;       /* [n_events] the largest of them                                                */
    uint32_t *kmer;       /* [n_events] pore-table row (k-mer rank) of the event within its chain          */
    int16_t  *level_raw;  /* [n_events] the noise-free ADC code of that k-mer (no level shift)             */
    uint8_t  *seg;        /* [n_events] 0 stall, 1 adaptor, 2 poly-A, 3 insert                             */
    float    *mean;       /* [n_events] mean of the event's samples, normalised by cfg->norm               */
    float    *sd;         /* [n_events] their standard deviation on the same scale                         */
    int32_t  *med2;       /* [n_reads] twice the median of the samples of the span cfg->trim selects       */
    int32_t  *mad4;       /* [n_reads] four times their median absolute deviation                          */
} sqg_event_out_t;

/* device: fills the outputs of *out that are not NULL; returns when they are complete.  The batch must have been run and still own its
 * device results AND its dwells (sqg.h: until two more batches have been run), else SQG_ESEQUENCE.  A NULL ctx, batch, cfg or out, an
 * unknown norm or a trim that is neither 0 nor 1: SQG_EINVAL, sqg_last_error says which.  An empty batch succeeds and writes nothing.
 * Works on the context's stream and waits for it. */
int sqg_batch_events(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_event_cfg_t *cfg, const sqg_event_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
