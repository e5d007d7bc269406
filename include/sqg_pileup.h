/*
 * sqg_pileup.h -- per-site event statistics of a batch, summed across reads on the device (an addition to sqg_events.h).
 *
 * sqg_events.h's table keeps the reads apart.  The tools it names do not stop there: their first step (m6Anet's dataprep, Nanocompore's
 * eventalign_collapse, xPore's dataprep) collapses the rows ACROSS reads by reference position -- coverage, mean and spread of the
 * event levels, dwell -- and that is what their models are fitted on.  sqg_batch_pileup does the collapse where the rows are made: the
 * events of a run batch are added into caller-owned device arrays that persist from batch to batch, so coverage builds up over a run and
 * no per-event row exists anywhere, on the device or on the host.  Keyed by pore-table row instead of by position the same sums are the
 * pore model re-estimated from the simulated signal (what `nanopolish train` computes), and an SQG_METH context can keep k-mers with and
 * without an 'M' apart: the ground truth of the two populations xPore and Nanocompore infer.
 *
 * HIP backend only, like the events; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * Contexts.  All that sqg_batch_events takes.  Like it, the call needs the batch's device results AND its dwells.
 *
 * Fixed point.  The result is bit-reproducible and independent of the order in which the device meets the events: every sum is an
 * integer sum, every add an integer atomic.  For an event, mean and sd are the floats sqg_batch_events writes for it with the same norm
 * and trim, and
 *     q(x) = (int64_t)rint((double)x * 4096.0)            ties to even; the product is exact in double, so q is one rounding
 * (mean and sd are finite and |x| * 4096 is far below 2^63 in every context: the samples are int16).  All sums are two's-complement and
 * wrap modulo 2^64 (n: modulo 2^32); a square is taken modulo 2^64 as well.  A pileup is exactly numpy's np.add.at over the columns of
 * the event table.  An event with ev_len == 0 has no mean: it adds to n only.
 *
 * Which events count, and their key.
 *   SQG_PILEUP_BY_REF   Let L be the read's own bases (the insert, without the attached prefix of an SQG_PREFIX context) and j the
 *                       index, within the insert, of the first base of an event's k-mer.  The event counts iff it is on chain 0 and
 *                       0 <= j <= L - k: all k bases of its k-mer are insert bases.  That leaves out the stall, adaptor and poly-A
 *                       events and chain 1 (the RNA stall), the last k-1 insert events of an RNA read with SQG_PREFIX, whose k-mers run
 *                       into the poly-A, and all five stand-in events of a read shorter than a k-mer (src/gensig.c:242-245).
 *                       key = key0 + step * j with the read's origin {key0, step}.
 *   SQG_PILEUP_BY_KMER  Every event whose segment (sqg_events.h's seg) has its bit set in cfg->segs counts, stand-in events included
 *                       (segs == 0 means 8: the insert).  key = the event's pore-table row (sqg_events.h's kmer); lo / hi window the
 *                       4^k (SQG_METH: 5^k) rows.
 *   Either way a read whose step is 0 is not counted, and an event whose key lies outside [cfg->lo, cfg->hi) is skipped.
 *
 * Origin.  origin == NULL takes it from the sampler (sqg_batch_sample*): the leftmost forward-strand coordinate of the k-mer in the
 * loaded genome, contigs laid end to end as sqg_genome_load was given them --
 *     '+'   key0 = contig_off[ref_idx] + ref_pos               step = +1
 *     '-'   key0 = contig_off[ref_idx] + ref_pos + rlen - k    step = -1
 * -- the k-mer coordinates --paf-ref reports (t_st = ref_pos_st, t_end = ref_pos_end - k + 1, src/sim.c:583-589), for every sampler
 * mode (DNA, RNA, CDNA, TRUNC, FULL).  A caller's origin replaces it, for staged batches or another coordinate system.  BY_KMER
 * without SQG_PILEUP_SPLIT_STRAND needs no origin: on a batch that was not sampled every read then has step +1.
 *
 * Planes.  S = 2 if SQG_PILEUP_SPLIT_STRAND is set, else 1.  Strand bit s = (step < 0); meth bit m = the event's k-mer has an 'M', a
 * base-5 digit 3 of its rank (src/seq.h:45-60); a bit whose split is not set is 0.  plane = s + S * m, and the event is added to element
 * plane * (hi - lo) + key - lo of every output that is not NULL.  planes = S * (SQG_PILEUP_SPLIT_METH ? 2 : 1).
 *
 * stat.  counted: the events added by this call.  outside: the events that would have counted but for a key outside [lo, hi).
 */
#ifndef SQG_PILEUP_H
#define SQG_PILEUP_H

#include "sqg_events.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SQG_PILEUP_BY_REF        0u   /* key: leftmost forward-strand coordinate of the event's k-mer in the loaded genome */
#define SQG_PILEUP_BY_KMER       1u   /* key: the event's pore-table row (sqg_events.h's kmer)                             */
#define SQG_PILEUP_SPLIT_STRAND  1u   /* a plane per strand                                                                */
#define SQG_PILEUP_SPLIT_METH    2u   /* a plane for k-mers that carry an 'M' (SQG_METH contexts only)                     */

typedef struct {
    uint32_t by, split;      /* SQG_PILEUP_BY_*, OR of SQG_PILEUP_SPLIT_*                                   */
    uint32_t norm;           /* SQG_CHUNK_PA | SQG_CHUNK_MEDMAD: the scale of sqg_events.h's mean / sd      */
    int32_t  trim;           /* as sqg_event_cfg_t.trim                                                     */
    uint32_t segs;           /* BY_KMER: bit q set = count events of segment q (sqg_events.h's seg); 0 = 8  */
    int64_t  lo, hi;         /* the key window [lo, hi): events with a key outside it are skipped           */
} sqg_pileup_cfg_t;

typedef struct {             /* HOST arrays [n_reads]; the whole struct may be NULL = take it from the sampler */
    const int64_t *key0;     /* key of the k-mer at the read's base 0                                       */
    const int8_t  *step;     /* +1: key0 + j.  -1: key0 - j ('-' strand).  0: the read is not counted       */
} sqg_pileup_origin_t;

typedef struct {             /* DEVICE, caller-owned, [planes][hi - lo], ADDED TO, never overwritten; any may be NULL */
    uint32_t *n;             /* events                                                                      */
    int64_t  *dwell;         /* sum of ev_len                                                               */
    int64_t  *dwell_sq;      /* sum of ev_len squared                                                       */
    int64_t  *mean_sum;      /* sum of q(mean)                                                              */
    int64_t  *mean_sq;       /* sum of q(mean) squared                                                      */
    int64_t  *sd_sum;        /* sum of q(sd)                                                                */
} sqg_pileup_out_t;

typedef struct { int64_t counted, outside; } sqg_pileup_stat_t;   /* host; may be NULL */

/* device: adds the batch's events to the outputs of *out that are not NULL; returns when the adds are complete.
 * SQG_EINVAL, sqg_last_error naming the cause: a NULL ctx, batch, cfg or out; an unknown by, split bit or norm; segs bits above 3; a trim
 * that is neither 0 nor 1; hi < lo; SQG_PILEUP_SPLIT_METH on a context without SQG_METH; BY_REF or SQG_PILEUP_SPLIT_STRAND with a NULL
 * origin on a batch that was not sampled; an origin with a NULL member; a step outside {-1, 0, +1}.
 * SQG_ESEQUENCE: the batch has not been run, or it no longer owns its device results and its dwells (sqg.h: until two more batches have
 * been run).  An empty batch or hi == lo succeeds and adds nothing (with hi == lo every event that would count is outside).
 * Works on the context's stream and waits for it; the caller's arrays must not be in use by another stream meanwhile. */
int sqg_batch_pileup(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_pileup_cfg_t *cfg, const sqg_pileup_origin_t *origin,
                     const sqg_pileup_out_t *out, sqg_pileup_stat_t *stat);

#ifdef __cplusplus
}
#endif
#endif
