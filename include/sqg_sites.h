/*
 * sqg_sites.h -- CpG-centred signal windows of a batch with their methylation labels, made on the device (an addition to sqg_chunks.h).
 *
 * A trainer of a modified-base model does not want a CTC chunk.  It wants one short window of signal around every candidate site, the
 * label of that site, the bases around it, and where each of those bases sits in the window: the shape of a Remora-style training
 * set, and the reason to simulate --meth-freq at all.  The simulator knows all of it exactly from what is on the device once a batch
 * has run: the reads' bytes (which carry 'M' where methylate_dna, src/genread.c:207-241, methylated a CpG), the per-event dwells, the
 * signal and the reads' offsets.  The outputs are caller-owned device arrays, so nothing crosses to the host but the plan.
 *
 * HIP backend only, like the chunks; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * Contexts.  DNA without an attached prefix.  SQG_RNA or SQG_PREFIX: SQG_EINVAL -- the reference methylates only in gen_read_dna, and
 * windows over the inserts of prefixed reads belong on top of sqg_segments.h's view of a read: a later addition.  With SQG_METH or
 * without: without it every label is 0, a canonical control set.  With SQG_IDEAL_TIME / SQG_IDEAL or without: there every dwell is
 * (int)dwell_mean, as in sqg_chunks.h.
 *
 * cfg       win_len      L, samples per window: a multiple of 8 in 16 .. 65536
 *           before       samples of the window in front of the anchor event's first sample: 0 .. L-1
 *           focus        f, the position of the site's base inside the anchor event's k-mer: 0 .. k-1
 *           ctx_len      B, bases per context row: 0 .. 255
 *           ctx_before   cb, bases of the row in front of the site: 0 .. B-1, and 0 when B = 0
 *           dtype, norm  as in sqg_chunk_cfg_t
 *
 * Per read r with bytes read[0..len), ne = len - k + 1 events, dwells d[], E their exclusive prefix sum, and n = sum of d stored samples
 * raw[0..n) (DNA: stored order is generation order):
 *   candidate   a base position p with p + 1 < len, read[p+1] == 'G', and read[p] == 'C' or -- in an SQG_METH context only -- 'M'.
 *               Upper case only: lower-case and IUPAC letters are no sites, as meth_code (src/seq.h:45-60) treats them; without
 *               SQG_METH an 'M' is the letter the kernels take for A, and no site.  Reads are separate: a 'C' that ends one and a
 *               'G' that begins the next are no candidate.
 *   anchor      the candidate's anchor event is a = p - f: the event in whose k-mer the site's base sits at position f.
 *   window      the samples [w0, w0 + L) of the read with w0 = E[a] - before.
 *   site        a candidate is a site if and only if 0 <= a < ne and 0 <= w0 and w0 + L <= n.  Every other candidate is dropped, as
 *               sqg_chunk_plan drops a tail.  A read shorter than a k-mer (src/gensig.c:242-245) has no sites, as it has no chunks.
 *   numbering   sites are numbered in read order, then by ascending p.
 *
 * out       signal     [n_sites][L] of dtype: raw[w0 + t] through sqg_chunks.h's MEDMAD / PA formula and F16 / F32 conversion with the
 *                      statistics of the WHOLE read -- the bits sqg_batch_chunks writes for that sample.
 *           label      [n_sites] 1 if and only if read[p] == 'M', else 0.
 *           site_read  [n_sites] r.            site_pos  [n_sites] p.            win_start  [n_sites] w0.
 *           context    [n_sites][B]: entry i is the label code of sqg_chunks.h (1 .. 4; 'M' -> 5 under SQG_METH) of read[p - cb + i],
 *                      0 where that position is outside the read.
 *           ctx_start  [n_sites][B+1]: entry i is min(max(X(p - cb + i - f) - w0, 0), L) with X(e) = 0 for e <= 0, n for e >= ne and
 *                      E[e] otherwise.  Context base i owns the window samples [ctx_start[i], ctx_start[i+1]): those of the event in
 *                      whose k-mer it sits at position f.  It follows that ctx_start[cb] == before.
 *           med2, mad4 [n_reads] as in sqg_chunk_out_t, written for every read.
 */
#ifndef SQG_SITES_H
#define SQG_SITES_H

#include "sqg_chunks.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t  win_len;     /* L: samples per window, 16 .. 65536, a multiple of 8                         */
    int32_t  before;      /* samples of the window in front of the anchor event's first sample, 0 .. L-1 */
    int32_t  focus;       /* f: position of the site's base in the anchor event's k-mer, 0 .. k-1        */
    int32_t  ctx_len;     /* B: bases per context row, 0 .. 255                                          */
    int32_t  ctx_before;  /* cb: bases of the row in front of the site, 0 .. B-1 (0 when B = 0)          */
    uint32_t dtype;       /* SQG_CHUNK_F16 | SQG_CHUNK_F32                                               */
    uint32_t norm;        /* SQG_CHUNK_MEDMAD | SQG_CHUNK_PA                                             */
} sqg_site_cfg_t;

typedef struct {          /* all DEVICE memory of the context's device, owned by the caller; any may be NULL = not wanted */
    void    *signal;      /* [n_sites][L] of dtype, row s at element s*L (16-byte aligned)  */
    uint8_t *label;       /* [n_sites] 1: the site's base is 'M'                            */
    int32_t *site_read;   /* [n_sites] read index within the batch                          */
    int32_t *site_pos;    /* [n_sites] p, the site's base within its read                   */
    int64_t *win_start;   /* [n_sites] w0, first sample of the window within its read       */
    uint8_t *context;     /* [n_sites][B] label codes around the site, 0 = outside the read */
    int32_t *ctx_start;   /* [n_sites][B+1] where each context base's samples start in the window */
    int32_t *med2;        /* [n_reads] twice the median of the read's int16 samples         */
    int32_t *mad4;        /* [n_reads] four times their median absolute deviation           */
} sqg_site_out_t;

/* site_off [n_reads+1] (host memory, may be NULL): the first site of every read; *n_sites their number.  Device work -- the sites
 * follow from the dwells -- plus a copy-back of the per-read counts, like sqg_chunk_plan_trimmed.  Only win_len, before and focus of
 * cfg bear on the plan; all of cfg is validated.  The batch must have been run and still own its device results AND its dwells (sqg.h:
 * until two more batches have been run), else SQG_ESEQUENCE.  A bad cfg or a NULL n_sites: SQG_EINVAL, sqg_last_error says which. */
int sqg_site_plan(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_site_cfg_t *cfg, int64_t *site_off, int64_t *n_sites);
/* device: fills *out, sites numbered as sqg_site_plan numbers them; returns when everything in *out is complete.  The lifetime rule
 * above holds.  A bad cfg, a NULL out or a signal that is not 16-byte aligned: SQG_EINVAL, sqg_last_error says which.  An empty batch
 * or a batch without sites succeeds and writes nothing but med2 / mad4.  Works on the context's stream and waits for it. */
int sqg_batch_sites(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_site_cfg_t *cfg, const sqg_site_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
