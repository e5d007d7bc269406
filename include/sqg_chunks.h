/*
 * sqg_chunks.h -- labelled, normalised signal chunks of a batch, made on the device (an addition to sqg.h).
 *
 * What a trainer of a basecaller or signal model builds from a BLOW5 file on the CPU: fixed-length windows of every
 * read's raw signal, normalised per read, and for every window the bases that were in the pore while it was recorded
 * (the CTC target) -- which a simulator knows exactly: they follow from the per-event dwells (aln->ss,
 * src/gensig.c:273-281) the library keeps on the device.  Everything stays in HBM: the outputs are caller-owned device
 * arrays (e.g. torch tensors), so a consumer on the same GPU takes the samples at the rate they are generated.
 *
 * These entry points live in a header of their own: sqg.h is the surface every backend implements, and there is no CPU
 * implementation of this one.  SQG_ABI_VERSION is unchanged.
 *
 * Per read i with n = sig_off[i+1] - sig_off[i] samples raw[0..n) as stored (RNA: already reversed, src/gensig.c:348-354):
 *   chunks      c_i = (n - L) / S + 1 if n >= L, else 0; chunk j covers stored samples [jS, jS + L); the tail is dropped.
 *               Chunks are numbered in read order, then by j.  A read shorter than a k-mer (src/gensig.c:242-245) has none.
 *   statistics  over all n samples: s = raw sorted, med2 = s[(n-1)/2] + s[n/2]; d = |2 raw - med2| sorted,
 *               mad4 = d[(n-1)/2] + d[n/2] (n = 0: both 0).  Exact integers, written for every read.
 *   MEDMAD      med = med2 / 2, mad' = mad4 / 4 (1 if mad4 = 0), inv = (float)(1.0 / (1.4826 * mad')) in double arithmetic,
 *               x = ((float)raw - (float)med) * inv: an exact difference and one float product.
 *   PA          x = (float)(((double)raw + offset) * range / digitisation), the three double operations in that order.
 *   F16         x rounded to nearest even, subnormals kept.
 *   labels      E[e] = first sample of event e in generation order (exclusive prefix sum of the read's dwells; with
 *               --ideal / --ideal-time e * (int)dwell_mean).  The chunk covers generation-order samples [g0, g1): DNA
 *               [jS, jS + L), RNA [n - jS - L, n - jS).  Its events are those with g0 <= E[e] < g1, a contiguous range
 *               [e0, e1); its bases are read[e] for them (the first base of the event's k-mer) in the order the signal shows
 *               them: ascending e for DNA, descending for RNA.  label_len = e1 - e0; the first min(label_len, W) codes go
 *               into the row, the rest of the row is 0.  Codes: rank 0/1/2/3 of src/seq.h:14-27 -> 1/2/3/4 (A C G T/U, the
 *               IUPAC letters as the kernels treat them, anything else 1); in an SQG_METH context 'M' -> 5.
 */
#ifndef SQG_CHUNKS_H
#define SQG_CHUNKS_H

#include "sqg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SQG_CHUNK_F16     0u      /* IEEE binary16 */
#define SQG_CHUNK_F32     1u
#define SQG_CHUNK_MEDMAD  0u      /* (raw - median) / (1.4826 * MAD), per read */
#define SQG_CHUNK_PA      1u      /* picoamperes: (raw + offset) * range / digitisation */

typedef struct {
    int32_t  chunk_len;   /* L: samples per chunk, 64 .. 1<<20, a multiple of 8            */
    int32_t  stride;      /* S: distance between chunk starts, >= 1 (S > L leaves gaps)    */
    int32_t  max_label;   /* W: width of a label row, 0 .. 65535; 0: no labels are written */
    uint32_t dtype;       /* SQG_CHUNK_F16 | SQG_CHUNK_F32                                 */
    uint32_t norm;        /* SQG_CHUNK_MEDMAD | SQG_CHUNK_PA                               */
} sqg_chunk_cfg_t;

typedef struct {          /* all DEVICE memory of the context's device, owned by the caller; any may be NULL = not wanted */
    void    *signal;      /* [n_chunks][L] of dtype, row c at element c*L (16-byte aligned) */
    uint8_t *labels;      /* [n_chunks][W], 0 = padding                                    */
    int32_t *label_len;   /* [n_chunks] bases belonging to the chunk (may exceed W)        */
    int32_t *chunk_read;  /* [n_chunks] read index within the batch                        */
    int64_t *chunk_start; /* [n_chunks] first sample of the chunk within its read          */
    int32_t *med2;        /* [n_reads] twice the median of the read's int16 samples        */
    int32_t *mad4;        /* [n_reads] four times their median absolute deviation          */
} sqg_chunk_out_t;

/* host only, no device work: chunk_off [n_reads+1] (may be NULL) and *n_chunks from the batch's sig_off.  Waits for the batch. */
int sqg_chunk_plan(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_chunk_cfg_t *cfg, int64_t *chunk_off, int64_t *n_chunks);
/* device: fills *out for a batch that has been run; returns when everything in *out is complete.  The batch must still own its
 * device results (sqg.h: until two more batches have been run), else SQG_ESEQUENCE.  Not for SQG_PREFIX contexts (SQG_EINVAL):
 * adaptor, poly-A and stall have no base labels; sqg_segments.h finds them and chunks the insert.  Works on the context's stream and waits for it. */
int sqg_batch_chunks(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_chunk_cfg_t *cfg, const sqg_chunk_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
