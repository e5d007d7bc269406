/*
 * sqg_segments.h -- the segments of reads with an attached prefix, and chunks of their inserts (an addition to sqg_targets.h).
 *
 * With SQG_PREFIX a read's signal has the shape of a real one: stall, adaptor, (RNA) poly-A tail, then the insert.  Adaptor, poly-A
 * and stall have no base labels, which is why sqg_batch_chunks and sqg_batch_chunk_targets refuse such a context.  A trainer does
 * with a real read what this header does: find the segments, cut them off, chunk the insert.  The simulator knows the boundaries
 * exactly -- they follow from the per-event dwells the library keeps on the device -- and they are a training target in their own
 * right (adaptor trimmers, poly-A length estimators).
 *
 * HIP backend only, like the chunks; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * Definitions.  attach_prefix (src/genread.c:95-123) makes chain 0, the read with its prefix: DNA stall (24 bases) + adaptor (61) +
 * read; RNA read + poly-A (158) + adaptor (79).  gen_sig_core (src/gensig.c:326-335) generates chain 0 and then, for RNA,
 * gen_prefix_rna (src/genread.c:71-93) generates chain 1, the stall (30 bases), behind it; the RNA signal is stored reversed
 * (src/gensig.c:348-354): stored index p = n - 1 - g for generation-order index g.  Per read with n stored samples: d[] the dwells
 * of chain 0's ne0 events, E their exclusive prefix sum, n0 their sum; chain 1 has ne1 events and n - n0 samples; len the bases of
 * the read itself (chain 0's bases - 85 for DNA, - 237 for RNA).  An event belongs to the segment of the FIRST base of its k-mer,
 * the convention of the labels (sqg_chunks.h).
 *
 *   seg[5]      the four segments in stored order -- stall, adaptor, poly-A, insert: segment q covers stored samples [seg[q], seg[q+1]),
 *               0 = seg[0] <= seg[1] <= seg[2] <= seg[3] <= seg[4] = n.
 *                 DNA with SQG_PREFIX   a = min(24, ne0), b = min(85, ne0): stall events [0, a), adaptor [a, b), insert [b, ne0), no
 *                                       poly-A: {0, E[a], E[b], E[b], n}.  (len < k: the adaptor loses events, the insert has none.)
 *                 RNA with SQG_PREFIX   insert events [0, i1), i1 = min(len, ne0); poly-A [i1, i2), i2 = min(len + 158, ne0); adaptor
 *                                       [i2, ne0); the stall is chain 1.  g1 = E[i1], g2 = E[i2]: {0, n - n0, n - g2, n - g1, n}.
 *                 no SQG_PREFIX         the whole read is insert: {0, 0, 0, 0, n}.
 *               A read whose chain 0 is shorter than a k-mer has no real events (src/gensig.c:242-245): {0, 0, 0, 0, n}, shift {0, 0},
 *               no chunks, as in sqg_chunks.h.  (Only without SQG_PREFIX: an attached chain has at least 85 bases.)
 *   shift[2]    the stored-order range [shift[0], shift[1]) of the samples gen_prefix_rna lowered by (int16)(30 digitisation / range)
 *               (src/genread.c:79-86): generation-order samples [max(0, n0 - 79 (int)dwell_mean), n0), so {n - n0, n - max(0, n0 -
 *               79 (int)dwell_mean)}; {0, 0} in every other kind of context.  The range follows no event boundary: it is 79 mean
 *               dwells long, whatever the adaptor's 79 - k + 1 events drew, so it ends a few events inside the poly-A or short of
 *               it.  A consumer that wants the clean level of those samples needs it.
 *
 * Trimmed calls.  Every rule of sqg_chunks.h and sqg_targets.h with "the read" replaced by its insert: n is seg[4] - seg[3], raw[] the
 * stored samples [seg[3], seg[4]), the events the insert's events, the bases the read's own; E counts from the insert's first
 * generation-order sample; chunk_start is relative to the insert (seg[3] + chunk_start is the position in the read); med2 / mad4 are
 * taken over the insert's samples only -- what a trainer has after trimming.  kmer is the pore-table row of the k-mer as it was in the
 * pore: the last k-1 insert events of an RNA read reach into the poly-A.  clean_raw follows src/gensig.c:270 and, where the sample
 * lies in the shift range, is then lowered by the int16 shift with int16 wrap-around (src/genread.c:83-86); clean is made from that.
 * The range reaches the insert only if the 229-odd poly-A and adaptor events together draw fewer than 79 (int)dwell_mean samples:
 * no input seen so far does (each dwell is at least 1 and about dwell_mean on average), but the rule is applied.
 * On a context without SQG_PREFIX the three trimmed calls produce the bytes of the plain ones.
 */
#ifndef SQG_SEGMENTS_H
#define SQG_SEGMENTS_H

#include "sqg_targets.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {          /* DEVICE memory of the context's device, owned by the caller; either may be NULL = not wanted */
    int64_t *seg;         /* [n_reads][5] stored-sample bounds of stall, adaptor, poly-A, insert, relative to the read */
    int64_t *shift;       /* [n_reads][2] stored-sample range of the RNA adaptor's level shift                         */
} sqg_segments_t;

/* device: fills *out for a batch that has been run (else SQG_ESEQUENCE); returns when it is complete.  The batch must still own its
 * device results AND its dwells (sqg.h: until two more batches have been run), else SQG_ESEQUENCE.  Any context, with SQG_PREFIX or
 * without.  Works on the context's stream and waits for it. */
int sqg_batch_segments(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_segments_t *out);
/* sqg_chunk_plan over the inserts.  Unlike it, device work: the spans come from the dwells, 2 n_reads integers are copied back.  The
 * lifetime rule above holds; cfg is validated as by sqg_chunk_plan, SQG_PREFIX allowed. */
int sqg_chunk_plan_trimmed(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_chunk_cfg_t *cfg, int64_t *chunk_off, int64_t *n_chunks);
/* sqg_batch_chunks / sqg_batch_chunk_targets over the inserts: chunks numbered as sqg_chunk_plan_trimmed numbers them, arguments
 * validated as by the plain calls, SQG_PREFIX allowed; the lifetime rule above holds for both. */
int sqg_batch_chunks_trimmed(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_chunk_cfg_t *cfg, const sqg_chunk_out_t *out);
int sqg_batch_chunk_targets_trimmed(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_chunk_cfg_t *cfg, const sqg_chunk_targets_t *tg);

#ifdef __cplusplus
}
#endif
#endif
