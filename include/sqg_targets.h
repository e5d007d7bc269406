/*
 * sqg_targets.h -- per-sample training targets for the chunks of a batch, made on the device (an addition to sqg_chunks.h).
 *
 * sqg_batch_chunks gives a trainer the noisy signal windows and their bases.  A simulator knows two more things about every
 * sample, and both are standard targets: where each event starts (a move table, the segmentation target) and the noise-free
 * signal under the noisy one (the pore-model level of the k-mer in the pore, digitised like the real sample: the target of a
 * denoiser or a k-mer-level model).  The clean signal is what the reference writes for the same seeded run with --ideal-amp
 * (src/gensig.c:264-270): the dwell, offset and sampler streams move identically, only the k-mer noise streams are left alone.
 * Everything needed is on the device once a batch has run -- the per-event dwells, the reads, the pore table, the reads'
 * offsets -- and the outputs are caller-owned device arrays, so nothing crosses to the host.
 *
 * HIP backend only, like the chunks; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * cfg is sqg_chunks.h's struct, validated the same way; max_label is ignored.  Chunks are numbered as sqg_chunk_plan numbers
 * them.  Per read i with n stored samples, chunk j, sample t in [0, L):
 *   event       the stored index is p = jS + t, the generation-order index g = p (DNA) or g = n - 1 - p (RNA).  The sample's event
 *               e is the one with E[e] <= g < E[e] + dwell[e]; E as in sqg_chunks.h (exclusive prefix sum of the read's dwells, each
 *               at least 1: src/gensig.c:255-256; with --ideal / --ideal-time e * (int)dwell_mean).
 *   kmer        the pore-table row of read[e .. e+k): 2 bits per base (src/seq.h:31-42), base-5 digits in an SQG_METH context
 *               (src/seq.h:62-74).
 *   clean_raw   (int16)((double)model[kmer].level_mean * digitisation / range - offset_i): the operations and the conversion of
 *               src/gensig.c:270 (a value outside int32 becomes INT32_MIN before the low half is taken, as on x86-64).
 *   moves       1 if and only if g == E[e], else 0.  For RNA that is the LAST stored sample of the event.  A row of moves sums to
 *               the chunk's label_len on both strands.
 *   clean       sqg_chunks.h's MEDMAD / PA formula and F16 / F32 conversion applied to clean_raw, with the statistics of the NOISY
 *               read (med2, mad4 over raw[0..n)): clean and noisy are on one scale.  med and inv are derived from med2 / mad4 as
 *               that header says, whether the arrays are passed in or computed by this call: the same bits either way.
 */
#ifndef SQG_TARGETS_H
#define SQG_TARGETS_H

#include "sqg_chunks.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {            /* DEVICE memory, caller-owned; any output may be NULL = not wanted */
    void          *clean;     /* [n_chunks][L] of cfg->dtype, 16-byte aligned: clean_raw normalised by cfg->norm       */
    int16_t       *clean_raw; /* [n_chunks][L], 16-byte aligned: the noise-free ADC code of every sample               */
    uint8_t       *moves;     /* [n_chunks][L], 8-byte aligned: 1 where an event starts, else 0                        */
    uint32_t      *kmer;      /* [n_chunks][L], 16-byte aligned: pore-table row (k-mer rank) of the sample's event     */
    const int32_t *med2;      /* INPUT [n_reads], optional: the arrays an earlier sqg_batch_chunks wrote for this      */
    const int32_t *mad4;      /*   batch; both or neither (else SQG_EINVAL). NULL: computed here when clean+MEDMAD     */
} sqg_chunk_targets_t;

/* device: fills the outputs of *tg that are not NULL for a batch that has been run; returns when they are complete.  The batch must
 * still own its device results AND its dwells (sqg.h: until two more batches have been run), else SQG_ESEQUENCE.  Not for SQG_PREFIX
 * contexts (SQG_EINVAL).  A read shorter than a k-mer has no chunks.  Works on the context's stream and waits for it. */
int sqg_batch_chunk_targets(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_chunk_cfg_t *cfg, const sqg_chunk_targets_t *tg);

#ifdef __cplusplus
}
#endif
#endif
