/*
 * sqg_align.h -- banded alignment of event rows to the k-mer events of their read, on the device (an addition to sqg_detect.h).
 *
 * sqg_batch_events hands out the table the simulator knows exactly, sqg_batch_detect the table a tool's event detector finds in the
 * stored samples.  The step every such tool takes next -- f5c / nanopolish eventalign, UNCALLED4, the resquiggle in front of m6Anet,
 * xPore and Nanocompore -- assigns each detected row to a k-mer of the read's sequence.  This call makes that assignment on the device
 * with a banded dynamic programme over (row, true event), so that an aligner's row-to-k-mer assignment can be compared with the truth
 * the simulator holds (sqg_detect_out_t.true_ev).  It is NOT f5c's aligner: no scaling is estimated (the simulator's is known; sqg_scale.h has the estimate and this call under one), the
 * score is an absolute difference of levels, not a log-probability, and every number is an exact integer.
 *
 * The rule below is the contract: exact integers throughout, no floating point.
 *
 * HIP backend only, like the detector; a header of its own for the same reason.  SQG_ABI_VERSION is unchanged.
 *
 * Contexts.  All that sqg_batch_events takes: DNA and RNA, with SQG_PREFIX or without, SQG_METH, constant dwell.  The rows are plain
 * device arrays of the caller's: the detector's (sum, dt_len, det_off), the true table's own (sum, ev_len in stored order, ev_off), or
 * any other segmentation of the reads.  The batch is read only through what sqg_batch_events provides.
 *
 * cfg       stay_pen   added when a row stays on the target of the row before it, 0 .. 1<<24
 *           skip_pen   added per target skipped, 0 .. 1<<24
 *           cost_cap   a cell's cost is capped here, 1 .. 1<<24
 *
 * Targets.  Read r has m = row_off[r+1] - row_off[r] rows and T = ev_off[r+1] - ev_off[r] true events.  Its targets j = 0 .. T-1 are
 *   its true events in stored-sample order: for DNA target j is event ev_off[r] + j, for RNA event ev_off[r+1] - 1 - j -- the order
 *   in which sqg_events.h's ev_start ascends.  Lv[j] = 256 * level_raw of that event: sqg_events.h's level_raw, which is not lowered
 *   in the RNA adaptor's level-shift range.  An event without samples is a target like any other; the skip move passes over it.
 *
 * Row values.  q[i] = floor(256 * sum[i] / max(len[i], 1)), floor toward minus infinity.  The product needs no more than 64 bits for
 *   |sum| < 2^55.  A larger |sum| is undefined behaviour of the arithmetic only, never of memory: the call still writes every output
 *   it is asked for and nothing else.
 *
 * Cell cost.  c(i,j) = min(|q[i] - Lv[j]|, cost_cap).
 *
 * Band.  SQG_ALIGN_BAND = 64 cells wide, moving with the path.  Row i covers the targets [lo_i, lo_i + 64), lo_0 = 0.  A cell with
 *   j >= T, and every cell of the previous row outside that row's band, is INF = 2^62.  After row i, a_i is the lowest j of the band at
 *   which D[i][j] is smallest (lo_i if the whole row is INF), and
 *     lo_{i+1} = lo_i + min(2, max(0, a_i - lo_i - 31)).
 *
 * Recurrence.
 *   Row 0:      D[0][j] = c(0,j) + j * skip_pen, move code 3.
 *   Row i >= 1: three candidates, in this order:
 *                 step  D[i-1][j-1]              code 0
 *                 stay  D[i-1][j]   + stay_pen   code 1
 *                 skip  D[i-1][j-2] + skip_pen   code 2
 *               the FIRST candidate with the smallest value wins, and D[i][j] is that value plus c(i,j).  If all three are at least
 *               INF the cell is INF with code 3.
 *   With m < 2^31 and the cfg ranges above D stays below 2^58.
 *
 * End and traceback.  e is the lowest j of the last row's band at which D[m-1][j] + (T-1-j) * skip_pen is smallest over the finite
 *   cells; al_cost[r] is that value.  The traceback starts at j_{m-1} = e and sets j_{i-1} = j_i - {1, 0, 2}[code of cell (i, j_i)].
 *   al_ev[row_off[r] + i]   the event index (batch-wide: a row of sqg_batch_events) of target j_i.
 *   al_edge[r]              the rows with j_i == lo_i + 63, or with j_i == lo_i and lo_i > 0: the path on the moving band's rim.
 *   m == 0: nothing is written for the read's rows, al_cost[r] = -1 and al_edge[r] = 0.
 *   T == 0, or no finite cell in the last row: every al_ev of the read is -1, al_cost[r] = -1 and al_edge[r] = 0.
 *
 * Limit.  A row moves at most two targets, and the band at most two targets per row.  A read segmented so coarsely that three or more
 *   true events fall into most rows loses the path.  al_cost shows it (every target that no row visits is charged skip_pen, and rows
 *   off their targets cost up to cost_cap each), and al_edge where the lost path is pushed to the band's rim.
 *
 * SQG_ALIGN_DEFAULT is the triple with the highest share of al_ev == true_ev on 32768 sampled 10-kb reads (dna-r10-prom) detected
 * under SQG_DETECT_DNA, among stay_pen, skip_pen in {0, 256, 1024, 4096} and cost_cap in {4096, 16384, 65536}: profiles/align.md.
 */
#ifndef SQG_ALIGN_H
#define SQG_ALIGN_H

#include "sqg_detect.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t stay_pen;     /* added when a row stays on the k-mer of the row before it, 0 .. 1<<24          */
    int32_t skip_pen;     /* added per k-mer event skipped, 0 .. 1<<24                                     */
    int32_t cost_cap;     /* a cell's cost is capped here, 1 .. 1<<24                                      */
} sqg_align_cfg_t;

#define SQG_ALIGN_BAND 64
#define SQG_ALIGN_DEFAULT { 4096, 4096, 65536 }

typedef struct {          /* DEVICE memory of the context's device, owned by the caller, each at its element's natural alignment */
    const int64_t *sum;   /* [n_rows] sum of each row's samples (sqg_detect_out_t.sum, or sqg_event_out_t.sum)  */
    const int32_t *len;   /* [n_rows] samples of each row (dt_len / ev_len); a value < 1 is taken as 1          */
} sqg_align_in_t;

typedef struct {          /* DEVICE memory of the context's device, owned by the caller; any may be NULL = not wanted */
    int64_t *al_ev;       /* [n_rows]  the row of sqg_batch_events (batch-wide index) the row is aligned to, -1: none */
    int64_t *al_cost;     /* [n_reads] the cost of the read's best path, -1: none                          */
    int32_t *al_edge;     /* [n_reads] rows whose cell lies on the moving band's rim                       */
} sqg_align_out_t;

/* device: aligns the rows [row_off[r], row_off[r+1]) of in->sum / in->len to the true events of read r, for every read of the batch, and
 * fills the outputs of *out that are not NULL; returns when they are complete.  n_rows = row_off[n_reads]; nothing outside
 * [row_off[0], row_off[n_reads]) of al_ev is written.  row_off is HOST memory, [n_reads+1]: det_off of sqg_detect_plan, or ev_off.
 * The lifetime rule of sqg_batch_events: the batch must have been run and still own its device results AND its dwells, else
 * SQG_ESEQUENCE.  A NULL ctx, batch, cfg, row_off, in, in->sum, in->len or out, a cfg field outside the ranges above, a row_off that
 * does not start at 0 or is not non-decreasing, or a read of 2^31 rows or more: SQG_EINVAL, sqg_last_error names the field.  An empty
 * batch succeeds and writes nothing.  Works on the context's stream and waits for it. */
int sqg_batch_align(sqg_ctx_t *ctx, sqg_batch_t *b, const sqg_align_cfg_t *cfg, const int64_t *row_off,
                    const sqg_align_in_t *in, const sqg_align_out_t *out);

#ifdef __cplusplus
}
#endif
#endif
