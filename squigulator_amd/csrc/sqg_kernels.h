// sqg_kernels.h -- gfx950 device code of the per-read signal path (included by sqg_hip.hip); the kernels live in
// k_common.h, k_events.h, k_part.h, k_part_events.h, k_samples.h, k_sampler.h, k_svb.h, k_blow5.h, k_chunks.h, k_targets.h, k_segments.h, k_sites.h, k_events_table.h, k_pileup.h, k_detect.h, k_rows.h, k_align.h, k_collapse.h, k_scale.h, k_call.h and k_map.h.
//
//   k_init_rows   per-(worker,k-mer) stream seeds                       (src/sim.c:238-257)
//   k_scan        read lengths -> output offsets
//   k_events      per worker chain: dwell draws (src/gensig.c:254-257), ranks, in-order hand-out of the k-mer streams
//   k_part_*      k > 6, few workers: the stream hand-out over events bucketed by the top bits of the rank (k_part.h)
//   k_samples     per 64-event tile: the samples                       (src/gensig.c:226-356)
//   k_fixup       FP64 recomputation of the samples the certified fp32 path could not decide
//   k_certify     exhaustive error sweep of the fp32 normal-deviate path over all 2^31-2 states
//   k_store_probe int16 streaming-store ceiling
//   k_items       one descriptor per work item of the lean sample kernel
//   k_sample, k_copy_reads   gen_read on the device-resident genome        (src/genread.c:125-370)
//   k_svb_*       slow5lib's svb-zd signal compression                    (slow5lib/src/slow5_press.c:1055-1087)
//   k_blow5_frame BLOW5 records (slow5_rec_to_mem's layout) in stored-block zlib streams (slow5lib/src/slow5.c:3928-4072)
//   k_blow5_huff_* the same records in streams of two dynamic-Huffman blocks (SQG_BLOW5_HUFFMAN; codes built by kh_huff.h)
//   k_chunk_*     per-read median / MAD (or the constants from statistics passed in), normalised fixed-length chunks and their base labels (include/sqg_chunks.h)
//   k_segments    the segments of a read with an attached prefix (stall, adaptor, poly-A, insert) from the dwell sums at its edges, and the insert's
//                 view for the chunk kernels; k_target_shift: the adaptor's level shift where it reaches an insert (include/sqg_segments.h)
//   k_site_*      the CpG sites of every read from the dwell scan, then a normalised window, the bases around it and their places in the window per site (include/sqg_sites.h)
//   k_evtab_*     the per-event table: every event's place, segment, k-mer and level from the dwell scan, then a flat segmented reduction of the int16 signal by event
//                 (sum, sum of squares, min, max; mean / sd in FP64), long events by a whole wavefront (include/sqg_events.h)
//   k_pileup      the same events added across reads into per-key integer sums the caller keeps: scatter-accumulate by no-return integer atomics (include/sqg_pileup.h)
//   k_detect_*    the two-window t-statistic event detector on the stored signal, one read per lane from LDS tiles of 64 reads, then the detected rows'
//                 sums by k_evtab's reduction and the true event under each row's first sample (include/sqg_detect.h)
//   k_align_*     the caller's event rows aligned to the read's true events: a banded dynamic programme, one wavefront per read and one band cell per lane,
//                 the move codes as lane masks, then the traceback over tiles of 64 trace rows (include/sqg_align.h)
//   k_collapse_*, k_pileup_rows   the caller's rows summed per event they are assigned to -- combined within the wavefront by a segmented scan, one
//                 atomic per run -- mean / sd of those sums, and their pileup under k_pileup's rules (include/sqg_collapse.h)
//   k_scale_*     per-read sums of the caller's rows and of the read's targets -- in registers over a wavefront's consecutive trips, one set of integer
//                 atomics per wavefront and read -- and the shift / scale estimate from them in FP64 (include/sqg_scale.h)
//   k_call_*      the CpG sites of every read from 16-byte loads of its bases, ranked by k_chunks.h's scan, then per site the base-5 ranks of its span's
//                 k-mers under C and under M, the two rows' levels against the caller's event sums in exact integers, the call, and the adds to a
//                 called frequency per position by no-return integer atomics (include/sqg_call.h)
//   k_map_*       the genome's expected level track of both strands, then subsequence DTW of every read's first rows against it: a wavefront walks a span of
//                 1024-position tiles, a strip of 16 positions per lane in registers, the rows as wavefront-uniform values, the path's start carried with
//                 the cell instead of a traceback; the spans' ends reduced per read in ascending order (include/sqg_map.h)
//   k_target_*    per-sample targets of those chunks: event starts, clean signal, moves, k-mer rows (include/sqg_targets.h); scan, normalisation and row store are k_chunks.h's
//
// Arithmetic modes.  EXACT: every draw goes through the FP64 restatement of nrng()
// (src/rand.h:87-94).  CERTIFIED: a draw is first evaluated with fp32 hardware transcendentals;
// the result is accepted only if the digitised value provably cannot differ from the FP64 one
// (|frac - 1/2| test against a bound built from the swept error delta_x), and
// is otherwise recomputed in FP64.  Both modes produce identical int16 streams.
#pragma once

#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>


#include "k_common.h"
#include "k_events.h"
#include "k_part.h"
#include "k_part_events.h"
#include "k_samples.h"
#include "k_sampler.h"
#include "k_svb.h"
#include "k_blow5.h"
#include "k_chunks.h"
#include "k_targets.h"
#include "k_segments.h"
#include "k_sites.h"
#include "k_events_table.h"
#include "k_pileup.h"
#include "k_detect.h"
#include "k_rows.h"
#include "k_align.h"
#include "k_collapse.h"
#include "k_scale.h"
#include "k_call.h"
#include "k_map.h"
