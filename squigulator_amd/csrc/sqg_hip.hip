// sqg_hip.hip -- MI355X (gfx950) implementation of include/sqg.h, include/sqg_chunks.h, include/sqg_targets.h, include/sqg_segments.h, include/sqg_sites.h, include/sqg_events.h, include/sqg_pileup.h, include/sqg_detect.h, include/sqg_align.h, include/sqg_collapse.h, include/sqg_scale.h, include/sqg_call.h and include/sqg_map.h.
//
// One translation unit: the gfx950 kernels (sqg_kernels.h: k_common.h, k_events.h, k_samples.h, k_sampler.h,
// k_svb.h) and the host side of the C ABI (h_*.h: context/batch management, staging, launches, results).
// No MFMA anywhere: this is an integer-LCG / transcendental / streaming-store path.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see squigulator_amd/build.py).
//
// The product path never touches oracle/: this file is self-contained.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/sqg.h"
#include "../../include/sqg_chunks.h"
#include "../../include/sqg_targets.h"
#include "../../include/sqg_segments.h"
#include "../../include/sqg_sites.h"
#include "../../include/sqg_events.h"
#include "../../include/sqg_pileup.h"
#include "../../include/sqg_detect.h"
#include "../../include/sqg_align.h"
#include "../../include/sqg_collapse.h"
#include "../../include/sqg_scale.h"
#include "../../include/sqg_call.h"
#include "../../include/sqg_map.h"

#include "sqg_kernels.h"

// the host side, in dependency order
#include "h_common.h"     // sqg_ctx, sqg_batch, HIPCHK, host_nrng, prefix constants
#include "h_context.h"    // sqg_create, sqg_destroy, ...
#include "h_stage.h"      // sqg_batch_stage, sqg_batch_free
#include "h_sampler.h"    // sqg_genome_load, sqg_batch_sample, sqg_batch_sample_range, sqg_skip_reads, sqg_fetch_reads
#include "h_run.h"        // sqg_batch_run, sqg_batch_run_begin / _end, sqg_set_range_mode
#include "h_results.h"    // sqg_batch_wait, sqg_fetch_*, sqg_batch_compress, sqg_get_timing, ...
#include "h_blow5.h"      // sqg_blow5_*: the native BLOW5 writer
#include "h_chunks.h"     // sqg_chunk_plan, sqg_batch_chunks (include/sqg_chunks.h)
#include "h_targets.h"    // sqg_batch_chunk_targets (include/sqg_targets.h)
#include "h_segments.h"   // sqg_batch_segments, sqg_chunk_plan_trimmed, sqg_batch_chunks_trimmed, sqg_batch_chunk_targets_trimmed (include/sqg_segments.h)
#include "h_sites.h"      // sqg_site_plan, sqg_batch_sites (include/sqg_sites.h)
#include "h_events_table.h"   // sqg_batch_events (include/sqg_events.h)
#include "h_pileup.h"     // sqg_batch_pileup (include/sqg_pileup.h)
#include "h_detect.h"     // sqg_detect_plan, sqg_batch_detect (include/sqg_detect.h)
#include "h_align.h"      // sqg_batch_align (include/sqg_align.h); align_run, which sqg_batch_align_scaled shares
#include "h_collapse.h"   // sqg_batch_collapse, sqg_batch_pileup_rows (include/sqg_collapse.h)
#include "h_scale.h"      // sqg_batch_scale, sqg_batch_align_scaled (include/sqg_scale.h)
#include "h_call.h"       // sqg_call_plan, sqg_batch_call (include/sqg_call.h)
#include "h_map.h"        // sqg_map_track, sqg_batch_map (include/sqg_map.h)
