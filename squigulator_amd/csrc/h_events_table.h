// h_events_table.h -- sqg_batch_events: the per-event signal table of a batch, left on the device
// Host side of include/sqg_events.h; included by sqg_hip.hip behind h_sites.h.  The opening of the checks, the batch's view, the lifetime rule and the statistics job are h_chunks.h's.
// What the calls with a row pass over events share is stated here once: the scan pass (evtab_scan_run, evtab_targets), the flat grid's size
// (flat_grid) and the six columns of sums among a call's outputs (evtab_outputs).  h_pileup.h, h_detect.h, h_align.h, h_collapse.h, h_scale.h.
#pragma once

enum : unsigned { EVC_START = 1, EVC_READ = 2, EVC_KMER = 4, EVC_SEG = 8, EVC_LEVEL = 16 };      // k_evtab_scan's columns that a later pass may need

// Pass 1 of every call that needs a column of the event table: k_evtab_scan on the context's stream, one workgroup per read.  Q holds the
// view, the number of events (not 0) and the caller's own columns, null where there are none; `need` names the columns the passes behind
// this one read, and those of them the caller did not give are pointed at the context's scratch.  Nothing is kept from call to call: the
// scan writes every column it is given, so every call rewrites all that it then reads, whoever used the scratch before.
static int evtab_scan_run(sqg_ctx* c, EventParams& Q, unsigned need) {
    EventScratch& X = c->event;
    const size_t ne = (size_t)Q.n_events;
    int rc = SQG_OK;
    const auto col = [&](unsigned bit, auto*& p, auto& buf) {
        if (!(need & bit) || p || rc) return;
        if (!(rc = buf.need(c, ne))) p = buf.p;
    };
    col(EVC_START, Q.ev_start, X.d_start); col(EVC_READ, Q.ev_read, X.d_read); col(EVC_KMER, Q.kmer, X.d_kmer);
    col(EVC_SEG, Q.seg, X.d_seg); col(EVC_LEVEL, Q.level_raw, X.d_level);
    if (rc) return rc;
    const void* const cols[5] = {Q.ev_start, Q.ev_read, Q.kmer, Q.seg, Q.level_raw};                 // (in the order of the EVC_ bits)
    for (int q = 0; q < 5; q++)                                                                      // no kernel is handed a null column it will read
        if ((need >> q & 1u) && !cols[q]) { c->err = "k_evtab_scan: a column a later pass reads has no memory"; return SQG_EDEVICE; }
    hipLaunchKernelGGL(k_evtab_scan, dim3((unsigned)Q.bv.n_reads), dim3(CHUNK_WG), 0, c->stream, Q);
    return launched(c, "k_evtab_scan");
}

// the targets of sqg_batch_align and sqg_batch_scale: every true event's level_raw, the scan pass with that column alone; null without events
static int evtab_targets(sqg_ctx* c, const BatchView& bv, long long n_events, const int16_t** level_raw) {
    EventParams Q{bv, (const float2*)nullptr, n_events};
    const int rc = n_events > 0 ? evtab_scan_run(c, Q, EVC_LEVEL) : SQG_OK;
    *level_raw = Q.level_raw;
    return rc;
}

// workgroups of a flat grid over n_rows rows, one row per lane (k_events_table.h: evtab_for_rows): one trip where the device holds them all
static unsigned flat_grid(const sqg_ctx* c, long long n_rows) {
    return (unsigned)std::min<long long>((n_rows + CHUNK_WG - 1) / CHUNK_WG, 32LL * c->num_cu);
}

// What a table call's outputs (sqg_event_out_t, sqg_detect_out_t: the names agree) ask for: sum .. sd go into Q as they are; `sums`: one
// of the six is wanted, `stats`: the statistics pass has to run, for med2 / mad4 or for the constants of MEDMAD rows
struct EventWants { bool sums, stats; };
template <class Out>
static EventWants evtab_outputs(EventParams& Q, const Out* out, uint32_t norm) {
    Q.sum = (long long*)out->sum; Q.sumsq = (long long*)out->sumsq; Q.vmin = out->vmin; Q.vmax = out->vmax; Q.mean = out->mean; Q.sd = out->sd;
    return {Q.sum || Q.sumsq || Q.vmin || Q.vmax || Q.mean || Q.sd, out->med2 || out->mad4 || ((Q.mean || Q.sd) && norm == SQG_CHUNK_MEDMAD)};
}

extern "C" int sqg_batch_events(sqg_ctx_t* c, sqg_batch_t* b, const sqg_event_cfg_t* cfg, const sqg_event_out_t* out) {
    static const char who[] = "sqg_batch_events";
    int rc = check_open(c, b, cfg, "cfg", who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = K.null(out, "out"))) return rc;
    if (!norm_ok(cfg->norm)) return K.bad("unknown norm");
    if (!trim_ok(cfg->trim)) return K.bad("trim must be 0 or 1");
    if ((rc = K.ran(b))) return rc;
    EventParams Q{};
    const EventWants want = evtab_outputs(Q, out, cfg->norm);
    const bool want_scan = want.sums || out->ev_read || out->ev_start || out->ev_len || out->kmer || out->level_raw || out->seg;
    // the statistics job of the reads (trim: of their inserts); without the statistics nothing needs the inserts' spans: the plain job, no
    // k_segments, for either trim
    ChunkJob J;
    if ((rc = spans_open(c, b, who, c->use_dwell_stream, want.stats && cfg->trim == 1, &J)) || J.P.bv.n_reads == 0) return rc;
    const hipStream_t st = J.st;
    if (want.stats && (rc = stats_run(c, b, J, out->med2, out->mad4))) return rc;
    if (want_scan && b->n_events > 0) {
        Q.bv = J.P.bv; Q.consts = want.stats ? J.P.consts : (const float2*)nullptr; Q.n_events = b->n_events;      // the job's view, the constants; then the columns
        Q.ev_start = (long long*)out->ev_start; Q.ev_read = out->ev_read; Q.ev_len = out->ev_len; Q.kmer = out->kmer; Q.level_raw = out->level_raw; Q.seg = out->seg;
        // pass 1, scan: where every event starts, and the columns that need no sample; the reduce pass finds an event's samples through ev_start and ev_read
        if ((rc = evtab_scan_run(c, Q, want.sums ? EVC_START | EVC_READ : 0))) return rc;
        // pass 2, reduce: the sums of every event's samples, mean / sd from them
        if (want.sums) {
            dispatch(false, cfg->norm == SQG_CHUNK_PA, [&](auto, auto A) { hipLaunchKernelGGL(k_evtab_reduce<decltype(A)::value>, dim3(flat_grid(c, b->n_events)), dim3(CHUNK_WG), 0, st, Q); });
            if ((rc = launched(c, "k_evtab_reduce"))) return rc;
        }
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}
