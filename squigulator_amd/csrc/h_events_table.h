// h_events_table.h -- sqg_batch_events: the per-event signal table of a batch, left on the device
// Host side of include/sqg_events.h; included by sqg_hip.hip behind h_sites.h.  The opening of the checks, the batch's view, the lifetime rule and the statistics job are h_chunks.h's.
#pragma once

extern "C" int sqg_batch_events(sqg_ctx_t* c, sqg_batch_t* b, const sqg_event_cfg_t* cfg, const sqg_event_out_t* out) {
    static const char who[] = "sqg_batch_events";
    int rc = check_open(c, b, cfg, "cfg", who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = K.null(out, "out"))) return rc;
    if (!norm_ok(cfg->norm)) return K.bad("unknown norm");
    if (!trim_ok(cfg->trim)) return K.bad("trim must be 0 or 1");
    if ((rc = K.ran(b))) return rc;
    const bool want_rows = out->mean || out->sd;
    const bool want_stats = out->med2 || out->mad4 || (want_rows && cfg->norm == SQG_CHUNK_MEDMAD);
    const bool want_reduce = want_rows || out->sum || out->sumsq || out->vmin || out->vmax;
    const bool want_scan = want_reduce || out->ev_read || out->ev_start || out->ev_len || out->kmer || out->level_raw || out->seg;
    // the statistics job of the reads (trim: of their inserts); without the statistics nothing needs the inserts' spans: the plain job, no
    // k_segments, for either trim
    ChunkJob J;
    if ((rc = spans_open(c, b, who, c->use_dwell_stream, want_stats && cfg->trim == 1, &J)) || J.P.bv.n_reads == 0) return rc;
    const int n = b->n;
    const hipStream_t st = J.st;
    if (want_stats && (rc = stats_run(c, b, J, out->med2, out->mad4))) return rc;
    if (want_scan && b->n_events > 0) {
        EventScratch& X = c->event;
        const size_t ne = (size_t)b->n_events;
        if (want_reduce && !out->ev_start && (rc = X.d_start.need(c, ne))) return rc;
        if (want_reduce && !out->ev_read && (rc = X.d_read.need(c, ne))) return rc;
        EventParams Q{J.P.bv, want_stats ? J.P.consts : (const float2*)nullptr, b->n_events};      // the job's view, the constants; then the columns
        Q.ev_start = out->ev_start ? (long long*)out->ev_start : want_reduce ? X.d_start.p : (long long*)nullptr;
        Q.ev_read = out->ev_read ? out->ev_read : want_reduce ? X.d_read.p : (int*)nullptr;
        Q.ev_len = out->ev_len; Q.kmer = out->kmer; Q.level_raw = out->level_raw; Q.seg = out->seg;
        Q.sum = (long long*)out->sum; Q.sumsq = (long long*)out->sumsq; Q.vmin = out->vmin; Q.vmax = out->vmax; Q.mean = out->mean; Q.sd = out->sd;
        // pass 1, scan: where every event starts, and the columns that need no sample
        hipLaunchKernelGGL(k_evtab_scan, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, Q);
        HIPCHK(c, hipGetLastError());
        if ((rc = dbg_sync(c, "k_evtab_scan"))) return rc;
        // pass 2, reduce: the sums of every event's samples, mean / sd from them
        if (want_reduce) {
            const unsigned wgs = (unsigned)std::min<long long>((b->n_events + CHUNK_WG - 1) / CHUNK_WG, 32LL * c->num_cu);
            dispatch(false, cfg->norm == SQG_CHUNK_PA, [&](auto, auto A) { hipLaunchKernelGGL(k_evtab_reduce<decltype(A)::value>, dim3(wgs), dim3(CHUNK_WG), 0, st, Q); });
            HIPCHK(c, hipGetLastError());
            if ((rc = dbg_sync(c, "k_evtab_reduce"))) return rc;
        }
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}
