// h_events_table.h -- sqg_batch_events: the per-event signal table of a batch, left on the device
// Host side of include/sqg_events.h; included by sqg_hip.hip behind h_sites.h.  The lifetime rule, the job and the statistics pass are h_chunks.h's.
#pragma once

// what the kernels of k_events_table.h take of a run batch, all but the columns: sqg_batch_events and sqg_batch_pileup (h_pileup.h)
static EventParams evtab_params(const sqg_ctx* c, const sqg_batch* b, const float2* consts) {
    const bool prefix = (c->cfg.flags & SQG_PREFIX) != 0, rna = (c->cfg.flags & SQG_RNA) != 0;
    EventParams Q{};
    Q.reads = (const ReadDesc*)b->d_reads; Q.bases = (const uint8_t*)b->d_bases; Q.model = c->d_model;
    Q.dwell = c->use_dwell_stream ? (const uint16_t*)c->cset[b->cset].d_dwell : (const uint16_t*)nullptr;
    Q.sig_off = c->slot[b->slot].d_sigoff; Q.sig = c->slot[b->slot].d_sig; Q.consts = consts;
    Q.const_sps = (int)c->cfg.profile.dwell_mean; Q.k = c->k; Q.meth = (c->cfg.flags & SQG_METH) ? 1 : 0; Q.rna = rna ? 1 : 0; Q.n_reads = b->n;
    Q.kind = !prefix ? SEG_NONE : rna ? SEG_RNA : SEG_DNA;
    if (Q.kind == SEG_DNA) { Q.p0 = (int)strlen(kStallDna); Q.p1 = Q.p0 + (int)strlen(kAdaptorDna); }
    if (Q.kind == SEG_RNA) { Q.p0 = kPolyA; Q.p1 = kPolyA + (int)strlen(kAdaptorRna); }
    Q.n_events = b->n_events; Q.range = c->cfg.profile.range; Q.dig = c->cfg.profile.digitisation;
    return Q;
}

extern "C" int sqg_batch_events(sqg_ctx_t* c, sqg_batch_t* b, const sqg_event_cfg_t* cfg, const sqg_event_out_t* out) {
    static const char who[] = "sqg_batch_events";
    if (!c) return SQG_EINVAL;
    auto bad = [&](const char* what) { c->err = std::string(who) + ": " + what; return SQG_EINVAL; };
    if (!b || !cfg) return bad("batch and cfg must not be NULL");
    if (!out) return bad("out must not be NULL");
    if (cfg->norm != SQG_CHUNK_MEDMAD && cfg->norm != SQG_CHUNK_PA) return bad("unknown norm");
    if (cfg->trim != 0 && cfg->trim != 1) return bad("trim must be 0 or 1");
    if (!b->ran) { c->err = std::string(who) + ": the batch has not been run"; return SQG_ESEQUENCE; }
    // the chunk job of the reads (trim: of their inserts), one chunk each at the most: its spans, parameters and scratch are what the
    // statistics pass takes
    sqg_chunk_cfg_t cf{};
    cf.chunk_len = 64; cf.stride = INT32_MAX; cf.max_label = 0; cf.dtype = SQG_CHUNK_F32; cf.norm = cfg->norm;
    const bool want_rows = out->mean || out->sd;
    const bool want_stats = out->med2 || out->mad4 || (want_rows && cfg->norm == SQG_CHUNK_MEDMAD);
    const bool want_reduce = want_rows || out->sum || out->sumsq || out->vmin || out->vmax;
    const bool want_scan = want_reduce || out->ev_read || out->ev_start || out->ev_len || out->kmer || out->level_raw || out->seg;
    int rc;
    ChunkJob J;
    // (without the statistics nothing needs the inserts' spans: the plain job, no k_segments, for either trim)
    if ((rc = chunk_begin(c, b, &cf, who, c->use_dwell_stream, &J, want_stats && cfg->trim == 1)) || J.P.n_reads == 0) return rc;
    const int n = b->n;
    const hipStream_t st = J.st;
    if (want_stats) {
        if ((rc = chunk_upload(c, &J))) return rc;
        J.P.med2 = out->med2; J.P.mad4 = out->mad4;
        if ((rc = chunk_stats_run(c, b, J))) return rc;
    }
    if (want_scan && b->n_events > 0) {
        EventScratch& X = c->event;
        const size_t ne = (size_t)b->n_events;
        if (want_reduce && !out->ev_start && (rc = ensure(c, (void**)&X.d_start, &X.start_cap, ne, sizeof(long long)))) return rc;
        if (want_reduce && !out->ev_read && (rc = ensure(c, (void**)&X.d_read, &X.read_cap, ne, sizeof(int)))) return rc;
        EventParams Q = evtab_params(c, b, want_stats ? J.P.consts : (const float2*)nullptr);
        Q.ev_start = out->ev_start ? (long long*)out->ev_start : want_reduce ? X.d_start : (long long*)nullptr;
        Q.ev_read = out->ev_read ? out->ev_read : want_reduce ? X.d_read : (int*)nullptr;
        Q.ev_len = out->ev_len; Q.kmer = out->kmer; Q.level_raw = out->level_raw; Q.seg = out->seg;
        Q.sum = (long long*)out->sum; Q.sumsq = (long long*)out->sumsq; Q.vmin = out->vmin; Q.vmax = out->vmax; Q.mean = out->mean; Q.sd = out->sd;
        // pass 1, scan: where every event starts, and the columns that need no sample
        hipLaunchKernelGGL(k_evtab_scan, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, Q);
        HIPCHK(c, hipGetLastError());
        if ((rc = dbg_sync(c, "k_evtab_scan"))) return rc;
        // pass 2, reduce: the sums of every event's samples, mean / sd from them
        if (want_reduce) {
            const unsigned wgs = (unsigned)std::min<long long>((b->n_events + CHUNK_WG - 1) / CHUNK_WG, 32LL * c->num_cu);
            if (cfg->norm == SQG_CHUNK_PA) hipLaunchKernelGGL(k_evtab_reduce<true>, dim3(wgs), dim3(CHUNK_WG), 0, st, Q);
            else hipLaunchKernelGGL(k_evtab_reduce<false>, dim3(wgs), dim3(CHUNK_WG), 0, st, Q);
            HIPCHK(c, hipGetLastError());
            if ((rc = dbg_sync(c, "k_evtab_reduce"))) return rc;
        }
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}
