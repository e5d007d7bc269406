// h_pileup.h -- sqg_batch_pileup: the events of a batch added across reads into the caller's per-key sums, on the device
// Host side of include/sqg_pileup.h; included by sqg_hip.hip behind h_events_table.h.  The lifetime rule, the job and the statistics pass are
// h_chunks.h's, the scan pass and its parameters h_events_table.h's.
#pragma once

extern "C" int sqg_batch_pileup(sqg_ctx_t* c, sqg_batch_t* b, const sqg_pileup_cfg_t* cfg, const sqg_pileup_origin_t* origin,
                                const sqg_pileup_out_t* out, sqg_pileup_stat_t* stat) {
    static const char who[] = "sqg_batch_pileup";
    if (!c) return SQG_EINVAL;
    auto bad = [&](const char* what) { c->err = std::string(who) + ": " + what; return SQG_EINVAL; };
    if (!b || !cfg) return bad("batch and cfg must not be NULL");
    if (!out) return bad("out must not be NULL");
    if (cfg->by != SQG_PILEUP_BY_REF && cfg->by != SQG_PILEUP_BY_KMER) return bad("unknown by");
    if (cfg->split & ~(SQG_PILEUP_SPLIT_STRAND | SQG_PILEUP_SPLIT_METH)) return bad("unknown split bits");
    if (cfg->norm != SQG_CHUNK_MEDMAD && cfg->norm != SQG_CHUNK_PA) return bad("unknown norm");
    if (cfg->trim != 0 && cfg->trim != 1) return bad("trim must be 0 or 1");
    if (cfg->segs & ~15u) return bad("segs has bits above 3");
    if (cfg->hi < cfg->lo) return bad("hi must not be below lo");
    const bool by_kmer = cfg->by == SQG_PILEUP_BY_KMER, split_strand = cfg->split & SQG_PILEUP_SPLIT_STRAND, split_meth = cfg->split & SQG_PILEUP_SPLIT_METH;
    if (split_meth && !(c->cfg.flags & SQG_METH)) return bad("SQG_PILEUP_SPLIT_METH needs a context created with SQG_METH");
    const bool sampled = !b->s_seq_off.empty();
    if (origin && (!origin->key0 || !origin->step)) return bad("origin: key0 and step must not be NULL");
    if (!origin && !sampled && (!by_kmer || split_strand)) return bad("origin must not be NULL: the batch was not sampled");
    const int n = b->n;
    if (origin)
        for (int i = 0; i < n; i++)
            if (origin->step[i] < -1 || origin->step[i] > 1) return bad("origin: step must be -1, 0 or +1");
    if (stat) { stat->counted = 0; stat->outside = 0; }
    if (!b->ran) { c->err = std::string(who) + ": the batch has not been run"; return SQG_ESEQUENCE; }
    // the chunk job as sqg_batch_events opens it: the statistics for MEDMAD, the inserts' spans for trim
    sqg_chunk_cfg_t cf{};
    cf.chunk_len = 64; cf.stride = INT32_MAX; cf.max_label = 0; cf.dtype = SQG_CHUNK_F32; cf.norm = cfg->norm;
    const bool want_samples = out->mean_sum || out->mean_sq || out->sd_sum;
    const bool want_stats = want_samples && cfg->norm == SQG_CHUNK_MEDMAD;
    int rc;
    ChunkJob J;
    if ((rc = chunk_begin(c, b, &cf, who, c->use_dwell_stream, &J, want_stats && cfg->trim == 1)) || J.P.n_reads == 0 || b->n_events == 0) return rc;
    const hipStream_t st = J.st;
    if (want_stats) {
        if ((rc = chunk_upload(c, &J))) return rc;
        J.P.med2 = nullptr; J.P.mad4 = nullptr;
        if ((rc = chunk_stats_run(c, b, J))) return rc;
    }
    EventScratch& X = c->event;
    PileupScratch& Y = c->pileup;
    const size_t ne = (size_t)b->n_events;
    const bool want_kmer = by_kmer || split_meth;
    if ((rc = ensure(c, (void**)&X.d_start, &X.start_cap, ne, sizeof(long long)))) return rc;
    if ((rc = ensure(c, (void**)&X.d_read, &X.read_cap, ne, sizeof(int)))) return rc;
    if (want_kmer && (rc = ensure(c, (void**)&Y.d_kmer, &Y.kmer_cap, ne, sizeof(uint32_t)))) return rc;
    if (by_kmer && (rc = ensure(c, (void**)&Y.d_seg, &Y.seg_cap, ne, sizeof(uint8_t)))) return rc;
    if ((rc = ensure(c, (void**)&Y.d_pr, &Y.pr_cap, (size_t)n, sizeof(PileRead)))) return rc;
    if ((rc = ensure(c, (void**)&Y.d_stat, &Y.stat_cap, 2, sizeof(unsigned long long)))) return rc;
    // every read's origin and insert: L from its events (ne0 = attached length - k + 1), 0 for a stand-in read
    const bool prefix = (c->cfg.flags & SQG_PREFIX) != 0, rna = (c->cfg.flags & SQG_RNA) != 0;
    const long long extra = !prefix ? 0 : rna ? kPolyA + (long long)strlen(kAdaptorRna) : (long long)(strlen(kStallDna) + strlen(kAdaptorDna));
    const long long ne1 = (prefix && rna) ? (long long)strlen(kStallRna) - c->k + 1 : 0;
    Y.h_pr.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        PileRead& p = Y.h_pr[(size_t)i];
        const bool stand_in = (size_t)i < b->short_read.size() && b->short_read[(size_t)i];
        const long long ne0 = b->ev_off[(size_t)i + 1] - b->ev_off[(size_t)i] - ne1;
        p.first = (prefix && !rna) ? (int)extra : 0;
        p.L = stand_in ? 0 : (int)(ne0 + c->k - 1 - extra);
        if (origin) { p.key0 = origin->key0[i]; p.step = origin->step[i]; }
        else if (sampled) {
            const bool minus = b->s_strand[(size_t)i] == '-';
            p.key0 = c->h_contig_off[(size_t)b->s_ref_idx[(size_t)i]] + b->s_ref_pos[(size_t)i] + (minus ? (long long)b->s_rlen[(size_t)i] - c->k : 0);
            p.step = minus ? -1 : 1;
        } else { p.key0 = 0; p.step = 1; }
    }
    HIPCHK(c, hipMemcpyAsync(Y.d_pr, Y.h_pr.data(), (size_t)n * sizeof(PileRead), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(Y.d_stat, 0, 2 * sizeof(unsigned long long), st));
    EventParams Q = evtab_params(c, b, want_stats ? J.P.consts : (const float2*)nullptr);
    Q.ev_start = X.d_start; Q.ev_read = X.d_read;
    Q.kmer = want_kmer ? Y.d_kmer : (uint32_t*)nullptr; Q.seg = by_kmer ? Y.d_seg : (uint8_t*)nullptr;
    // pass 1, scan (k_events_table.h): where every event starts, its read, and k-mer / segment where the key or a split needs them
    hipLaunchKernelGGL(k_evtab_scan, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, Q);
    HIPCHK(c, hipGetLastError());
    if ((rc = dbg_sync(c, "k_evtab_scan"))) return rc;
    // pass 2: the samples of the events that count, their mean / sd, the adds
    PileupParams U{};
    U.pr = Y.d_pr; U.kmer = Q.kmer; U.seg = Q.seg;
    U.by_kmer = by_kmer ? 1 : 0; U.split_strand = split_strand ? 1 : 0; U.split_meth = split_meth ? 1 : 0; U.k = c->k;
    U.segs = cfg->segs ? cfg->segs : 8u; U.lo = cfg->lo; U.hi = cfg->hi;
    U.n = out->n; U.dwell = (long long*)out->dwell; U.dwell_sq = (long long*)out->dwell_sq;
    U.mean_sum = (long long*)out->mean_sum; U.mean_sq = (long long*)out->mean_sq; U.sd_sum = (long long*)out->sd_sum;
    U.stat = Y.d_stat;
    const unsigned wgs = (unsigned)std::min<long long>((b->n_events + CHUNK_WG - 1) / CHUNK_WG, 32LL * c->num_cu);
    if (cfg->norm == SQG_CHUNK_PA) hipLaunchKernelGGL(k_pileup<true>, dim3(wgs), dim3(CHUNK_WG), 0, st, Q, U);
    else hipLaunchKernelGGL(k_pileup<false>, dim3(wgs), dim3(CHUNK_WG), 0, st, Q, U);
    HIPCHK(c, hipGetLastError());
    if ((rc = dbg_sync(c, "k_pileup"))) return rc;
    unsigned long long h_stat[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h_stat, Y.d_stat, sizeof h_stat, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (stat) { stat->counted = (int64_t)h_stat[0]; stat->outside = (int64_t)h_stat[1]; }
    return SQG_OK;
}
