// h_pileup.h -- sqg_batch_pileup: the events of a batch added across reads into the caller's per-key sums, on the device
// Host side of include/sqg_pileup.h; included by sqg_hip.hip behind h_events_table.h.  The opening of the checks, the batch's view, the lifetime
// rule and the statistics job are h_chunks.h's, the scan pass and its parameters h_events_table.h's.  The cfg / origin checks (pileup_check),
// the reads' table (pileup_reads) and the kernels' parameters (pileup_params) are stated here once: sqg_batch_pileup_rows (h_collapse.h) uses them.
#pragma once

// The cfg / origin checks of include/sqg_pileup.h, behind the call's own NULL checks: sqg_batch_pileup and sqg_batch_pileup_rows (h_collapse.h)
static int pileup_check(const Check& K, sqg_ctx* c, const sqg_batch* b, const sqg_pileup_cfg_t* cfg, const sqg_pileup_origin_t* origin) {
    if (cfg->by != SQG_PILEUP_BY_REF && cfg->by != SQG_PILEUP_BY_KMER) return K.bad("unknown by");
    if (cfg->split & ~(SQG_PILEUP_SPLIT_STRAND | SQG_PILEUP_SPLIT_METH)) return K.bad("unknown split bits");
    if (!norm_ok(cfg->norm)) return K.bad("unknown norm");
    if (!trim_ok(cfg->trim)) return K.bad("trim must be 0 or 1");
    if (cfg->segs & ~15u) return K.bad("segs has bits above 3");
    if (cfg->hi < cfg->lo) return K.bad("hi must not be below lo");
    const bool by_kmer = cfg->by == SQG_PILEUP_BY_KMER, split_strand = cfg->split & SQG_PILEUP_SPLIT_STRAND, split_meth = cfg->split & SQG_PILEUP_SPLIT_METH;
    if (split_meth && !(c->cfg.flags & SQG_METH)) return K.bad("SQG_PILEUP_SPLIT_METH needs a context created with SQG_METH");
    const bool sampled = !b->s_seq_off.empty();
    if (origin && (!origin->key0 || !origin->step)) return K.bad("origin: key0 and step must not be NULL");
    if (!origin && !sampled && (!by_kmer || split_strand)) return K.bad("origin must not be NULL: the batch was not sampled");
    if (origin)
        for (int i = 0; i < b->n; i++)
            if (origin->step[i] < -1 || origin->step[i] > 1) return K.bad("origin: step must be -1, 0 or +1");
    return SQG_OK;
}

// Every read's origin and insert into the scratch's table, and its upload on st: L from the read's events (ne0 = attached length - k + 1), 0
// for a stand-in read; the origin the caller's, the sampler's, or {0, +1}
static int pileup_reads(sqg_ctx* c, const sqg_batch* b, const sqg_pileup_origin_t* origin, const BatchView& bv, hipStream_t st) {
    PileupScratch& Y = c->pileup;
    const int n = b->n;
    if (int rc = Y.d_pr.need(c, (size_t)n)) return rc;
    const bool sampled = !b->s_seq_off.empty();
    const long long extra = bv.p1, ne1 = batch_stall_events(c);      // the attached prefix's bases in chain 0 (either kind); chain 1's events
    Y.h_pr.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        PileRead& p = Y.h_pr[(size_t)i];
        const bool stand_in = (size_t)i < b->short_read.size() && b->short_read[(size_t)i];
        const long long ne0 = b->ev_off[(size_t)i + 1] - b->ev_off[(size_t)i] - ne1;
        p.first = bv.kind == SEG_DNA ? (int)extra : 0;
        p.L = stand_in ? 0 : (int)(ne0 + c->k - 1 - extra);
        if (origin) { p.key0 = origin->key0[i]; p.step = origin->step[i]; }
        else if (sampled) {
            const bool minus = b->s_strand[(size_t)i] == '-';
            p.key0 = c->h_contig_off[(size_t)b->s_ref_idx[(size_t)i]] + b->s_ref_pos[(size_t)i] + (minus ? (long long)b->s_rlen[(size_t)i] - c->k : 0);
            p.step = minus ? -1 : 1;
        } else { p.key0 = 0; p.step = 1; }
    }
    HIPCHK(c, hipMemcpyAsync(Y.d_pr.p, Y.h_pr.data(), (size_t)n * sizeof(PileRead), hipMemcpyHostToDevice, st));
    return SQG_OK;
}

// The kernels' parameters from cfg and the caller's arrays (stat: the scratch's counter block)
static PileupParams pileup_params(const sqg_ctx* c, const sqg_pileup_cfg_t* cfg, const sqg_pileup_out_t* out, const EventParams& Q) {
    PileupParams U{};
    U.pr = c->pileup.d_pr.p; U.kmer = Q.kmer; U.seg = Q.seg;
    U.by_kmer = cfg->by == SQG_PILEUP_BY_KMER ? 1 : 0; U.split_strand = cfg->split & SQG_PILEUP_SPLIT_STRAND ? 1 : 0; U.split_meth = cfg->split & SQG_PILEUP_SPLIT_METH ? 1 : 0; U.k = c->k;
    U.segs = cfg->segs ? cfg->segs : 8u; U.lo = cfg->lo; U.hi = cfg->hi;
    U.n = out->n; U.dwell = (long long*)out->dwell; U.dwell_sq = (long long*)out->dwell_sq;
    U.mean_sum = (long long*)out->mean_sum; U.mean_sq = (long long*)out->mean_sq; U.sd_sum = (long long*)out->sd_sum;
    U.stat = c->pileup.d_stat.p;
    return U;
}

extern "C" int sqg_batch_pileup(sqg_ctx_t* c, sqg_batch_t* b, const sqg_pileup_cfg_t* cfg, const sqg_pileup_origin_t* origin,
                                const sqg_pileup_out_t* out, sqg_pileup_stat_t* stat) {
    static const char who[] = "sqg_batch_pileup";
    int rc = check_open(c, b, cfg, "cfg", who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = K.null(out, "out"))) return rc;
    if ((rc = pileup_check(K, c, b, cfg, origin))) return rc;
    const bool by_kmer = cfg->by == SQG_PILEUP_BY_KMER, split_meth = cfg->split & SQG_PILEUP_SPLIT_METH;
    if (stat) { stat->counted = 0; stat->outside = 0; }
    if ((rc = K.ran(b))) return rc;
    const bool want_samples = out->mean_sum || out->mean_sq || out->sd_sum;
    const bool want_stats = want_samples && cfg->norm == SQG_CHUNK_MEDMAD;
    // the statistics job as sqg_batch_events opens it: the statistics for MEDMAD, the inserts' spans for trim
    ChunkJob J;
    if ((rc = spans_open(c, b, who, c->use_dwell_stream, want_stats && cfg->trim == 1, &J)) || J.P.bv.n_reads == 0 || b->n_events == 0) return rc;
    const hipStream_t st = J.st;
    if (want_stats && (rc = stats_run(c, b, J, nullptr, nullptr))) return rc;
    PileupScratch& Y = c->pileup;
    if ((rc = Y.d_stat.need(c, 4))) return rc;
    EventParams Q{J.P.bv, want_stats ? J.P.consts : (const float2*)nullptr, b->n_events};
    if ((rc = pileup_reads(c, b, origin, Q.bv, st))) return rc;
    HIPCHK(c, hipMemsetAsync(Y.d_stat.p, 0, 2 * sizeof(unsigned long long), st));
    // pass 1, scan (k_events_table.h): where every event starts, its read, and k-mer / segment where the key or a split needs them
    if ((rc = evtab_scan_run(c, Q, EVC_START | EVC_READ | (by_kmer || split_meth ? EVC_KMER : 0) | (by_kmer ? EVC_SEG : 0)))) return rc;
    // pass 2: the samples of the events that count, their mean / sd, the adds
    const PileupParams U = pileup_params(c, cfg, out, Q);
    dispatch(false, cfg->norm == SQG_CHUNK_PA, [&](auto, auto A) { hipLaunchKernelGGL(k_pileup<decltype(A)::value>, dim3(flat_grid(c, b->n_events)), dim3(CHUNK_WG), 0, st, Q, U); });
    if ((rc = launched(c, "k_pileup"))) return rc;
    unsigned long long h_stat[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h_stat, Y.d_stat.p, sizeof h_stat, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (stat) { stat->counted = (int64_t)h_stat[0]; stat->outside = (int64_t)h_stat[1]; }
    return SQG_OK;
}
