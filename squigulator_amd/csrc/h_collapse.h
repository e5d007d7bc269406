// h_collapse.h -- sqg_batch_collapse, sqg_batch_pileup_rows: the caller's event rows summed per true event, and the pileup of those sums, on the device
// Host side of include/sqg_collapse.h; included by sqg_hip.hip behind h_align.h.  The opening of the checks, the batch's view, the lifetime
// rule and the statistics job are h_chunks.h's, the scan pass and the flat grid h_events_table.h's, the cfg / origin checks, the reads'
// table and the kernels' parameters of the pileup h_pileup.h's.  What the two calls share is stated here once: the checks of the rows
// (collapse_check) and the row pass with its scratch (collapse_rows_run).
#pragma once

// the rows' arguments, behind check_open: the NULL checks in the header's order, then row_off (h_align.h: rows_off_check)
static int collapse_check(const Check& K, const sqg_batch* b, const int64_t* row_off, const sqg_collapse_in_t* in, const void* out) {
    int rc;
    if ((rc = K.null(row_off, "row_off")) || (rc = K.null(in, "in")) || (rc = K.null(in->ev, "in->ev")) || (rc = K.null(in->sum, "in->sum")) ||
        (rc = K.null(in->len, "in->len")) || (rc = K.null(out, "out"))) return rc;
    return rows_off_check(K, b->n, row_off);
}

// The row pass on st: the upload of row_off, the sums named in `need` (bit 0 rows, 1 len, 2 sum, 3 sumsq) into the caller's arrays of *own
// where given, else into the scratch, all zeroed first; rd_dropped (the caller's, may be null) and `dropped` (a counter, may be null) beside
// them.  *S is what the passes behind it read.  A sum that is needed and has no memory is refused before any launch.
static int collapse_rows_run(sqg_ctx* c, sqg_batch* b, const BatchView& bv, const int64_t* row_off, const sqg_collapse_in_t* in, unsigned need,
                             const sqg_collapse_out_t* own, unsigned long long* dropped, hipStream_t st, CollapseSums* S) {
    CollapseScratch& X = c->collapse;
    const int n = b->n;
    const size_t ne = (size_t)b->n_events;
    int rc = SQG_OK;
    CollapseParams P{};
    P.ev = (const long long*)in->ev; P.sum = (const long long*)in->sum; P.sumsq = (const long long*)in->sumsq; P.len = in->len;
    P.ob_rows = own ? own->ob_rows : nullptr; P.ob_len = own ? (unsigned long long*)own->ob_len : nullptr;
    P.ob_sum = own ? (unsigned long long*)own->ob_sum : nullptr; P.ob_sumsq = own ? (unsigned long long*)own->ob_sumsq : nullptr;
    P.rd_dropped = own ? own->rd_dropped : nullptr; P.dropped = dropped;
    const auto col = [&](unsigned bit, auto*& p, auto& buf) {
        if (!(need & bit) || p || rc) return;
        if (!(rc = buf.need(c, ne))) p = buf.p;
    };
    col(1, P.ob_rows, X.d_rows); col(2, P.ob_len, X.d_len); col(4, P.ob_sum, X.d_sum); col(8, P.ob_sumsq, X.d_sumsq);
    if (rc) return rc;
    const void* const cols[4] = {P.ob_rows, P.ob_len, P.ob_sum, P.ob_sumsq};
    for (int q = 0; q < 4; q++)                                                                      // no kernel is handed a null column it will read
        if (ne && (need >> q & 1u) && !cols[q]) { c->err = "k_collapse_rows: a sum a later pass reads has no memory"; return SQG_EDEVICE; }
    if (P.ob_sumsq && !P.sumsq) { c->err = "k_collapse_rows: ob_sumsq without in->sumsq"; return SQG_EDEVICE; }      // (the callers have refused it)
    if ((rc = rows_upload(c, bv, row_off, &P.rows))) return rc;
    if (P.ob_rows) HIPCHK(c, hipMemsetAsync(P.ob_rows, 0, ne * sizeof(unsigned int), st));
    if (P.ob_len) HIPCHK(c, hipMemsetAsync(P.ob_len, 0, ne * sizeof(unsigned long long), st));
    if (P.ob_sum) HIPCHK(c, hipMemsetAsync(P.ob_sum, 0, ne * sizeof(unsigned long long), st));
    if (P.ob_sumsq) HIPCHK(c, hipMemsetAsync(P.ob_sumsq, 0, ne * sizeof(unsigned long long), st));
    if (P.rd_dropped) HIPCHK(c, hipMemsetAsync(P.rd_dropped, 0, (size_t)n * sizeof(int), st));
    *S = CollapseSums{P.ob_rows, (const long long*)P.ob_len, (const long long*)P.ob_sum, (const long long*)P.ob_sumsq};
    if (P.rows.n_rows == 0) return SQG_OK;
    hipLaunchKernelGGL(k_collapse_rows, dim3(flat_grid(c, P.rows.n_rows)), dim3(CHUNK_WG), 0, st, P);
    return launched(c, "k_collapse_rows");
}

extern "C" int sqg_batch_collapse(sqg_ctx_t* c, sqg_batch_t* b, const sqg_collapse_cfg_t* cfg, const int64_t* row_off,
                                  const sqg_collapse_in_t* in, const sqg_collapse_out_t* out) {
    static const char who[] = "sqg_batch_collapse";
    int rc = check_open(c, b, cfg, "cfg", who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = collapse_check(K, b, row_off, in, out))) return rc;
    if (!norm_ok(cfg->norm)) return K.bad("unknown norm");
    if (!trim_ok(cfg->trim)) return K.bad("trim must be 0 or 1");
    if (!in->sumsq && (out->ob_sumsq || out->sd)) return K.bad("in->sumsq must not be NULL: ob_sumsq or sd is wanted");
    if ((rc = K.ran(b))) return rc;
    const bool want_derive = out->mean || out->sd;
    const bool want_stats = want_derive && cfg->norm == SQG_CHUNK_MEDMAD;
    // the statistics job as sqg_batch_events opens it: the statistics for MEDMAD, the inserts' spans for trim
    ChunkJob J;
    if ((rc = spans_open(c, b, who, c->use_dwell_stream, want_stats && cfg->trim == 1, &J)) || J.P.bv.n_reads == 0) return rc;
    const hipStream_t st = J.st;
    if (want_stats && (rc = stats_run(c, b, J, nullptr, nullptr))) return rc;
    // pass 1, the rows: what the caller asked for, and what mean / sd are derived from
    const unsigned need = (out->ob_rows ? 1u : 0u) | (out->ob_len || want_derive ? 2u : 0u) | (out->ob_sum || want_derive ? 4u : 0u) | (out->ob_sumsq || out->sd ? 8u : 0u);
    CollapseSums S{};
    if ((rc = collapse_rows_run(c, b, J.P.bv, row_off, in, need, out, nullptr, st, &S))) return rc;
    // pass 2, the events: their read from the scan pass, mean / sd from the finished sums
    if (want_derive && b->n_events > 0) {
        EventParams Q{J.P.bv, want_stats ? J.P.consts : (const float2*)nullptr, b->n_events};
        if ((rc = evtab_scan_run(c, Q, EVC_READ))) return rc;
        Q.mean = out->mean; Q.sd = out->sd;
        dispatch(false, cfg->norm == SQG_CHUNK_PA, [&](auto, auto A) { hipLaunchKernelGGL(k_collapse_derive<decltype(A)::value>, dim3(flat_grid(c, b->n_events)), dim3(CHUNK_WG), 0, st, Q, S); });
        if ((rc = launched(c, "k_collapse_derive"))) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}

extern "C" int sqg_batch_pileup_rows(sqg_ctx_t* c, sqg_batch_t* b, const sqg_pileup_cfg_t* cfg, const sqg_pileup_origin_t* origin,
                                     const int64_t* row_off, const sqg_collapse_in_t* in, const sqg_pileup_out_t* out, sqg_pileup_rows_stat_t* stat) {
    static const char who[] = "sqg_batch_pileup_rows";
    int rc = check_open(c, b, cfg, "cfg", who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = collapse_check(K, b, row_off, in, out)) || (rc = pileup_check(K, c, b, cfg, origin))) return rc;
    if (!in->sumsq && out->sd_sum) return K.bad("in->sumsq must not be NULL: sd_sum is wanted");
    if (stat) *stat = sqg_pileup_rows_stat_t{0, 0, 0, 0};
    if ((rc = K.ran(b))) return rc;
    const bool by_kmer = cfg->by == SQG_PILEUP_BY_KMER, split_meth = cfg->split & SQG_PILEUP_SPLIT_METH;
    const bool want_samples = out->mean_sum || out->mean_sq || out->sd_sum;
    const bool want_stats = want_samples && cfg->norm == SQG_CHUNK_MEDMAD;
    ChunkJob J;
    if ((rc = spans_open(c, b, who, c->use_dwell_stream, want_stats && cfg->trim == 1, &J)) || J.P.bv.n_reads == 0) return rc;
    const hipStream_t st = J.st;
    if (want_stats && (rc = stats_run(c, b, J, nullptr, nullptr))) return rc;
    PileupScratch& Y = c->pileup;
    if ((rc = Y.d_stat.need(c, 4))) return rc;
    EventParams Q{J.P.bv, want_stats ? J.P.consts : (const float2*)nullptr, b->n_events};
    if ((rc = pileup_reads(c, b, origin, Q.bv, st))) return rc;
    HIPCHK(c, hipMemsetAsync(Y.d_stat.p, 0, 4 * sizeof(unsigned long long), st));
    // pass 1, the rows: how many every event has, their samples, and the sums a mean or an sd is derived from
    const unsigned need = 1u | 2u | (want_samples ? 4u : 0u) | (out->sd_sum ? 8u : 0u);
    CollapseSums S{};
    if ((rc = collapse_rows_run(c, b, Q.bv, row_off, in, need, nullptr, Y.d_stat.p + 3, st, &S))) return rc;
    if (b->n_events > 0) {
        // pass 2, scan (k_events_table.h): every event's read, and k-mer / segment where the key or a split needs them
        if ((rc = evtab_scan_run(c, Q, EVC_READ | (by_kmer || split_meth ? EVC_KMER : 0) | (by_kmer ? EVC_SEG : 0)))) return rc;
        // pass 3: the observed events that count, their mean / sd, the adds
        const PileupParams U = pileup_params(c, cfg, out, Q);
        dispatch(false, cfg->norm == SQG_CHUNK_PA, [&](auto, auto A) { hipLaunchKernelGGL(k_pileup_rows<decltype(A)::value>, dim3(flat_grid(c, b->n_events)), dim3(CHUNK_WG), 0, st, Q, U, S); });
        if ((rc = launched(c, "k_pileup_rows"))) return rc;
    }
    unsigned long long h_stat[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h_stat, Y.d_stat.p, sizeof h_stat, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (stat) *stat = sqg_pileup_rows_stat_t{(int64_t)h_stat[0], (int64_t)h_stat[1], (int64_t)h_stat[2], (int64_t)h_stat[3]};
    return SQG_OK;
}
