// h_detect.h -- sqg_detect_plan, sqg_batch_detect: the t-statistic event detector on a batch's stored signal, its rows left on the device
// Host side of include/sqg_detect.h; included by sqg_hip.hip behind h_pileup.h.  The opening of the checks, the batch's view, the lifetime
// rule and the statistics job are h_chunks.h's, the scan pass and its parameters h_events_table.h's.
#pragma once

static int detect_check(sqg_ctx* c, sqg_batch* b, const sqg_detect_cfg_t* cfg, const char* who) {
    if (int rc = check_open(c, b, cfg, "cfg", who)) return rc;
    const Check K{c, who};
    if (cfg->w_short < 1) return K.bad("w_short must be at least 1");
    if (cfg->w_long <= cfg->w_short || cfg->w_long > DET_H) return K.bad("w_long must be in w_short + 1 .. 64");
    if (!(std::isfinite(cfg->thr_short) && cfg->thr_short >= 0)) return K.bad("thr_short must be finite and >= 0");
    if (!(std::isfinite(cfg->thr_long) && cfg->thr_long >= 0)) return K.bad("thr_long must be finite and >= 0");
    if (!(std::isfinite(cfg->peak_height) && cfg->peak_height >= 0)) return K.bad("peak_height must be finite and >= 0");
    if (!norm_ok(cfg->norm)) return K.bad("unknown norm");
    if (!trim_ok(cfg->trim)) return K.bad("trim must be 0 or 1");
    return SQG_OK;
}

static DetectParams detect_params(const sqg_ctx* c, const sqg_batch* b, const sqg_detect_cfg_t* cfg) {
    DetectParams P{};
    P.bv = batch_view(c, b);
    P.w[0] = cfg->w_short; P.w[1] = cfg->w_long; P.th[0] = cfg->thr_short; P.th[1] = cfg->thr_long; P.h = cfg->peak_height;
    return P;
}

// The plan of a non-empty batch that has finished and owns its results: DetectScratch::plan (h_common.h: ReadPlan), h_off [n+1] and its
// copy on the device, from k_detect_walk<false>'s counts.  It is made afresh by every call: it depends on the samples themselves, not
// only on the batch's geometry, and one walk costs less than a plan that no longer fits them.
static int detect_plan_run(sqg_ctx* c, sqg_batch* b, const sqg_detect_cfg_t* cfg) {
    ReadPlan& X = c->detect.plan;
    const size_t n = (size_t)b->n;
    if (int rc = X.begin(c, n)) return rc;
    DetectParams P = detect_params(c, b, cfg);
    P.count = X.d_count.p;
    hipLaunchKernelGGL(k_detect_walk<false>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, P);
    return X.finish(c, n, c->stream);
}

extern "C" int sqg_detect_plan(sqg_ctx_t* c, sqg_batch_t* b, const sqg_detect_cfg_t* cfg, int64_t* det_off, int64_t* n_rows) {
    static const char who[] = "sqg_detect_plan";
    int rc = detect_check(c, b, cfg, who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = K.null(n_rows, "n_rows")) || (rc = K.ran(b))) return rc;
    if ((rc = chunk_owned(c, b, who, c->use_dwell_stream))) return rc;
    if (b->n > 0 && (rc = detect_plan_run(c, b, cfg))) return rc;
    c->detect.plan.give(b->n, det_off, n_rows);
    return SQG_OK;
}

extern "C" int sqg_batch_detect(sqg_ctx_t* c, sqg_batch_t* b, const sqg_detect_cfg_t* cfg, const sqg_detect_out_t* out) {
    static const char who[] = "sqg_batch_detect";
    int rc = detect_check(c, b, cfg, who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = K.null(out, "out")) || (rc = K.ran(b))) return rc;
    EventParams Q{};
    const EventWants want = evtab_outputs(Q, out, cfg->norm);
    const bool want_rows = want.sums || out->dt_len || out->true_ev;
    const bool want_walk = want_rows || out->dt_read || out->dt_start;
    // the statistics job as sqg_batch_events opens it: the inserts' spans only where the statistics are wanted over them
    ChunkJob J;
    if ((rc = spans_open(c, b, who, c->use_dwell_stream, want.stats && cfg->trim == 1, &J)) || J.P.bv.n_reads == 0) return rc;
    const int n = b->n;
    const hipStream_t st = J.st;
    if (want.stats && (rc = stats_run(c, b, J, out->med2, out->mad4))) return rc;
    if (want_walk) {
        DetectScratch& X = c->detect;
        // pass 1, the plan: every read's rows
        if ((rc = detect_plan_run(c, b, cfg))) return rc;
        const long long n_rows = X.plan.h_off[(size_t)n];
        if (n_rows > 0) {
            if (!out->dt_start && (rc = X.d_start.need(c, (size_t)n_rows))) return rc;
            if (!out->dt_read && (rc = X.d_read.need(c, (size_t)n_rows))) return rc;
            // pass 2, the same walk again: where every row starts, and its read
            DetectParams P = detect_params(c, b, cfg);
            P.det_off = X.plan.d_off.p;
            P.dt_start = out->dt_start ? (long long*)out->dt_start : X.d_start.p;
            P.dt_read = out->dt_read ? out->dt_read : X.d_read.p;
            hipLaunchKernelGGL(k_detect_walk<true>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, P);
            if ((rc = launched(c, "k_detect_walk"))) return rc;
            if (want_rows) {
                Q.bv = J.P.bv; Q.consts = want.stats ? J.P.consts : (const float2*)nullptr; Q.n_events = b->n_events;
                DetectRowParams U{X.plan.d_off.p, n_rows, P.dt_start, P.dt_read, out->dt_len, (long long*)out->true_ev, nullptr};
                // true_ev: where every true event starts (k_events_table.h's scan pass, that column alone)
                if (out->true_ev && b->n_events > 0) {
                    if ((rc = evtab_scan_run(c, Q, EVC_START))) return rc;
                    U.ev_start = Q.ev_start;
                } else U.true_ev = nullptr;
                // pass 3, the rows: their lengths, the sums of their samples, mean / sd from them, the event under their first sample
                dispatch(false, cfg->norm == SQG_CHUNK_PA, [&](auto, auto A) { hipLaunchKernelGGL(k_detect_rows<decltype(A)::value>, dim3(flat_grid(c, n_rows)), dim3(CHUNK_WG), 0, st, Q, U); });
                if ((rc = launched(c, "k_detect_rows"))) return rc;
            }
        }
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}
