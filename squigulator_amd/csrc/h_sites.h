// h_sites.h -- sqg_site_plan, sqg_batch_sites: CpG-centred signal windows of a batch with their methylation labels, left on the device
// Host side of include/sqg_sites.h; included by sqg_hip.hip behind h_segments.h.  The opening of the checks, the batch's view, the lifetime rule and the statistics job are h_chunks.h's.
#pragma once

static int site_check(sqg_ctx* c, sqg_batch* b, const sqg_site_cfg_t* cfg, const char* who) {
    if (int rc = check_open(c, b, cfg, "cfg", who)) return rc;
    const Check K{c, who};
    if (c->cfg.flags & SQG_RNA) return K.bad("sites: not with SQG_RNA");
    if (c->cfg.flags & SQG_PREFIX) return K.bad("sites: not with SQG_PREFIX");
    if (cfg->win_len < 16 || cfg->win_len > 65536 || (cfg->win_len & 7)) return K.bad("win_len must be a multiple of 8 in 16 .. 65536");
    if (cfg->before < 0 || cfg->before >= cfg->win_len) return K.bad("before must be in 0 .. win_len - 1");
    if (cfg->focus < 0 || cfg->focus >= c->k) return K.bad("focus must be in 0 .. k - 1");
    if (cfg->ctx_len < 0 || cfg->ctx_len > 255) return K.bad("ctx_len must be in 0 .. 255");
    if (cfg->ctx_before < 0 || cfg->ctx_before > std::max(cfg->ctx_len - 1, 0)) return K.bad("ctx_before must be in 0 .. ctx_len - 1 (0 when ctx_len is 0)");
    if (!dtype_ok(cfg->dtype)) return K.bad("unknown dtype");
    if (!norm_ok(cfg->norm)) return K.bad("unknown norm");
    return K.ran(b);
}

// what both kernels take, all but the caller's outputs, for a batch that owns its device results and dwells
static SiteParams site_params(sqg_ctx* c, sqg_batch* b, const sqg_site_cfg_t* cfg) {
    SiteParams Q{};
    Q.bv = batch_view(c, b);
    Q.skip = b->short_read.empty() ? nullptr : c->site.d_skip.p;
    Q.L = cfg->win_len; Q.before = cfg->before; Q.focus = cfg->focus; Q.B = cfg->ctx_len; Q.cb = cfg->ctx_before;
    Q.count = c->site.plan.d_count.p; Q.site_off = c->site.plan.d_off.p; Q.rec = c->site.d_rec.p;
    return Q;
}

// The plan of a non-empty batch that has finished and owns its results and dwells: SiteScratch::plan (h_common.h: ReadPlan), h_off [n+1]
// and its copy on the device, from k_site_scan<0>'s counts -- once per batch and (win_len, before, focus): a call that follows another
// with the same three (the plan, then the sites) finds it in the scratch, whatever other calls ran between the two.
static int site_plan_run(sqg_ctx* c, sqg_batch* b, const sqg_site_cfg_t* cfg) {
    SiteScratch& X = c->site;
    const size_t n = (size_t)b->n;
    if (X.plan_of == (const void*)b && X.plan_run == b->run_idx && X.plan.h_off.size() == n + 1 &&
        X.plan_key[0] == cfg->win_len && X.plan_key[1] == cfg->before && X.plan_key[2] == cfg->focus) return SQG_OK;
    X.plan_of = nullptr;                                                // (until the new plan is there)
    int rc;
    if ((rc = X.plan.begin(c, n))) return rc;
    const hipStream_t st = c->stream;
    if (!b->short_read.empty()) {
        if ((rc = X.d_skip.need(c, n))) return rc;
        HIPCHK(c, hipMemcpyAsync(X.d_skip.p, b->short_read.data(), n, hipMemcpyHostToDevice, st));
    }
    const SiteParams Q = site_params(c, b, cfg);
    hipLaunchKernelGGL(k_site_scan<0>, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, Q);
    if ((rc = X.plan.finish(c, n, st))) return rc;
    X.plan_of = b; X.plan_run = b->run_idx;
    X.plan_key[0] = cfg->win_len; X.plan_key[1] = cfg->before; X.plan_key[2] = cfg->focus;
    return SQG_OK;
}

extern "C" int sqg_site_plan(sqg_ctx_t* c, sqg_batch_t* b, const sqg_site_cfg_t* cfg, int64_t* site_off, int64_t* n_sites) {
    static const char who[] = "sqg_site_plan";
    int rc = site_check(c, b, cfg, who);
    if (rc) return rc;
    if ((rc = Check{c, who}.null(n_sites, "n_sites"))) return rc;
    if ((rc = chunk_owned(c, b, who, c->use_dwell_stream))) return rc;
    if (b->n > 0 && (rc = site_plan_run(c, b, cfg))) return rc;
    c->site.plan.give(b->n, site_off, n_sites);
    return SQG_OK;
}

extern "C" int sqg_batch_sites(sqg_ctx_t* c, sqg_batch_t* b, const sqg_site_cfg_t* cfg, const sqg_site_out_t* out) {
    static const char who[] = "sqg_batch_sites";
    int rc = site_check(c, b, cfg, who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = K.null(out, "out"))) return rc;
    if (out->signal && ((uintptr_t)out->signal & 15)) return K.bad("signal must be 16-byte aligned");
    ChunkJob J;                                                         // the statistics job of the whole reads
    if ((rc = spans_open(c, b, who, c->use_dwell_stream, false, &J)) || J.P.bv.n_reads == 0) return rc;
    if ((rc = site_plan_run(c, b, cfg))) return rc;
    const int n = b->n;
    const long long n_sites = c->site.plan.h_off[(size_t)n];
    const hipStream_t st = J.st;
    const bool want_rows = n_sites > 0 && (out->signal || out->context || out->ctx_start);
    const bool want_stats = out->med2 || out->mad4 || (out->signal && n_sites > 0 && cfg->norm == SQG_CHUNK_MEDMAD);
    if (want_stats && (rc = stats_run(c, b, J, out->med2, out->mad4))) return rc;
    if (n_sites > 0) {
        if ((rc = c->site.d_rec.need(c, (size_t)n_sites))) return rc;
        SiteParams Q = site_params(c, b, cfg);
        Q.n_sites = n_sites; Q.consts = J.P.consts;
        Q.label = out->label; Q.site_read = out->site_read; Q.site_pos = out->site_pos; Q.win_start = (long long*)out->win_start;
        Q.signal = out->signal; Q.context = cfg->ctx_len > 0 ? out->context : (uint8_t*)nullptr; Q.ctx_start = out->ctx_start;
        if (want_rows || Q.label || Q.site_read || Q.site_pos || Q.win_start)
            hipLaunchKernelGGL(k_site_scan<1>, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, Q);
        if (want_rows) {
            const int per = CHUNK_WG / 64;
            const unsigned wgs = (unsigned)std::min<long long>((n_sites + per - 1) / per, 1LL << 20);
            dispatch(cfg->dtype == SQG_CHUNK_F32, cfg->norm == SQG_CHUNK_PA, [&](auto F, auto A) {
                hipLaunchKernelGGL((k_site_emit<decltype(F)::value, decltype(A)::value>), dim3(wgs), dim3(CHUNK_WG), 0, st, Q);
            });
        }
        if ((rc = launched(c, "k_site_emit"))) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}
