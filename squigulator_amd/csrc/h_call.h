// h_call.h -- sqg_call_plan, sqg_batch_call: per-read CpG methylation calls of a batch scored from event rows, left on the device
// Host side of include/sqg_call.h; included by sqg_hip.hip behind h_scale.h.  The opening of the checks, the batch's view and the lifetime
// rule are h_chunks.h's, the origin's checks and the reads' origins h_pileup.h's (pileup_check, pileup_reads), the scaling's h_align.h's.
#pragma once

// the contexts of include/sqg_call.h, behind check_open
static int call_context(const Check& K, const sqg_ctx* c) {
    if (c->cfg.flags & SQG_RNA) return K.bad("calls: not with SQG_RNA");
    if (c->cfg.flags & SQG_PREFIX) return K.bad("calls: not with SQG_PREFIX");
    if (!(c->cfg.flags & SQG_METH)) return K.bad("calls: needs a context created with SQG_METH");
    return SQG_OK;
}

// what both kernels take of the batch and of the plan, for a batch that owns its device results
static CallParams call_params(sqg_ctx* c, sqg_batch* b) {
    CallParams Q{};
    Q.bv = batch_view(c, b);
    Q.skip = b->short_read.empty() ? nullptr : c->call.d_skip.p;
    Q.count = c->call.plan.d_count.p; Q.site_off = c->call.plan.d_off.p; Q.rec = c->call.d_rec.p;
    return Q;
}

// The plan of a non-empty batch that has finished and owns its results: CallScratch::plan (h_common.h: ReadPlan) from k_call_scan<0>'s
// counts -- once per batch: a call that follows another on the batch (the plan, then the calls) finds it in the scratch.
static int call_plan_run(sqg_ctx* c, sqg_batch* b) {
    CallScratch& X = c->call;
    const size_t n = (size_t)b->n;
    if (X.plan_of == (const void*)b && X.plan_run == b->run_idx && X.plan.h_off.size() == n + 1) return SQG_OK;
    X.plan_of = nullptr;                                                // (until the new plan is there)
    int rc;
    if ((rc = X.plan.begin(c, n))) return rc;
    const hipStream_t st = c->stream;
    if (!b->short_read.empty()) {
        if ((rc = X.d_skip.need(c, n))) return rc;
        HIPCHK(c, hipMemcpyAsync(X.d_skip.p, b->short_read.data(), n, hipMemcpyHostToDevice, st));
    }
    const CallParams Q = call_params(c, b);
    hipLaunchKernelGGL(k_call_scan<0>, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, Q);
    if ((rc = X.plan.finish(c, n, st))) return rc;
    X.plan_of = b; X.plan_run = b->run_idx;
    return SQG_OK;
}

extern "C" int sqg_call_plan(sqg_ctx_t* c, sqg_batch_t* b, int64_t* site_off, int64_t* n_sites) {
    static const char who[] = "sqg_call_plan";
    int rc = check_open(c, b, n_sites, "n_sites", who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = call_context(K, c)) || (rc = K.ran(b))) return rc;
    if ((rc = chunk_owned(c, b, who, c->use_dwell_stream))) return rc;
    if (b->n > 0 && (rc = call_plan_run(c, b))) return rc;
    c->call.plan.give(b->n, site_off, n_sites);
    return SQG_OK;
}

// workgroups of k_call_score's flat grid over n sites (the development build takes another cap from SQG_TEST_CALL_GRID: a test reaches
// the second trip on a few hundred sites)
static unsigned call_grid(const sqg_ctx* c, long long n) {
    const long long cap = std::max(1, dev_env_int(SQG_DEV_ENV("SQG_TEST_CALL_GRID"), 32 * c->num_cu));
    return (unsigned)std::min<long long>((n + CHUNK_WG - 1) / CHUNK_WG, cap);
}

extern "C" int sqg_batch_call(sqg_ctx_t* c, sqg_batch_t* b, const sqg_call_cfg_t* cfg, const sqg_call_in_t* in, const sqg_call_model_t* model,
                              const sqg_align_scale_t* scale, const sqg_pileup_origin_t* origin,
                              const sqg_call_out_t* out, const sqg_call_freq_t* freq, sqg_call_stat_t* stat) {
    static const char who[] = "sqg_batch_call";
    int rc = check_open(c, b, cfg, "cfg", who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = call_context(K, c))) return rc;
    if ((rc = K.null(in, "in")) || (rc = K.null(in->sum, "in->sum")) || (rc = K.null(model, "model")) || (rc = K.null(model->w, "model->w")) ||
        (rc = K.null(model->c, "model->c")) || (rc = K.null(out, "out"))) return rc;
    if (!in->len64 == !in->len32) return K.bad("exactly one of in->len64 and in->len32 must not be NULL");
    if (cfg->neigh != SQG_CALL_NEIGH_READ && cfg->neigh != SQG_CALL_NEIGH_SAME) return K.bad("unknown neigh");
    if (cfg->term_cap < 0 || cfg->term_cap > (1 << 26)) return K.bad("term_cap must be in 0 .. 1<<26");
    if (cfg->llr_min < 0) return K.bad("llr_min must not be negative");
    if (cfg->min_obs < 0 || cfg->min_obs > (1 << 20)) return K.bad("min_obs must be in 0 .. 1<<20");
    if (scale && ((rc = K.null(scale->gain, "scale->gain")) || (rc = K.null(scale->shift, "scale->shift")))) return rc;
    if (freq && freq->hi < freq->lo) return K.bad("freq: hi must not be below lo");
    // the origin by sqg_batch_pileup's rules: those of a pileup by position where a key is wanted, else of one that needs no origin
    const bool want_key = out->site_key || freq;
    const sqg_pileup_cfg_t as_pileup{want_key ? SQG_PILEUP_BY_REF : SQG_PILEUP_BY_KMER, 0u, SQG_CHUNK_PA, 0, 0u, 0, 0};
    if ((rc = pileup_check(K, c, b, &as_pileup, origin))) return rc;
    if (stat) *stat = sqg_call_stat_t{0, 0, 0, 0};
    if ((rc = K.ran(b))) return rc;
    const int n = b->n;
    if ((rc = chunk_owned(c, b, who, c->use_dwell_stream)) || n == 0) return rc;
    if ((rc = call_plan_run(c, b))) return rc;
    CallScratch& X = c->call;
    const long long n_sites = X.plan.h_off[(size_t)n];
    if (n_sites == 0) return SQG_OK;
    if ((rc = X.d_rec.need(c, (size_t)n_sites)) || (rc = X.d_stat.need(c, 4))) return rc;
    const hipStream_t st = c->stream;
    CallParams Q = call_params(c, b);
    Q.n_sites = n_sites;
    Q.site_read = out->site_read; Q.site_pos = out->site_pos; Q.label = out->label;
    Q.sum = (const long long*)in->sum; Q.len64 = (const long long*)in->len64; Q.len32 = in->len32;
    Q.w = model->w; Q.c = model->c;
    Q.gain = scale ? scale->gain : nullptr; Q.shift = scale ? scale->shift : nullptr;
    if (want_key) {
        if ((rc = pileup_reads(c, b, origin, Q.bv, st))) return rc;
        Q.pr = c->pileup.d_pr.p;
    }
    Q.neigh = (int)cfg->neigh; Q.term_cap = cfg->term_cap; Q.llr_min = cfg->llr_min; Q.min_obs = cfg->min_obs;
    Q.pow_k1 = 1;
    for (int i = 1; i < c->k; i++) Q.pow_k1 *= 5u;
    Q.site_key = (long long*)out->site_key; Q.n_obs = out->n_obs; Q.nll_c = out->nll_c; Q.nll_m = out->nll_m; Q.llr = out->llr; Q.call = out->call;
    if (freq) { Q.have_freq = 1; Q.lo = freq->lo; Q.hi = freq->hi; Q.cov = freq->cov; Q.truth = freq->truth; Q.called = freq->called; Q.meth = freq->meth; }
    Q.stat = X.d_stat.p;
    HIPCHK(c, hipMemsetAsync(X.d_stat.p, 0, 4 * sizeof(unsigned long long), st));
    // pass 1, the sites: one record each, and the caller's site_read / site_pos / label
    hipLaunchKernelGGL(k_call_scan<1>, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, Q);
    if ((rc = launched(c, "k_call_scan"))) return rc;
    // pass 2, the scores: the sites' rows, the adds to the frequency arrays, the counters
    hipLaunchKernelGGL(k_call_score, dim3(call_grid(c, n_sites)), dim3(CHUNK_WG), 0, st, Q);
    if ((rc = launched(c, "k_call_score"))) return rc;
    unsigned long long h_stat[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h_stat, X.d_stat.p, sizeof h_stat, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (stat) *stat = sqg_call_stat_t{(int64_t)n_sites, (int64_t)h_stat[0], (int64_t)h_stat[1], (int64_t)h_stat[2]};
    return SQG_OK;
}
