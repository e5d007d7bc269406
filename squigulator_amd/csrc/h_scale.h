// h_scale.h -- sqg_batch_scale, sqg_batch_align_scaled: a per-read shift and scale estimated from the caller's event rows, and the aligner under one
// Host side of include/sqg_scale.h; included by sqg_hip.hip behind h_collapse.h.  The opening of the checks, the batch's view and the
// lifetime rule are h_chunks.h's, the targets h_events_table.h's, the rows' check and upload and the aligner's body h_align.h's (align_run).
#pragma once

// k_scale_sums' launch over n rows: `trips` consecutive 64-row trips per wavefront, workgroups of CHUNK_WG / 64 wavefronts, at most 8 of
// them per compute unit -- what fills the device at the kernel's register count.  (The development build takes another cap from
// SQG_TEST_SCALE_GRID: a test reaches the second trip on a few hundred rows.)
static unsigned scale_grid(const sqg_ctx* c, long long n, long long* trips) {
    const long long waves_wg = CHUNK_WG / 64, tiles = (n + 63) / 64;
    const long long cap = std::max(1, dev_env_int(SQG_DEV_ENV("SQG_TEST_SCALE_GRID"), 8 * c->num_cu));
    *trips = std::max(1LL, (tiles + cap * waves_wg - 1) / (cap * waves_wg));
    const long long waves = (tiles + *trips - 1) / *trips;
    return (unsigned)((waves + waves_wg - 1) / waves_wg);
}

extern "C" int sqg_batch_scale(sqg_ctx_t* c, sqg_batch_t* b, const sqg_scale_cfg_t* cfg, const int64_t* row_off,
                               const sqg_scale_in_t* in, const sqg_scale_out_t* out) {
    static const char who[] = "sqg_batch_scale";
    int rc = check_open(c, b, cfg, "cfg", who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = K.null(row_off, "row_off")) || (rc = K.null(in, "in")) || (rc = K.null(in->sum, "in->sum")) || (rc = K.null(in->len, "in->len")) ||
        (rc = K.null(out, "out"))) return rc;
    if (cfg->mode != SQG_SCALE_MOMENTS && cfg->mode != SQG_SCALE_FIT) return K.bad("unknown mode");
    const bool fit = cfg->mode == SQG_SCALE_FIT;
    if (fit && (rc = K.null(in->ev, "in->ev"))) return rc;
    const int n = b->n;
    if ((rc = rows_off_check(K, n, row_off)) || (rc = K.ran(b))) return rc;
    if ((rc = chunk_owned(c, b, who, c->use_dwell_stream)) || n == 0) return rc;
    ScaleScratch& X = c->scale;
    const BatchView bv = batch_view(c, b);
    ScaleParams P{};
    if ((rc = rows_upload(c, bv, row_off, &P.rows)) || (rc = X.d_acc.need(c, (size_t)SCL_COLS * (size_t)n))) return rc;
    const hipStream_t st = c->stream;
    HIPCHK(c, hipMemsetAsync(X.d_acc.p, 0, (size_t)SCL_COLS * (size_t)n * sizeof(unsigned long long), st));
    P.n_events = b->n_events; P.sum = (const long long*)in->sum; P.len = in->len; P.ev = (const long long*)in->ev; P.acc = X.d_acc.p;
    if (P.rows.n_rows > 0) {
        if ((rc = evtab_targets(c, bv, b->n_events, &P.level_raw))) return rc;      // the targets, as sqg_batch_align gets them
        // pass 1, the sums: over the rows, and for MOMENTS once more over the events
        const unsigned grid = scale_grid(c, P.rows.n_rows, &P.trips);
        if (fit) hipLaunchKernelGGL(k_scale_sums<SCL_FIT>, dim3(grid), dim3(CHUNK_WG), 0, st, P);
        else hipLaunchKernelGGL(k_scale_sums<SCL_ROWS>, dim3(grid), dim3(CHUNK_WG), 0, st, P);
        if ((rc = launched(c, "k_scale_sums"))) return rc;
        if (!fit && b->n_events > 0) {
            const unsigned tgrid = scale_grid(c, b->n_events, &P.trips);
            hipLaunchKernelGGL(k_scale_sums<SCL_TARGETS>, dim3(tgrid), dim3(CHUNK_WG), 0, st, P);
            if ((rc = launched(c, "k_scale_sums"))) return rc;
        }
    }
    // pass 2, the reads: the finished sums to the caller, gain / shift from them
    const ScaleOut O{(long long*)out->n, (long long*)out->nx, (long long*)out->sy, (long long*)out->syy, (long long*)out->sx, (long long*)out->sxx,
                     (long long*)out->sxy, out->gain, out->shift, out->rd_dropped};
    const unsigned dgrid = (unsigned)((n + CHUNK_WG - 1) / CHUNK_WG);
    const int no_rows = P.rows.n_rows == 0;
    if (fit) hipLaunchKernelGGL(k_scale_derive<true>, dim3(dgrid), dim3(CHUNK_WG), 0, st, P, O, no_rows);
    else hipLaunchKernelGGL(k_scale_derive<false>, dim3(dgrid), dim3(CHUNK_WG), 0, st, P, O, no_rows);
    if ((rc = launched(c, "k_scale_derive"))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}

extern "C" int sqg_batch_align_scaled(sqg_ctx_t* c, sqg_batch_t* b, const sqg_align_cfg_t* cfg, const int64_t* row_off,
                                      const sqg_align_in_t* in, const sqg_align_scale_t* scale, const sqg_align_out_t* out) {
    return align_run(c, b, cfg, row_off, in, true, scale, out, "sqg_batch_align_scaled");
}
