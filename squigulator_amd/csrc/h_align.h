// h_align.h -- sqg_batch_align: banded alignment of the caller's event rows to the true events of their reads, left on the device
// Host side of include/sqg_align.h; included by sqg_hip.hip behind h_detect.h.  The opening of the checks, the batch's view and the lifetime rule
// are h_chunks.h's, the scan pass and the targets h_events_table.h's.  Stated once here: the body (align_run: sqg_batch_align runs it without a
// scaling, sqg_batch_align_scaled of h_scale.h with the caller's) and, for h_collapse.h and h_scale.h too, the caller's rows (rows_off_check, rows_upload).
#pragma once

// row_off[n+1] of the caller, not NULL: the first row of every read, the rows' number behind them
static int rows_off_check(const Check& K, int n, const int64_t* row_off) {
    if (row_off[0] != 0) return K.bad("row_off must start at 0");
    for (int i = 0; i < n; i++) {
        if (row_off[i + 1] < row_off[i]) return K.bad("row_off must not decrease");
        if (row_off[i + 1] - row_off[i] > 0x7fffffffLL) return K.bad("row_off: a read has 2^31 rows or more");
    }
    return SQG_OK;
}

// the checked row_off to the context's scratch, on its stream; *R: the rows as the call's kernels take them
static int rows_upload(sqg_ctx* c, const BatchView& bv, const int64_t* row_off, RowsIn* R) {
    const size_t n = (size_t)bv.n_reads;
    const int rc = c->rows.d_off.need(c, n + 1);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->rows.d_off.p, row_off, (n + 1) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    *R = RowsIn{bv.reads, c->rows.d_off.p, bv.n_reads, (long long)row_off[n]};
    return SQG_OK;
}

// `scaled`: the call takes a scaling, *scale (checked behind out); else scale is null and the rows are taken as they stand
static int align_run(sqg_ctx_t* c, sqg_batch_t* b, const sqg_align_cfg_t* cfg, const int64_t* row_off, const sqg_align_in_t* in,
                     const bool scaled, const sqg_align_scale_t* scale, const sqg_align_out_t* out, const char* who) {
    int rc = check_open(c, b, cfg, "cfg", who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = K.null(row_off, "row_off")) || (rc = K.null(in, "in")) || (rc = K.null(in->sum, "in->sum")) || (rc = K.null(in->len, "in->len")) ||
        (rc = K.null(out, "out"))) return rc;
    if (scaled && ((rc = K.null(scale, "scale")) || (rc = K.null(scale->gain, "scale->gain")) || (rc = K.null(scale->shift, "scale->shift")))) return rc;
    if (cfg->stay_pen < 0 || cfg->stay_pen > (1 << 24)) return K.bad("stay_pen must be in 0 .. 1<<24");
    if (cfg->skip_pen < 0 || cfg->skip_pen > (1 << 24)) return K.bad("skip_pen must be in 0 .. 1<<24");
    if (cfg->cost_cap < 1 || cfg->cost_cap > (1 << 24)) return K.bad("cost_cap must be in 1 .. 1<<24");
    const int n = b->n;
    if ((rc = rows_off_check(K, n, row_off)) || (rc = K.ran(b))) return rc;
    if ((rc = chunk_owned(c, b, who, c->use_dwell_stream)) || n == 0) return rc;
    const bool want_trace = out->al_ev || out->al_edge;
    if (!want_trace && !out->al_cost) return SQG_OK;
    AlignScratch& X = c->align;
    AlignParams P{}; RowsIn R{};
    P.bv = batch_view(c, b);
    if ((rc = rows_upload(c, P.bv, row_off, &R)) || (rc = X.d_end.need(c, (size_t)n))) return rc;
    const size_t n_trace = (size_t)std::max<long long>(R.n_rows, 1);
    if (want_trace && ((rc = X.d_mask.need(c, n_trace)) || (rc = X.d_lo.need(c, n_trace)))) return rc;
    const hipStream_t st = c->stream;
    P.row_off = R.row_off; P.sum = (const long long*)in->sum; P.len = in->len;
    P.stay_pen = cfg->stay_pen; P.skip_pen = cfg->skip_pen; P.cost_cap = cfg->cost_cap;
    P.tr_mask = X.d_mask.p; P.tr_lo = X.d_lo.p; P.end_j = X.d_end.p;
    P.al_ev = (long long*)out->al_ev; P.al_cost = (long long*)out->al_cost; P.al_edge = out->al_edge;
    P.gain = scaled ? scale->gain : nullptr; P.shift = scaled ? scale->shift : nullptr;
    if ((rc = evtab_targets(c, P.bv, b->n_events, &P.level_raw))) return rc;      // the targets: every true event's level_raw
    // the forward pass: every read's band row by row, its end, and the trace when a path is wanted
    const auto forward = [&](auto TR, auto SC) { hipLaunchKernelGGL((k_align_forward<decltype(TR)::value, decltype(SC)::value>), dim3((unsigned)n), dim3(64), 0, st, P); };
    dispatch(want_trace, scaled, forward);
    if ((rc = launched(c, "k_align_forward"))) return rc;
    // the traceback
    if (want_trace) {
        hipLaunchKernelGGL(k_align_trace, dim3((unsigned)n), dim3(64), 0, st, P);
        if ((rc = launched(c, "k_align_trace"))) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}

extern "C" int sqg_batch_align(sqg_ctx_t* c, sqg_batch_t* b, const sqg_align_cfg_t* cfg, const int64_t* row_off,
                               const sqg_align_in_t* in, const sqg_align_out_t* out) {
    return align_run(c, b, cfg, row_off, in, false, nullptr, out, "sqg_batch_align");
}
