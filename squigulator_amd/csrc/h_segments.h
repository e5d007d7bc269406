// h_segments.h -- sqg_batch_segments and the trimmed chunk calls: the segments of reads with an attached prefix, chunks of their inserts
// Host side of include/sqg_segments.h; included by sqg_hip.hip behind h_chunks.h and h_targets.h, whose jobs the trimmed calls run.
#pragma once

// (int16)(30 dig / range), the amount gen_prefix_rna lowers the adaptor by (src/genread.c:83): double -> int16 as the CPU does it
static int segments_shift_code(const sqg_ctx* c) {
    const double v = 30 * c->cfg.profile.digitisation / c->cfg.profile.range;
    const int32_t t = (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : (int32_t)0x80000000u;
    return (int)(int16_t)(uint16_t)((uint32_t)t & 0xffffu);
}

// k_segments for a batch that has finished and owns its results and dwells: seg / shift (device, may be null) for the caller, spans and
// views into the context's scratch, the spans copied to ChunkScratch::h_span.  Returns when they are there.
static int segments_run(sqg_ctx* c, sqg_batch* b, long long* seg, long long* shift) {
    ChunkScratch& X = c->chunk;
    const size_t n = (size_t)b->n;
    int rc;
    if ((rc = X.d_span.need(c, 2 * n)) || (rc = X.d_view.need(c, n))) return rc;
    X.h_span.resize(2 * n);
    X.span_of = nullptr;                                                // (until the new spans are there)
    SegParams Q{};
    Q.bv = batch_view(c, b);
    if (Q.bv.kind == SEG_RNA) {
        // development build: SQG_TEST_SEG_SPS=N makes the window 79 N samples long here (not in the generator), so that it reaches into
        // the inserts and k_target_shift has samples to lower
        const int sps = dev_env_int(SQG_DEV_ENV("SQG_TEST_SEG_SPS"), Q.bv.const_sps);
        Q.shift_len = (long long)(Q.bv.p1 - Q.bv.p0) * sps;             // (the adaptor's bases)
    }
    Q.seg = seg; Q.shift = shift; Q.lo = X.d_span.p; Q.hi = X.d_span.p + n; Q.view = X.d_view.p;
    hipLaunchKernelGGL(k_segments, dim3((unsigned)n), dim3(64), 0, c->stream, Q);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(X.h_span.data(), X.d_span.p, 2 * n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    X.span_of = b; X.span_run = b->run_idx;
    return SQG_OK;
}

extern "C" int sqg_batch_segments(sqg_ctx_t* c, sqg_batch_t* b, const sqg_segments_t* out) {
    static const char who[] = "sqg_batch_segments";
    int rc = check_open(c, b, out, "out", who);
    if (rc || (rc = Check{c, who}.ran(b))) return rc;
    if ((rc = chunk_owned(c, b, who, c->use_dwell_stream))) return rc;
    if (b->n == 0 || !(out->seg || out->shift)) return SQG_OK;
    return segments_run(c, b, (long long*)out->seg, (long long*)out->shift);
}

extern "C" int sqg_chunk_plan_trimmed(sqg_ctx_t* c, sqg_batch_t* b, const sqg_chunk_cfg_t* cfg, int64_t* chunk_off, int64_t* n_chunks) {
    static const char who[] = "sqg_chunk_plan_trimmed";
    int rc = chunk_check(c, b, cfg, who, true);
    if (rc) return rc;
    if ((rc = Check{c, who}.null(n_chunks, "n_chunks"))) return rc;
    ChunkJob J;
    if ((rc = chunk_begin(c, b, cfg, who, c->use_dwell_stream, &J, true))) return rc;
    if (chunk_off) { chunk_off[0] = 0; for (int i = 0; i < b->n; i++) chunk_off[i + 1] = (int64_t)J.plan[i + 1]; }
    *n_chunks = (int64_t)J.n_chunks;
    return SQG_OK;
}

extern "C" int sqg_batch_chunks_trimmed(sqg_ctx_t* c, sqg_batch_t* b, const sqg_chunk_cfg_t* cfg, const sqg_chunk_out_t* out) {
    return chunks_run(c, b, cfg, out, "sqg_batch_chunks_trimmed", true);
}

extern "C" int sqg_batch_chunk_targets_trimmed(sqg_ctx_t* c, sqg_batch_t* b, const sqg_chunk_cfg_t* cfg, const sqg_chunk_targets_t* tg) {
    return targets_run(c, b, cfg, tg, "sqg_batch_chunk_targets_trimmed", true);
}
