// h_chunks.h -- sqg_chunk_plan, sqg_batch_chunks: labelled, normalised chunks of a batch's signal, left on the device
// Host side of include/sqg_chunks.h (and, with `trimmed`, of the chunk calls of include/sqg_segments.h: h_segments.h); included by sqg_hip.hip (one translation unit with the kernels), in the order listed there.
#pragma once

// trimmed: the calls of include/sqg_segments.h, which cut the insert of a read with an attached prefix and so take SQG_PREFIX contexts
static int chunk_check(sqg_ctx* c, sqg_batch* b, const sqg_chunk_cfg_t* cfg, const char* who, bool trimmed = false) {
    if (!c) return SQG_EINVAL;
    auto bad = [&](const char* what) { c->err = std::string(who) + ": " + what; return SQG_EINVAL; };
    if (!b || !cfg) return bad("batch and cfg must not be NULL");
    if (!trimmed && (c->cfg.flags & SQG_PREFIX)) return bad("chunks: not with SQG_PREFIX");
    if (cfg->chunk_len < 64 || cfg->chunk_len > (1 << 20) || (cfg->chunk_len & 7)) return bad("chunk_len must be a multiple of 8 in 64 .. 1<<20");
    if (cfg->stride < 1) return bad("stride must be >= 1");
    if (cfg->max_label < 0 || cfg->max_label > 65535) return bad("max_label must be in 0 .. 65535");
    if (cfg->dtype != SQG_CHUNK_F16 && cfg->dtype != SQG_CHUNK_F32) return bad("unknown dtype");
    if (cfg->norm != SQG_CHUNK_MEDMAD && cfg->norm != SQG_CHUNK_PA) return bad("unknown norm");
    if (!b->ran) { c->err = std::string(who) + ": the batch has not been run"; return SQG_ESEQUENCE; }
    return SQG_OK;
}

// chunk_off [n+1] from the reads' spans [lo[i], hi[i]) -- the batch's sig_off and sig_off + 1 (the batch has been waited for), or the
// inserts' spans; a read shorter than a k-mer has no chunks
static void chunk_plan(const sqg_batch* b, const sqg_chunk_cfg_t* cfg, const long long* lo, const long long* hi, long long* off) {
    const long long L = cfg->chunk_len, S = cfg->stride;
    off[0] = 0;
    for (int i = 0; i < b->n; i++) {
        const long long n = hi[i] - lo[i];
        const bool none = n < L || ((size_t)i < b->short_read.size() && b->short_read[(size_t)i]);
        off[i + 1] = off[i] + (none ? 0 : (n - L) / S + 1);
    }
}

extern "C" int sqg_chunk_plan(sqg_ctx_t* c, sqg_batch_t* b, const sqg_chunk_cfg_t* cfg, int64_t* chunk_off, int64_t* n_chunks) {
    int rc = chunk_check(c, b, cfg, "sqg_chunk_plan");
    if (rc) return rc;
    if (!n_chunks) { c->err = "sqg_chunk_plan: n_chunks must not be NULL"; return SQG_EINVAL; }
    if ((rc = sqg_batch_wait(c, b, nullptr))) return rc;
    std::vector<long long>& off = c->chunk.h_off;
    off.resize((size_t)b->n + 1);
    chunk_plan(b, cfg, b->sig_off.data(), b->sig_off.data() + 1, off.data());
    if (chunk_off) for (int i = 0; i <= b->n; i++) chunk_off[i] = (int64_t)off[(size_t)i];
    *n_chunks = (int64_t)off[(size_t)b->n];
    return SQG_OK;
}

// What sqg_batch_chunks and sqg_batch_chunk_targets (h_targets.h) share of one call
struct ChunkJob {
    const long long* plan = nullptr; long long n_chunks = 0;   // [n_reads+1] first chunk of every read (host: ChunkScratch::h_off)
    ChunkParams P{};                                           // all but the caller's outputs
    const long long* lo = nullptr; const long long* hi = nullptr;   // host: the spans the plan was made from
    int force = 0; hipStream_t st = nullptr;                   // development build: SQG_TEST_CHUNK_GENERIC; the context's stream
};

static int segments_run(sqg_ctx* c, sqg_batch* b, long long* seg, long long* shift);   // h_segments.h
static int segments_shift_code(const sqg_ctx* c);

// The lifetime rule of every call on a batch's device results, in one place: the batch still owns its slabs (and its dwell set, if
// need_dwell), else SQG_ESEQUENCE; then it is waited for (its own kernels; fills sig_off) and the context's device is made current.
static int chunk_owned(sqg_ctx* c, sqg_batch* b, const char* who, bool need_dwell) {
    if (b->run_idx + 2 < c->runs || !slot_is_mine(c, b) || (need_dwell && !cset_is_mine(c, b))) {
        c->err = std::string(who) + ": the batch's device results have been handed to a later batch";
        return SQG_ESEQUENCE;
    }
    if (int rc = sqg_batch_wait(c, b, nullptr)) return rc;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return SQG_OK;
}

// The shared opening of both calls, behind chunk_check and the caller's own argument checks: the batch still owns its device results (and
// its dwell set, if need_dwell), it has finished, the plan, the parameters.  Host work only, unless trimmed: then the spans come from
// k_segments and the host waits for them, the one synchronisation the plan needs -- once per batch: a trimmed call that follows another
// on the same batch (the plan, then the chunks) finds spans and views in the scratch.  An empty batch leaves J->P.n_reads 0.
static int chunk_begin(sqg_ctx* c, sqg_batch* b, const sqg_chunk_cfg_t* cfg, const char* who, bool need_dwell, ChunkJob* J, bool trimmed = false) {
    if (trimmed && c->use_dwell_stream) need_dwell = true;              // (k_segments reads the dwells)
    if (int rc = chunk_owned(c, b, who, need_dwell)) return rc;
    const int n = b->n;
    if (n == 0) return SQG_OK;
    ChunkParams& P = J->P;
    if (trimmed) {
        const bool have = c->chunk.span_of == (const void*)b && c->chunk.span_run == b->run_idx && c->chunk.h_span.size() == 2 * (size_t)n;
        if (!have) { if (int rc = segments_run(c, b, nullptr, nullptr)) return rc; }
        J->lo = c->chunk.h_span.data(); J->hi = J->lo + n;
        P.lo = c->chunk.d_span; P.hi = c->chunk.d_span + n; P.view = c->chunk.d_view;
    } else {
        J->lo = b->sig_off.data(); J->hi = J->lo + 1;
        P.lo = c->slot[b->slot].d_sigoff; P.hi = P.lo + 1; P.view = nullptr;
    }
    c->chunk.h_off.resize((size_t)n + 1);
    chunk_plan(b, cfg, J->lo, J->hi, c->chunk.h_off.data());
    J->plan = c->chunk.h_off.data(); J->n_chunks = J->plan[n]; J->st = c->stream;
    P.sig = c->slot[b->slot].d_sig; P.n_reads = n; P.n_chunks = J->n_chunks;
    P.L = cfg->chunk_len; P.S = cfg->stride; P.W = cfg->max_label;
    // development build: 1 sends every read through the wide path (global histograms), 2 through the long one (several workgroups per read);
    // 3 leaves the statistics alone and makes k_chunk_labels divide in 64 bits, as it does for a read of 2^31 samples or more
    J->force = dev_env_int(SQG_DEV_ENV("SQG_TEST_CHUNK_GENERIC"), 0);
    P.hist_max = J->force == 1 ? 0 : CHUNK_HIST; P.one_wg_max = J->force == 2 ? 0 : 1LL << 22;
    P.range = c->cfg.profile.range; P.dig = c->cfg.profile.digitisation;
    return SQG_OK;
}

// ... and the first device work of both: the scratch of the shared passes, the plan uploaded
static int chunk_upload(sqg_ctx* c, ChunkJob* J) {
    ChunkScratch& X = c->chunk;
    const size_t n = (size_t)J->P.n_reads;
    int rc;
    if ((rc = ensure(c, (void**)&X.d_off, &X.off_cap, n + 1, sizeof(long long)))) return rc;
    if ((rc = ensure(c, (void**)&X.d_const, &X.const_cap, n, sizeof(float2)))) return rc;
    if ((rc = ensure(c, (void**)&X.d_wide, &X.wide_cap, n + 1, sizeof(unsigned int)))) return rc;
    if ((rc = ensure(c, (void**)&X.d_ghist, &X.ghist_cap, (size_t)CHUNK_WIDE_SLOTS * 2 * CHUNK_GBINS, sizeof(unsigned int)))) return rc;
    if ((rc = ensure(c, (void**)&X.d_read, &X.read_cap, (size_t)J->n_chunks + 1, sizeof(int)))) return rc;
    J->P.chunk_off = X.d_off; J->P.consts = X.d_const; J->P.wide_list = X.d_wide; J->P.ghist = X.d_ghist; J->P.chunk_read = X.d_read;
    HIPCHK(c, hipMemcpyAsync(X.d_off, J->plan, (n + 1) * sizeof(long long), hipMemcpyHostToDevice, J->st));
    return SQG_OK;
}

// the statistics pass on the context's stream: every read's {median, 1 / (1.4826 MAD)} into P.consts, med2 / mad4 where P has them
static int chunk_stats_run(sqg_ctx* c, sqg_batch* b, const ChunkJob& J) {
    const ChunkParams& P = J.P;
    const hipStream_t st = c->stream;
    const int n = b->n;
    HIPCHK(c, hipMemsetAsync(P.wide_list, 0, sizeof(unsigned int), st));
    hipLaunchKernelGGL(k_chunk_stats, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, P);
    hipLaunchKernelGGL(k_chunk_stats_wide, dim3(CHUNK_WIDE_SLOTS), dim3(CHUNK_WG), 0, st, P);
    for (int i = 0; i < n; i++) {
        const long long ns = J.hi[i] - J.lo[i];
        if (ns <= 0 || ns <= P.one_wg_max) continue;
        HIPCHK(c, hipMemsetAsync(P.ghist, 0, (size_t)2 * CHUNK_GBINS * sizeof(unsigned int), st));
        const unsigned wgs = (unsigned)std::min<long long>((ns + 16 * CHUNK_WG - 1) / (16 * CHUNK_WG), 4LL * c->num_cu);
        hipLaunchKernelGGL(k_chunk_hist_long, dim3(wgs), dim3(CHUNK_WG), 0, st, P, i);
        hipLaunchKernelGGL(k_chunk_select_long, dim3(1), dim3(CHUNK_WG), 0, st, P, i);
    }
    HIPCHK(c, hipGetLastError());
    return dbg_sync(c, "k_chunk_stats");
}

// sqg_batch_chunks, and sqg_batch_chunks_trimmed (h_segments.h) with trimmed
static int chunks_run(sqg_ctx* c, sqg_batch* b, const sqg_chunk_cfg_t* cfg, const sqg_chunk_out_t* out, const char* who, bool trimmed) {
    int rc = chunk_check(c, b, cfg, who, trimmed);
    if (rc) return rc;
    if (!out) { c->err = std::string(who) + ": out must not be NULL"; return SQG_EINVAL; }
    if (out->signal && ((uintptr_t)out->signal & 15)) { c->err = std::string(who) + ": signal must be 16-byte aligned"; return SQG_EINVAL; }
    ChunkJob J;
    if ((rc = chunk_begin(c, b, cfg, who, c->use_dwell_stream && (out->labels || out->label_len), &J, trimmed)) || J.P.n_reads == 0) return rc;
    if ((rc = chunk_upload(c, &J))) return rc;
    const long long n_chunks = J.n_chunks;
    const int n = b->n;
    const hipStream_t st = J.st;
    ChunkParams& P = J.P;                                               // ... and the caller's outputs
    P.med2 = out->med2; P.mad4 = out->mad4;
    P.chunk_read_out = out->chunk_read; P.chunk_start_out = (long long*)out->chunk_start;
    const bool want_labels = n_chunks > 0 && ((out->labels && cfg->max_label > 0) || out->label_len);
    if (want_labels && (rc = ensure(c, (void**)&c->chunk.d_ev, &c->chunk.ev_cap, (size_t)n_chunks, sizeof(int2)))) return rc;
    // pass 1, statistics: the read's constants for the emit kernel, med2 / mad4 for the caller
    const bool want_stats = out->med2 || out->mad4 || (out->signal && n_chunks > 0 && cfg->norm == SQG_CHUNK_MEDMAD);
    if (want_stats && (rc = chunk_stats_run(c, b, J))) return rc;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(k_chunk_index, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, P);
        // pass 2, emit
        if (out->signal) {
            const int cpb = chunk_emit_geom(P.L).cpb;
            const unsigned wgs = (unsigned)std::min<long long>((n_chunks + cpb - 1) / cpb, 1LL << 20);
            const bool f32 = cfg->dtype == SQG_CHUNK_F32, pa = cfg->norm == SQG_CHUNK_PA;
#define CHUNK_EMIT(F, A) hipLaunchKernelGGL((k_chunk_emit<F, A>), dim3(wgs), dim3(CHUNK_WG), 0, st, P, (const ReadDesc*)b->d_reads, out->signal)
            if (f32) { if (pa) CHUNK_EMIT(true, true); else CHUNK_EMIT(true, false); }
            else { if (pa) CHUNK_EMIT(false, true); else CHUNK_EMIT(false, false); }
#undef CHUNK_EMIT
        }
        // pass 3, labels
        if (want_labels)
            hipLaunchKernelGGL(k_chunk_labels, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, P, (const ReadDesc*)b->d_reads, (const uint8_t*)b->d_bases,
                               c->use_dwell_stream ? (const uint16_t*)c->cset[b->cset].d_dwell : (const uint16_t*)nullptr, (int)c->cfg.profile.dwell_mean,
                               (c->cfg.flags & SQG_RNA) ? 1 : 0, (c->cfg.flags & SQG_METH) ? 1 : 0, J.force == 3 ? 1 : 0, c->chunk.d_ev,
                               cfg->max_label > 0 ? out->labels : (uint8_t*)nullptr, out->label_len);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}

extern "C" int sqg_batch_chunks(sqg_ctx_t* c, sqg_batch_t* b, const sqg_chunk_cfg_t* cfg, const sqg_chunk_out_t* out) {
    return chunks_run(c, b, cfg, out, "sqg_batch_chunks", false);
}
