// h_chunks.h -- sqg_chunk_plan, sqg_batch_chunks: labelled, normalised chunks of a batch's signal, left on the device
// Host side of include/sqg_chunks.h (and, with `trimmed`, of the chunk calls of include/sqg_segments.h: h_segments.h); included by sqg_hip.hip (one translation unit with the kernels), in the order listed there.
// What every call that reads a finished batch shares is stated here once: the opening of the argument checks (check_open, Check), the
// kernels' view of the batch (batch_view), the lifetime rule (chunk_owned), the statistics job over the reads' spans (spans_open,
// stats_run) and the choice of a kernel's F32 / PA variant (dispatch).  The chunk calls put their plan on top of the statistics job.
#pragma once

// The opening of a consumer call's checks: no context, then no batch or no second argument (named in the message)
static int check_open(sqg_ctx* c, const void* b, const void* arg, const char* arg_name, const char* who) {
    if (!c) return SQG_EINVAL;
    if (!b || !arg) { c->err = std::string(who) + ": batch and " + arg_name + " must not be NULL"; return SQG_EINVAL; }
    return SQG_OK;
}
// ... and the rest of them, each call in its own order: the message prefix, a NULL argument, "has not been run"
struct Check {
    sqg_ctx* c; const char* who;
    int bad(const std::string& what) const { c->err = std::string(who) + ": " + what; return SQG_EINVAL; }
    int null(const void* p, const char* name) const { return p ? SQG_OK : bad(std::string(name) + " must not be NULL"); }
    int ran(const sqg_batch* b) const { if (b->ran) return SQG_OK; c->err = std::string(who) + ": the batch has not been run"; return SQG_ESEQUENCE; }
};
static bool dtype_ok(uint32_t dtype) { return dtype == SQG_CHUNK_F16 || dtype == SQG_CHUNK_F32; }
static bool norm_ok(uint32_t norm) { return norm == SQG_CHUNK_MEDMAD || norm == SQG_CHUNK_PA; }
static bool trim_ok(int trim) { return trim == 0 || trim == 1; }

// fn(F32, PA) with the two as std::true_type / std::false_type: the launch of the kernel variant a call's dtype and norm ask for
template <class Fn>
static void dispatch(bool f32, bool pa, Fn fn) {
    if (f32) { if (pa) fn(std::true_type{}, std::true_type{}); else fn(std::true_type{}, std::false_type{}); }
    else { if (pa) fn(std::false_type{}, std::true_type{}); else fn(std::false_type{}, std::false_type{}); }
}

// What the consumer kernels take of a run batch (k_chunks.h: BatchView).  The one place on this side that reads the prefix constants.
static BatchView batch_view(const sqg_ctx* c, const sqg_batch* b) {
    const bool prefix = (c->cfg.flags & SQG_PREFIX) != 0, rna = (c->cfg.flags & SQG_RNA) != 0;
    BatchView V{};
    V.reads = (const ReadDesc*)b->d_reads; V.bases = (const uint8_t*)b->d_bases; V.model = c->d_model;
    V.dwell = c->use_dwell_stream ? (const uint16_t*)c->cset[b->cset].d_dwell : (const uint16_t*)nullptr;
    V.sig_off = c->slot[b->slot].d_sigoff; V.sig = c->slot[b->slot].d_sig;
    V.const_sps = (int)c->cfg.profile.dwell_mean;                       // (at least 1: sqg_create refuses dwell_mean < 1.0, h_context.h:78)
    V.k = c->k; V.meth = (c->cfg.flags & SQG_METH) ? 1 : 0; V.rna = rna ? 1 : 0; V.n_reads = b->n;
    V.kind = !prefix ? SEG_NONE : rna ? SEG_RNA : SEG_DNA;
    if (V.kind == SEG_DNA) { V.p0 = (int)strlen(kStallDna); V.p1 = V.p0 + (int)strlen(kAdaptorDna); }
    if (V.kind == SEG_RNA) { V.p0 = kPolyA; V.p1 = kPolyA + (int)strlen(kAdaptorRna); }
    V.range = c->cfg.profile.range; V.dig = c->cfg.profile.digitisation;
    return V;
}
// ... and the events of the RNA stall, chain 1 of every read of an SQG_PREFIX context (ReadDesc::ne1 as h_stage.h sets it); 0 elsewhere
static int batch_stall_events(const sqg_ctx* c) {
    return (c->cfg.flags & SQG_PREFIX) && (c->cfg.flags & SQG_RNA) ? (int)strlen(kStallRna) - c->k + 1 : 0;
}

// trimmed: the calls of include/sqg_segments.h, which cut the insert of a read with an attached prefix and so take SQG_PREFIX contexts
static int chunk_check(sqg_ctx* c, sqg_batch* b, const sqg_chunk_cfg_t* cfg, const char* who, bool trimmed = false) {
    if (int rc = check_open(c, b, cfg, "cfg", who)) return rc;
    const Check K{c, who};
    if (!trimmed && (c->cfg.flags & SQG_PREFIX)) return K.bad("chunks: not with SQG_PREFIX");
    if (cfg->chunk_len < 64 || cfg->chunk_len > (1 << 20) || (cfg->chunk_len & 7)) return K.bad("chunk_len must be a multiple of 8 in 64 .. 1<<20");
    if (cfg->stride < 1) return K.bad("stride must be >= 1");
    if (cfg->max_label < 0 || cfg->max_label > 65535) return K.bad("max_label must be in 0 .. 65535");
    if (!dtype_ok(cfg->dtype)) return K.bad("unknown dtype");
    if (!norm_ok(cfg->norm)) return K.bad("unknown norm");
    return K.ran(b);
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
    if ((rc = Check{c, "sqg_chunk_plan"}.null(n_chunks, "n_chunks"))) return rc;
    if ((rc = sqg_batch_wait(c, b, nullptr))) return rc;
    std::vector<long long>& off = c->chunk.h_off;
    off.resize((size_t)b->n + 1);
    chunk_plan(b, cfg, b->sig_off.data(), b->sig_off.data() + 1, off.data());
    if (chunk_off) for (int i = 0; i <= b->n; i++) chunk_off[i] = (int64_t)off[(size_t)i];
    *n_chunks = (int64_t)off[(size_t)b->n];
    return SQG_OK;
}

// One call's job on a batch: the reads' spans and what the statistics pass needs (spans_open) -- all that sqg_batch_sites,
// sqg_batch_events and sqg_batch_pileup take of it --, and for the chunk calls their plan on top (chunk_begin)
struct ChunkJob {
    ChunkParams P{};                                           // all but the caller's outputs
    const long long* lo = nullptr; const long long* hi = nullptr;   // host: the spans
    int force = 0; hipStream_t st = nullptr;                   // development build: SQG_TEST_CHUNK_GENERIC; the context's stream
    const long long* plan = nullptr; long long n_chunks = 0;   // [n_reads+1] first chunk of every read (host: ChunkScratch::h_off)
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

// The shared opening of every job, behind the caller's argument checks: the batch still owns its device results (and its dwell set, if
// need_dwell), it has finished, the view, the spans.  Host work only, unless trimmed: then the spans come from k_segments and the host
// waits for them, the one synchronisation they need -- once per batch: a trimmed call that follows another on the same batch (the plan,
// then the chunks) finds spans and views in the scratch.  An empty batch leaves J->P.bv.n_reads 0.
static int spans_open(sqg_ctx* c, sqg_batch* b, const char* who, bool need_dwell, bool trimmed, ChunkJob* J) {
    if (trimmed && c->use_dwell_stream) need_dwell = true;              // (k_segments reads the dwells)
    if (int rc = chunk_owned(c, b, who, need_dwell)) return rc;
    const int n = b->n;
    if (n == 0) return SQG_OK;
    ChunkParams& P = J->P;
    P.bv = batch_view(c, b);
    if (trimmed) {
        const bool have = c->chunk.span_of == (const void*)b && c->chunk.span_run == b->run_idx && c->chunk.h_span.size() == 2 * (size_t)n;
        if (!have) { if (int rc = segments_run(c, b, nullptr, nullptr)) return rc; }
        J->lo = c->chunk.h_span.data(); J->hi = J->lo + n;
        P.lo = c->chunk.d_span.p; P.hi = P.lo + n; P.view = c->chunk.d_view.p;
    } else {
        J->lo = b->sig_off.data(); J->hi = J->lo + 1;
        P.lo = P.bv.sig_off; P.hi = P.lo + 1; P.view = nullptr;
    }
    J->st = c->stream;
    // development build: 1 sends every read through the wide path (global histograms), 2 through the long one (several workgroups per read);
    // 3 leaves the statistics alone and makes k_chunk_labels divide in 64 bits, as it does for a read of 2^31 samples or more
    J->force = dev_env_int(SQG_DEV_ENV("SQG_TEST_CHUNK_GENERIC"), 0);
    P.hist_max = J->force == 1 ? 0 : CHUNK_HIST; P.one_wg_max = J->force == 2 ? 0 : 1LL << 22;
    return SQG_OK;
}

// the scratch of the statistics pass, which is also where the emit kernels find the reads' constants
static int stats_scratch(sqg_ctx* c, ChunkJob* J) {
    ChunkScratch& X = c->chunk;
    const size_t n = (size_t)J->P.bv.n_reads;
    int rc;
    if ((rc = X.d_const.need(c, n)) || (rc = X.d_wide.need(c, n + 1)) || (rc = X.d_ghist.need(c, (size_t)CHUNK_WIDE_SLOTS * 2 * CHUNK_GBINS))) return rc;
    J->P.consts = X.d_const.p; J->P.wide_list = X.d_wide.p; J->P.ghist = X.d_ghist.p;
    return SQG_OK;
}

// the statistics pass on the context's stream: every read's {median, 1 / (1.4826 MAD)} over its span into P.consts, med2 / mad4 (the
// caller's, may be null) beside them
static int stats_run(sqg_ctx* c, sqg_batch* b, ChunkJob& J, int* med2, int* mad4) {
    if (int rc = stats_scratch(c, &J)) return rc;
    ChunkParams& P = J.P;
    P.med2 = med2; P.mad4 = mad4;
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
    return launched(c, "k_chunk_stats");
}

// The chunk calls' opening: the statistics job and the plan of cfg over its spans
static int chunk_begin(sqg_ctx* c, sqg_batch* b, const sqg_chunk_cfg_t* cfg, const char* who, bool need_dwell, ChunkJob* J, bool trimmed = false) {
    if (int rc = spans_open(c, b, who, need_dwell, trimmed, J)) return rc;
    const int n = b->n;
    if (n == 0) return SQG_OK;
    c->chunk.h_off.resize((size_t)n + 1);
    chunk_plan(b, cfg, J->lo, J->hi, c->chunk.h_off.data());
    J->plan = c->chunk.h_off.data(); J->n_chunks = J->plan[n];
    ChunkParams& P = J->P;
    P.n_chunks = J->n_chunks; P.L = cfg->chunk_len; P.S = cfg->stride; P.W = cfg->max_label;
    return SQG_OK;
}

// ... and their first device work: the scratch of the shared passes, the plan uploaded
static int chunk_upload(sqg_ctx* c, ChunkJob* J) {
    ChunkScratch& X = c->chunk;
    const size_t n = (size_t)J->P.bv.n_reads;
    int rc;
    if ((rc = stats_scratch(c, J)) || (rc = X.d_off.need(c, n + 1)) || (rc = X.d_read.need(c, (size_t)J->n_chunks + 1))) return rc;
    J->P.chunk_off = X.d_off.p; J->P.chunk_read = X.d_read.p;
    HIPCHK(c, hipMemcpyAsync(X.d_off.p, J->plan, (n + 1) * sizeof(long long), hipMemcpyHostToDevice, J->st));
    return SQG_OK;
}

// sqg_batch_chunks, and sqg_batch_chunks_trimmed (h_segments.h) with trimmed
static int chunks_run(sqg_ctx* c, sqg_batch* b, const sqg_chunk_cfg_t* cfg, const sqg_chunk_out_t* out, const char* who, bool trimmed) {
    int rc = chunk_check(c, b, cfg, who, trimmed);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = K.null(out, "out"))) return rc;
    if (out->signal && ((uintptr_t)out->signal & 15)) return K.bad("signal must be 16-byte aligned");
    ChunkJob J;
    if ((rc = chunk_begin(c, b, cfg, who, c->use_dwell_stream && (out->labels || out->label_len), &J, trimmed)) || J.P.bv.n_reads == 0) return rc;
    if ((rc = chunk_upload(c, &J))) return rc;
    const long long n_chunks = J.n_chunks;
    const int n = b->n;
    const hipStream_t st = J.st;
    ChunkParams& P = J.P;                                               // ... and the caller's outputs
    P.chunk_read_out = out->chunk_read; P.chunk_start_out = (long long*)out->chunk_start;
    const bool want_labels = n_chunks > 0 && ((out->labels && cfg->max_label > 0) || out->label_len);
    if (want_labels && (rc = c->chunk.d_ev.need(c, (size_t)n_chunks))) return rc;
    // pass 1, statistics: the read's constants for the emit kernel, med2 / mad4 for the caller
    const bool want_stats = out->med2 || out->mad4 || (out->signal && n_chunks > 0 && cfg->norm == SQG_CHUNK_MEDMAD);
    if (want_stats && (rc = stats_run(c, b, J, out->med2, out->mad4))) return rc;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(k_chunk_index, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, P);
        // pass 2, emit
        if (out->signal) {
            const int cpb = chunk_emit_geom(P.L).cpb;
            const unsigned wgs = (unsigned)std::min<long long>((n_chunks + cpb - 1) / cpb, 1LL << 20);
            dispatch(cfg->dtype == SQG_CHUNK_F32, cfg->norm == SQG_CHUNK_PA, [&](auto F, auto A) {
                hipLaunchKernelGGL((k_chunk_emit<decltype(F)::value, decltype(A)::value>), dim3(wgs), dim3(CHUNK_WG), 0, st, P, out->signal);
            });
        }
        // pass 3, labels
        if (want_labels)
            hipLaunchKernelGGL(k_chunk_labels, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, P, J.force == 3 ? 1 : 0, c->chunk.d_ev.p,
                               cfg->max_label > 0 ? out->labels : (uint8_t*)nullptr, out->label_len);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}

extern "C" int sqg_batch_chunks(sqg_ctx_t* c, sqg_batch_t* b, const sqg_chunk_cfg_t* cfg, const sqg_chunk_out_t* out) {
    return chunks_run(c, b, cfg, out, "sqg_batch_chunks", false);
}
