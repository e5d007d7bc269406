// h_map.h -- sqg_map_track, sqg_batch_map: the genome's level track and subsequence DTW of the caller's event rows against it, left on the device
// Host side of include/sqg_map.h; included by sqg_hip.hip behind h_call.h.  The opening of the checks and the lifetime rule are h_chunks.h's,
// the rows' check and upload h_align.h's (rows_off_check, rows_upload).
#pragma once

// the contexts of include/sqg_map.h
static int map_context(const Check& K, const sqg_ctx* c) {
    if (c->cfg.flags & SQG_RNA) return K.bad("mapping: not with SQG_RNA");
    if (c->cfg.flags & SQG_PREFIX) return K.bad("mapping: not with SQG_PREFIX");
    return SQG_OK;
}

extern "C" int sqg_map_track(sqg_ctx_t* c, int64_t lo, int64_t hi, const int32_t* levels, int32_t* fwd, int32_t* rev) {
    static const char who[] = "sqg_map_track";
    if (!c) return SQG_EINVAL;
    const Check K{c, who};
    int rc;
    if ((rc = map_context(K, c)) || (rc = K.null(levels, "levels"))) return rc;
    if (!c->genome_loaded) { c->err = std::string(who) + ": no genome is loaded"; return SQG_ESEQUENCE; }
    if (lo < 0) return K.bad("lo must not be negative");
    if (hi < lo) return K.bad("hi must not be below lo");
    if (hi > c->genome.sum) return K.bad("hi must not exceed the genome's length");
    if (hi - lo > SQG_MAP_MAX_WINDOW) return K.bad("hi - lo must not exceed 1<<24");
    if (hi == lo || (!fwd && !rev)) return SQG_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const MapTrackParams T{c->d_genome, c->d_contig_off, c->genome.n_contigs, c->genome.sum, lo, hi, c->k, (c->cfg.flags & SQG_METH) ? 1 : 0, levels, fwd, rev};
    hipLaunchKernelGGL(k_map_track, dim3((unsigned)((hi - lo + 255) / 256)), dim3(256), 0, c->stream, T);
    if ((rc = launched(c, "k_map_track"))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SQG_OK;
}

// The spans of k_map_dp over n_tiles tiles: enough of them that n_waves wavefronts of (read, strand) oversubscribe the device two-fold (32
// per compute unit, at the kernel's 4 per SIMD), but none shorter than twice the halo it walks first, so that at most a third of a
// wavefront's tiles are walked for nothing.  A launch holds at most 2^30 wavefronts: runs of spans, and of reads within them.  (The
// development build takes a cap N from SQG_TEST_MAP_TILES: a span is at most N tiles long, a launch holds at most N tiles of the window
// and at most N wavefronts -- one read's at the least --, so a test reaches a span whose halo is cut at u = 0, a second launch over the
// same window and a launch that does not begin at read 0 with a window of two tiles and a bit and a handful of reads.)
static void map_spans(const sqg_ctx* c, long long n_waves, int n_tiles, int max_m, int* span_tiles, int* spans_per_launch, long long* waves_per_launch) {
    const int halo = (2 * (max_m - 1) + MAP_TILE - 1) / MAP_TILE;
    const long long want = std::max(1LL, (32LL * c->num_cu + n_waves - 1) / n_waves);
    long long st = (n_tiles + want - 1) / want;
    st = std::min<long long>(std::max<long long>(st, std::max(1, 2 * halo)), n_tiles);
    const char* knob = SQG_DEV_ENV("SQG_TEST_MAP_TILES");
    const long long cap = std::max(1, dev_env_int(knob, 1 << 20));
    st = std::min(st, cap);
    *span_tiles = (int)st;
    *spans_per_launch = (int)std::max(1LL, cap / st);
    *waves_per_launch = knob ? cap : 1LL << 30;
}

extern "C" int sqg_batch_map(sqg_ctx_t* c, sqg_batch_t* b, const sqg_map_cfg_t* cfg, const int64_t* row_off, const sqg_align_in_t* in,
                             const sqg_align_scale_t* scale, const sqg_map_track_t* track, const sqg_map_out_t* out) {
    static const char who[] = "sqg_batch_map";
    int rc = check_open(c, b, cfg, "cfg", who);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = map_context(K, c))) return rc;
    if ((rc = K.null(row_off, "row_off")) || (rc = K.null(in, "in")) || (rc = K.null(in->sum, "in->sum")) || (rc = K.null(in->len, "in->len")) ||
        (rc = K.null(track, "track")) || (rc = K.null(out, "out"))) return rc;
    if (scale && ((rc = K.null(scale->gain, "scale->gain")) || (rc = K.null(scale->shift, "scale->shift")))) return rc;
    if (cfg->stay_pen < 0 || cfg->stay_pen > (1 << 17)) return K.bad("stay_pen must be in 0 .. 1<<17");
    if (cfg->skip_pen < 0 || cfg->skip_pen > (1 << 17)) return K.bad("skip_pen must be in 0 .. 1<<17");
    if (cfg->cost_cap < 1 || cfg->cost_cap > (1 << 17)) return K.bad("cost_cap must be in 1 .. 1<<17");
    if (cfg->row_first < 0) return K.bad("row_first must not be negative");
    if (cfg->row_count < 1 || cfg->row_count > SQG_MAP_MAX_ROWS) return K.bad("row_count must be in 1 .. 4096");
    if (cfg->strands == 0 || (cfg->strands & ~(SQG_MAP_PLUS | SQG_MAP_MINUS))) return K.bad("strands must be SQG_MAP_PLUS, SQG_MAP_MINUS or both");
    if (track->hi < track->lo) return K.bad("track: hi must not be below lo");
    if (track->hi - track->lo > SQG_MAP_MAX_WINDOW) return K.bad("track: hi - lo must not exceed 1<<24");
    const int W = (int)(track->hi - track->lo);
    if (W > 0 && (cfg->strands & SQG_MAP_PLUS) && (rc = K.null(track->fwd, "track->fwd"))) return rc;
    if (W > 0 && (cfg->strands & SQG_MAP_MINUS) && (rc = K.null(track->rev, "track->rev"))) return rc;
    const int n = b->n;
    if ((rc = rows_off_check(K, n, row_off)) || (rc = K.ran(b))) return rc;
    if ((rc = chunk_owned(c, b, who, c->use_dwell_stream)) || n == 0) return rc;
    if (!out->map_cost && !out->map_step && !out->map_key0 && !out->map_key1 && !out->map_cost_other) return SQG_OK;
    MapScratch& X = c->map;
    MapParams P{}; RowsIn R{};
    if ((rc = rows_upload(c, batch_view(c, b), row_off, &R))) return rc;
    // the mapped rows of every read, and where its q starts
    std::vector<long long> q_off((size_t)n + 1);
    int max_m = 0;
    q_off[0] = 0;
    for (int r = 0; r < n; r++) {
        const long long m = std::min<long long>(std::max<long long>(row_off[r + 1] - row_off[r] - cfg->row_first, 0), cfg->row_count);
        q_off[(size_t)r + 1] = q_off[(size_t)r] + m;
        max_m = std::max(max_m, (int)m);
    }
    const hipStream_t st = c->stream;
    P.row_off = R.row_off; P.sum = (const long long*)in->sum; P.len = in->len;
    P.gain = scale ? scale->gain : nullptr; P.shift = scale ? scale->shift : nullptr;
    P.fwd = track->fwd; P.rev = track->rev; P.lo = track->lo; P.hi = track->hi;
    P.W = W; P.n_reads = n; P.row_first = cfg->row_first; P.row_count = cfg->row_count;
    P.stay_pen = cfg->stay_pen; P.skip_pen = cfg->skip_pen; P.cost_cap = cfg->cost_cap;
    if (cfg->strands & SQG_MAP_PLUS) P.strand_of[P.n_strands++] = 0;
    if (cfg->strands & SQG_MAP_MINUS) P.strand_of[P.n_strands++] = 1;
    P.map_cost = out->map_cost; P.map_step = (signed char*)out->map_step; P.map_key0 = (long long*)out->map_key0;
    P.map_key1 = (long long*)out->map_key1; P.map_cost_other = out->map_cost_other;
    if (max_m > 0 && W > 0) {
        P.n_tiles = (W + MAP_TILE - 1) / MAP_TILE;
        int spans_per_launch; long long waves_per_launch;
        map_spans(c, (long long)n * P.n_strands, P.n_tiles, max_m, &P.span_tiles, &spans_per_launch, &waves_per_launch);
        P.n_spans = (P.n_tiles + P.span_tiles - 1) / P.span_tiles;
        if ((rc = X.d_qoff.need(c, (size_t)n + 1)) || (rc = X.d_q.need(c, (size_t)q_off[(size_t)n])) ||
            (rc = X.d_rec.need(c, (size_t)n * P.n_strands * P.n_spans))) return rc;
        HIPCHK(c, hipMemcpyAsync(X.d_qoff.p, q_off.data(), ((size_t)n + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
        P.q_off = X.d_qoff.p; P.q = X.d_q.p; P.rec = X.d_rec.p;
        hipLaunchKernelGGL(k_map_rows, dim3((unsigned)n), dim3(256), 0, st, P);
        if ((rc = launched(c, "k_map_rows"))) return rc;
        // the programme: launches over runs of spans, and of reads where the grid would pass the launch's wavefronts
        const size_t lds = sizeof(int4) * (size_t)std::max(max_m - 1, 1);
        for (P.span_lo = 0; P.span_lo < P.n_spans; P.span_lo += spans_per_launch) {
            P.spans_here = std::min(spans_per_launch, P.n_spans - P.span_lo);
            const int reads_per_launch = (int)std::min<long long>(n, std::max(1LL, waves_per_launch / ((long long)P.n_strands * P.spans_here)));
            for (P.read_lo = 0; P.read_lo < n; P.read_lo += reads_per_launch) {
                const long long reads_here = std::min(reads_per_launch, n - P.read_lo);
                hipLaunchKernelGGL(k_map_dp, dim3((unsigned)(reads_here * P.n_strands * P.spans_here)), dim3(64), lds, st, P);
                if ((rc = launched(c, "k_map_dp"))) return rc;
            }
        }
    }
    // (without a mapped row or a position k_map_finish reads neither the offsets nor a record: row_off alone says so)
    hipLaunchKernelGGL(k_map_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P);
    if ((rc = launched(c, "k_map_finish"))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}
