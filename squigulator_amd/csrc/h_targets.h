// h_targets.h -- sqg_batch_chunk_targets: clean signal, moves and k-mer rows for the chunks of a batch, left on the device
// Host side of include/sqg_targets.h; included by sqg_hip.hip behind h_chunks.h, whose checks, job (the batch's view, the plan) and statistics pass it uses.
#pragma once

// sqg_batch_chunk_targets, and sqg_batch_chunk_targets_trimmed (h_segments.h) with trimmed
static int targets_run(sqg_ctx* c, sqg_batch* b, const sqg_chunk_cfg_t* cfg, const sqg_chunk_targets_t* tg, const char* who, bool trimmed) {
    sqg_chunk_cfg_t cf{};
    if (cfg) { cf = *cfg; cf.max_label = 0; }                            // (ignored here)
    int rc = chunk_check(c, b, cfg ? &cf : nullptr, who, trimmed);
    if (rc) return rc;
    const Check K{c, who};
    if ((rc = K.null(tg, "tg"))) return rc;
    if (((uintptr_t)tg->clean & 15) || ((uintptr_t)tg->clean_raw & 15) || ((uintptr_t)tg->kmer & 15)) return K.bad("clean, clean_raw and kmer must be 16-byte aligned");
    if ((uintptr_t)tg->moves & 7) return K.bad("moves must be 8-byte aligned");
    if (!tg->med2 != !tg->mad4) return K.bad("med2 and mad4: both or neither");
    // (stricter than every output set needs -- only the statistics read the signal slab, a constant-dwell context reads no dwells -- but
    // one rule for the call, the one sqg_batch_chunks has: the batch owns its device results and its dwell set, or nothing is written)
    ChunkJob J;
    if ((rc = chunk_begin(c, b, &cf, who, c->use_dwell_stream, &J, trimmed))) return rc;
    const int n = b->n;
    const long long n_chunks = J.n_chunks;
    if (n_chunks == 0 || !(tg->clean || tg->clean_raw || tg->moves || tg->kmer)) return SQG_OK;      // (n == 0 too) before the device is touched
    for (int i = 0; i < n; i++)
        if (J.plan[i + 1] > J.plan[i] && J.hi[i] - J.lo[i] > (long long)UINT32_MAX) {
            c->err = std::string(who) + ": a read exceeds UINT32_MAX samples";
            return SQG_EOVERFLOW;
        }
    if ((rc = chunk_upload(c, &J))) return rc;
    if (c->use_dwell_stream && (rc = c->chunk.d_start.need(c, (size_t)std::max<long long>(b->n_events, 1)))) return rc;
    const ChunkParams& P = J.P;
    const hipStream_t st = J.st;
    const bool want_consts = tg->clean && cf.norm == SQG_CHUNK_MEDMAD;
    if (want_consts && !tg->med2) { if ((rc = stats_run(c, b, J, nullptr, nullptr))) return rc; }
    else if (want_consts) hipLaunchKernelGGL(k_chunk_consts, dim3((unsigned)((n + CHUNK_WG - 1) / CHUNK_WG)), dim3(CHUNK_WG), 0, st, P, (const int*)tg->med2, (const int*)tg->mad4);
    hipLaunchKernelGGL(k_chunk_index, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, P);
    // pass A: the event starts
    if (c->use_dwell_stream)
        hipLaunchKernelGGL(k_target_scan, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, P, c->chunk.d_start.p);
    // pass B: the rows
    const TargetParams T{c->use_dwell_stream ? c->chunk.d_start.p : nullptr, tg->clean, tg->clean_raw, tg->moves, tg->kmer};
    const TargetGeom geom = tgt_geom(P.L);
    const unsigned wgs = (unsigned)std::min<long long>((n_chunks * geom.n_tiles + geom.cpb - 1) / geom.cpb, 1LL << 20);
    const int clean = !tg->clean ? 0 : 1 + (cf.dtype == SQG_CHUNK_F32 ? 2 : 0) + (cf.norm == SQG_CHUNK_PA ? 1 : 0);
    const int which = clean * 8 + (tg->clean_raw ? 4 : 0) + (tg->moves ? 2 : 0) + (tg->kmer ? 1 : 0);
    switch (which) {
#define TGT_CASE(C, R, M, K) case (C) * 8 + (R) * 4 + (M) * 2 + (K): hipLaunchKernelGGL((k_target_emit<C, R != 0, M != 0, K != 0>), dim3(wgs), dim3(CHUNK_WG), 0, st, P, T); break;
#define TGT_CLEAN(C) TGT_CASE(C, 0, 0, 0) TGT_CASE(C, 0, 0, 1) TGT_CASE(C, 0, 1, 0) TGT_CASE(C, 0, 1, 1) TGT_CASE(C, 1, 0, 0) TGT_CASE(C, 1, 0, 1) TGT_CASE(C, 1, 1, 0) TGT_CASE(C, 1, 1, 1)
    TGT_CLEAN(0) TGT_CLEAN(1) TGT_CLEAN(2) TGT_CLEAN(3) TGT_CLEAN(4)
#undef TGT_CLEAN
#undef TGT_CASE
    }
    // the RNA adaptor's level-shift window, where it reaches into an insert (include/sqg_segments.h)
    if (trimmed && P.bv.rna && (c->cfg.flags & SQG_PREFIX) && (tg->clean || tg->clean_raw))
        hipLaunchKernelGGL(k_target_shift, dim3((unsigned)std::min<long long>(n_chunks, 4096)), dim3(64), 0, st, P, T, clean, segments_shift_code(c));
    HIPCHK(c, hipGetLastError());
    if ((rc = dbg_sync(c, "k_target_emit"))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}

extern "C" int sqg_batch_chunk_targets(sqg_ctx_t* c, sqg_batch_t* b, const sqg_chunk_cfg_t* cfg, const sqg_chunk_targets_t* tg) {
    return targets_run(c, b, cfg, tg, "sqg_batch_chunk_targets", false);
}
