// h_targets.h -- sqg_batch_chunk_targets: clean signal, moves and k-mer rows for the chunks of a batch, left on the device
// Host side of include/sqg_targets.h; included by sqg_hip.hip behind h_chunks.h, whose checks, plan and statistics pass it uses.
#pragma once

extern "C" int sqg_batch_chunk_targets(sqg_ctx_t* c, sqg_batch_t* b, const sqg_chunk_cfg_t* cfg, const sqg_chunk_targets_t* tg) {
    static const char who[] = "sqg_batch_chunk_targets";
    sqg_chunk_cfg_t cf{};
    if (cfg) { cf = *cfg; cf.max_label = 0; }                            // (ignored here)
    int rc = chunk_check(c, b, cfg ? &cf : nullptr, who);
    if (rc) return rc;
    auto bad = [&](const char* what) { c->err = std::string(who) + ": " + what; return SQG_EINVAL; };
    if (!tg) return bad("tg must not be NULL");
    if (((uintptr_t)tg->clean & 15) || ((uintptr_t)tg->clean_raw & 15) || ((uintptr_t)tg->kmer & 15)) return bad("clean, clean_raw and kmer must be 16-byte aligned");
    if ((uintptr_t)tg->moves & 7) return bad("moves must be 8-byte aligned");
    if (!tg->med2 != !tg->mad4) return bad("med2 and mad4: both or neither");
    // (stricter than every output set needs -- only the statistics read the signal slab, a constant-dwell context reads no dwells -- but
    // one rule for the call, the one sqg_batch_chunks has: the batch owns its device results and its dwell set, or nothing is written)
    if (b->run_idx + 2 < c->runs || !slot_is_mine(c, b) || (c->use_dwell_stream && !cset_is_mine(c, b))) {
        c->err = std::string(who) + ": the batch's device results have been handed to a later batch";
        return SQG_ESEQUENCE;
    }
    if ((rc = sqg_batch_wait(c, b, nullptr))) return rc;                 // waits for the batch's own kernels; fills sig_off
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int n = b->n;
    if (n == 0 || !(tg->clean || tg->clean_raw || tg->moves || tg->kmer)) return SQG_OK;
    sqg_ctx::Slot& Z = c->slot[b->slot];
    std::vector<long long>& off = c->h_chunk_off;
    off.resize((size_t)n + 1);
    chunk_plan(b, &cf, off.data());
    const long long n_chunks = off[(size_t)n];
    if (n_chunks == 0) return SQG_OK;
    for (int i = 0; i < n; i++)
        if (off[(size_t)i + 1] > off[(size_t)i] && b->sig_off[(size_t)i + 1] - b->sig_off[(size_t)i] > (long long)UINT32_MAX) {
            c->err = std::string(who) + ": a read exceeds UINT32_MAX samples";
            return SQG_EOVERFLOW;
        }

    ChunkParams P{};
    P.sig = Z.d_sig; P.sig_off = Z.d_sigoff; P.n_reads = n; P.n_chunks = n_chunks;
    P.L = cf.chunk_len; P.S = cf.stride; P.W = 0;
    P.hist_max = CHUNK_HIST; P.one_wg_max = 1LL << 22;
    const int force = dev_env_int(SQG_DEV_ENV("SQG_TEST_CHUNK_GENERIC"), 0);      // as in sqg_batch_chunks: which statistics path
    if (force == 1) P.hist_max = 0;
    if (force == 2) P.one_wg_max = 0;
    P.range = c->cfg.profile.range; P.dig = c->cfg.profile.digitisation;
    const bool want_consts = tg->clean && cf.norm == SQG_CHUNK_MEDMAD, own_stats = want_consts && !tg->med2;

    if ((rc = ensure(c, (void**)&c->d_chunk_off, &c->chunk_off_cap, (size_t)n + 1, sizeof(long long)))) return rc;
    if ((rc = ensure(c, (void**)&c->d_chunk_read, &c->chunk_read_cap, (size_t)n_chunks + 1, sizeof(int)))) return rc;
    if (want_consts && (rc = ensure(c, (void**)&c->d_chunk_const, &c->chunk_const_cap, (size_t)n, sizeof(float2)))) return rc;
    if (own_stats) {
        if ((rc = ensure(c, (void**)&c->d_chunk_wide, &c->chunk_wide_cap, (size_t)n + 1, sizeof(unsigned int)))) return rc;
        if ((rc = ensure(c, (void**)&c->d_chunk_ghist, &c->chunk_ghist_cap, (size_t)CHUNK_WIDE_SLOTS * 2 * CHUNK_GBINS, sizeof(unsigned int)))) return rc;
    }
    if (c->use_dwell_stream && (rc = ensure(c, (void**)&c->d_target_start, &c->target_start_cap, (size_t)std::max<long long>(b->n_events, 1), sizeof(uint32_t)))) return rc;
    P.chunk_off = c->d_chunk_off; P.consts = c->d_chunk_const; P.wide_list = c->d_chunk_wide; P.ghist = c->d_chunk_ghist;
    P.chunk_read = c->d_chunk_read;

    const hipStream_t st = c->stream;
    const ReadDesc* reads = (const ReadDesc*)b->d_reads;
    HIPCHK(c, hipMemcpyAsync(c->d_chunk_off, off.data(), ((size_t)n + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    if (own_stats) { if ((rc = chunk_stats_run(c, b, P))) return rc; }
    else if (want_consts) hipLaunchKernelGGL(k_target_consts, dim3((unsigned)((n + CHUNK_WG - 1) / CHUNK_WG)), dim3(CHUNK_WG), 0, st, P, (const int*)tg->med2, (const int*)tg->mad4);
    hipLaunchKernelGGL(k_chunk_index, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, P);
    // pass A: the event starts
    if (c->use_dwell_stream)
        hipLaunchKernelGGL(k_target_scan, dim3((unsigned)n), dim3(CHUNK_WG), 0, st, P, reads, (const uint16_t*)c->cset[b->cset].d_dwell, c->d_target_start);
    // pass B: the rows
    TargetParams T{};
    T.reads = reads; T.bases = (const uint8_t*)b->d_bases; T.model = c->d_model;
    T.ev_start = c->use_dwell_stream ? c->d_target_start : nullptr;
    T.k = c->k; T.meth = (c->cfg.flags & SQG_METH) ? 1 : 0; T.rna = (c->cfg.flags & SQG_RNA) ? 1 : 0; T.const_sps = std::max((int)c->cfg.profile.dwell_mean, 1);
    T.clean = tg->clean; T.clean_raw = tg->clean_raw; T.moves = tg->moves; T.kmer = tg->kmer;
    const int n_tiles = (P.L + TGT_TILE - 1) / TGT_TILE, tpc = (std::min(P.L, TGT_TILE) + TGT_SPT - 1) / TGT_SPT, cpb = CHUNK_WG / tpc;
    const unsigned wgs = (unsigned)std::min<long long>((n_chunks * n_tiles + cpb - 1) / cpb, 1LL << 20);
    const int clean = !tg->clean ? 0 : 1 + (cf.dtype == SQG_CHUNK_F32 ? 2 : 0) + (cf.norm == SQG_CHUNK_PA ? 1 : 0);
    const int which = clean * 8 + (tg->clean_raw ? 4 : 0) + (tg->moves ? 2 : 0) + (tg->kmer ? 1 : 0);
    switch (which) {
#define TGT_CASE(C, R, M, K) case (C) * 8 + (R) * 4 + (M) * 2 + (K): hipLaunchKernelGGL((k_target_emit<C, R != 0, M != 0, K != 0>), dim3(wgs), dim3(CHUNK_WG), 0, st, P, T); break;
#define TGT_CLEAN(C) TGT_CASE(C, 0, 0, 0) TGT_CASE(C, 0, 0, 1) TGT_CASE(C, 0, 1, 0) TGT_CASE(C, 0, 1, 1) TGT_CASE(C, 1, 0, 0) TGT_CASE(C, 1, 0, 1) TGT_CASE(C, 1, 1, 0) TGT_CASE(C, 1, 1, 1)
    TGT_CLEAN(0) TGT_CLEAN(1) TGT_CLEAN(2) TGT_CLEAN(3) TGT_CLEAN(4)
#undef TGT_CLEAN
#undef TGT_CASE
    }
    HIPCHK(c, hipGetLastError());
    if ((rc = dbg_sync(c, "k_target_emit"))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return SQG_OK;
}
