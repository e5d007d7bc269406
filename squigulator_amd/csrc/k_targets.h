// k_targets.h -- per-sample targets of a batch's chunks (include/sqg_targets.h): event starts, then clean signal / moves / k-mer rows
// Part of the device code of the per-read signal path; included through sqg_kernels.h (see there for the overview).
//
//   k_target_scan    pass A, one workgroup per read: ev_start[e] = E[e], the first generation-order sample of event e, relative to the read
//                    (chunk_for_event_starts, k_chunks.h: the scan k_chunk_labels runs).  Not run in constant-dwell contexts, where E[e] = e * sps.
//   k_target_emit    pass B, streaming: writes up to 9 B per sample and reads next to nothing.  A workgroup takes TGT_TILE generation-order
//                    samples of one chunk at a time (or 256 / (L / 16) whole chunks when L is smaller), a thread 16 consecutive ones:
//                      1. the first event that starts in the tile: one search over ev_start, eight probes a round (their loads in flight
//                         together: 5 rounds of latency for 2^15 events instead of 15)
//                      2. every event that starts in the tile sets the byte of its first sample in LDS (one byte per sample: 16 B per thread,
//                         read back conflict-free in one ds_read_b128) -- that byte row IS the moves row
//                      3. a scan of the bytes counts the tile's events and gives every thread the event of its first sample; rank, level and
//                         code are computed once per event, all lanes busy, into LDS (computed per thread as it walks its samples -- 16
//                         divergent, dependent base -> pore-table gathers per wavefront -- the kernel took 81 ms instead of 4 on the
//                         headline batch: measured); a thread then walks its 16 samples and picks the entries up
//                      4. 16-byte stores: one per 8 samples of clean_raw / F16 clean, two of kmer / F32 clean, one per 16 samples of moves
//                    RNA: the same in generation order; a thread's 16 samples are 16 consecutive stored ones in reverse.
// The template parameters say which outputs are wanted: the others cost nothing.
#pragma once

#define TGT_SPT 16                        // samples per thread: a row of moves leaves in 16-byte stores
#define TGT_TILE (CHUNK_WG * TGT_SPT)     // samples per workgroup and pass

struct TargetParams {                     // beside the job's ChunkParams
    const uint32_t* ev_start;             // [n_events] pass A's output; null: constant dwell
    void* clean; int16_t* clean_raw; uint8_t* moves; uint32_t* kmer;
};

__global__ __launch_bounds__(CHUNK_WG) void k_target_scan(ChunkParams P, uint32_t* __restrict__ ev_start) {
    __shared__ unsigned long long sh[8];
    const int r = blockIdx.x;
    if (P.chunk_off[r + 1] == P.chunk_off[r]) return;       // no chunk asks for this read's events
    const ChunkOrigin og = chunk_origin(P, P.bv.reads[r], r);
    const uint16_t* __restrict__ dwell = P.bv.dwell;
    __builtin_assume(dwell != nullptr);                     // (the host launches this pass in dwell-stream contexts only)
    chunk_for_event_starts(og, dwell, 0, sh, [&](int e, unsigned long long E, int) {
        ev_start[og.ev_off + e] = (uint32_t)E;              // (the host has checked: the read has at most UINT32_MAX samples)
    });
}

// k_target_emit's split of its work, for the kernel and the host that sizes its grid: tiles per chunk, threads per tile, tiles of a workgroup at a time
struct TargetGeom { int n_tiles, tpc, cpb; };
__host__ __device__ static inline TargetGeom tgt_geom(int L) {
    const int tpc = ((L < TGT_TILE ? L : TGT_TILE) + TGT_SPT - 1) / TGT_SPT;
    return {(L + TGT_TILE - 1) / TGT_TILE, tpc, CHUNK_WG / tpc};
}

// the first e in [0, ne) with E[e] >= g, ne if there is none.  E ascends.  Eight probes a round cut [lo, hi] to less than an eighth.
__device__ static inline int tgt_lower_bound(const uint32_t* __restrict__ E, int ne, uint32_t g) {
    int lo = 0, hi = ne;                                    // the answer is in [lo, hi]
    while (lo < hi) {
        const int step = (hi - lo + 7) >> 3;
        uint32_t v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = E[min(lo + (i + 1) * step - 1, hi - 1)];
        int cnt = 0;                                        // probes below g: a prefix of those inside [lo, hi)
#pragma unroll
        for (int i = 0; i < 8; i++) cnt += (lo + (i + 1) * step - 1 <= hi - 1 && v[i] < g) ? 1 : 0;
        lo += cnt * step;                                   // E[lo - 1] < g
        const int p = lo + step - 1;                        // the next probe, if it was inside: E[p] >= g
        if (cnt < 8 && p <= hi - 1) hi = p;
    }
    return lo;
}

// CLEAN: 0 not wanted, 1 F16 MEDMAD, 2 F16 PA, 3 F32 MEDMAD, 4 F32 PA
template <int CLEAN, bool RAW, bool MOVES, bool KMER>
__global__ __launch_bounds__(CHUNK_WG) void k_target_emit(ChunkParams P, TargetParams T) {
    constexpr bool F32 = CLEAN >= 3, PA = CLEAN == 2 || CLEAN == 4, VALUES = CLEAN != 0 || RAW || KMER;
    __shared__ uint32_t mark[CHUNK_WG * (TGT_SPT / 4)];     // one byte per sample of the tile: 1 where an event starts
    __shared__ unsigned long long sh[8];
    __shared__ uint32_t before[CHUNK_WG], upto[CHUNK_WG];   // event starts in front of every thread's samples / up to its last one
    // what the tile's events give: entry q of a chunk's region is event e_lo - 1 + q (the one that holds the sample in front of the tile's
    // first, then those that start in the tile: at most tile + 1 per chunk, dwell being at least 1).  Only the wanted ones take LDS.
    constexpr int EV_N = TGT_TILE + CHUNK_WG / 4;           // chunks of a workgroup: at most 64 (L = 64), one spare entry each
    __shared__ uint32_t ev_rank[KMER ? EV_N : 1];
    __shared__ int ev_code[RAW ? EV_N : 1];
    __shared__ float ev_x[CLEAN != 0 ? EV_N : 1];
    const BatchView& V = P.bv;
    const int t = threadIdx.x;
    const auto [n_tiles, tpc, cpb] = tgt_geom(P.L);
    const int sub = t / tpc, w0 = t - sub * tpc;
    const long long n_items = P.n_chunks * n_tiles;
    for (long long base = (long long)blockIdx.x * cpb; base < n_items; base += (long long)gridDim.x * cpb) {
        const long long item = base + sub;
        const bool active = sub < cpb && item < n_items;
        *reinterpret_cast<uint4*>(&mark[4 * t]) = make_uint4(0u, 0u, 0u, 0u);
        long long c = 0, gt0 = 0, ev_off = 0, base_off = 0;
        int tl = 0, r = 0, ne = 0, tlen = 0, e_lo = 0;
        double offset = 0.0;
        const uint32_t* E = nullptr;
        if (active) {
            c = n_tiles == 1 ? item : item / n_tiles;
            tl = (int)(item - c * n_tiles);
            r = P.chunk_read[c];
            const long long j = c - P.chunk_off[r], n = P.hi[r] - P.lo[r];
            gt0 = (V.rna ? n - j * P.S - P.L : j * P.S) + (long long)tl * TGT_TILE;        // the tile's first generation-order sample
            tlen = min(TGT_TILE, P.L - tl * TGT_TILE);
            const ReadDesc rd = V.reads[r];
            const ChunkOrigin og = chunk_origin(P, rd, r);
            ne = og.ne; ev_off = og.ev_off; base_off = og.base_off; offset = rd.offset;
            if (T.ev_start) { E = T.ev_start + ev_off; e_lo = tgt_lower_bound(E, ne, (uint32_t)gt0); }
            else e_lo = (int)min((gt0 + V.const_sps - 1) / V.const_sps, (long long)ne);
        }
        __syncthreads();
        if (active) {
            const long long gt1 = gt0 + tlen;
            for (int e = e_lo + w0; e < ne; e += tpc) {
                const long long v = E ? (long long)E[e] : (long long)e * V.const_sps;
                if (v >= gt1) break;
                const int x = (int)(v - gt0);               // 0 <= x < tlen <= 16 tpc: inside this chunk's 4 tpc words
                atomicOr(&mark[4 * sub * tpc + (x >> 2)], 1u << (8 * (x & 3)));
            }
        }
        __syncthreads();
        const uint4 mw = *reinterpret_cast<const uint4*>(&mark[4 * t]);
        const uint32_t m4[4] = {mw.x, mw.y, mw.z, mw.w};
        uint32_t ex = 0;
        if (VALUES) {
            unsigned long long total;
            ex = (uint32_t)chunk_scan_excl((unsigned long long)(active ? __popc(mw.x) + __popc(mw.y) + __popc(mw.z) + __popc(mw.w) : 0), sh, &total);
            before[t] = ex;
            upto[t] = ex + (uint32_t)(active ? __popc(mw.x) + __popc(mw.y) + __popc(mw.z) + __popc(mw.w) : 0);
            __syncthreads();
            if (active) {                                   // rank, level and code ONCE per event, all lanes busy, the loads of a round in flight together
                const int nq = (int)(upto[sub * tpc + tpc - 1] - before[sub * tpc]) + 1;
                float2 cs = make_float2(0.f, 0.f);
                if (CLEAN != 0 && !PA) cs = P.consts[r];
                for (int q = w0; q < nq; q += tpc) {
                    const int ec = min(max(e_lo - 1 + q, 0), ne - 1);          // (every index stays inside the read)
                    const uint32_t rank = kmer_rank_wide(V.bases + base_off + ec, V.k, V.meth);
                    const int at = sub * (TGT_SPT * tpc + 1) + q;
                    if (KMER) ev_rank[at] = rank;
                    if (CLEAN != 0 || RAW) {
                        const int code = (int)level_code(V.model, rank, V.dig, V.range, offset);
                        if (RAW) ev_code[at] = code;
                        if (CLEAN != 0) ev_x[at] = PA ? chunk_norm_pa(code, offset, V.range, V.dig) : chunk_norm_medmad(code, cs);
                    }
                }
            }
            __syncthreads();
        }
        if (!active || TGT_SPT * w0 >= tlen) continue;
        const int xc = tl * TGT_TILE + TGT_SPT * w0;        // the thread's first sample within the chunk, generation order
        const bool two = TGT_SPT * w0 + 8 < tlen;           // L is a multiple of 8: the last thread of a row may have 8 samples
        if (VALUES) {
            int q = sub * (TGT_SPT * tpc + 1) + (int)(ex - before[sub * tpc]);   // the entry of the sample in front of the thread's first
#pragma unroll
            for (int grp = 0; grp < 2; grp++) {
                if (grp == 1 && !two) break;
                int rr[8]; uint32_t kk[8]; float xx[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    q += (int)((m4[2 * grp + (i >> 2)] >> (8 * (i & 3))) & 1u);
                    rr[i] = RAW ? ev_code[q] : 0; kk[i] = KMER ? ev_rank[q] : 0u; xx[i] = CLEAN != 0 ? ev_x[q] : 0.f;
                }
                const int xg = xc + 8 * grp;
                const long long at = c * (long long)P.L + (V.rna ? P.L - 8 - xg : xg);
                if (V.rna) {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int a = rr[i]; rr[i] = rr[7 - i]; rr[7 - i] = a;
                        const uint32_t b = kk[i]; kk[i] = kk[7 - i]; kk[7 - i] = b;
                        const float f = xx[i]; xx[i] = xx[7 - i]; xx[7 - i] = f;
                    }
                }
                if (RAW) {
                    uint4 v;
                    v.x = ((uint32_t)rr[0] & 0xffffu) | ((uint32_t)rr[1] << 16); v.y = ((uint32_t)rr[2] & 0xffffu) | ((uint32_t)rr[3] << 16);
                    v.z = ((uint32_t)rr[4] & 0xffffu) | ((uint32_t)rr[5] << 16); v.w = ((uint32_t)rr[6] & 0xffffu) | ((uint32_t)rr[7] << 16);
                    *reinterpret_cast<uint4*>(T.clean_raw + at) = v;
                }
                if (KMER) {
                    uint4* o = reinterpret_cast<uint4*>(T.kmer + at);
                    o[0] = make_uint4(kk[0], kk[1], kk[2], kk[3]);
                    o[1] = make_uint4(kk[4], kk[5], kk[6], kk[7]);
                }
                if (CLEAN != 0) chunk_store8<F32>(T.clean, at, xx);
            }
        }
        if (MOVES) {
            // the bytes of LDS are the row; RNA: in reverse.  One 16-byte store where the row's address allows (always when L is a multiple
            // of 16 and the array is 16-byte aligned), else 8-byte ones -- the interface asks for 8-byte alignment only.
            const int len = two ? 16 : 8;
            uint8_t* dst = T.moves + c * (long long)P.L + (V.rna ? P.L - len - xc : xc);
            uint32_t w[4];
            if (!V.rna) { w[0] = m4[0]; w[1] = m4[1]; w[2] = m4[2]; w[3] = m4[3]; }
            else if (two) { w[0] = __builtin_bswap32(m4[3]); w[1] = __builtin_bswap32(m4[2]); w[2] = __builtin_bswap32(m4[1]); w[3] = __builtin_bswap32(m4[0]); }
            else { w[0] = __builtin_bswap32(m4[1]); w[1] = __builtin_bswap32(m4[0]); w[2] = 0u; w[3] = 0u; }
            if (two && ((uintptr_t)dst & 15u) == 0) *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
            else {
                *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
                if (two) *reinterpret_cast<uint2*>(dst + 8) = make_uint2(w[2], w[3]);
            }
        }
    }
}
