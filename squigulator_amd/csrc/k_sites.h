// k_sites.h -- CpG-centred signal windows of a batch and their methylation labels (include/sqg_sites.h): the sites of every read, then their rows
// Part of the device code of the per-read signal path; included through sqg_kernels.h (see there for the overview).
//
//   k_site_scan<MODE>    one workgroup per read over the dwell scan of k_chunks.h (chunk_for_event_tiles): event a tests the candidate at
//                        p = a + f from two byte loads, takes w0 and the fit test from the E the scan carries, and the fits are ranked in
//                        event order by a second workgroup scan with a carry from tile to tile.  MODE 0 writes the read's count (the plan);
//                        MODE 1 one record per site at site_off[r] + rank, and site_read / site_pos / win_start / label for the caller.  No
//                        per-event array is made.
//   k_site_emit<F32, PA> one wavefront per site at a time.  The signal row through k_chunks.h's row function (chunk_row8: the window starts
//                        at any sample of the read), a lane 8 samples.  context straight from the bases.  ctx_start
//                        needs no global prefix sum: E[a] = w0 + before is known, and the at most 256 boundaries around it are a prefix
//                        sum, inside the wavefront, of the dwells on either side of a.
// The statistics are k_chunks.h's pass over the whole reads (h_sites.h runs stats_run).
#pragma once

#define SITE_CTX_SEGS 4                              // 64-entry steps of a ctx_start row: B + 1 <= 256 entries

struct SiteRec {                                     // 16 bytes
    long long w0;                                    // first sample of the window within its read
    int p, read;                                     // the site's base within its read; the read
};

struct SiteParams {
    BatchView bv;
    const uint8_t* skip;                             // [n_reads] 1: a read shorter than a k-mer (its stand-in sequence has no sites); null: none is
    int L, before, focus, B, cb;
    int* count;                                      // [n_reads] MODE 0: sites of every read
    const long long* site_off;                       // [n_reads+1] MODE 1 and the emit: first site of every read
    long long n_sites;
    SiteRec* rec;                                    // [n_sites]
    uint8_t* label; int* site_read; int* site_pos; long long* win_start;   // the caller's, may be null
    const float2* consts;                            // [n_reads] {median, 1 / (1.4826 MAD)} (k_chunk_stats)
    void* signal; uint8_t* context; int* ctx_start;  // the caller's, may be null
};

template <int MODE>
__global__ __launch_bounds__(CHUNK_WG) void k_site_scan(SiteParams Q) {
    __shared__ unsigned long long sh[8];
    const BatchView& V = Q.bv;
    const int r = blockIdx.x;
    if (Q.skip && Q.skip[r]) { if (MODE == 0 && threadIdx.x == 0) Q.count[r] = 0; return; }
    const ReadDesc rd = V.reads[r];
    const long long n = V.sig_off[r + 1] - V.sig_off[r];
    const int ne = rd.ne0, len = rd.len0, f = Q.focus, meth = V.meth;
    const uint8_t* bp = V.bases + rd.base_off;
    const long long first = MODE ? Q.site_off[r] : 0;
    const long long before = Q.before, L = Q.L;
    unsigned long long ranked = 0;                          // sites of the tiles so far
    chunk_for_event_tiles(ChunkOrigin{rd.ev_off, rd.base_off, ne}, V.dwell, V.const_sps, sh, [&](int e0, unsigned long long E, const int (&d)[4]) {
        unsigned int fit = 0;
        uint8_t b0[4];
        long long w0[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int p = e0 + q + f;                       // (e < ne: p <= len - 1)
            b0[q] = 0; w0[q] = (long long)E - before;
            if (e0 + q < ne && p + 1 < len) {
                b0[q] = bp[p];
                const bool cand = bp[p + 1] == 'G' && (b0[q] == 'C' || (meth && b0[q] == 'M'));
                if (cand && w0[q] >= 0 && w0[q] + L <= n) fit |= 1u << q;
            }
            E += (unsigned long long)d[q];
        }
        unsigned long long total;
        unsigned long long rank = ranked + chunk_scan_excl((unsigned long long)__popc(fit), sh, &total);
        ranked += total;
        if (MODE) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (!(fit >> q & 1u)) continue;
                const long long s = first + (long long)rank++;
                const int p = e0 + q + f;
                Q.rec[s] = SiteRec{w0[q], p, r};
                if (Q.label) Q.label[s] = b0[q] == 'M' ? 1 : 0;
                if (Q.site_read) Q.site_read[s] = r;
                if (Q.site_pos) Q.site_pos[s] = p;
                if (Q.win_start) Q.win_start[s] = w0[q];
            }
        }
    });
    if (MODE == 0 && threadIdx.x == 0) Q.count[r] = (int)ranked;
}

// A workgroup takes CHUNK_WG / 64 sites at a time, one per wavefront (every loop bound below is the same for the lanes of a wavefront).
template <bool F32, bool PA>
__global__ __launch_bounds__(CHUNK_WG) void k_site_emit(SiteParams Q) {
    const BatchView& V = Q.bv;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int per = CHUNK_WG / 64, g8 = Q.L >> 3, B = Q.B, cb = Q.cb;
    for (long long s = (long long)blockIdx.x * per + wv; s < Q.n_sites; s += (long long)gridDim.x * per) {
        const SiteRec sr = Q.rec[s];
        const int r = sr.read;
        const ReadDesc rd = V.reads[r];
        if (Q.signal) {
            const int16_t* src0 = V.sig + V.sig_off[r] + sr.w0;
            const float2 cs = PA ? make_float2(0.f, 0.f) : Q.consts[r];          // (PA: no statistics pass has run)
            const double offset = PA ? rd.offset : 0.0;
            for (int w = lane; w < g8; w += 64) chunk_row8<F32, PA>(V, src0 + (long long)w * 8, cs, offset, Q.signal, s * (long long)Q.L + (long long)w * 8);
        }
        if (Q.context) {
            uint8_t* row = Q.context + s * (long long)B;
            for (int i = lane; i < B; i += 64) {
                const int pos = sr.p - cb + i;
                row[i] = (pos >= 0 && pos < rd.len0) ? (uint8_t)chunk_label_code(V.bases[rd.base_off + pos], V.meth) : (uint8_t)0;
            }
        }
        if (Q.ctx_start) {
            // entry i belongs to event e = a - cb + i; S[i]: the dwells of the row's events in front of it (those outside the read count 0),
            // so that E[e] = E[a] + S[i] - S[cb], and E[a] - w0 = before
            const int ea = sr.p - Q.focus - cb, ne = rd.ne0, segs = (B + 1 + 63) >> 6;
            int S[SITE_CTX_SEGS], carry = 0;
#pragma unroll
            for (int g = 0; g < SITE_CTX_SEGS; g++) {
                S[g] = 0;
                if (g >= segs) continue;
                const int i = 64 * g + lane, e = ea + i;
                const int v = (i < B && e >= 0 && e < ne) ? (V.dwell ? (int)V.dwell[rd.ev_off + e] : V.const_sps) : 0;
                int inc = v;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int o = __shfl_up(inc, d, 64);
                    if (lane >= d) inc += o;
                }
                S[g] = carry + inc - v;
                carry += __shfl(inc, 63, 64);
            }
            int at = S[0];
#pragma unroll
            for (int g = 1; g < SITE_CTX_SEGS; g++) if ((cb >> 6) == g) at = S[g];
            const int s_cb = __shfl(at, cb & 63, 64);
            int* row = Q.ctx_start + s * (long long)(B + 1);
#pragma unroll
            for (int g = 0; g < SITE_CTX_SEGS; g++) {
                const int i = 64 * g + lane, e = ea + i;
                if (g >= segs || i > B) continue;
                row[i] = e <= 0 ? 0 : e >= ne ? Q.L : min(max(Q.before + S[g] - s_cb, 0), Q.L);
            }
        }
    }
}
