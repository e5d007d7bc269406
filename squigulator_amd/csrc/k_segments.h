// k_segments.h -- the segments of a read with an attached prefix (include/sqg_segments.h): stall, adaptor, poly-A, insert; the insert's view
// Part of the device code of the per-read signal path; included through sqg_kernels.h (see there for the overview).
//
//   k_segments       one wavefront per read: the dwell sums of the prefix events at the edges of the read -- at most 85 events (DNA) or
//                    ne0 - len + ne1 <= 267 (RNA), under 600 B of 2-byte dwells -- give every bound; the insert is never scanned.  Writes
//                    seg / shift for the caller and, into context scratch, the span [lo, hi) and the ChunkView (k_chunks.h) the chunk
//                    kernels then take for "the read".  A constant-dwell context (no dwell stream) gets the same numbers from the event
//                    counts, with no loads.  seg_ranges: the event ranges of the segments, for this kernel and k_evtab_scan (k_events_table.h).
//   k_target_shift   the trimmed targets of an RNA prefix context: lowers clean_raw / clean where the adaptor's level-shift window reaches
//                    into the insert.  The window does not follow an event boundary, so k_target_emit's per-event values cannot carry it.
//                    A chunk outside the window (every chunk of every input seen so far: include/sqg_segments.h) costs one comparison.
#pragma once

struct SegParams {
    BatchView bv;                    // (kind, p0, p1: k_chunks.h)
    long long shift_len;             // SEG_RNA: samples of the level-shift window, strlen(adaptor) * (int)dwell_mean (src/genread.c:79)
    long long* seg;                  // [n_reads][5] output, may be null
    long long* shift;                // [n_reads][2] output, may be null
    long long* lo; long long* hi;    // [n_reads] the insert's span of the slab
    ChunkView* view;                 // [n_reads]
};

__device__ static inline long long seg_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The event ranges of a read with an attached prefix (include/sqg_segments.h), within chain 0's ne0 events: DNA [0, a) stall, [a, b) adaptor,
// then the insert; RNA [0, a) insert, [a, b) poly-A, [b, ne0) adaptor (chain 1 is the stall).  SEG_NONE: a = b = 0.
struct SegRanges { int a, b; };
__device__ static inline SegRanges seg_ranges(const BatchView& V, const ReadDesc& rd) {
    if (V.kind == SEG_DNA) return {min(V.p0, rd.ne0), min(V.p1, rd.ne0)};
    if (V.kind != SEG_RNA) return {0, 0};
    const int len = max(rd.len0 - V.p1, 0);                 // the read's own bases
    return {min(len, rd.ne0), min(len + V.p0, rd.ne0)};
}

__global__ __launch_bounds__(64) void k_segments(SegParams Q) {
    const BatchView& V = Q.bv;
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= V.n_reads) return;
    const ReadDesc rd = V.reads[r];
    const long long o = V.sig_off[r], n = V.sig_off[r + 1] - o;
    const uint16_t* d = V.dwell ? V.dwell + rd.ev_off : nullptr;
    const long long sps = V.const_sps;
    const auto [a, b] = seg_ranges(V, rd);
    long long s1 = 0, s2 = 0, s3 = 0, w0 = 0, w1 = 0;       // seg = {0, s1, s2, s3, n}, shift = {w0, w1}
    ChunkView v;
    v.sh_lo = 0; v.sh_hi = 0; v.ev0 = 0; v.nev = rd.ne0; v.base0 = 0; v.pad = 0;
    if (V.kind == SEG_DNA) {
        long long sa = 0, sb = 0;
        for (int e = lane; e < b; e += 64) {
            const long long x = d ? (long long)d[e] : sps;
            sb += x;
            if (e < a) sa += x;
        }
        s1 = seg_wave_sum(sa); s2 = s3 = seg_wave_sum(sb);
        v.ev0 = b; v.nev = rd.ne0 - b; v.base0 = b;
    } else if (V.kind == SEG_RNA) {
        const int i1 = a, i2 = b, ne = read_events(rd);
        long long pa = 0, ad = 0, st = 0;                   // samples of poly-A, adaptor, stall
        for (int e = i1 + lane; e < ne; e += 64) {
            const long long x = d ? (long long)d[e] : sps;
            if (e < i2) pa += x; else if (e < rd.ne0) ad += x; else st += x;
        }
        pa = seg_wave_sum(pa); ad = seg_wave_sum(ad); st = seg_wave_sum(st);
        const long long n0 = n - st, g2 = n0 - ad, g1 = g2 - pa;
        s1 = n - n0; s2 = n - g2; s3 = n - g1;
        const long long wl = max(n0 - Q.shift_len, 0LL);    // generation samples [wl, n0) were lowered
        w0 = n - n0; w1 = n - wl;
        v.nev = i1; v.sh_lo = min(wl, g1); v.sh_hi = g1;
    }
    if (lane == 0) {
        if (Q.seg) { long long* q = Q.seg + 5LL * r; q[0] = 0; q[1] = s1; q[2] = s2; q[3] = s3; q[4] = n; }
        if (Q.shift) { Q.shift[2LL * r] = w0; Q.shift[2LL * r + 1] = w1; }
        Q.lo[r] = o + s3; Q.hi[r] = o + n;
        Q.view[r] = v;
    }
}

// One wavefront per chunk at a time.  CLEAN as k_target_emit's template parameter: 0 not wanted, 1 F16 MEDMAD, 2 F16 PA, 3 F32 MEDMAD, 4 F32 PA.
// Runs behind k_target_emit on the same stream and rewrites only the samples inside the window; shift: (int16)(30 dig / range).
__global__ __launch_bounds__(64) void k_target_shift(ChunkParams P, TargetParams T, int clean, int shift) {
    const BatchView& V = P.bv;
    const int lane = threadIdx.x;
    for (long long c = blockIdx.x; c < P.n_chunks; c += gridDim.x) {
        const int r = P.chunk_read[c];
        const ChunkView v = P.view[r];
        if (v.sh_hi <= v.sh_lo) continue;
        const long long n = P.hi[r] - P.lo[r], j = c - P.chunk_off[r];
        const long long cg0 = V.rna ? n - j * P.S - P.L : j * P.S;           // the chunk's first generation-order sample
        const long long lo = max(cg0, v.sh_lo), hi = min(cg0 + P.L, v.sh_hi);
        if (hi <= lo || v.nev <= 0) continue;
        const ReadDesc rd = V.reads[r];
        const uint32_t* E = T.ev_start ? T.ev_start + rd.ev_off + v.ev0 : nullptr;
        const float2 cs = P.consts[r];
        for (long long g = lo + lane; g < hi; g += 64) {
            // the event with E[e] <= g < E[e] + dwell[e]: the one in front of the first that starts behind g
            int e = E ? tgt_lower_bound(E, v.nev, (uint32_t)g + 1u) - 1 : (int)(g / V.const_sps);
            e = min(max(e, 0), v.nev - 1);
            const uint32_t rank = kmer_rank_wide(V.bases + rd.base_off + v.base0 + e, V.k, V.meth);
            int code = (int)level_code(V.model, rank, V.dig, V.range, rd.offset);
            code = (int)(int16_t)(uint16_t)((code - shift) & 0xffff);                             // src/genread.c:83-86: int16 arithmetic wraps
            const long long at = c * (long long)P.L + (V.rna ? cg0 + P.L - 1 - g : g - cg0);
            if (T.clean_raw) T.clean_raw[at] = (int16_t)code;
            if (T.clean && clean) {
                const float x = (clean == 2 || clean == 4) ? chunk_norm_pa(code, rd.offset, V.range, V.dig) : chunk_norm_medmad(code, cs);
                if (clean >= 3) static_cast<float*>(T.clean)[at] = x;
                else static_cast<unsigned short*>(T.clean)[at] = (unsigned short)chunk_f16_bits(x);
            }
        }
    }
}
