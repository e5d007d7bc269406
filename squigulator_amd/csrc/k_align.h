// k_align.h -- banded alignment of event rows to the true events of their read (include/sqg_align.h): the forward pass, then the traceback
// Part of the device code of the per-read signal path; included through sqg_kernels.h behind k_detect.h.
//
//   k_align_forward<TRACE, SCALED>  a row of the dynamic programme has no dependency inside itself, so one wavefront holds one read's band, one cell per
//                        lane, one wavefront per workgroup (the hardware hands the reads out: they differ in length).  D of the row before lives
//                        in registers; a row takes its three predecessors from them by lane shift, offset by how far the band moved (0..2).
//                        The band's move is one wavefront argmin per row: a 64-bit minimum as two 32-bit ones (four DPP steps inside the rows
//                        of 16 lanes, then four lane reads), and the lowest lane of a ballot.  q is clamped to +-2^26 when it is made: |Lv| <=
//                        2^23 and cost_cap <= 2^24, so the cell costs are the header's, and they are 32-bit.  q is fetched and divided 64
//                        rows at a time (one row per lane, read back by lane index); Lv 64 targets at a time into two registers that
//                        cover [tb, tb + 128), from which the band's levels are re-read by lane shift on the rows at which the band moves.
//                        TRACE: the move codes of a row are two ballots, one per code bit; lane 0 stores them (16 B) and lo_i (4 B).
//                        No LDS, no floating point.  SCALED (sqg_batch_align_scaled, include/sqg_scale.h): the read's gain and shift, two
//                        wavefront-uniform values clamped into their ranges, are applied where the tile's q is made -- a multiply, a shift
//                        and an add per 64 rows and lane -- and nothing in the per-row loop changes.
//   k_align_trace        one wavefront per read again.  The traceback is a dependent chain along the read, but only in j: the trace rows'
//                        addresses do not depend on it.  So the wavefront loads 64 trace rows at once, one per lane, walks them back with
//                        lane reads -- wavefront-uniform, scalar arithmetic --, each lane keeps the j of its own row, and al_ev goes out as
//                        one coalesced store per 64 rows.
#pragma once

#define ALN_INF (1ULL << 62)

struct AlignParams {
    BatchView bv;
    const long long* row_off;                        // [n_reads+1] device copy of the caller's
    const long long* sum; const int* len;            // [n_rows] the caller's rows
    const int16_t* level_raw;                        // [n_events] k_evtab_scan's column (scratch)
    int stay_pen, skip_pen, cost_cap;
    ulonglong2* tr_mask; int* tr_lo;                 // [n_rows] the trace: the two code bits of the band's cells, lo_i (scratch)
    int* end_j;                                      // [n_reads] e, -1: none (scratch)
    long long* al_ev; long long* al_cost; int* al_edge;   // the caller's, may be null
    const int* gain; const int* shift;               // [n_reads] the caller's scaling (k_align_forward<., true> alone; null otherwise)
};

// the smallest of v over the wavefront, in every lane (all 64 lanes active): quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
// leave every row of 16 lanes with its minimum, four lane reads join the rows
__device__ __forceinline__ unsigned aln_wave_min(unsigned v) {
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 0), b = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 32), d = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}

// the lowest lane at which D is smallest
__device__ __forceinline__ int aln_argmin(const unsigned long long D) {
    const unsigned hi = (unsigned)(D >> 32), lo = (unsigned)D;
    const unsigned mh = aln_wave_min(hi);
    const unsigned ml = aln_wave_min(hi == mh ? lo : 0xffffffffu);
    return __builtin_ctzll(__ballot(hi == mh && lo == ml));      // (never empty: the lane that holds the minimum)
}

// D of the row before at lane `src` of its band; outside the band INF
__device__ __forceinline__ unsigned long long aln_prev(const unsigned long long Dp, const int src) {
    const unsigned long long v = __shfl(Dp, src & 63, 64);
    return (unsigned)src < 64u ? v : ALN_INF;
}

template <bool TRACE, bool SCALED>
__global__ __launch_bounds__(64) void k_align_forward(AlignParams P) {
    const BatchView& V = P.bv;
    const int r = blockIdx.x, lane = threadIdx.x;
    const long long R0 = P.row_off[r];
    const int m = (int)(P.row_off[r + 1] - R0);                   // (below 2^31: the host's check)
    const ReadDesc rd = V.reads[r];
    const int T = read_events(rd);
    if (m <= 0 || T <= 0) {
        if (lane == 0) { P.end_j[r] = -1; if (P.al_cost) P.al_cost[r] = -1; }
        return;
    }
    const int16_t* lvp = P.level_raw + rd.ev_off;
    const bool rna = V.rna;
    auto level = [&](const long long j) { return j < T ? 256 * (int)lvp[rna ? T - 1 - j : j] : 0; };      // Lv[j]; past the read 0, never used
    const unsigned long long stay = (unsigned long long)P.stay_pen, skip = (unsigned long long)P.skip_pen;
    const int cap = P.cost_cap;
    const long long gain = SCALED ? min(max(P.gain[r], 1), 1 << 20) : 65536;                 // (out of range: clamped, as the header says)
    const long long off = SCALED ? min(max(P.shift[r], -(1 << 26)), 1 << 26) : 0;
    long long tb = 0;                                             // L0 holds Lv[tb + lane], L1 Lv[tb + 64 + lane]
    int L0 = level(lane), L1 = level(64 + lane);
    int lo = 0, lv = L0, shift = 0;                               // the band's first target, its levels, how far it moved before this row
    unsigned long long D = ALN_INF, Dp = ALN_INF;
    for (long long i0 = 0; i0 < m; i0 += 64) {
        const int cnt = (int)min(64LL, m - i0);
        // q of the tile's rows, one per lane, clamped to +-2^26
        int qt = 0;
        if (lane < cnt) qt = rows_q<SCALED>(P.sum[R0 + i0 + lane], P.len[R0 + i0 + lane], gain, off);      // (k_rows.h)
        for (int t = 0; t < cnt; t++) {
            const int i = (int)i0 + t;
            const int q = __builtin_amdgcn_readlane(qt, t);
            const bool valid = lane < T - lo;                     // j = lo + lane < T  (lo < T always)
            const unsigned long long c = (unsigned long long)min(abs(q - lv), cap);
            int code = 3;
            if (i == 0) D = valid ? c + (unsigned long long)lane * skip : ALN_INF;
            else {
                const int src = lane + shift;                     // this cell's place in the band of the row before
                unsigned long long best = aln_prev(Dp, src - 1);
                const unsigned long long c1 = aln_prev(Dp, src) + stay, c2 = aln_prev(Dp, src - 2) + skip;
                code = 0;
                if (c1 < best) { best = c1; code = 1; }
                if (c2 < best) { best = c2; code = 2; }
                if (best >= ALN_INF || !valid) { D = ALN_INF; code = 3; } else D = best + c;
            }
            if (TRACE) {
                const unsigned long long b0 = __ballot(code & 1), b1 = __ballot(code & 2);
                if (lane == 0) { P.tr_mask[R0 + i] = make_ulonglong2(b0, b1); P.tr_lo[R0 + i] = lo; }
            }
            Dp = D;
            if (i + 1 < m) {
                const int a = aln_argmin(D);
                shift = min(2, max(0, a - 31));
                if (shift) {                                      // (the same in every lane)
                    lo += shift;
                    if (lo - tb >= 64) { tb += 64; L0 = L1; L1 = level(tb + 64 + lane); }
                    const int at = (int)(lo - tb) + lane;         // 0 .. 126
                    const int v0 = __shfl(L0, at & 63, 64), v1 = __shfl(L1, at & 63, 64);
                    lv = at < 64 ? v0 : v1;
                }
            }
        }
    }
    // the end: the lowest j at which D + (T-1-j) skip_pen is smallest over the finite cells.  The value is below 2^58, so it packs with its lane
    unsigned long long key = ~0ULL;
    if (D < ALN_INF) key = ((D + (unsigned long long)(T - 1 - lo - lane) * skip) << 6) | (unsigned)lane;
#pragma unroll
    for (int d = 32; d; d >>= 1) key = min(key, (unsigned long long)__shfl_xor(key, d, 64));
    if (lane == 0) {
        const bool none = key == ~0ULL;
        P.end_j[r] = none ? -1 : lo + (int)(key & 63);
        if (P.al_cost) P.al_cost[r] = none ? -1 : (long long)(key >> 6);
    }
}

__global__ __launch_bounds__(64) void k_align_trace(AlignParams P) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const long long R0 = P.row_off[r];
    const int m = (int)(P.row_off[r + 1] - R0);
    const ReadDesc rd = P.bv.reads[r];
    const int T = read_events(rd);
    int j = P.end_j[r];                                           // the same in every lane
    if (m <= 0 || j < 0) {
        if (P.al_ev) for (int i = lane; i < m; i += 64) P.al_ev[R0 + i] = -1;
        if (P.al_edge && lane == 0) P.al_edge[r] = 0;
        return;
    }
    int edge = 0;
    for (int hi = m; hi > 0; hi -= 64) {
        const int i0 = max(hi - 64, 0), cnt = hi - i0;
        ulonglong2 mk = make_ulonglong2(0, 0);
        int lo = 0, mine = 0;
        if (lane < cnt) { mk = P.tr_mask[R0 + i0 + lane]; lo = P.tr_lo[R0 + i0 + lane]; }
        const int b0l = (int)(unsigned)mk.x, b0h = (int)(unsigned)(mk.x >> 32), b1l = (int)(unsigned)mk.y, b1h = (int)(unsigned)(mk.y >> 32);
        for (int t = cnt - 1; t >= 0; t--) {
            const int lo_t = __builtin_amdgcn_readlane(lo, t);
            const unsigned long long b0 = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(b0l, t) | ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(b0h, t) << 32);
            const unsigned long long b1 = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(b1l, t) | ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(b1h, t) << 32);
            if (lane == t) mine = j;
            const int at = (j - lo_t) & 63;                       // (inside the band by construction)
            edge += (at == 63 || (at == 0 && lo_t > 0)) ? 1 : 0;
            const int code = (int)((b0 >> at) & 1) | ((int)((b1 >> at) & 1) << 1);
            j -= code == 0 ? 1 : code == 2 ? 2 : 0;
        }
        if (P.al_ev && lane < cnt) P.al_ev[R0 + i0 + lane] = rd.ev_off + (P.bv.rna ? T - 1 - mine : mine);
    }
    if (P.al_edge && lane == 0) P.al_edge[r] = edge;
}
