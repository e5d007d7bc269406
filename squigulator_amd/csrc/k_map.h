// k_map.h -- subsequence DTW of event rows against the genome's level track (include/sqg_map.h): the track, the rows' values, the programme, the reads' results
// Part of the device code of the per-read signal path; included through sqg_kernels.h behind k_call.h.
//
//   k_map_track   a flat grid over the window, one position per lane: the contig's end from the resident offsets, at most k byte loads, the
//                 two rows, two loads of the caller's levels.  Runs once per window; not hot.
//   k_map_rows    q of every mapped row (k_rows.h: rows_q, the aligner's), once per call (a 64-bit division each): both strands and every span of a read take it from there.
//   k_map_dp      the hot kernel.  A row of the programme has no dependency inside itself and a stretch of the track never changes while the
//                 rows go by.  One wavefront (a workgroup of its own: the hardware hands them out) walks a SPAN of consecutive TILES of
//                 MAP_TILE = 64 * MAP_STRIP positions from left to right; a lane owns MAP_STRIP consecutive positions of the tile, their Lv,
//                 D and S in registers (3 * MAP_STRIP of them; the compiler's count is in profiles/map.md).  A row is updated in place from
//                 the strip's top down, so the row before is still there where it is read.  The two left neighbours of a strip's first
//                 cells come from the lane below by a DPP wave shift; those of lane 0 are the last two cells of the tile before, which the
//                 wavefront left, row by row, in LDS ({D, S} of u-1 and of u-2: 16 bytes per row, so at most 64 KiB) -- read 64 rows at a
//                 time ahead of the stores that replace them.  q reaches the lanes as a wavefront-uniform value, 64 rows per fetch.
//                 A span that does not begin at u = 0 first walks the tiles that hold the 2 (m - 1) positions in front of it -- the halo:
//                 every cell of the span depends on nothing further left -- and reports none of them.  No floating point, no atomics.
//                 Every (read, strand, span) writes {smallest D of the last row, lowest u, S} to MapParams.rec.
//   k_map_finish  one lane per read: the spans in ascending order, so the result does not depend on arrival order, then the strand and the keys.
#pragma once

#define MAP_STRIP 16
#define MAP_TILE (64 * MAP_STRIP)
#define MAP_INF (1 << 30)                            // above every D; INF + a penalty still fits an int
#define MAP_FAR (1 << 28)                            // stands for SQG_MAP_NONE in the registers: |q - MAP_FAR| >= 2^28 - 2^26 > cost_cap
#define MAP_NONE_LEVEL ((int)0x80000000)             // SQG_MAP_NONE

struct MapTrackParams {
    const uint8_t* seq; const long long* contig_off; int n_contigs; long long total;
    long long lo, hi; int k, meth;
    const int* levels; int* fwd; int* rev;
};

__device__ __forceinline__ int map_clamp_level(const int v) { return min(max(v, -(1 << 23)), 1 << 23); }

__global__ __launch_bounds__(256) void k_map_track(const MapTrackParams P) {
    const long long g = P.lo + (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= P.hi) return;
    // g's contig: the last one whose first base is <= g (contigs without bases are stepped over)
    int a = 0, b = P.n_contigs - 1;
    while (a < b) {
        const int mid = a + (b - a + 1) / 2;
        if (P.contig_off[mid] <= g) a = mid; else b = mid - 1;
    }
    const long long end = min(P.contig_off[a + 1], P.total);
    bool ok = g + P.k <= end;
    uint32_t rf = 0, rr = 0, pw = 1;                 // the rows of the k-mer and of its reverse complement; the digit's weight in the latter
    const uint32_t base = P.meth ? 5u : 4u;
    if (ok) {
        for (int i = 0; i < P.k; i++) {
            const uint8_t c = P.seq[g + i];
            uint8_t cm;                              // the complement table of k_copy_reads: upper case for either case
            switch (c) {
            case 'A': case 'a': cm = 'T'; break;
            case 'C': case 'c': cm = 'G'; break;
            case 'G': case 'g': cm = 'C'; break;
            case 'T': case 't': cm = 'A'; break;
            default: cm = 0; ok = false; break;
            }
            rf = rf * base + (P.meth ? meth_code(c) : base_code(c));          // '+': the byte as it stands
            rr += pw * (P.meth ? meth_code(cm) : base_code(cm));              // '-': base i is digit i from the right
            pw *= base;
        }
    }
    if (P.fwd) P.fwd[g - P.lo] = ok ? map_clamp_level(P.levels[rf]) : MAP_NONE_LEVEL;
    if (P.rev) P.rev[g - P.lo] = ok ? map_clamp_level(P.levels[rr]) : MAP_NONE_LEVEL;
}

struct MapParams {
    const long long* row_off;                        // [n_reads+1] device copy of the caller's
    const long long* q_off;                          // [n_reads+1] first mapped row of every read in q
    const long long* sum; const int* len;            // the caller's rows
    const int* gain; const int* shift;               // [n_reads] the caller's scaling, or null
    int* q;                                          // [q_off[n_reads]] the mapped rows' values (scratch)
    const int* fwd; const int* rev; long long lo, hi;
    int W, n_reads, row_first, row_count;
    int stay_pen, skip_pen, cost_cap;
    int strand_of[2], n_strands;                     // the strands asked for, '+' (0) first
    int n_tiles, span_tiles, n_spans;                // tiles of the window, tiles per span, spans
    int span_lo, spans_here, read_lo;                // this launch: its first span, its spans, its first read
    int4* rec;                                       // [n_reads][n_strands][n_spans] {D, e, S, -} (scratch)
    int* map_cost; signed char* map_step; long long* map_key0; long long* map_key1; int* map_cost_other;
};

__device__ __forceinline__ int map_rows_of(const MapParams& P, const int r) {
    const long long have = P.row_off[r + 1] - P.row_off[r] - P.row_first;
    return (int)min(max(have, 0LL), (long long)P.row_count);
}

__global__ __launch_bounds__(256) void k_map_rows(const MapParams P) {
    const int r = blockIdx.x;
    const int m = map_rows_of(P, r);
    const long long R0 = P.row_off[r] + P.row_first, Q0 = P.q_off[r];
    const long long gain = P.gain ? min(max(P.gain[r], 1), 1 << 20) : 65536;
    const long long off = P.shift ? min(max(P.shift[r], -(1 << 26)), 1 << 26) : 0;
    for (int i = threadIdx.x; i < m; i += 256)
        P.q[Q0 + i] = P.gain ? rows_q<true>(P.sum[R0 + i], P.len[R0 + i], gain, off) : rows_q<false>(P.sum[R0 + i], P.len[R0 + i], gain, off);      // (k_rows.h)
}

// v of the lane below; lane 0 keeps `first` (wave_shr:1, bound_ctrl off)
__device__ __forceinline__ int map_from_below(const int first, const int v) {
    return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xF, 0xF, false);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void k_map_dp(const MapParams P) {
    extern __shared__ int4 map_carry[];              // [m - 1] {D, S} of the tile before at its last position and at the one before it
    const int lane = threadIdx.x;
    int id = blockIdx.x;
    const int sp = P.span_lo + id % P.spans_here; id /= P.spans_here;
    const int si = id % P.n_strands;
    const int r = P.read_lo + id / P.n_strands;
    const int m = map_rows_of(P, r), W = P.W;
    if (m <= 0) return;                              // (k_map_finish reads no record of such a read)
    const bool minus = P.strand_of[si] != 0;
    const int* lvp = minus ? P.rev : P.fwd;
    const int* qp = P.q + P.q_off[r];
    const int stay = P.stay_pen, skip = P.skip_pen, cap = P.cost_cap;
    const int t_lo = sp * P.span_tiles, t_hi = min(t_lo + P.span_tiles, P.n_tiles);
    const int halo = (2 * (m - 1) + MAP_TILE - 1) / MAP_TILE;
    const int t_from = max(t_lo - halo, 0);
    for (int i = lane; i < m - 1; i += 64) map_carry[i] = make_int4(MAP_INF, 0, MAP_INF, 0);
    unsigned long long best = ~0ULL; int bestS = 0;  // (D << 24) | e over the span's tiles so far
    int D[MAP_STRIP], S[MAP_STRIP], L[MAP_STRIP];
    for (int tile = t_from; tile < t_hi; tile++) {
        const int u0 = tile * MAP_TILE + lane * MAP_STRIP;
#pragma unroll
        for (int j = 0; j < MAP_STRIP; j++) {
            const int u = u0 + j;
            const int at = min(u, W - 1);            // (past the window: loaded from inside it, and taken as NONE)
            const int v = lvp[minus ? W - 1 - at : at];
            L[j] = v == MAP_NONE_LEVEL || u >= W ? MAP_FAR : map_clamp_level(v);
            D[j] = 0; S[j] = 0;
        }
        int4 sv = make_int4(MAP_INF, 0, MAP_INF, 0); // the carry of the row before this 64-row block's first
        for (int i0 = 0; i0 < m; i0 += 64) {
            const int cnt = min(64, m - i0);
            const int qt = lane < cnt ? qp[i0 + lane] : 0;
            const int4 cv = i0 + lane < m - 1 ? map_carry[i0 + lane] : make_int4(MAP_INF, 0, MAP_INF, 0);
            for (int t = 0; t < cnt; t++) {
                const int i = i0 + t;
                const int q = __builtin_amdgcn_readlane(qt, t);
                if (i == 0) {
#pragma unroll
                    for (int j = 0; j < MAP_STRIP; j++) { D[j] = min(abs(q - L[j]), cap); S[j] = u0 + j; }
                } else {
                    const int tp = max(t - 1, 0);
                    const int c1D = t ? __builtin_amdgcn_readlane(cv.x, tp) : sv.x, c1S = t ? __builtin_amdgcn_readlane(cv.y, tp) : sv.y;
                    const int c2D = t ? __builtin_amdgcn_readlane(cv.z, tp) : sv.z, c2S = t ? __builtin_amdgcn_readlane(cv.w, tp) : sv.w;
                    const int n1D = map_from_below(c1D, D[MAP_STRIP - 1]), n1S = map_from_below(c1S, S[MAP_STRIP - 1]);      // u0 - 1
                    const int n2D = map_from_below(c2D, D[MAP_STRIP - 2]), n2S = map_from_below(c2S, S[MAP_STRIP - 2]);      // u0 - 2
#pragma unroll
                    for (int j = MAP_STRIP - 1; j >= 0; j--) {
                        const int aD = j >= 1 ? D[j - 1] : n1D, aS = j >= 1 ? S[j - 1] : n1S;                               // step
                        const int bD = D[j] + stay, bS = S[j];                                                               // stay
                        const int cD = (j >= 2 ? D[j - 2] : j == 1 ? n1D : n2D) + skip, cS = j >= 2 ? S[j - 2] : j == 1 ? n1S : n2S;   // skip
                        int w = aD, ws = aS;
                        if (bD < w) { w = bD; ws = bS; }
                        if (cD < w) { w = cD; ws = cS; }
                        D[j] = w + min(abs(q - L[j]), cap); S[j] = ws;
                    }
                }
                if (lane == 63 && i < m - 1) map_carry[i] = make_int4(D[MAP_STRIP - 1], S[MAP_STRIP - 1], D[MAP_STRIP - 2], S[MAP_STRIP - 2]);
            }
            sv = make_int4(__builtin_amdgcn_readlane(cv.x, 63), __builtin_amdgcn_readlane(cv.y, 63), __builtin_amdgcn_readlane(cv.z, 63),
                           __builtin_amdgcn_readlane(cv.w, 63));
        }
        if (tile < t_lo) continue;                   // the halo reports nothing
        // the tile's end: the lowest u < W at which the last row is smallest.  D < 2^30 and u < 2^24: the two pack into one key
        unsigned long long key = ~0ULL; int myS = 0;
        const int inside = W - u0;                   // the strip's positions below W
#pragma unroll
        for (int j = 0; j < MAP_STRIP; j++) {
            const unsigned long long kj = ((unsigned long long)(unsigned)D[j] << 24) | (unsigned)(u0 + j);
            if (j < inside && kj < key) { key = kj; myS = S[j]; }
        }
        unsigned long long kmin = key;
#pragma unroll
        for (int d = 32; d; d >>= 1) kmin = min(kmin, (unsigned long long)__shfl_xor(kmin, d, 64));
        const int owner = __builtin_ctzll(__ballot(key == kmin));             // (never empty: every tile of the window has a position below W)
        const int tS = __shfl(myS, owner, 64);
        if (kmin < best) { best = kmin; bestS = tS; }
    }
    if (lane == 0)
        P.rec[((size_t)r * P.n_strands + si) * P.n_spans + sp] = make_int4((int)(best >> 24), (int)(best & 0xffffffu), bestS, 0);
}

__global__ __launch_bounds__(256) void k_map_finish(const MapParams P) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= P.n_reads) return;
    const long long none = (long long)0x8000000000000000ULL;
    int cost = -1, other = -1, step = 0; long long key0 = none, key1 = none;
    if (map_rows_of(P, r) > 0 && P.W > 0) {
        int eD[2] = {0, 0}, eU[2] = {0, 0}, eS[2] = {0, 0};
        for (int si = 0; si < P.n_strands; si++) {
            const int4* rp = P.rec + ((size_t)r * P.n_strands + si) * P.n_spans;
            int4 b = rp[0];
            for (int sp = 1; sp < P.n_spans; sp++) { const int4 v = rp[sp]; if (v.x < b.x) b = v; }      // ascending: the lowest u stays
            eD[si] = b.x; eU[si] = b.y; eS[si] = b.z;
        }
        const int win = P.n_strands == 2 && eD[1] < eD[0] ? 1 : 0;               // a tie goes to '+'
        cost = eD[win];
        if (P.n_strands == 2) other = eD[1 - win];
        if (P.strand_of[win]) { step = -1; key0 = P.hi - 1 - eS[win]; key1 = P.hi - 1 - eU[win]; }
        else { step = 1; key0 = P.lo + eS[win]; key1 = P.lo + eU[win]; }
    }
    if (P.map_cost) P.map_cost[r] = cost;
    if (P.map_step) P.map_step[r] = (signed char)step;
    if (P.map_key0) P.map_key0[r] = key0;
    if (P.map_key1) P.map_key1[r] = key1;
    if (P.map_cost_other) P.map_cost_other[r] = other;
}
