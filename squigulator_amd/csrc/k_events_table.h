// k_events_table.h -- the per-event signal table of a batch (include/sqg_events.h): one row per event, its place, k-mer and level, then the sums of its samples
// Part of the device code of the per-read signal path; included through sqg_kernels.h (see there for the overview).  (k_events.h is the generator's event pass.)
//
//   k_evtab_scan         one workgroup per read over the dwell scan of k_chunks.h (chunk_for_event_tiles) with an origin that spans both chains:
//                        ev_start from the E the scan carries, and the columns that need no sample -- ev_read, ev_len, seg (k_segments.h's event
//                        ranges: seg_ranges), kmer (k_targets.h's rank, on the event's own chain) and level_raw (k_common.h: level_code).  ev_start and ev_read go
//                        to scratch when the caller does not want them: the reduce pass finds an event's samples through them.
//   k_evtab_reduce<PA>   a flat grid over the batch's events, one event per lane: a read of 100 events and one of 100 000 load the device alike,
//                        and no workgroup walks a read's events one behind the other (the label pass's latency chain: profiles/chunks.md).  An event
//                        of at most EVT_LANE_MAX samples is reduced by its lane; a longer one -- a dwell goes up to 65 535 -- by the whole
//                        wavefront, one after the other in lane order: the bounds of those loops come from a ballot and a broadcast, the same for
//                        every lane.  An event starts at any sample of the slab, so the loads are the aligned 4-byte words that cover it, their
//                        halves taken or left (k_chunk_emit's scheme; no misaligned wide load is issued, no word without a sample of the event is
//                        touched).  mean / sd are derived in the same pass, in FP64 as the header states them.
// The statistics are k_chunks.h's pass (h_events_table.h runs stats_run over the whole reads or their inserts).
#pragma once

#define EVT_LANE_MAX 64                              // samples up to which a lane reduces an event alone (33 word loads at the most)

struct EventParams {
    BatchView bv;
    const float2* consts;                            // [n_reads] {median, 1 / (1.4826 MAD)} (k_chunk_stats); MEDMAD rows only
    long long n_events;
    long long* ev_start; int* ev_read;               // the caller's or scratch: never null when the reduce pass runs
    int* ev_len; uint32_t* kmer; int16_t* level_raw; uint8_t* seg;                          // the caller's, may be null
    long long* sum; long long* sumsq; int16_t* vmin; int16_t* vmax; float* mean; float* sd;   // the caller's, may be null
};

__global__ __launch_bounds__(CHUNK_WG) void k_evtab_scan(EventParams Q) {
    __shared__ unsigned long long sh[8];
    const BatchView& V = Q.bv;
    const int r = blockIdx.x;
    const ReadDesc rd = V.reads[r];
    const long long n = V.sig_off[r + 1] - V.sig_off[r];
    const int ne0 = rd.ne0, ne = read_events(rd), kind = V.kind;
    const SegRanges sr = seg_ranges(V, rd);
    const int a = sr.a, b = sr.b;
    const uint8_t* bp0 = V.bases + rd.base_off;
    const uint8_t* bp1 = bp0 + rd.len0 - ne0;               // chain 1's event e has its k-mer at bp0 + len0 + (e - ne0)
    chunk_for_event_tiles(ChunkOrigin{rd.ev_off, rd.base_off, ne}, V.dwell, V.const_sps, sh, [&](int e0, unsigned long long E, const int (&d)[4]) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = e0 + q;
            if (e < ne) {
                const long long at = rd.ev_off + e;
                if (Q.ev_start) Q.ev_start[at] = V.rna ? n - (long long)E - d[q] : (long long)E;
                if (Q.ev_read) Q.ev_read[at] = r;
                if (Q.ev_len) Q.ev_len[at] = d[q];
                if (Q.seg) Q.seg[at] = (uint8_t)(kind == SEG_DNA ? (e < a ? 0 : e < b ? 1 : 3) : kind == SEG_RNA ? (e < a ? 3 : e < b ? 2 : e < ne0 ? 1 : 0) : 3);
                if (Q.kmer || Q.level_raw) {
                    const uint32_t rank = kmer_rank_wide((e < ne0 ? bp0 : bp1) + e, V.k, V.meth);
                    if (Q.kmer) Q.kmer[at] = rank;
                    if (Q.level_raw) Q.level_raw[at] = level_code(V.model, rank, V.dig, V.range, rd.offset);
                }
            }
            E += (unsigned long long)d[q];
        }
    });
}

struct EventAcc {
    long long sum; unsigned long long sq; int mn, mx;
    __device__ void take(uint32_t half) {
        const int v = (int)(int16_t)(half & 0xffffu);
        sum += v; sq += (unsigned long long)(v * v); mn = min(mn, v); mx = max(mx, v);      // (v * v <= 2^30)
    }
};

// The samples of the events of one wavefront, one event per lane: `take` says whether this lane's event [s0, s0 + len) of the slab is wanted
// (the same code for every lane of the wavefront: the long events are reduced by all of them).  k_evtab_reduce and k_pileup (k_pileup.h).
__device__ __forceinline__ EventAcc evtab_take(const uint32_t* W, const bool take, const int len, const long long s0, const int lane) {
    EventAcc A{0, 0, 32767, -32768};
    if (take && len <= EVT_LANE_MAX) {
        long long s = s0;
        const long long end = s0 + len;
        if ((s & 1) && s < end) { A.take(W[s >> 1] >> 16); s++; }
        for (; s + 2 <= end; s += 2) { const uint32_t w = W[s >> 1]; A.take(w); A.take(w >> 16); }
        if (s < end) A.take(W[s >> 1]);
    }
    // the long events of this wavefront, one at a time by all of its lanes: `todo`, `ls0` and `lend` are the same in every lane
    unsigned long long todo = __ballot(take && len > EVT_LANE_MAX);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const long long ls0 = __shfl(s0, src, 64);
        const long long lend = ls0 + (long long)__shfl(len, src, 64);
        const long long w_lo = ls0 >> 1, w_hi = (lend - 1) >> 1;            // the words that hold a sample of the event
        EventAcc B{0, 0, 32767, -32768};
        for (long long wb = w_lo; wb <= w_hi; wb += 64) {
            const long long w = wb + lane;
            if (w <= w_hi) {
                const uint32_t x = W[w];
                if (2 * w >= ls0) B.take(x);                                // (2 w < lend: w <= w_hi)
                if (2 * w + 1 < lend) B.take(x >> 16);                      // (2 w + 1 >= ls0: w >= w_lo)
            }
        }
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            B.sum += __shfl_xor(B.sum, d, 64); B.sq += __shfl_xor(B.sq, d, 64);
            B.mn = min(B.mn, __shfl_xor(B.mn, d, 64)); B.mx = max(B.mx, __shfl_xor(B.mx, d, 64));
        }
        if (lane == src) A = B;
    }
    return A;
}

// Event i of a flat grid over the batch's events: its read, its samples and the first of them in the slab (through the scan pass's ev_read
// and ev_start).  k_evtab_reduce and k_pileup.
struct EventAt { int r, len; long long s0; };
__device__ __forceinline__ EventAt evtab_event(const EventParams& Q, const long long i) {
    const int r = Q.ev_read[i];
    return {r, Q.bv.dwell ? (int)Q.bv.dwell[i] : Q.bv.const_sps, Q.bv.sig_off[r] + Q.ev_start[i]};
}

// mean / sd of an event of read r from its sums, as include/sqg_events.h states them: one rounding per operation (the build has
// -ffp-contract=off); double sqrt is correctly rounded on this device, as the exact sample path relies on (k_common.h: box_muller_exact)
// (evtab_derive_d: on the three as doubles -- evtab_derive for an event's own sums, k_collapse.h for sums over rows, whose length has 64 bits)
template <bool PA>
__device__ __forceinline__ void evtab_derive_d(const EventParams& Q, const int r, const double dl, const double ds, const double dq, float* mean, float* sd) {
    const double m = ds / dl;
    double v = (dq - ds * m) / dl;
    v = v < 0 ? 0 : v;
    const double s = sqrt(v);
    if (PA) {
        const double offset = Q.bv.reads[r].offset;
        *mean = (float)(((m + offset) * Q.bv.range) / Q.bv.dig);
        *sd = (float)((s * Q.bv.range) / Q.bv.dig);
    } else {
        const float2 cs = Q.consts[r];                                   // cs.x = med2 / 2 exactly: |med2| < 2^17
        *mean = (float)((m - (double)cs.x) * (double)cs.y);
        *sd = (float)(s * (double)cs.y);
    }
}
template <bool PA>
__device__ __forceinline__ void evtab_derive(const EventParams& Q, const int r, const int len, const EventAcc& A, float* mean, float* sd) {
    evtab_derive_d<PA>(Q, r, (double)len, (double)A.sum, (double)A.sq, mean, sd);
}

// The six columns of sums of row i (an event of the table, a row of the detector's) of read r, mean / sd among them: those the caller
// asked for.  k_evtab_reduce and k_detect_rows (k_detect.h).
template <bool PA>
__device__ __forceinline__ void evtab_store(const EventParams& Q, const long long i, const int r, const int len, const EventAcc& A) {
    if (Q.sum) Q.sum[i] = A.sum;
    if (Q.sumsq) Q.sumsq[i] = (long long)A.sq;
    if (Q.vmin) Q.vmin[i] = (int16_t)A.mn;
    if (Q.vmax) Q.vmax[i] = (int16_t)A.mx;
    if (Q.mean || Q.sd) {
        float mean, sd;
        evtab_derive<PA>(Q, r, len, A, &mean, &sd);
        if (Q.mean) Q.mean[i] = mean;
        if (Q.sd) Q.sd[i] = sd;
    }
}

// A flat grid over n rows, one row per lane, in as many trips as the grid needs: f(i, have, lane) for row i of every trip, `have`
// saying whether there is such a row.  f is called in ALL 64 lanes of a wavefront on every trip the wavefront makes, the lanes behind
// the last row included: evtab_take and k_pileup's ballots are wave-wide, so f reaches them before it returns for want of a row.
// k_evtab_reduce, k_pileup (k_pileup.h) and k_detect_rows (k_detect.h).
template <class F>
__device__ __forceinline__ void evtab_for_rows(const long long n, F f) {
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * CHUNK_WG; base < n; base += (long long)gridDim.x * CHUNK_WG) {
        const long long i = base + threadIdx.x;
        f(i, i < n, lane);
    }
}

template <bool PA>
__global__ __launch_bounds__(CHUNK_WG) void k_evtab_reduce(EventParams Q) {
    const uint32_t* W = reinterpret_cast<const uint32_t*>(Q.bv.sig);              // the slab in aligned words: sample s is half s & 1 of word s >> 1
    evtab_for_rows(Q.n_events, [&](const long long i, const bool have, const int lane) {
        const auto [r, len, s0] = have ? evtab_event(Q, i) : EventAt{0, 0, 0};
        const EventAcc A = evtab_take(W, have, len, s0, lane);
        if (have) evtab_store<PA>(Q, i, r, len, A);
    });
}
