// k_collapse.h -- the caller's event rows summed per true event they are assigned to, mean / sd of those sums, and their pileup (include/sqg_collapse.h)
// Part of the device code of the per-read signal path; included through sqg_kernels.h behind k_pileup.h, whose key rule and adds it uses.
//
//   k_collapse_rows      a flat grid over the ROWS (evtab_for_rows), one row per lane.  A lane finds its read by a search in the device copy of
//                        row_off (k_rows.h: rows_read_of) -- one search each for the wavefront's first and last row, and no other when the two
//                        agree -- and tests the range rule.  A detector over-segments: many consecutive rows go to one event, and raw per-row
//                        atomics would pile onto one address (profiles/pileup.md).  So the rows are combined within the wavefront first
//                        (k_rows.h: wave_runs, wave_run_scan): a lane is a HEAD if its row is dropped or its ev differs from the lane before;
//                        the scan over (rows, len, sum, sumsq) gives the run's sums, and only the LAST lane of a run issues the adds: no-return
//                        relaxed agent-scope atomics, as in k_pileup.  Runs that cross a wavefront, a workgroup or a trip meet in the atomic:
//                        integer adds commute, the result does not depend on where the cuts fall.  Dropped rows are counted per read the same
//                        way (a ballot, one add per run of equal reads), and batch-wide in a register over the wavefront's trips, added once.
//   k_collapse_derive<PA> a flat grid over the events: mean / sd from the finished sums (evtab_derive_d: the event table's code on a 64-bit length).
//   k_pileup_rows<PA>    the same grid: pileup_where decides eligibility, key and plane, pileup_add adds (k_pileup.h); unseen / outside / counted
//                        in registers over the trips, one add each per wavefront at the end.
#pragma once

struct CollapseParams {
    RowsIn rows;
    const long long *ev, *sum, *sumsq; const int* len;        // the caller's rows; sumsq may be null when ob_sumsq is
    unsigned int* ob_rows; unsigned long long *ob_len, *ob_sum, *ob_sumsq;   // [n_events] the caller's or scratch, zeroed; null: not needed
    int* rd_dropped;                                          // [n_reads] zeroed, may be null
    unsigned long long* dropped;                              // the batch-wide counter, may be null
};

__global__ __launch_bounds__(CHUNK_WG) void k_collapse_rows(CollapseParams P) {
    unsigned long long dropped_here = 0;                      // this wavefront's dropped rows over all its trips (the same in every lane)
    const RowsIn& R = P.rows;
    const auto off = [&](const int r) { return R.row_off[r]; };
    evtab_for_rows(R.n_rows, [&](const long long i, const bool have, const int lane) {
        // the wavefront's first and last row (the first lane always has a row when any lane has: the trips start at multiples of 64)
        const long long w0 = i - lane, w1 = min(w0 + 63, R.n_rows - 1);
        int r = 0;
        if (w0 < R.n_rows) {
            const int r0 = rows_read_of(off, 0, R.n_reads - 1, w0);
            const int r1 = rows_read_of(off, r0, R.n_reads - 1, w1);
            r = r0 == r1 || !have ? r0 : rows_read_of(off, r0, r1, i);
        }
        long long e = -1;
        bool counts = false;
        if (have) {
            e = P.ev[i];
            const EventRange own = read_event_range(R.reads[r]);
            counts = e >= own.lo && e < own.hi;
        }
        // (every lane of the wavefront is here: the ballots and the shuffles below are wave-wide)
        const long long e_up = __shfl_up(e, 1, 64);
        const bool counts_up = __shfl_up((int)counts, 1, 64) != 0;
        const auto [first, tail] = wave_runs(!counts || lane == 0 || e != e_up || !counts_up, lane);
        unsigned int v_rows = counts ? 1u : 0u;
        const int ln = counts ? P.len[i] : 0;
        const bool some = ln >= 1;
        unsigned long long v_len = some ? (unsigned long long)ln : 0ull;
        unsigned long long v_sum = some && P.ob_sum ? (unsigned long long)P.sum[i] : 0ull;
        unsigned long long v_sq = some && P.ob_sumsq ? (unsigned long long)P.sumsq[i] : 0ull;
        wave_run_scan(first, lane, v_rows, v_len, v_sum, v_sq);
        if (counts && tail) {
            if (P.ob_rows) __hip_atomic_fetch_add(P.ob_rows + e, v_rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (P.ob_len) __hip_atomic_fetch_add(P.ob_len + e, v_len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (P.ob_sum) __hip_atomic_fetch_add(P.ob_sum + e, v_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (P.ob_sumsq) __hip_atomic_fetch_add(P.ob_sumsq + e, v_sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // the dropped rows: per read one add from the first lane of every run of equal reads, batch-wide into the register
        const unsigned long long drops = __ballot(have && !counts);
        if (drops) {
            dropped_here += (unsigned long long)__popcll(drops);
            const int r_up = __shfl_up(r, 1, 64);
            const unsigned long long starts = __ballot(have && (lane == 0 || r != r_up));
            const unsigned long long above = (starts >> 1) >> lane;                 // the run starts behind this lane, bit 0: the next lane
            const int run = above ? __builtin_ctzll(above) + 1 : 64 - lane;
            const unsigned long long mine = (run == 64 ? ~0ull : (1ull << run) - 1ull) << lane;
            const int cnt = __popcll(drops & mine);
            if (P.rd_dropped && have && ((starts >> lane) & 1ull) && cnt) __hip_atomic_fetch_add(P.rd_dropped + r, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    });
    if (P.dropped && dropped_here && (threadIdx.x & 63) == 0) __hip_atomic_fetch_add(P.dropped, dropped_here, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the finished sums of the events, [n_events]: what k_collapse_rows left; sumsq null: no sd is asked for
struct CollapseSums { const unsigned int* rows; const long long *len, *sum, *sumsq; };

// mean / sd of event i of read r from its rows' sums, 0 for an event without a sample
template <bool PA>
__device__ __forceinline__ void collapse_derive(const EventParams& Q, const CollapseSums& S, const long long i, const int r, const long long len, float* mean, float* sd) {
    *mean = 0.f; *sd = 0.f;
    if (len > 0) evtab_derive_d<PA>(Q, r, (double)len, (double)S.sum[i], S.sumsq ? (double)S.sumsq[i] : 0.0, mean, sd);
}

template <bool PA>
__global__ __launch_bounds__(CHUNK_WG) void k_collapse_derive(EventParams Q, CollapseSums S) {
    evtab_for_rows(Q.n_events, [&](const long long i, const bool have, const int) {
        if (!have) return;
        float mean, sd;
        collapse_derive<PA>(Q, S, i, Q.ev_read[i], S.len[i], &mean, &sd);
        if (Q.mean) Q.mean[i] = mean;
        if (Q.sd) Q.sd[i] = sd;
    });
}

template <bool PA>
__global__ __launch_bounds__(CHUNK_WG) void k_pileup_rows(EventParams Q, PileupParams U, CollapseSums S) {
    const long long width = U.hi - U.lo;
    const bool want_samples = U.mean_sum || U.mean_sq || U.sd_sum;
    unsigned long long n_in = 0, n_out = 0, n_unseen = 0;                            // this wavefront's, over all its trips
    evtab_for_rows(Q.n_events, [&](const long long i, const bool have, const int) {
        const int r = have ? Q.ev_read[i] : 0;
        const auto [eligible, key, plane] = have ? pileup_where(Q, U, i, r) : PileWhere{false, 0, 0};
        const bool seen = have && S.rows[i] != 0u;
        const bool inside = eligible && seen && key >= U.lo && key < U.hi;
        // (every lane of the wavefront is here: the ballots are wave-wide)
        n_in += (unsigned long long)__popcll(__ballot(inside));
        n_out += (unsigned long long)__popcll(__ballot(eligible && seen && !inside));
        n_unseen += (unsigned long long)__popcll(__ballot(eligible && !seen));
        if (!inside) return;
        const long long at = (long long)plane * width + (key - U.lo);
        const long long len = S.len[i];
        pileup_add(U, at, len, want_samples, [&](float* mean, float* sd) { collapse_derive<PA>(Q, S, i, r, len, mean, sd); });
    });
    if ((threadIdx.x & 63) == 0) {
        if (n_in) __hip_atomic_fetch_add(U.stat, n_in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_out) __hip_atomic_fetch_add(U.stat + 1, n_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_unseen) __hip_atomic_fetch_add(U.stat + 2, n_unseen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
