// k_pileup.h -- the events of a batch added, across reads, into per-key sums the caller keeps from batch to batch (include/sqg_pileup.h)
// Part of the device code of the per-read signal path; included through sqg_kernels.h behind k_events_table.h, whose scan pass and sample reduction it uses.
//
//   k_pileup<PA>   k_evtab_reduce's grid: a flat grid over the batch's events, one event per lane (evtab_event), the samples taken by evtab_take and mean / sd
//                  derived by evtab_derive -- the very code of the event table, so q(mean) is q of the float the table holds.  Whether an event
//                  counts and where is decided BEFORE its samples are loaded: an event outside the key window costs its descriptor and no sample.
//                  No per-event column is written.  The adds are no-return relaxed integer atomics at agent scope; consecutive lanes hold
//                  consecutive events of one read, hence consecutive keys (BY_REF), so a wave's atomic instruction touches one run of 256 B
//                  (n) or 512 B (the 64-bit sums).  Integer adds commute: the sums do not depend on the order the events arrive in.
//                  counted / outside: a ballot per wavefront, one atomic each from its first lane into a 16-byte counter block.
#pragma once

struct PileRead { long long key0; int first, L, step; };      // origin; the insert's first base within chain 0, its bases (0: a stand-in read); +1 / -1 / 0

struct PileupParams {
    const PileRead* pr;                                       // [n_reads]
    const uint32_t* kmer; const uint8_t* seg;                 // [n_events] of the scan pass; null where neither key nor split needs them
    int by_kmer, split_strand, split_meth, k;
    unsigned int segs;
    long long lo, hi;
    unsigned int* n; long long *dwell, *dwell_sq, *mean_sum, *mean_sq, *sd_sum;   // the caller's [planes][hi - lo], may be null
    unsigned long long* stat;                                 // {counted, outside}; k_pileup_rows: {counted, outside, unseen}
};

__device__ __forceinline__ long long pileup_q(const float x) { return (long long)rint((double)x * 4096.0); }

// Whether event i of read r counts before the window is looked at, its key and its plane: include/sqg_pileup.h's rules as k_pileup below
// states them, as a function for k_pileup_rows (k_collapse.h).  k_pileup keeps its own lines: calling these two functions from it reorders
// three pairs of its instructions (same 680 / 708 instructions, same registers), and it is to stay instruction-identical.
struct PileWhere { bool eligible; long long key; int plane; };
__device__ __forceinline__ PileWhere pileup_where(const EventParams& Q, const PileupParams& U, const long long i, const int r) {
    long long key = 0;
    bool eligible = false;
    int plane = 0;
    const PileRead pr = U.pr[r];
    if (U.by_kmer) {
        eligible = pr.step != 0 && ((U.segs >> U.seg[i]) & 1u);
        key = (long long)U.kmer[i];
    } else {
        const ReadDesc rd = Q.bv.reads[r];
        const long long e = i - rd.ev_off;
        const long long j = e - pr.first;
        eligible = pr.step != 0 && e < rd.ne0 && j >= 0 && j <= (long long)pr.L - U.k;
        key = pr.key0 + (long long)pr.step * j;
    }
    if (U.split_strand) plane = pr.step < 0 ? 1 : 0;
    if (U.split_meth && eligible) {
        bool m = false;
        uint32_t x = U.kmer[i];
        for (int q = 0; q < U.k; q++) { m |= x % 5u == 3u; x /= 5u; }
        plane += m ? (U.split_strand ? 2 : 1) : 0;
    }
    return {eligible, key, plane};
}

// The adds of one counted event of `len` samples -- the sum over its rows: 64 bits -- into element `at` of the caller's arrays; derive(&mean,
// &sd) is called only where a mean is wanted and len > 0.  k_pileup_rows; k_pileup's own adds below are the same lines on an int.
template <class Derive>
__device__ __forceinline__ void pileup_add(const PileupParams& U, const long long at, const long long len, const bool want_samples, Derive derive) {
    if (U.n) __hip_atomic_fetch_add(U.n + at, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (len <= 0) return;                                                     // no sample, no mean: n only
    if (U.dwell) __hip_atomic_fetch_add(U.dwell + at, len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (U.dwell_sq) __hip_atomic_fetch_add(U.dwell_sq + at, (long long)((unsigned long long)len * (unsigned long long)len), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // modulo 2^64
    if (want_samples) {
        float mean, sd;
        derive(&mean, &sd);
        const long long qm = pileup_q(mean);
        if (U.mean_sum) __hip_atomic_fetch_add(U.mean_sum + at, qm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (U.mean_sq) __hip_atomic_fetch_add(U.mean_sq + at, (long long)((unsigned long long)qm * (unsigned long long)qm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (U.sd_sum) __hip_atomic_fetch_add(U.sd_sum + at, pileup_q(sd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool PA>
__global__ __launch_bounds__(CHUNK_WG) void k_pileup(EventParams Q, PileupParams U) {
    const uint32_t* W = reinterpret_cast<const uint32_t*>(Q.bv.sig);
    const long long width = U.hi - U.lo;
    const bool want_samples = U.mean_sum || U.mean_sq || U.sd_sum;
    evtab_for_rows(Q.n_events, [&](const long long i, const bool have, const int lane) {
        const auto [r, len, s0] = have ? evtab_event(Q, i) : EventAt{0, 0, 0};
        long long key = 0;
        bool eligible = false;
        int plane = 0;
        if (have) {
            const PileRead pr = U.pr[r];
            if (U.by_kmer) {
                eligible = pr.step != 0 && ((U.segs >> U.seg[i]) & 1u);
                key = (long long)U.kmer[i];
            } else {
                const ReadDesc rd = Q.bv.reads[r];
                const long long e = i - rd.ev_off;
                const long long j = e - pr.first;
                eligible = pr.step != 0 && e < rd.ne0 && j >= 0 && j <= (long long)pr.L - U.k;
                key = pr.key0 + (long long)pr.step * j;
            }
            if (U.split_strand) plane = pr.step < 0 ? 1 : 0;
            if (U.split_meth && eligible) {
                bool m = false;
                uint32_t x = U.kmer[i];
                for (int q = 0; q < U.k; q++) { m |= x % 5u == 3u; x /= 5u; }
                plane += m ? (U.split_strand ? 2 : 1) : 0;
            }
        }
        const bool inside = eligible && key >= U.lo && key < U.hi;
        // (every lane of the wavefront is here: evtab_take and the ballots are wave-wide)
        const EventAcc A = evtab_take(W, inside && want_samples && len > 0, len, s0, lane);
        const unsigned long long m_in = __ballot(inside), m_out = __ballot(eligible && !inside);
        if (lane == 0) {
            if (m_in) __hip_atomic_fetch_add(U.stat, (unsigned long long)__popcll(m_in), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (m_out) __hip_atomic_fetch_add(U.stat + 1, (unsigned long long)__popcll(m_out), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!inside) return;
        const long long at = (long long)plane * width + (key - U.lo);
        if (U.n) __hip_atomic_fetch_add(U.n + at, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (len <= 0) return;                                                     // no sample, no mean: n only
        if (U.dwell) __hip_atomic_fetch_add(U.dwell + at, (long long)len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (U.dwell_sq) __hip_atomic_fetch_add(U.dwell_sq + at, (long long)len * len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (want_samples) {
            float mean, sd;
            evtab_derive<PA>(Q, r, len, A, &mean, &sd);
            const long long qm = pileup_q(mean);
            if (U.mean_sum) __hip_atomic_fetch_add(U.mean_sum + at, qm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (U.mean_sq) __hip_atomic_fetch_add(U.mean_sq + at, (long long)((unsigned long long)qm * (unsigned long long)qm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (U.sd_sum) __hip_atomic_fetch_add(U.sd_sum + at, pileup_q(sd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    });
}
