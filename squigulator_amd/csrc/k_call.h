// k_call.h -- per-read CpG methylation calls of a batch from event rows (include/sqg_call.h): the sites of every read, then their scores
// Part of the device code of the per-read signal path; included through sqg_kernels.h behind k_scale.h.
//
//   k_call_scan<MODE>   one workgroup per read over the read's BYTES: no dwell is read, a site needs no window.  A thread takes the 16 bytes
//                       of one aligned 16-byte load (the read starts anywhere in it: the bytes in front of the read and behind its last
//                       candidate position are masked) and the one byte behind them, tests its 16 candidates and the workgroup ranks them
//                       by k_chunks.h's scan (chunk_scan_excl) with a carry from tile to tile; a tile is 16 * CHUNK_WG bytes.  MODE 0
//                       writes the read's count (the plan); MODE 1 one record per site at site_off[r] + rank, and site_read / site_pos /
//                       label for the caller.
//   k_call_score        a flat grid over the sites, one site per lane.  The base-5 digits of the at most 2k - 1 bases under the span, as
//                       the read has them but for the bases that take the hypothesis, are packed 3 bits a digit into one 64-bit word
//                       per hypothesis; the first event's two ranks come from k digits, every further one by dropping the leading digit
//                       and taking one in.  Per event: sum / len to q (h_align's floor and clamps, the scaling where there is one), the
//                       two rows' levels by the event table's level_code, w / c, the capped term.  Then the site's row, the adds to the
//                       frequency arrays -- no-return relaxed integer atomics at agent scope; integer adds commute -- and the counters
//                       by a ballot per wavefront, one atomic each from its first lane.  No LDS.
#pragma once

#define CALL_LOAD 16                                 // bytes of a thread's load in k_call_scan

struct CallParams {
    BatchView bv;
    const uint8_t* skip;                             // [n_reads] 1: a read shorter than a k-mer (its stand-in sequence has no sites); null: none is
    int* count;                                      // [n_reads] MODE 0: sites of every read
    const long long* site_off;                       // [n_reads+1] MODE 1: first site of every read
    long long n_sites;
    int2* rec;                                       // [n_sites] {p, read} (k_call_scan<1> -> k_call_score)
    int* site_read; int* site_pos; uint8_t* label;   // the caller's, may be null
    const long long* sum; const long long* len64; const int* len32;   // the caller's rows, [n_events]; one of the two lengths
    const int* w; const int* c;                      // [5^k] the caller's model
    const int* gain; const int* shift;               // [n_reads] the caller's scaling; null: none
    const PileRead* pr;                              // [n_reads] the reads' origins; null: no key is wanted
    int neigh, term_cap, llr_min, min_obs;
    uint32_t pow_k1;                                 // 5^(k-1)
    long long* site_key; int* n_obs; int* nll_c; int* nll_m; int* llr; uint8_t* call;   // the caller's, may be null
    int have_freq; long long lo, hi;
    unsigned int *cov, *truth, *called, *meth;       // the caller's [hi - lo], may be null
    unsigned long long* stat;                        // {outside, called, agree}
};

template <int MODE>
__global__ __launch_bounds__(CHUNK_WG) void k_call_scan(CallParams Q) {
    __shared__ unsigned long long sh[8];
    const BatchView& V = Q.bv;
    const int r = blockIdx.x;
    const ReadDesc rd = V.reads[r];
    const int len = rd.len0;
    if ((Q.skip && Q.skip[r]) || len < V.k) { if (MODE == 0 && threadIdx.x == 0) Q.count[r] = 0; return; }
    const uint8_t* bp = V.bases + rd.base_off;
    const int s = (int)((uintptr_t)bp & (CALL_LOAD - 1));   // the read's first base within its aligned load
    const uint8_t* ap = bp - s;
    const int span = s + len;                               // bytes from ap up to the read's end
    const long long first = MODE ? Q.site_off[r] : 0;
    unsigned long long ranked = 0;                          // sites of the tiles so far
    for (int base = 0; base < span; base += CALL_LOAD * CHUNK_WG) {
        const int at = base + CALL_LOAD * (int)threadIdx.x; // this thread's bytes: ap[at .. at + 16), position p = at + q - s of the read
        unsigned int cand = 0, meth = 0;
        if (at < span) {
            const uint4 w = *reinterpret_cast<const uint4*>(ap + at);      // (the batch's base buffer ends with slack: a load may reach behind the last read)
            const unsigned int x[5] = {w.x, w.y, w.z, w.w, at + CALL_LOAD < span ? (unsigned int)ap[at + CALL_LOAD] : 0u};
#pragma unroll
            for (int q = 0; q < CALL_LOAD; q++) {
                const unsigned int b = (x[q >> 2] >> (8 * (q & 3))) & 0xffu, g = (x[(q + 1) >> 2] >> (8 * ((q + 1) & 3))) & 0xffu;
                const int p = at + q - s;
                if (p >= 0 && p + 1 < len && g == 'G' && (b == 'C' || b == 'M')) { cand |= 1u << q; meth |= (b == 'M' ? 1u : 0u) << q; }
            }
        }
        unsigned long long total;
        unsigned long long rank = ranked + chunk_scan_excl((unsigned long long)__popc(cand), sh, &total);
        ranked += total;
        if (MODE) {
            while (cand) {
                const int q = __builtin_ctz(cand);
                cand &= cand - 1;
                const long long i = first + (long long)rank++;
                const int p = at + q - s;
                Q.rec[i] = make_int2(p, r);
                if (Q.site_read) Q.site_read[i] = r;
                if (Q.site_pos) Q.site_pos[i] = p;
                if (Q.label) Q.label[i] = (uint8_t)(meth >> q & 1u);
            }
        }
    }
    if (MODE == 0 && threadIdx.x == 0) Q.count[r] = (int)ranked;
}

// q of an event's row: sqg_scale.h's q0 -- floor(256 sum / L), the product modulo 2^64, clamped to +-2^26 -- and under a scaling its q
__device__ __forceinline__ long long call_row_value(const long long sum, const long long L, const bool scaled, const long long gain, const long long off) {
    const long long p = (long long)((unsigned long long)sum << 8);
    long long q = p / L;                                                  // (L >= 1)
    if (p % L != 0 && p < 0) q--;                                         // floor
    q = min(max(q, -(1LL << 26)), 1LL << 26);
    if (scaled) q = min(max(((gain * q) >> 16) + off, -(1LL << 26)), 1LL << 26);      // (>> of a negative: arithmetic, a floor)
    return q;
}

// Cc + t of one event under pore-table row R: include/sqg_call.h's term
__device__ __forceinline__ int call_term(const CallParams& Q, const ReadDesc& rd, const uint32_t R, const long long q) {
    const BatchView& V = Q.bv;
    const long long Lv = 256 * (long long)level_code(V.model, R, V.dig, V.range, rd.offset);
    const long long d = min(max(q - Lv, -(1LL << 19)), 1LL << 19);
    const long long W = min(max(Q.w[R], 0), 1 << 24);
    const int Cc = min(max(Q.c[R], -(1 << 20)), 1 << 20);
    const long long t = min((W * d * d) >> 32, (long long)Q.term_cap);    // (W d d <= 2^62)
    return Cc + (int)t;
}

__global__ __launch_bounds__(CHUNK_WG) void k_call_score(CallParams Q) {
    const BatchView& V = Q.bv;
    const int lane = threadIdx.x & 63, k = V.k;
    for (long long base = (long long)blockIdx.x * CHUNK_WG; base < Q.n_sites; base += (long long)gridDim.x * CHUNK_WG) {
        const long long s = base + threadIdx.x;
        const bool have = s < Q.n_sites;                                  // (the lanes behind the last site reach the ballots below)
        bool inside = false, outside = false, called = false, agree = false;
        if (have) {
            const int2 rec = Q.rec[s];
            const int p = rec.x, r = rec.y;
            const ReadDesc rd = V.reads[r];
            const uint8_t* bp = V.bases + rd.base_off;
            const int len = rd.len0, ne = len - k + 1;
            const int e0 = max(0, p - k + 1), e1 = min(p, ne - 1);         // the span: e0 <= e1
            // the digits of the bases e0 .. e1 + k - 1 under either hypothesis, 3 bits each (at most 17 digits)
            unsigned long long dC = 0, dM = 0;
            unsigned int b = bp[e0];
            const int label = bp[p] == 'M' ? 1 : 0;
            for (int j = e0; j <= e1 + k - 1; j++) {
                const unsigned int g = j + 1 < len ? bp[j + 1] : 0u;
                const bool take = Q.neigh == 1 ? (g == 'G' && (b == 'C' || b == 'M')) : j == p;
                const unsigned long long own = meth_code((uint8_t)b);
                dC |= (take ? 1ULL : own) << (3 * (j - e0));
                dM |= (take ? 3ULL : own) << (3 * (j - e0));
                b = g;
            }
            uint32_t RC = 0, RM = 0;
            for (int i = 0; i < k; i++) { RC = RC * 5u + (uint32_t)(dC >> (3 * i) & 7u); RM = RM * 5u + (uint32_t)(dM >> (3 * i) & 7u); }
            const bool scaled = Q.gain != nullptr;
            const long long gain = scaled ? min(max(Q.gain[r], 1), 1 << 20) : 65536;          // (out of range: clamped, as the header says)
            const long long off = scaled ? min(max(Q.shift[r], -(1 << 26)), 1 << 26) : 0;
            int nobs = 0, nc = 0, nm = 0;
            for (int e = e0; e <= e1; e++) {
                if (e > e0) {                                             // the next k-mer: the leading digit out, one digit in
                    const int o = 3 * (e - 1 - e0), in = 3 * (e + k - 1 - e0);
                    RC = (RC - (uint32_t)(dC >> o & 7u) * Q.pow_k1) * 5u + (uint32_t)(dC >> in & 7u);
                    RM = (RM - (uint32_t)(dM >> o & 7u) * Q.pow_k1) * 5u + (uint32_t)(dM >> in & 7u);
                }
                const long long x = rd.ev_off + e;
                const long long L = Q.len64 ? Q.len64[x] : (long long)Q.len32[x];
                if (L < 1) continue;                                      // unobserved
                const long long q = call_row_value(Q.sum[x], L, scaled, gain, off);
                nc += call_term(Q, rd, RC, q);
                nm += call_term(Q, rd, RM, q);
                nobs++;
            }
            const int llr = nc - nm;
            const int cl = (nobs < Q.min_obs || abs(llr) < Q.llr_min) ? 0 : llr > 0 ? 2 : 1;
            long long key = INT64_MIN;
            if (Q.pr) {
                const PileRead pr = Q.pr[r];
                if (pr.step > 0) key = pr.key0 + p;
                else if (pr.step < 0) key = pr.key0 + k - 2 - p;
                inside = Q.have_freq && pr.step != 0 && key >= Q.lo && key < Q.hi;
            }
            outside = Q.have_freq && !inside;
            called = cl != 0; agree = called && (cl == 2) == (label == 1);
            if (Q.site_key) Q.site_key[s] = key;
            if (Q.n_obs) Q.n_obs[s] = nobs;
            if (Q.nll_c) Q.nll_c[s] = nc;
            if (Q.nll_m) Q.nll_m[s] = nm;
            if (Q.llr) Q.llr[s] = llr;
            if (Q.call) Q.call[s] = (uint8_t)cl;
            if (inside) {
                const long long at = key - Q.lo;
                if (Q.cov) __hip_atomic_fetch_add(Q.cov + at, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (Q.truth && label) __hip_atomic_fetch_add(Q.truth + at, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (Q.called && cl != 0) __hip_atomic_fetch_add(Q.called + at, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (Q.meth && cl == 2) __hip_atomic_fetch_add(Q.meth + at, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        const unsigned long long m_out = __ballot(outside), m_called = __ballot(called), m_agree = __ballot(agree);
        if (lane == 0) {
            if (m_out) __hip_atomic_fetch_add(Q.stat, (unsigned long long)__popcll(m_out), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (m_called) __hip_atomic_fetch_add(Q.stat + 1, (unsigned long long)__popcll(m_called), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (m_agree) __hip_atomic_fetch_add(Q.stat + 2, (unsigned long long)__popcll(m_agree), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
